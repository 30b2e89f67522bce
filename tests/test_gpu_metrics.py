"""GPU: the accuracy / prediction kernels (csrc/loss.hip) against metrics.py's CPU restatement (itself held to the
reference's semantics in tests/test_metrics.py), the trainer's topk=(1, 5) against a topk=None twin, and the graph-replayed
Evaluator against an eager eval forward.  Indices and hit counts must be EXACT; the loss and gradient of the hits variant
must be the same bits as the plain loss kernel's."""
import pytest
import torch

from kernel_harness import dev
from oracle import seeded
from vqa_playground_pytorch_amd import metrics

pytestmark = pytest.mark.gpu


def case(B, C, seed, specials=True):
    """Random logits with exact ties (every 7th column rounded), soft targets with zeros; with specials, a row of tied
    targets, an all-zero target row, an all-equal logit row and NaN rows."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, C, generator=g)
    z[:, ::7] = torch.round(z[:, ::7])
    a = torch.softmax(3 * torch.randn(B, C, generator=g), 1)
    a[a < 0.5 / C] = 0
    if specials and B >= 7:
        a[1] = 0                                              # all-zero target: column 0
        a[2, :] = 0
        a[2, C // 2:] = 1.0 / max(C - C // 2, 1)             # tied targets: the first of them
        z[3] = 0.25                                           # every logit tied
        z[4, ::3] = float("nan")                              # NaNs rank first
        z[5] = float("nan")
        z[6, C // 3] = float("nan")
    return z, a


def cpu_ref(z, a, k):
    return metrics.predict_topk(z, k, target=a)


def bits(t):
    return t.contiguous().view(torch.int32)


SIZES = [(B, C, k) for B in (1, 7, 512, 1501) for C in (1, 5, 300, 3000, 4096) for k in (1, 5, 16) if k <= C]


@pytest.mark.parametrize("B,C,k", SIZES)
def test_predict_topk_and_hits_match_the_restatement(B, C, k):
    from vqa_playground_pytorch_amd import ops
    z, a = case(B, C, 1000 * B + C)
    idx, prob, hits = ops.predict_topk(z.to(dev()), k, target=a.to(dev()))
    r_idx, _, r_hits = cpu_ref(z, a, k)
    assert idx.dtype == torch.int64 and hits.dtype == torch.int32
    assert torch.equal(idx.cpu(), r_idx)
    assert torch.equal(hits.cpu(), r_hits)
    sm = torch.softmax(z.double(), 1).gather(1, r_idx)
    assert torch.allclose(prob.cpu().double(), sm, rtol=0, atol=1e-6, equal_nan=True)
    idx2, prob2, hits2 = ops.predict_topk(z.to(dev()), k, probs=False)
    assert prob2 is None and hits2 is None and torch.equal(idx2.cpu(), r_idx)


@pytest.mark.parametrize("B,C,k", SIZES)
def test_kld_loss_hits_is_the_loss_kernel_plus_hits(B, C, k):
    from vqa_playground_pytorch_amd import ops
    z, a = case(B, C, 7 + B + C)
    zd, ad = z.to(dev()), a.to(dev())
    loss0, d0 = ops.kld_sum_loss_and_grad(zd, ad)
    loss1, d1, hits = ops.kld_sum_loss_and_grad_hits(zd, ad, k)
    assert torch.equal(bits(loss0), bits(loss1))              # bit for bit, NaN rows included
    assert torch.equal(bits(d0), bits(d1))
    assert torch.equal(hits.cpu(), cpu_ref(z, a, k)[2])
    z, a = case(B, C, 11 + B + C, specials=False)             # finite rows: plain torch.equal as well
    loss0, d0 = ops.kld_sum_loss_and_grad(z.to(dev()), a.to(dev()))
    loss1, d1, _ = ops.kld_sum_loss_and_grad_hits(z.to(dev()), a.to(dev()), k)
    assert torch.equal(loss0, loss1) and torch.equal(d0, d1)


def test_hits_kernels_refuse_bad_k():
    from vqa_playground_pytorch_amd import ops
    z, a = case(4, 10, 0)
    with pytest.raises(ValueError):
        ops.predict_topk(z.to(dev()), 11)
    with pytest.raises(ValueError):
        ops.kld_sum_loss_and_grad_hits(z.to(dev()), a.to(dev()), 17)


@pytest.mark.parametrize("B,C,M", [(1, 1, 1), (7, 5, 4), (1600, 12, 18), (512, 3000, 50), (1501, 4096, 256), (33, 9000, 50)])
def test_predict_candidates_matches_the_restatement(B, C, M):
    from vqa_playground_pytorch_amd import ops
    z, _ = case(B, C, B + C + M)
    g = torch.Generator().manual_seed(M)
    cand = torch.randint(-1, C + 3, (B, M), generator=g)      # -1 padding and out-of-range entries
    if B >= 7:
        cand[0] = -1                                          # no valid candidate: -1
        cand[1, :] = -1
        cand[1, : M // 2 + 1] = C // 2                        # one candidate, repeated
        z[2] = 1.0                                            # all tied: the lowest candidate column
        cand[2, -1] = C - 1
        z[3] = 0.0                                            # the answer in column 0, -1 padding after it
        z[3, 0] = 5.0
        cand[3, :] = -1
        cand[3, 0], cand[3, 1] = 0, C // 2
        z[4] = 0.0                                            # the answer in column C-1, an entry >= C after it
        z[4, C - 1] = 5.0
        cand[4, :] = C + 1
        cand[4, 0], cand[4, 1] = C - 1, 0
    got = ops.predict_candidates(z.to(dev()), cand.to(dev()))
    assert got.dtype == torch.int64
    assert torch.equal(got.cpu(), metrics.predict_candidates(z, cand))
    if B >= 7:
        assert got[:5].tolist() == [-1, C // 2, min(c for c in cand[2].tolist() if 0 <= c < C), 0, C - 1]


# ---- the trainer ---------------------------------------------------------------------------------------------------------
def build(cls, nans):
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel
    model = {"cor2": CoR2Model, "oda": ODAModel}[cls](["PAD", "UNK"], nans)
    return seeded.load_state(model, 0).to(dev())


def batch(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, 36, 2048, generator=g).to(dev())
    q = torch.randn(B, 2400, generator=g).to(dev())
    a = torch.softmax(2.0 * torch.randn(B, C, generator=g), 1).to(dev())
    return {"v": v, "q_idxes": q}, a


@pytest.mark.parametrize("overlap", [False, "force"])
def test_trainer_topk_replays_match_a_twin_without_it(overlap):
    """CoR2 at B = 512 in train mode (dropout on), graph-replayed over two input slots: with topk=(1, 5) every step's
    last_hits are the hits of last_logits, and losses, norms, weights and captured graph nodes are those of topk=None."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    C = 3000
    ring = [batch(512, C, 40 + i) for i in range(2)]
    runs = {}
    for topk in (None, (1, 5)):
        torch.manual_seed(5)
        model = build("cor2", C).train()
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True, adopt_inputs=True, input_slots=2, overlap=overlap,
                                 topk=topk)
        hist = []
        for i in range(9):
            sample, a = ring[i % 2]
            loss, norm = tr.step(sample, a)
            hist.append((loss.clone(), norm.clone()))
            if topk:
                assert tr.last_logits.shape == (512, C)
                want = metrics.topk_hits(tr.last_logits.cpu(), a.cpu(), 5)
                assert torch.equal(tr.last_hits.cpu(), want), (i, tr.last_hits.tolist(), want.tolist())
                if i >= 3:                                  # both slots captured: the graph's own outputs, one per slot
                    slot = tr._slot_of(sample, a)
                    assert slot is not None and tr.last_hits is slot["out"][0] and tr.last_logits is slot["out"][1]
        torch.cuda.synchronize()
        assert tr._graph is not None and len(tr._slots) == 2
        assert bool(tr.overlap) == bool(overlap)
        acc = tr.accuracy() if topk else None
        runs[topk] = ([(bits(l).item(), bits(n).item()) for l, n in hist], tr.flat.p.clone(), tr.graph_nodes, acc)
    (h0, p0, n0, _), (h1, p1, n1, acc) = runs[None], runs[(1, 5)]
    assert h0 == h1
    assert torch.equal(p0, p1)
    assert n0 == n1, (n0, n1)                                 # the hits variant is two kernels, like the loss it replaces
    assert all(c.get("memset", 0) == 0 for c in n1.values())
    assert len(acc) == 2 and 0.0 <= acc[0] <= acc[1] <= 100.0


@pytest.mark.parametrize("graph", [False, True])
def test_trainer_topk_eager_steps_match_a_twin_without_it(graph):
    """The kernel-by-kernel step with topk (step_eager: graph=False, and the odd-shaped last batch of an epoch after a
    capture) backpropagates d_logits from the hits kernel instead of calling loss.backward(): losses, norms and weights
    must be bitwise those of topk=None, and last_hits the hits of last_logits."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    C = 3000
    data = [batch(512, C, 60 + i) for i in range(2)] + [batch(100, C, 62)]
    order = [0, 1, 0, 1, 0, 2]                                 # the last batch: another shape
    runs = {}
    for topk in (None, (1, 5)):
        torch.manual_seed(8)
        tr = DataParallelTrainer(build("cor2", C).train(), lr=2e-5, clip=0.25, graph=graph, topk=topk)
        hist = []
        for i in order:
            sample, a = data[i]
            loss, norm = tr.step(sample, a)
            hist.append((bits(loss).item(), bits(norm).item()))
            if topk:
                assert tr.last_logits.shape == (a.size(0), C)
                want = metrics.topk_hits(tr.last_logits.cpu(), a.cpu(), 5)
                assert torch.equal(tr.last_hits.cpu(), want)
        assert (tr._graph is not None) == graph
        runs[topk] = (hist, tr.flat.p.clone())
    assert runs[None][0] == runs[(1, 5)][0]
    assert torch.equal(runs[None][1], runs[(1, 5)][1])


# ---- evaluation ----------------------------------------------------------------------------------------------------------
def _eager_logits(model, sample):
    model.eval()
    with torch.no_grad():
        return model(sample)


@pytest.mark.parametrize("cls", ["cor2", "oda"])
def test_evaluator_graph_and_eager(cls):
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    C = 3000
    model = build(cls, C).eval()
    batches = []
    for i, B in enumerate((512, 512, 512, 512, 100)):
        sample, a = batch(B, C, 90 + i)
        g = torch.Generator().manual_seed(i)
        cand = torch.randint(-1, C, (B, 50), generator=g)
        batches.append(dict(sample, a=a, a_mc_idx=cand, q_id=torch.arange(B)))
    ev = Evaluator(model, graph=True, k=5)
    for i, b in enumerate(batches):
        out = ev.step(b)
        logits = _eager_logits(model, {"v": b["v"], "q_idxes": b["q_idxes"]})
        # the replayed forward is the eager one, kernel for kernel: predictions and hits must agree EXACTLY with the
        # restatement applied to the eager logits
        r_idx, _, r_hits = metrics.predict_topk(logits.cpu(), 5, target=b["a"].cpu())
        assert torch.equal(out["top_idx"].cpu(), r_idx)
        assert torch.equal(out["pred"].cpu(), logits.argmax(1).cpu())
        assert torch.equal(out["pred"], out["top_idx"][:, 0])
        assert torch.equal(out["hits"].cpu(), r_hits)
        sm = torch.softmax(logits.double(), 1).gather(1, r_idx.to(logits.device))
        assert torch.allclose(out["top_prob"].double(), sm, rtol=0, atol=1e-6)
        assert torch.equal(out["pred_mc"].cpu(), metrics.predict_candidates(logits.cpu(), b["a_mc_idx"]))
        if i >= 2 and b["v"].size(0) == 512:
            assert ev._graph is not None and out is ev._graph["out"]          # replayed
        if b["v"].size(0) == 100:
            assert out is not ev._graph["out"]                                # another shape: eager
    assert ev.graph_nodes.get("kernel", 0) > 10 and ev.graph_nodes.get("memset", 0) == 0, ev.graph_nodes
    results, acc = ev.run(batches)
    assert len(results) == 4 * 512 + 100 and acc is not None and 0.0 <= acc[0] <= acc[1] <= 100.0


def test_trainer_graphs_survive_an_evaluation():
    """A trainer's next replayed step after a graph-replayed evaluation of its model equals that of a twin that did not
    evaluate (same seeds, same batches): the Evaluator's graph and pool leave the trainer's alone."""
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    C = 3000
    sample, a = batch(512, C, 7)
    ev_batch = dict(batch(512, C, 8)[0], q_id=torch.arange(512))
    got = {}
    for evaluate in (False, True):
        torch.manual_seed(3)
        model = build("cor2", C).train()
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True, topk=(1, 5))
        for _ in range(5):
            tr.step(sample, a)
        assert tr._graph is not None
        if evaluate:
            ev = Evaluator(model, graph=True)
            for _ in range(4):
                ev.step(ev_batch)
            assert ev._graph is not None and model.training
        loss, norm = tr.step(sample, a)
        torch.cuda.synchronize()
        got[evaluate] = (bits(loss).item(), bits(norm).item(), tr.last_hits.clone(), tr.flat.p.clone())
    assert got[False][:2] == got[True][:2]
    assert torch.equal(got[False][2], got[True][2]) and torch.equal(got[False][3], got[True][3])
