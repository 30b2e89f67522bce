"""Top-k accuracy and predictions on the CPU: metrics.py's torch restatement against the reference's semantics written out
independently here (accuracy(), train.py:22-38; test()'s OpenEnded / MultipleChoice loops, train.py:110-191; visu.py's top-5
softmax, :188-194), the trainer's topk=(1, 5) on two gloo ranks, the evaluation's file layout and the new C-ABI symbols."""
import json
import math
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from vqa_playground_pytorch_amd import metrics


# ---- independent restatement -------------------------------------------------------------------------------------------
def _key(v, c):
    """Sort key of (value, column), best first: NaN above every number, larger value, then lower column."""
    return (0, 0.0, c) if math.isnan(v) else (1, -v, c)


def ref_order(row):
    return sorted(range(len(row)), key=lambda c: _key(row[c], c))


def ref_target(trow):
    """torch.max(target, 1): the first index of the largest value (NaN largest)."""
    best = 0
    for c in range(1, len(trow)):
        if _key(trow[c], c) < _key(trow[best], best):
            best = c
    return best


def ref_hits(logits, target, kmax):
    hits = [0] * kmax
    for row, trow in zip(logits.tolist(), target.tolist()):
        rank = ref_order(row).index(ref_target(trow))
        for j in range(kmax):
            hits[j] += rank <= j
    return hits


def ref_candidates(logits, cand):
    """The reference's MultipleChoice loop (train.py:151-161): columns in order, replace only on a better logit."""
    out = []
    for row, mc in zip(logits.tolist(), cand.tolist()):
        allowed = {e for e in mc if 0 <= e < len(row)}
        pred, best = -1, None
        for k in range(len(row)):
            if k in allowed and (pred == -1 or _key(row[k], k) < _key(best, pred)):
                pred, best = k, row[k]
        out.append(pred)
    return out


def hard_cases():
    """Rows with tied targets, an all-zero target, exactly tied logits, NaNs, -inf; C = 6."""
    nan, inf = float("nan"), float("inf")
    logits = torch.tensor([[0.1, 0.5, 0.5, 0.2, 0.5, -1.0],
                           [1.0, 1.0, 1.0, 1.0, 1.0, 1.0],
                           [0.3, nan, 2.0, nan, -0.5, 0.0],
                           [nan, nan, nan, nan, nan, nan],
                           [-inf, -inf, 0.0, -inf, 1.0, -inf],
                           [2.0, 1.0, 3.0, 0.0, 3.0, 1.0]])
    target = torch.tensor([[0.0, 0.0, 0.3, 0.0, 0.3, 0.1],     # tie: column 2 is the target
                           [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],     # all zero: column 0
                           [0.0, 0.0, 0.0, 0.9, 0.0, 0.0],     # target on the second NaN
                           [0.0, 0.0, 0.0, 0.0, 0.0, 1.0],
                           [0.0, 0.0, 0.0, 0.5, 0.0, 0.0],     # -inf target, tied with lower columns
                           [0.0, 0.0, 0.0, 0.0, 1.0, 0.0]])    # tied logit, behind column 2
    return logits, target


def random_case(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, C, generator=g)
    logits[:, ::7] = torch.round(logits[:, ::7])          # plenty of exact ties
    target = torch.softmax(3 * torch.randn(B, C, generator=g), 1)
    target[target < 0.05] = 0
    return logits, target


@pytest.mark.parametrize("kmax", [1, 5, 6])
def test_topk_hits_hard_cases(kmax):
    logits, target = hard_cases()
    got = metrics.topk_hits(logits, target, kmax)
    assert got.dtype == torch.int32
    assert got.tolist() == ref_hits(logits, target, kmax)


@pytest.mark.parametrize("B,C,kmax", [(1, 1, 1), (7, 5, 5), (33, 300, 16), (9, 16, 16)])
def test_topk_hits_random(B, C, kmax):
    logits, target = random_case(B, C, B * C)
    assert metrics.topk_hits(logits, target, kmax).tolist() == ref_hits(logits, target, kmax)


def test_topk_hits_match_the_reference_accuracy():
    """accuracy(output, a, topk=(1, 5)) of train.py on rows without ties: output.topk + torch.max(target, 1)."""
    logits, target = random_case(64, 40, 3)
    logits = logits + 1e-3 * torch.arange(40.0)         # no ties
    _, pred = logits.topk(5, 1, True, True)
    correct = pred.t().eq(torch.max(target, 1)[1].view(1, -1).expand(5, -1))
    want = [100.0 * correct[:k].reshape(-1).float().sum().item() / 64 for k in (1, 5)]
    hits = metrics.topk_hits(logits, target, 5)
    assert metrics.accuracy(hits, 64, (1, 5)) == pytest.approx(want, abs=1e-9)


@pytest.mark.parametrize("k", [1, 5, 6])
def test_predict_topk_hard_cases(k):
    logits, target = hard_cases()
    idx, prob, hits = metrics.predict_topk(logits, k, target=target)
    assert idx.dtype == torch.int64 and idx.shape == (6, k)
    assert idx.tolist() == [ref_order(r)[:k] for r in logits.tolist()]
    assert hits.tolist() == ref_hits(logits, target, k)
    sm = torch.softmax(logits.double(), 1).gather(1, idx)
    assert torch.allclose(prob.double(), sm, atol=1e-6, equal_nan=True)


def test_predict_topk_random_and_k_equals_c():
    logits, target = random_case(20, 16, 8)
    idx, prob, hits = metrics.predict_topk(logits, 16, target=target)
    assert idx.tolist() == [ref_order(r) for r in logits.tolist()]
    assert idx[:, 0].tolist() == logits.max(1)[1].tolist()           # test()'s OpenEnded answer
    # visu.py: softmax(sorted scores)[:, :5]
    sort_score, _ = logits.sort(1, descending=True)
    assert torch.allclose(prob[:, :5], torch.softmax(sort_score, 1)[:, :5], atol=1e-6)
    assert hits.tolist() == ref_hits(logits, target, 16)
    idx, prob, hits = metrics.predict_topk(logits, 3, probs=False)
    assert prob is None and hits is None and idx.shape == (20, 3)


def test_k_limits():
    logits, target = random_case(2, 5, 0)
    for k in (0, 6):
        with pytest.raises(ValueError):
            metrics.topk_hits(logits, target, k)
    with pytest.raises(ValueError):
        metrics.predict_topk(torch.zeros(2, 40), 17)


def test_predict_candidates():
    nan = float("nan")
    logits = torch.tensor([[0.1, 0.9, 0.3, 0.9, 0.0],
                           [0.1, 0.9, 0.3, 0.9, 0.0],
                           [5.0, 1.0, nan, 2.0, 3.0],
                           [1.0, 2.0, 3.0, 4.0, 5.0],
                           [1.0, 2.0, 3.0, 4.0, 5.0],
                           [-1.0, -1.0, -1.0, -1.0, -1.0]])
    cand = torch.tensor([[3, 1, -1, -1],        # tie: the lower column wins, whatever the candidate order
                         [0, 2, 4, -1],
                         [0, 2, 3, -1],         # NaN ranks above every number
                         [-1, -1, -1, -1],      # no valid candidate
                         [7, -3, 5, 2],         # out-of-range entries are ignored
                         [4, 2, 2, -1]])        # duplicates
    got = metrics.predict_candidates(logits, cand)
    assert got.dtype == torch.int64
    assert got.tolist() == ref_candidates(logits, cand) == [1, 2, 2, -1, 2, 2]
    logits, _ = random_case(30, 300, 4)
    g = torch.Generator().manual_seed(9)
    cand = torch.randint(-1, 320, (30, 50), generator=g)
    assert metrics.predict_candidates(logits, cand).tolist() == ref_candidates(logits, cand)


def test_predict_candidates_at_the_edge_columns():
    """The answer in column 0 followed by -1 padding, and in column C-1 followed by an entry >= C: an ignored entry must not
    clear the mark of a real candidate in the column it would be clamped to."""
    got = metrics.predict_candidates(torch.tensor([[5.0, 1.0, 2.0, 0.0], [0.0, 1.0, 2.0, 9.0]]),
                                     torch.tensor([[0, 2, -1, -1], [3, 1, 7, -1]]))
    assert got.tolist() == [0, 3]
    # small rows, many candidates: every edge case many times over
    g = torch.Generator().manual_seed(12)
    logits = torch.randn(1600, 12, generator=g)
    logits[:, ::3] = torch.round(logits[:, ::3])
    cand = torch.randint(-2, 15, (1600, 18), generator=g)
    cand[::4, 5:] = -1
    assert metrics.predict_candidates(logits, cand).tolist() == ref_candidates(logits, cand)


def test_accuracy_percentages():
    assert metrics.accuracy(torch.tensor([3, 5, 6, 7, 8], dtype=torch.int32), 10) == [30.0, 80.0]
    assert metrics.accuracy([1, 2], 4, topk=(2,)) == [50.0]


# ---- the trainer on two gloo ranks -------------------------------------------------------------------------------------
class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(12, 16)
        self.b = nn.Linear(16, 9)

    def forward(self, sample):
        return self.b(torch.tanh(self.a(sample["x"])))


def make_data(steps=4, batch=8):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(batch, 12, generator=g), torch.softmax(2 * torch.randn(batch, 9, generator=g), 1))
            for _ in range(steps)]


def run_single(topk):
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    torch.manual_seed(0)
    model = Tiny()
    tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, topk=topk)
    out, acc, logits = [], [], []
    for x, a in make_data():
        loss, norm = tr.step({"x": x}, a)
        out.append((loss.item(), norm.item()))
        if topk:
            assert tr.last_logits.shape == (8, 9)
            assert tr.last_hits.tolist() == ref_hits(tr.last_logits, a, 5)
            acc.append(tr.accuracy())
            logits.append(tr.last_logits.clone())
    return out, [p.detach().clone() for p in model.parameters()], (acc, logits)


def _worker(rank, world, port, q):
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    model = Tiny()
    tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, topk=(1, 5))
    acc, local = [], []
    for x, a in make_data():
        tr.step({"x": tr.shard(x)}, tr.shard(a))
        local.append(tr.last_hits.tolist())
        acc.append(tr.accuracy())
    q.put((rank, acc, local))
    dist.barrier()
    dist.destroy_process_group()


def test_trainer_topk_on_two_ranks_equals_one_process():
    base, w_base, _ = run_single(None)
    with_k, w_k, (acc_single, logits_single) = run_single((1, 5))
    assert base == with_k                                    # loss and norm: the same numbers, bit for bit
    assert all(torch.equal(a, b) for a, b in zip(w_base, w_k))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=120) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    (_, acc0, local0), (_, acc1, local1) = results
    assert acc0 == acc1 == acc_single                        # accuracy() is over the global batch on every rank
    whole = [ref_hits(tr_logits, a, 5) for tr_logits, (_, a) in zip(logits_single, make_data())]
    assert [[a + b for a, b in zip(x, y)] for x, y in zip(local0, local1)] == whole     # each rank counts its own half


def test_trainer_refuses_bad_topk_at_construction():
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    for topk in ((0,), (1, 17), (-1, 5)):
        with pytest.raises(ValueError):
            DataParallelTrainer(Tiny(), lr=1e-2, topk=topk)


def test_trainer_without_topk_has_no_accuracy():
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    tr = DataParallelTrainer(Tiny(), lr=1e-2)
    x, a = make_data(1)[0]
    tr.step({"x": x}, a)
    assert tr.last_hits is None and tr.last_logits is None
    with pytest.raises(RuntimeError):
        tr.accuracy()


# ---- evaluation: batches, files, CPU evaluator -------------------------------------------------------------------------
def test_collate_pads_multiple_choice_candidates():
    from vqa_playground_pytorch_amd import feed
    items = [{"v": torch.zeros(2, 3), "q_idxes": [1, 2], "q_id": 7, "a": torch.zeros(4), "a_mc_idx": [3, 1, 2]},
             {"v": torch.ones(2, 3), "q_idxes": [2, 3], "q_id": 8, "a": torch.ones(4), "a_mc_idx": list(range(50))}]
    b = feed.collate(items, 4)
    assert b["a_mc_idx"].dtype == torch.int64 and b["a_mc_idx"].shape == (2, 50)
    assert b["a_mc_idx"][0].tolist() == [3, 1, 2] + [-1] * 47
    assert b["a_mc_idx"][1].tolist() == list(range(50))
    assert "a_mc_idx" not in feed.collate([{k: v for k, v in it.items() if k != "a_mc_idx"} for it in items], 4)
    with pytest.raises(ValueError):
        feed.collate([dict(items[0], a_mc_idx=list(range(51)))], 4)


def test_results_file_layout_round_trips(tmp_path):
    from vqa_playground_pytorch_amd.evaluate import results_filename, write_results
    log_dir = str(tmp_path / "cor2_run")
    path = results_filename(log_dir, "test_dev", "OpenEnded", 7)
    assert path == os.path.join(log_dir, "epoch_7", "vqa_OpenEnded_mscoco_test-dev2015_cor2_run007_results.json")
    results = [{"question_id": 1, "answer": "yes"}, {"question_id": 22, "answer": "2"}]
    assert write_results(results, path) == path
    with open(path) as fh:
        assert json.load(fh) == results


class Vocab:
    def idx2word(self, i):
        return "w%d" % i


class Lin(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(6, 12)
        self.drop = nn.Dropout(0.5)

    def forward(self, sample):
        return self.lin(self.drop(sample["v"].mean(1) + sample["q_idxes"].float().mean(1, keepdim=True)))


def test_cpu_evaluator_runs_the_reference_loops():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    torch.manual_seed(3)
    model = Lin().train()
    g = torch.Generator().manual_seed(1)
    batches = []
    for i in range(3):
        B = 5 if i < 2 else 3
        batches.append({"v": torch.randn(B, 4, 6, generator=g), "q_idxes": torch.randint(0, 9, (B, 3), generator=g),
                        "q_id": torch.arange(10 * i, 10 * i + B), "a": torch.softmax(torch.randn(B, 12, generator=g), 1),
                        "a_mc_idx": torch.randint(-1, 12, (B, 50), generator=g)})
    ev = Evaluator(model, graph=True, k=5)          # a CPU model: eager whatever graph says
    results, acc = ev.run(batches, Vocab())
    assert model.training                            # mode restored
    model.eval()
    with torch.no_grad():
        logits = [model(b) for b in batches]
    want = [{"question_id": int(q), "answer": "w%d" % int(p)} for b, lg in zip(batches, logits)
            for q, p in zip(b["q_id"], lg.argmax(1))]
    assert results == want
    hits = [sum(x) for x in zip(*[ref_hits(lg, b["a"], 5) for b, lg in zip(batches, logits)])]
    assert acc == pytest.approx((100.0 * hits[0] / 13, 100.0 * hits[4] / 13))
    batches[0]["a_mc_idx"][1] = -1                  # a question without a valid candidate: answer None, never idx2word(-1)
    mc, _ = ev.run(batches, None, eval_metric="MultipleChoice", max_step=2)
    want = [None if p < 0 else p for b, lg in zip(batches[:2], logits) for p in ref_candidates(lg, b["a_mc_idx"])]
    assert [r["answer"] for r in mc] == want and len(mc) == 10 and mc[1]["answer"] is None
    mc, _ = ev.run(batches, Vocab(), eval_metric="MultipleChoice", max_step=1)
    assert [r["answer"] for r in mc] == [None if p is None else "w%d" % p for p in want[:5]]
    out = ev.step(batches[0])
    assert set(out) == {"pred", "top_idx", "top_prob", "pred_mc", "hits"}
    with pytest.raises(ValueError):
        ev.run(batches, eval_metric="WUPS")


# ---- the C ABI -----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_abi_is_14():
    from vqa_playground_pytorch_amd import _lib
    assert _lib.ABI_VERSION == 14
    handle = _lib.lib()
    assert handle.vqa_version() == 14
    for name in ("vqa_kld_sum_loss_hits", "vqa_kld_sum_loss_hits_workspace_bytes", "vqa_predict_topk",
                 "vqa_predict_topk_workspace_bytes", "vqa_predict_candidates"):
        assert name in _lib.SIGNATURES and hasattr(handle, name)
    assert handle.vqa_kld_sum_loss_hits_workspace_bytes(512, 5) >= 512 * 8
    assert handle.vqa_predict_topk_workspace_bytes(512, 5) >= 512 * 4


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    from vqa_playground_pytorch_amd import _lib
    h = _lib.lib()
    p = 16     # never dereferenced: the checks come first
    assert h.vqa_kld_sum_loss_hits(p, p, p, p, p, 5, p, 1 << 20, 4, 4097, None) == -2     # C over 4096
    assert h.vqa_kld_sum_loss_hits(p, p, p, p, p, 17, p, 1 << 20, 4, 300, None) == -1     # kmax over 16
    assert h.vqa_kld_sum_loss_hits(p, p, p, p, p, 6, p, 1 << 20, 4, 5, None) == -1        # kmax over C
    assert h.vqa_kld_sum_loss_hits(p, p, p, p, p, 5, p, 8, 4, 300, None) == -1            # workspace too small
    assert h.vqa_predict_topk(p, None, p, p, None, 0, None, 0, 4, 300, None) == -1
    assert h.vqa_predict_topk(p, p, p, p, None, 5, p, 1 << 20, 4, 300, None) == -1       # a target needs hits
    assert h.vqa_predict_candidates(p, p, p, 4, 300, 257, None) == -2
    assert b"257" in h.vqa_last_error()
