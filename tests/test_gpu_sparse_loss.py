"""Kernel-level checks of the sparse-target loss kernels (csrc/loss_sparse.hip) and of the train step that uses them.

Float64 parity against torch's criteria on the densified target, at the 256-thread boundaries and the 4096-column register
limit of a row, the 256-row stride of the one-workgroup total and the ends of the pair loop (K = 1, 10, 16); the dense kernels
of csrc/loss.hip on the same densified target; hit counts against the dense _hits forms and metrics.topk_hits; the sampled CE
against a CPU restatement of its hash-to-label rule and against the dense CE kernel on the labels it drew.

Bars: those of tests/test_gpu_loss_optim_kernels.py -- 1e-5 relative on a loss, 1e-5 of the float64 (or dense) gradient's maximum
on d_logits.  Logits are uniform in [-15, 15] as there, except at C <= 2, where they are drawn in [-2, 2]: with one or two columns
a row's whole loss can be log(1 + e^-d) for a large d, far below the fp32 resolution of logsumexp and softplus themselves
(~6e-8 absolute next to values of order 1 .. 10), and a RELATIVE bar on it would measure the seed rather than the kernel; in [-2, 2]
every row's loss is at least 0.018."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from kernel_harness import dev
from vqa_playground_pytorch_amd import _lib, metrics, ops

pytestmark = pytest.mark.gpu

BAR = 1e-5


def reference_dense(a_idx, a_val, C):
    """datasets.py:963-969 per row: a = zeros; for c_id, c_prob in pairs: a[c_id] = c_prob -- ids outside [0, C) skipped."""
    out = np.zeros((len(a_idx), C), np.float32)
    for b, (ids, vals) in enumerate(zip(a_idx.tolist(), a_val.numpy())):
        for c_id, c_prob in zip(ids, vals):
            if 0 <= c_id < C:
                out[b, c_id] = c_prob
    return torch.from_numpy(out)


# ---- the CPU restatement of the draw: hash -> u -> label ------------------------------------------------------------------------
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def mask_word(counter, seed):
    """common.hpp's counter hash: the lowbias32 finaliser of the counter's low word xor-ed with a key made of the seed's two halves
    and the counter's high word."""
    counter, seed = counter & M64, seed & M64
    key = (seed & M32) ^ (((seed >> 32) * 0x9E3779B9) & M32) ^ (((counter >> 32) * 0x85EBCA6B) & M32)
    x = (counter & M32) ^ key
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def draw_labels(a_idx, a_val, C, seed, row_offset=0):
    """label_b = the id of the first live pair whose running fp32 sum of a_val exceeds u_b * (fp32 sum of the live a_val), with
    u_b = (mask_word(row_offset + b, seed) >> 8) * 2^-24; pairs with a_val = 0 are never drawn; -1 without a live positive pair."""
    f = np.float32
    labels = []
    for b, (ids, vals) in enumerate(zip(a_idx.tolist(), a_val.numpy())):
        K = len(ids)
        live = [0 <= ids[j] < C and ids[j] not in ids[j + 1:] for j in range(K)]
        total = f(0)
        for j in range(K):
            if live[j]:
                total = f(total + vals[j])
        thr = f(f(mask_word(row_offset + b, seed) >> 8) * f(2.0 ** -24) * total)
        run, pick = f(0), -1
        for j in range(K):
            if live[j] and vals[j] > 0:
                run = f(run + vals[j])
                if run > thr:
                    pick = ids[j]
                    break
        labels.append(pick)
    return torch.tensor(labels, dtype=torch.int64)


# ---- the inputs and their float64 references, made once per shape ---------------------------------------------------------------
_cases = {}


def sparse_case(B, C, K):
    """logits as the module docstring says; rows of random pairs with padding anywhere, and (as far as B and K have room) a row that
    holds a duplicated id whose later value differs + an id at C - 1 + an id >= C + a pair with value 0 + a pair with value 1.0, an
    all-padding row, a single pair, and each of those traits on a row of its own.  The float64 loss and gradient of torch's KLD
    and BCE criteria on the densified target."""
    if (B, C, K) not in _cases:
        g = torch.Generator().manual_seed(100000 * K + 1000 * B + C)
        span = 15.0 if C > 2 else 2.0
        z = ((torch.rand(B, C, generator=g) * 2 - 1) * span).float()
        a_idx = torch.randint(0, C, (B, K), generator=g).to(torch.int32)
        a_val = torch.rand(B, K, generator=g)
        a_idx[torch.rand(B, K, generator=g) < 0.35] = -1
        c1, c2, c3 = C // 3, C // 2, (2 * C) // 3

        def put(b, pairs):
            if b < B:
                a_idx[b], a_val[b] = -1, 0.0
                for j, (c, v) in enumerate(pairs[:K]):
                    a_idx[b, j], a_val[b, j] = c, v
        put(0, [(C - 1, 1.0)] if K < 6 else [(c1, 0.3), (C - 1, 0.25), (C, 0.9), (c1, 0.6), (c2, 0.0), (c3, 1.0)])
        put(1, [])
        put(2, [(c2, 0.8)])
        put(3, [(c1, 0.2), (c1, 0.5)])
        put(4, [(C - 1, 0.4), (C + 3, 0.7)])
        put(5, [(c3, 0.0), (c1, 0.3)])
        put(6, [(c2, 1.0)])
        dense = reference_dense(a_idx, a_val, C)
        ref = {}
        zd = z.double().requires_grad_()
        loss = F.kl_div(F.log_softmax(zd, dim=1), dense.double(), reduction="sum")
        loss.backward()
        ref["kld"] = (loss.item(), zd.grad.clone())
        zd = z.double().requires_grad_()
        loss = torch.nn.BCELoss()(torch.sigmoid(zd), dense.double())
        loss.backward()
        ref["bce"] = (loss.item(), zd.grad.clone())
        _cases[(B, C, K)] = (z, a_idx, a_val, dense, ref)
    return _cases[(B, C, K)]


def errors(loss, d, want, want_d):
    e_loss = abs(loss - want) / abs(want) if want != 0.0 else abs(loss)
    top = want_d.abs().max().item()
    e_grad = (d - want_d).abs().max().item() / top if top > 0 else d.abs().max().item()
    return e_loss, e_grad


SHAPES_C = [1, 2, 255, 256, 257, 2000, 4095, 4096]


@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("C", SHAPES_C)
@pytest.mark.parametrize("B", [1, 3, 257])
def test_kld_and_bce_match_torch_in_float64_and_the_dense_kernels(B, C, K, measured):
    z, a_idx, a_val, dense, ref = sparse_case(B, C, K)
    assert torch.equal(ops.densify(a_idx, a_val, C), dense)
    zg, ig, vg, dg = z.to(dev()), a_idx.to(dev()), a_val.to(dev()), dense.to(dev())
    for kind, got, same in (("kld", ops.kld_sum_loss_and_grad_sparse(zg, ig, vg), ops.kld_sum_loss_and_grad(zg, dg)),
                            ("bce", ops.bce_mean_loss_and_grad_sparse(zg, ig, vg), ops.bce_mean_loss_and_grad(zg, dg))):
        loss, d = got[0].item(), got[1].cpu().double()
        assert np.isfinite(loss) and torch.isfinite(d).all()
        e_loss, e_grad = errors(loss, d, *ref[kind])
        d_loss, d_grad = errors(loss, d, same[0].item(), same[1].cpu().double())
        measured("%s loss rel B=%d C=%d K=%d" % (kind, B, C, K), e_loss, BAR)
        measured("%s grad/max B=%d C=%d K=%d" % (kind, B, C, K), e_grad, BAR)
        measured("%s loss vs dense B=%d C=%d K=%d" % (kind, B, C, K), d_loss, BAR)
        measured("%s grad vs dense B=%d C=%d K=%d" % (kind, B, C, K), d_grad, BAR)
        assert e_loss <= BAR, (kind, loss, ref[kind][0])
        assert e_grad <= BAR, kind
        assert d_loss <= BAR, (kind, loss, same[0].item())
        assert d_grad <= BAR, kind
    if B > 1:       # a row without a live pair: gradient 0 under KLD
        assert not ops.kld_sum_loss_and_grad_sparse(zg, ig, vg)[1][1].any()


def test_scale_is_the_callers():
    z, a_idx, a_val, dense, ref = sparse_case(3, 257, 10)
    zg, ig, vg = z.to(dev()), a_idx.to(dev()), a_val.to(dev())
    loss, d = ops.bce_mean_loss_and_grad_sparse(zg, ig, vg, 1.0 / (2 * 3 * 257))
    want, want_d = ref["bce"]
    assert abs(loss.item() - want / 2) <= BAR * abs(want / 2)
    assert (d.cpu().double() - want_d / 2).abs().max().item() <= BAR * (want_d / 2).abs().max().item()
    full = ops.ce_mean_loss_and_grad_sampled(zg, ig, vg, seed=5)
    half = ops.ce_mean_loss_and_grad_sampled(zg, ig, vg, scale=1.0 / 6, seed=5)
    assert torch.equal(full[2], half[2])
    assert abs(half[0].item() - full[0].item() / 2) <= BAR * abs(full[0].item() / 2)


# ---- hits -----------------------------------------------------------------------------------------------------------------------
def hits_case(B, C, K, seed):
    """tests/test_gpu_loss_optim_kernels.py's hits_case on pairs: logits with heavy ties, rows of NaNs, a row that is all NaN; an
    all-padding row (the target is column 0), tied target maxima given highest id first (the lowest id is the target), a row whose
    pairs all hold 0 (column 0 again)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-3, 4, (B, C), generator=g).float()
    z[B // 2:] += torch.randn(B - B // 2, C, generator=g)
    a_idx = torch.randint(0, C, (B, K), generator=g).to(torch.int32)
    a_val = (torch.randint(1, 4, (B, K), generator=g) / 4.0).float()          # few distinct values: tied maxima in many rows
    a_idx[torch.rand(B, K, generator=g) < 0.3] = -1
    a_idx[0] = -1
    if B > 2:
        a_idx[1], a_val[1] = -1, 0.0
        a_idx[1, 0], a_val[1, 0] = C - 1, 0.7
        if K > 1:
            a_idx[1, K - 1], a_val[1, K - 1] = C // 3, 0.7
        z[2, ::3] = float("nan")
    if B > 3:
        z[3] = float("nan")
    if B > 4:
        a_val[4] = 0.0
    return z, a_idx, a_val


@pytest.mark.parametrize("B,C,K,k", [(1, 1, 1, 1), (3, 5, 4, 5), (9, 257, 10, 5), (257, 300, 16, 16), (7, 4096, 10, 16)])
def test_hits_equal_the_dense_forms_and_leave_the_loss_alone(B, C, K, k):
    z, a_idx, a_val = hits_case(B, C, K, 7 * B + C)
    dense = reference_dense(a_idx, a_val, C)
    zg, ig, vg, dg = z.to(dev()), a_idx.to(dev()), a_val.to(dev()), dense.to(dev())
    want = metrics.topk_hits(z, dense, k).tolist()
    for kind in ("kld_sum", "bce_mean"):
        plain = getattr(ops, kind + "_loss_and_grad_sparse")(zg, ig, vg)
        loss, d, hits = getattr(ops, kind + "_loss_and_grad_sparse_hits")(zg, ig, vg, k)
        assert hits.dtype == torch.int32 and hits.cpu().tolist() == want, kind
        assert hits.cpu().tolist() == getattr(ops, kind + "_loss_and_grad_hits")(zg, dg, k)[2].cpu().tolist(), kind
        assert hits.cpu().tolist() == metrics.topk_hits(zg, (ig, vg), k).cpu().tolist(), kind
        assert torch.equal(loss.view(torch.int32), plain[0].view(torch.int32)), kind
        assert torch.equal(d.view(torch.int32), plain[1].view(torch.int32)), kind
    plain = ops.ce_mean_loss_and_grad_sampled(zg, ig, vg, seed=11 + B)
    loss, d, hits, labels = ops.ce_mean_loss_and_grad_sampled_hits(zg, ig, vg, k, seed=11 + B)
    assert torch.equal(labels, plain[2])
    assert torch.equal(loss.view(torch.int32), plain[0].view(torch.int32))
    assert torch.equal(d.view(torch.int32), plain[1].view(torch.int32))
    lab = labels.cpu()
    keep = lab >= 0
    want = metrics.topk_hits(z[keep], lab[keep], k).tolist() if keep.any() else [0] * k     # a row without a label is never a hit
    assert hits.cpu().tolist() == want


# ---- the sampled CE ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 10, 16])
@pytest.mark.parametrize("C", SHAPES_C)
@pytest.mark.parametrize("B", [1, 3, 257])
def test_sampled_ce_draws_live_labels_and_is_ce_on_them(B, C, K, measured):
    z, a_idx, a_val, dense, _ = sparse_case(B, C, K)
    zg, ig, vg = z.to(dev()), a_idx.to(dev()), a_val.to(dev())
    k = min(5, C)
    seed = 977 * B + C + K
    loss, d, hits, labels = ops.ce_mean_loss_and_grad_sampled_hits(zg, ig, vg, k, seed=seed)
    lab = labels.cpu()
    assert lab.dtype == torch.int64 and lab.shape == (B,)
    drawable = dense.max(1).values > 0
    assert torch.equal(lab >= 0, drawable)                                    # -1 exactly for the rows without a positive pair
    assert (lab[~drawable] == -1).all() and (lab[drawable] < C).all()
    assert (dense[drawable].gather(1, lab[drawable][:, None]) > 0).all()      # a live id with positive value
    assert torch.equal(lab, draw_labels(a_idx, a_val, C, seed))
    assert not d.cpu()[~drawable].any()                                       # no label: zero gradient
    keep = drawable.to(dev())
    want = ops.ce_mean_loss_and_grad_hits(zg[keep], labels[keep], k, scale=1.0 / B)
    e_loss, e_grad = errors(loss.item(), d[keep].cpu().double(), want[0].item(), want[1].cpu().double())
    measured("ce sampled loss vs ce B=%d C=%d K=%d" % (B, C, K), e_loss, BAR)
    measured("ce sampled grad vs ce B=%d C=%d K=%d" % (B, C, K), e_grad, BAR)
    assert e_loss <= BAR and e_grad <= BAR
    assert hits.cpu().tolist() == want[2].cpu().tolist()
    # and torch's own criterion in float64 on those labels
    zd = z[drawable].double().requires_grad_()
    ref = F.cross_entropy(zd, lab[drawable], reduction="sum") / B
    ref.backward()
    e_loss, e_grad = errors(loss.item(), d[keep].cpu().double(), ref.item(), zd.grad)
    measured("ce sampled loss rel B=%d C=%d K=%d" % (B, C, K), e_loss, BAR)
    measured("ce sampled grad/max B=%d C=%d K=%d" % (B, C, K), e_grad, BAR)
    assert e_loss <= BAR and e_grad <= BAR


def test_the_draw_is_a_function_of_seed_salt_and_row():
    B, C, K = 128, 300, 10
    g = torch.Generator().manual_seed(3)
    z = torch.randn(2 * B, C, generator=g).to(dev())
    a_idx = torch.stack([torch.randperm(C, generator=g)[:K] for _ in range(2 * B)]).to(torch.int32).to(dev())
    a_val = (torch.rand(2 * B, K, generator=g) + 0.1).to(dev())
    draw = lambda rows, **kw: ops.ce_mean_loss_and_grad_sampled(z[rows], a_idx[rows], a_val[rows], **kw)[2]      # noqa: E731
    both, lo, hi = slice(0, 2 * B), slice(0, B), slice(B, 2 * B)
    first = draw(both, seed=1234)
    assert torch.equal(first, draw(both, seed=1234))                                   # the same seed: the same labels
    assert not torch.equal(first, draw(both, seed=1235))                               # another seed: others
    assert torch.equal(first.cpu(), draw_labels(a_idx.cpu(), a_val.cpu(), C, 1234))
    assert torch.equal(draw(hi, seed=1234, row_offset=B), first[B:])                   # the second half of the 2B call
    assert torch.equal(draw(lo, seed=1234), first[:B])
    assert not torch.equal(draw(hi, seed=1234), first[B:])                             # (without the offset: rows 0 .. B-1 again)
    # the device word + salt is the host seed of that sum; another salt, or the word moved on, draws others
    word = torch.tensor([1000], dtype=torch.int64, device=dev())
    assert torch.equal(draw(both, seed=(word, 234)), first)
    assert not torch.equal(draw(both, seed=(word, 235)), first)
    word += 1
    assert torch.equal(draw(both, seed=(word, 233)), first)
    assert torch.equal(draw(both, seed=(word, 234)), draw(both, seed=1235))
    # a 64-bit seed and a counter past 2^32 reach the hash's key
    big, far = 0x123456789ABCDEF, (1 << 32) + 5
    assert torch.equal(draw(lo, seed=big, row_offset=far).cpu(), draw_labels(a_idx[lo].cpu(), a_val[lo].cpu(), C, big, far))


def test_draw_frequencies_follow_the_probabilities():
    """4096 rows holding the same three pairs with values 6 / 3 / 1: each label's count lies within 5 binomial standard deviations
    of its expectation.  The draw is a fixed function of the seed: the seed is the first one whose CPU restatement sits inside
    the bound (almost every seed does), and the GPU labels equal that restatement exactly."""
    N, C = 4096, 2000
    a_idx = torch.tensor([[7, 1999, 300]], dtype=torch.int32).repeat(N, 1)
    a_val = torch.tensor([[6.0, 3.0, 1.0]]).repeat(N, 1)
    expect = {7: 0.6, 1999: 0.3, 300: 0.1}

    def inside(labels):
        return all(abs((labels == c).sum().item() - N * p) <= 5 * (N * p * (1 - p)) ** 0.5 for c, p in expect.items())
    seed = next(s for s in range(1, 50) if inside(draw_labels(a_idx, a_val, C, s)))
    z = torch.zeros(N, C, device=dev())
    labels = ops.ce_mean_loss_and_grad_sampled(z, a_idx.to(dev()), a_val.to(dev()), seed=seed)[2].cpu()
    assert torch.equal(labels, draw_labels(a_idx, a_val, C, seed))
    assert inside(labels) and set(labels.tolist()) == set(expect)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    h = _lib.lib()
    B, C, K = 4, 300, 10
    z = torch.zeros(B, 4097, device=dev())
    a_idx = torch.zeros(B, 17, dtype=torch.int32, device=dev())
    a_val = torch.zeros(B, 17, device=dev())
    out, loss = torch.zeros(B, 4097, device=dev()), torch.zeros((), device=dev())
    labels = torch.zeros(B, dtype=torch.int64, device=dev())
    ws = torch.zeros(64, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    buf = (ctypes.c_ulonglong * 16)()

    def launches(fn, *args):
        h.vqa_launch_log_reset()
        rc = fn(*args, None)
        return rc, h.vqa_launch_log(buf, 16)
    for bad_c, bad_k, code in ((4097, K, -2), (C, 17, -1), (C, 0, -1)):
        tail = (p(ws), 256, B, bad_c, bad_k)
        assert launches(h.vqa_kld_sum_loss_sparse, p(z), p(a_idx), p(a_val), p(loss), p(out), *tail) == (code, 0)
        assert launches(h.vqa_bce_mean_loss_sparse, p(z), p(a_idx), p(a_val), p(loss), p(out), 0.5, *tail) == (code, 0)
        assert launches(h.vqa_ce_mean_loss_sampled, p(z), p(a_idx), p(a_val), p(labels), p(loss), p(out), 0.5, 1, None, 0,
                        *tail) == (code, 0)
        assert h.vqa_last_error()
    torch.cuda.synchronize()
    assert not out.any() and loss.item() == 0.0
    # and a call that passes its checks launches the row kernel and the total
    rc, n = launches(h.vqa_kld_sum_loss_sparse, p(z), p(a_idx), p(a_val), p(loss), p(out), p(ws), 256, B, C, K)
    assert (rc, n) == (0, 2) and int(buf[0]) == B * 256 and int(buf[1]) == 256
    torch.cuda.synchronize()
    for bad in ((z[:, :4097], a_idx[:, :K], a_val[:, :K]), (z[:, :C], a_idx, a_val)):                     # the wrappers: ValueError / the code
        with pytest.raises((ValueError, _lib.VqaLibraryError)):
            ops.kld_sum_loss_and_grad_sparse(bad[0].contiguous(), bad[1].contiguous(), bad[2].contiguous())


# ---- the train step ---------------------------------------------------------------------------------------------------------------
def _step_inputs(B, C, K, seed):
    from oracle import seeded
    v, q, _ = (torch.from_numpy(x) for x in seeded.seeded_inputs(B, answers=C, seed=seed))
    g = torch.Generator().manual_seed(seed)
    a_idx = torch.stack([torch.randperm(C, generator=g)[:K] for _ in range(B)]).to(torch.int32)
    a_val = torch.rand(B, K, generator=g) + 0.05
    a_idx[:, K - 3:][torch.rand(B, 3, generator=g) < 0.5] = -1                 # 7 .. 10 pairs a row
    a_val = torch.where(a_idx >= 0, a_val, torch.zeros_like(a_val))
    a_val = a_val / a_val.sum(1, keepdim=True)
    return v.to(dev()), q.to(dev()), a_idx.to(dev()), a_val.to(dev())


def _model(C):
    from oracle import seeded
    from vqa_playground_pytorch_amd import CoR2Model
    return seeded.load_state(CoR2Model(["PAD", "UNK"], C, seq2vec="vector"), 0).eval().to(dev())


def test_kld_step_from_a_sparse_target_replays_as_it_runs_eagerly():
    """CoR2 at B = 64, KLD from a sparse target, four steps (two launched kernel by kernel, then the capture, then replays): the
    bars tests/test_gpu_loss_optim_models.py holds dense replay to, no memset node, and the first step's loss is the dense step's."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    v, q, a_idx, a_val = _step_inputs(64, 300, 10, 21)
    out = {}
    for mode in (False, True):
        model = _model(300)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=mode, topk=(1, 5))
        steps = []
        for step in range(4):
            value, norm = tr.step({"v": v, "q_idxes": q}, {"a_idx": a_idx, "a_val": a_val})
            steps.append((value.item(), norm.item()))
            want = metrics.topk_hits(tr.last_logits.cpu(), ops.densify(a_idx, a_val, 300).cpu(), 5)
            assert tr.last_hits.cpu().tolist() == want.tolist() and tr.last_labels is None
        if mode:
            assert tr._graph is not None, "step was not captured"
            assert tr.graph_nodes and all("memset" not in c for c in tr.graph_nodes.values())
        out[mode] = (steps, [p.detach().clone() for p in model.parameters()], tr.lr)
    for (l0, n0), (l1, n1) in zip(out[False][0], out[True][0]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6)
    assert out[False][2] == out[True][2]
    for p0, p1 in zip(out[False][1], out[True][1]):
        assert (p0 - p1).abs().max().item() <= 2e-3 * max(p0.abs().max().item(), 1e-3)
    dense = DataParallelTrainer(_model(300), lr=2e-5, clip=0.25)
    value, norm = dense.step({"v": v, "q_idxes": q}, ops.densify(a_idx, a_val, 300))
    assert abs(value.item() - out[False][0][0][0]) <= BAR * abs(value.item())
    assert abs(norm.item() - out[False][0][0][1]) <= 1e-4 * abs(norm.item())


def test_sampled_ce_step_draws_fresh_labels_on_every_replay():
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    v, q, a_idx, a_val = _step_inputs(64, 300, 10, 22)
    dense = ops.densify(a_idx, a_val, 300)
    torch.manual_seed(5)
    tr = DataParallelTrainer(_model(300), lr=2e-5, clip=0.25, graph=True, loss="CE", topk=(1, 5))
    drawn = []
    for step in range(5):
        value, _ = tr.step({"v": v, "q_idxes": q}, {"a_idx": a_idx, "a_val": a_val})
        labels = tr.last_labels.clone()
        assert labels.dtype == torch.int64 and (dense.gather(1, labels[:, None]) > 0).all()      # valid, every step
        assert np.isfinite(value.item())
        pred = tr.last_logits.topk(5, 1, True, True).indices
        want = [100.0 * (pred[:, :k] == labels[:, None]).any(1).sum().item() / 64 for k in (1, 5)]
        assert list(tr.accuracy()) == want                                                       # against the DRAWN labels
        drawn.append(labels)
    assert tr._graph is not None, "step was not captured"
    assert all("memset" not in c for c in tr.graph_nodes.values())
    assert not torch.equal(drawn[3], drawn[4])                                                   # two replays of the same batch
    assert not torch.equal(drawn[0], drawn[1])                                                   # and two launched steps
