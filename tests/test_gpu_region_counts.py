"""Per-sample region counts on the GPU: the K3 `_len_` kernels (csrc/attention_pool_masked.hip) through the C ABI against float64,
and 'v_len' through CoR2Model, the trainer's captured step and the evaluator's replayed forward.

  A  kernels against float64: the reference is oracle/kernels_np.py's K3 applied per sample to the rows n < len_b, zeros filled in
     beyond; bar as tests/test_gpu_region_kernels.py reports it (Bars: four times the error of the same formulas in float32 on the
     CPU plus one ulp; 2^-8 |ref| on top for a bf16 d_v; an exactly-zero reference asks for exactly zero).  The padded rows of the
     INPUTS hold large finite values (sample 0's first padded logit +80): a kernel that reads one fails every bar.
  B  full length equals the unmasked entry points (forward bit for bit), the masked backward is reproducible bit for bit.
  C  refusals launch nothing.
  D  CoR2Model with v_len against the float64 restatement run per sample on the cut input; alpha exactly 0 on the padding.
  E  padding is invisible: a training step at a size that takes the fast paths gives the same bits whatever the padded rows hold.
  F  the trainer's captured graph and the evaluator's replayed forward read the counts of the batch they are given."""
import numpy as np
import pytest
import torch

from oracle import reference_faithful as RF
from oracle import seeded
from kernel_harness import (BF, E_BADARG, E_UNSUPPORTED, F32, PAD, _call, _ceil, _out, _ptr, _sentinel, _untouched, _win, dev,
                            ops)  # noqa: F401  (ops: the fixture)
from test_gpu_region_kernels import Bars, _dp64, _dt_id, _sfx, k3_mask

pytestmark = pytest.mark.gpu

BIG = 1.0e30            # what the padded rows of the inputs hold (finite in fp32 and in bf16)
K3L_FWD = "(attention_pool_len_fwd_kernel<T,NT,G>)"
K3L_ROWS, K3L_SOFTMAX = "(attention_pool_len_bwd_kernel<T,NT,G,false>)", "attention_softmax_len_bwd_kernel"
K3L_WHOLE = "(attention_pool_len_bwd_kernel<T,NT,G,true>)"
ROWS = 16               # region rows per workgroup of the two-launch backward's first kernel
WHOLE_MIN_B = "VQA_K3_LEN_WHOLE_MIN_B"      # the batch from which the backward is one launch, one workgroup per sample (default 256)


def _lens_of(N):
    return (1, N, _ceil(N, 2))


def len_inputs(B, N, D, G, dt, lens, seed):
    """CPU fp32: logits, v (dt-exact), d_pooled, d_first, d_alpha_ext -- the rows n >= len_b of logits, v and d_alpha_ext hold BIG
    (with either sign), sample 0's first padded logit +80"""
    gen = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(B, N, G, generator=gen)
    v = torch.randn(B, N, D, generator=gen).to(dt).float()
    d_pooled, d_first, d_ext = torch.randn(B, G, D, generator=gen), torch.randn(B, D, generator=gen), torch.randn(B, N, G, generator=gen)
    for b, L in enumerate(lens):
        sign = torch.where(torch.rand(N - L, 1, generator=gen) < 0.5, -1.0, 1.0)
        logits[b, L:], v[b, L:], d_ext[b, L:] = BIG * sign, (BIG * sign).to(dt).float(), BIG * sign
    if lens[0] < N:
        logits[0, lens[0]] = 80.0
    return logits, v, d_pooled, d_first, d_ext


def fwd_reference(logits, v, lens):
    """(alpha, pooled) in float64 (oracle/kernels_np.py per cut sample, zeros beyond) and in float32 (torch, the same formulas)"""
    import oracle.kernels_np as knp
    B, N, G = logits.shape
    a64, a32 = torch.zeros(B, N, G, dtype=torch.float64), torch.zeros(B, N, G)
    p64, p32 = torch.zeros(B, G, v.size(2), dtype=torch.float64), torch.zeros(B, G, v.size(2))
    for b, L in enumerate(lens):
        a, p = knp.softmax_attention_pool_fwd(logits[b:b + 1, :L].numpy(), v[b:b + 1, :L].numpy())
        a64[b, :L], p64[b] = torch.from_numpy(a[0]), torch.from_numpy(p[0])
        a32[b, :L] = torch.softmax(logits[b, :L], 0)
        p32[b] = torch.einsum("ng,nd->gd", a32[b, :L], v[b, :L])
    return a64, p64, a32, p32


def _lens_d(lens):
    return torch.tensor(lens, dtype=torch.int32, device=dev())


def run_len_fwd(ops, dt, logits_d, v_d, lens_d, B, N, D, G, want_first, p, seed):
    L = ops._lib.lib()
    b_a, b_p, b_f = _out(B * N * G), _out(B * G * D), _out(B * D) if want_first else None
    rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_len_fwd" + _sfx(dt)), _ptr(logits_d), _ptr(v_d), _ptr(lens_d),
                    _ptr(b_a, PAD), _ptr(b_p, PAD), _ptr(b_f, PAD) if want_first else None, p, seed, None, B, N, D, G)
    return rc, log, b_a, b_p, b_f


def len_fwd_case(ops, bars, dt, B, N, D, G, lens, want_first, p, seed):
    logits, v, _, _, _ = len_inputs(B, N, D, G, dt, lens, seed)
    mask = k3_mask(ops, B, G, D, p, seed)
    rc, log, b_a, b_p, b_f = run_len_fwd(ops, dt, logits.to(dev()), v.to(dt).to(dev()), _lens_d(lens), B, N, D, G, want_first, p, seed)
    what = "len fwd %s G=%d N=%d D=%d lens=%s first=%d p=%g" % (_dt_id(dt), G, N, D, lens, want_first, p)
    assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
    assert log == [(K3L_FWD, _ceil(D // 4, 256) * B * 256)], (what, log)
    a64, p64, a32, p32 = fwd_reference(logits, v, lens)
    alpha = _win(b_a, (B, N, G), what).cpu()
    for b, L in enumerate(lens):
        assert not bool(alpha[b, L:].any()), (what, "alpha is not exactly 0 on the padding of sample %d" % b)
    bars.check(what + " alpha", alpha, a64, a32)
    assert float((alpha.double().sum(1) - 1.0).abs().max()) <= (_ceil(N, 64) + 10) * 2.0 ** -23, what
    if want_first:
        bars.check(what + " first", _win(b_f, (B, D), what), p64[:, 0].contiguous(), p32[:, 0].contiguous())
    if mask is not None:
        p64, p32 = p64 * mask.double(), p32 * mask
    bars.check(what + " pooled", _win(b_p, (B, G, D), what), p64, p32)


def run_len_bwd(ops, dt, a_d, v_d, lens_d, dp_d, df_d, de_d, B, N, D, G, want_dv, p, seed):
    L = ops._lib.lib()
    b_l, b_v = _out(B * N * G), _out(B * N * D, dt) if want_dv else None
    rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_len_bwd" + _sfx(dt)), _ptr(a_d), _ptr(v_d), _ptr(lens_d), _ptr(dp_d),
                    _ptr(df_d), _ptr(de_d), _ptr(b_l, PAD), _ptr(b_v, PAD) if want_dv else None, p, seed, None, B, N, D, G)
    return rc, log, b_l, b_v


def len_bwd_case(ops, bars, dt, B, N, D, G, lens, ext, want_dv, first, p, seed, whole):
    """alpha is an input: the float32 rounding of the float64 masked softmax, zero on the padding (what the forward writes)"""
    import oracle.kernels_np as knp
    logits, v, d_pooled, d_first, d_ext = len_inputs(B, N, D, G, dt, lens, seed)
    alpha = fwd_reference(logits, v, lens)[0].float()
    mask = k3_mask(ops, B, G, D, p, seed)
    rc, log, b_l, b_v = run_len_bwd(ops, dt, alpha.to(dev()), v.to(dt).to(dev()), _lens_d(lens), d_pooled.to(dev()),
                                    d_first.to(dev()) if first else None, d_ext.to(dev()) if ext else None, B, N, D, G, want_dv, p, seed)
    what = "len bwd %s %s G=%d N=%d D=%d lens=%s ext=%d d_v=%d first=%d p=%g" % (
        "whole" if whole else "rows", _dt_id(dt), G, N, D, lens, ext, want_dv, first, p)
    assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
    assert log == ([(K3L_WHOLE, B * 256)] if whole else [(K3L_ROWS, _ceil(N, ROWS) * B * 256), (K3L_SOFTMAX, B * 256)]), (what, log)
    dp64 = _dp64(d_pooled, mask, d_first if first else None)
    dp32 = d_pooled if mask is None else d_pooled * mask
    if first:
        dp32 = dp32.clone()
        dp32[:, 0] += d_first
    dl64, dl32 = torch.zeros(B, N, G, dtype=torch.float64), torch.zeros(B, N, G)
    dv64, dv32 = torch.zeros(B, N, D, dtype=torch.float64), torch.zeros(B, N, D)
    for b, L in enumerate(lens):
        dl, dv = knp.softmax_attention_pool_bwd(alpha[b:b + 1, :L].numpy(), v[b:b + 1, :L].numpy(), dp64[b:b + 1],
                                                d_ext[b:b + 1, :L].numpy() if ext else None)
        dl64[b, :L], dv64[b, :L] = torch.from_numpy(dl[0]), torch.from_numpy(dv[0])
        dal = torch.einsum("gd,nd->ng", dp32[b], v[b, :L]) + (d_ext[b, :L] if ext else 0.0)
        dl32[b, :L] = alpha[b, :L] * (dal - (alpha[b, :L] * dal).sum(0, keepdim=True))
        dv32[b, :L] = torch.einsum("ng,gd->nd", alpha[b, :L], dp32[b])
    d_logits = _win(b_l, (B, N, G), what).cpu()
    d_v = _win(b_v, (B, N, D), what).cpu() if want_dv else None
    for b, L in enumerate(lens):
        assert not bool(d_logits[b, L:].any()), (what, "d_logits is not exactly 0 on the padding of sample %d" % b)
        assert d_v is None or not bool(d_v[b, L:].any()), (what, "d_v is not exactly 0 on the padding of sample %d" % b)
    bars.check(what + " d_logits", d_logits, dl64, dl32)
    if want_dv:
        bars.check(what + " d_v", d_v, dv64, dv32)


# N in {1, 37, 100, 257} x D in {8, 1028, 2048}: twelve consecutive entries hold every pair, four consecutive ones every N
SHAPES = [((1, 37, 100, 257)[i % 4], (8, 1028, 2048)[i % 3]) for i in range(12)]
CASES = [(dt, G) for dt in (F32, BF) for G in range(1, 9)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-G%d" % (_dt_id(c[0]), c[1]))
def test_len_forward_against_float64(ops, measured, case):
    """B = 3, lens = (1, N, ceil(N / 2)); every G; four shapes each with `first` and p in {0, 0.5, 0.25} in rotation; G = 8 also at
    N = 1024 with lens = (1, 1024, 3)"""
    dt, G = case
    runs = [(*SHAPES[(3 * G + i) % 12], None, bool((G + i) % 2), (0.0, 0.5, 0.25)[(G + i) % 3]) for i in range(4)]
    if G == 8:
        runs.append((1024, 1028, (1, 1024, 3), True, 0.5))
    for i, (N, D, lens, want_first, p) in enumerate(runs):
        bars = Bars(measured, "len fwd %s G%d N%d D%d f%d p%g" % (_dt_id(dt), G, N, D, want_first, p))
        len_fwd_case(ops, bars, dt, 3, N, D, G, lens or _lens_of(N), want_first, p, 37 * G + i)
        bars.close()


@pytest.mark.parametrize("whole", [False, True], ids=["rows", "whole"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-G%d" % (_dt_id(c[0]), c[1]))
def test_len_backward_against_float64(ops, lib_option, measured, case, whole):
    """both forms of the backward -- a chunk of 16 rows per workgroup + the softmax kernel (small batches), and one workgroup per
    sample in one launch (VQA_K3_LEN_WHOLE_MIN_B, here 1) -- over the eight combinations of d_alpha_ext x d_v x d_first over eight shapes, p in rotation; G = 8 also at N = 1024 (lens = (1, 1024,
    3)) and every G at D = 2052: one column block more than a pass of the row kernel holds"""
    dt, G = case
    lib_option(WHOLE_MIN_B, 1 if whole else 1 << 30)
    runs = [(*SHAPES[(5 * G + i) % 12], None, bool(i & 1), bool(i & 2), bool(i & 4), (0.0, 0.5, 0.25)[(G + i) % 3]) for i in range(8)]
    runs.append((37, 2052, None, True, True, True, 0.5))
    if G == 8:
        runs.append((1024, 1028, (1, 1024, 3), True, True, True, 0.5))
    for i, (N, D, lens, ext, want_dv, first, p) in enumerate(runs):
        bars = Bars(measured, "len bwd %s %s G%d N%d D%d e%d v%d f%d p%g" % ("whole" if whole else "rows", _dt_id(dt), G, N, D, ext, want_dv,
                                                                             first, p))
        len_bwd_case(ops, bars, dt, 3, N, D, G, lens or _lens_of(N), ext, want_dv, first, p, 1000 * G + i, whole)
        bars.close()


def test_backward_takes_one_launch_from_256_samples_on(ops):
    """the default threshold: B = 255 is the two-launch form, B = 256 the one-launch form (N = 2, D = 8: tiny)"""
    L = ops._lib.lib()
    for B, want in ((255, [(K3L_ROWS, 255 * 256), (K3L_SOFTMAX, 255 * 256)]), (256, [(K3L_WHOLE, 256 * 256)])):
        N, D, G = 2, 8, 4
        alpha, v, d_pooled = (torch.zeros(*shape, device=dev()) for shape in ((B, N, G), (B, N, D), (B, G, D)))
        lens = torch.ones(B, dtype=torch.int32, device=dev())
        out = torch.empty(B, N, G, device=dev())
        rc, log = _call(ops, L.vqa_softmax_attention_pool_len_bwd, _ptr(alpha), _ptr(v), _ptr(lens), _ptr(d_pooled), None, None,
                        _ptr(out), None, 0.0, 0, None, B, N, D, G)
        assert (rc, log) == (0, want), (B, rc, log)
        assert not bool(out.any())


# ================================================================================================================================ B
@pytest.mark.parametrize("dt,B,N,D,G", [(F32, 3, 37, 1028, 4), (F32, 64, 36, 2048, 4), (BF, 16, 100, 2048, 4), (F32, 3, 257, 8, 3)],
                         ids=["f32-small", "f32-B64", "bf16-N100", "f32-G3"])
@pytest.mark.parametrize("whole", [False, True], ids=["rows", "whole"])
def test_full_length_equals_the_unmasked_entry_points(ops, lib_option, measured, dt, B, N, D, G, whole):
    """(both forms of the masked backward)  lens[b] = N: alpha, pooled and first carry the bits of the `_drop` entry points; the backward of both agrees with float64
    within the bars (they sum in different orders), and two runs of the masked backward carry the same bits"""
    import oracle.kernels_np as knp
    L = ops._lib.lib()
    lib_option(WHOLE_MIN_B, 1 if whole else 1 << 30)
    lens, p, seed = (N,) * B, 0.5, 99
    logits, v, d_pooled, d_first, d_ext = len_inputs(B, N, D, G, dt, lens, 7 * B + N)
    logits_d, v_d, lens_d = logits.to(dev()), v.to(dt).to(dev()), _lens_d(lens)
    rc, _, b_a, b_p, b_f = run_len_fwd(ops, dt, logits_d, v_d, lens_d, B, N, D, G, True, p, seed)
    assert rc == 0, L.vqa_last_error()
    alpha, pooled, first = torch.empty(B, N, G, device=dev()), torch.empty(B, G, D, device=dev()), torch.empty(B, D, device=dev())
    rc, _ = _call(ops, getattr(L, "vqa_softmax_attention_pool_drop_fwd" + _sfx(dt)), _ptr(logits_d), _ptr(v_d), _ptr(alpha), _ptr(pooled),
                  _ptr(first), p, seed, None, B, N, D, G)
    assert rc == 0, L.vqa_last_error()
    assert torch.equal(_win(b_a, (B, N, G), "alpha"), alpha)
    assert torch.equal(_win(b_p, (B, G, D), "pooled"), pooled)
    assert torch.equal(_win(b_f, (B, D), "first"), first)
    dp_d, df_d, de_d = d_pooled.to(dev()), d_first.to(dev()), d_ext.to(dev())
    got = []
    for _ in range(2):
        rc, _, b_l, b_v = run_len_bwd(ops, dt, alpha, v_d, lens_d, dp_d, df_d, de_d, B, N, D, G, True, p, seed)
        assert rc == 0, L.vqa_last_error()
        got.append((_win(b_l, (B, N, G), "d_logits"), _win(b_v, (B, N, D), "d_v")))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1].float(), got[1][1].float())
    dl_u, dv_u = torch.empty(B, N, G, device=dev()), torch.empty(B, N, D, device=dev(), dtype=dt)
    rc, _ = _call(ops, getattr(L, "vqa_softmax_attention_pool_drop_bwd" + _sfx(dt)), _ptr(alpha), _ptr(v_d), _ptr(dp_d), _ptr(df_d),
                  _ptr(de_d), _ptr(dl_u), _ptr(dv_u), p, seed, None, B, N, D, G)
    assert rc == 0, L.vqa_last_error()
    mask = k3_mask(ops, B, G, D, p, seed)
    a_c = alpha.cpu()
    dl64, dv64 = (torch.from_numpy(x) for x in knp.softmax_attention_pool_bwd(a_c.numpy(), v.numpy(), _dp64(d_pooled, mask, d_first),
                                                                               d_ext.numpy()))
    dp32 = d_pooled * mask
    dp32[:, 0] += d_first
    dal32 = torch.einsum("bgd,bnd->bng", dp32, v) + d_ext
    dl32 = a_c * (dal32 - (a_c * dal32).sum(1, keepdim=True))
    dv32 = torch.einsum("bng,bgd->bnd", a_c, dp32)
    for name, (dl, dvv) in (("masked", got[0]), ("unmasked", (dl_u, dv_u))):
        bars = Bars(measured, "full length %s %s B%d N%d" % (name, _dt_id(dt), B, N))
        bars.check("d_logits", dl, dl64, dl32)
        bars.check("d_v", dvv, dv64, dv32)
        bars.close()


# ================================================================================================================================ C
def test_refusals_launch_nothing(ops):
    """the documented codes, an empty launch log and untouched outputs for: lens == NULL, G = 9, N = 1025, D = 6, a misaligned v and
    p = 1.  (Counts outside 1..N are the host's to refuse -- tests/test_region_counts.py -- and are not run here.)"""
    L = ops._lib.lib()
    for dt in (F32, BF):
        B, N, D, G = 2, 5, 8, 2
        x = torch.zeros(4096, device=dev())
        v = torch.zeros(4096, device=dev(), dtype=dt)
        lens = _lens_d((5, 2))
        cases = [("lens == NULL", E_BADARG, dict(lens=None)), ("G = 9", E_UNSUPPORTED, dict(G=9)), ("N = 1025", E_UNSUPPORTED, dict(N=1025)),
                 ("D = 6", E_UNSUPPORTED, dict(D=6)), ("misaligned v", E_UNSUPPORTED, dict(v_off=1)), ("p = 1", E_BADARG, dict(p=1.0))]
        for name, code, kw in cases:
            n, d, g, p = kw.get("N", N), kw.get("D", D), kw.get("G", G), kw.get("p", 0.0)
            lens_p = _ptr(lens) if "lens" not in kw else None
            outs = [_sentinel(64), _sentinel(64), _sentinel(64), _sentinel(64, dtype=dt)]
            rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_len_fwd" + _sfx(dt)), _ptr(x), _ptr(v, kw.get("v_off", 0)), lens_p,
                            _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), p, 1, None, B, n, d, g)
            assert (rc, log) == (code, []), ("fwd", name, _dt_id(dt), rc, log)
            rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_len_bwd" + _sfx(dt)), _ptr(x), _ptr(v, kw.get("v_off", 0)), lens_p,
                            _ptr(x), _ptr(x), _ptr(x), _ptr(outs[0]), _ptr(outs[3]), p, 1, None, B, n, d, g)
            assert (rc, log) == (code, []), ("bwd", name, _dt_id(dt), rc, log)
            assert all(_untouched(o) for o in outs), (name, _dt_id(dt))


# ================================================================================================================================ D
RTOL, ATOL = 1e-3, 1e-7                  # tests/test_gpu_models.py's bars
V_LEN = [36, 20, 2, 7]


def _rel(got, want):
    got, want = got.detach().cpu().numpy().astype(np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-20)


def _padded_inputs(B, v_len, N=36, nans=2000, seed=1, fill="noise"):
    """seeded inputs whose rows n >= v_len[b] are overwritten: N(0, 10^2) noise, or zeros"""
    v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=seed)
    noise = seeded.seeded_array(v.shape, 4242, scale=10.0)
    for b, L in enumerate(v_len):
        v[b, L:] = noise[b, L:] if fill == "noise" else 0.0
    return v, q, a


@pytest.fixture(scope="module")
def cut_reference():
    """CoR2Oracle in float64, eval mode, every sample on its own cut to [1, len_b, 2048]: computed once, shared, never changed"""
    ref = seeded.load_state(RF.CoR2Oracle(2000), 0).eval().double()
    v, q, a = _padded_inputs(4, V_LEN)
    out = {"logits": [], "dq": [], "alpha1": [], "alpha2": [], "loss": 0.0}
    for b, L in enumerate(V_LEN):
        qb = torch.from_numpy(q[b:b + 1]).double().requires_grad_()
        lo = ref({"v": torch.from_numpy(v[b:b + 1, :L]).double(), "q": qb})
        loss = RF.kld_sum_loss(lo, torch.from_numpy(a[b:b + 1]).double())
        loss.backward()                                                    # parameter gradients add up over the four samples
        out["loss"] += float(loss)
        out["logits"].append(lo.detach().numpy())
        out["dq"].append(qb.grad.numpy())
        for k in ("alpha1", "alpha2"):
            out[k].append(torch.cat(ref.alpha_dict[k], 2).detach().numpy()[0])        # [len_b, 4]
    out["logits"], out["dq"] = np.concatenate(out["logits"]), np.concatenate(out["dq"])
    out["grads"] = {n: p.grad.numpy().copy() for n, p in ref.named_parameters()}
    return out


def _check_alphas(model, want, v_len, rtol, what):
    for k in ("alpha1", "alpha2"):
        got = torch.cat(model.alpha_dict[k], 2)
        assert got.shape == (len(v_len), 36, 4)
        for b, L in enumerate(v_len):
            assert not bool(got[b, L:].any()), (what, k, "not exactly 0 on the padding of sample %d" % b)
            assert _rel(got[b, :L], want[k][b]) <= rtol, (what, k, b)


@pytest.mark.parametrize("head_form", ["grouped", "legacy"])
@pytest.mark.parametrize("mode", [1, 0])
def test_cor2_with_counts_matches_the_reference_per_cut_sample(cut_reference, mode, head_form, monkeypatch, measured):
    from vqa_playground_pytorch_amd import CoR2Model, head
    monkeypatch.setattr(head, "MODE", head_form)
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], 2000, relation_mode=mode), 0).eval().to(dev())
    v, q, a = _padded_inputs(4, V_LEN)
    qt = torch.from_numpy(q).to(dev()).requires_grad_()
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": qt, "v_len": torch.tensor(V_LEN)})      # (host int64 counts)
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    want = cut_reference
    worst = max((float(np.abs(p.grad.detach().cpu().numpy().astype(np.float64) - want["grads"][n]).max()
                       / (RTOL * np.abs(want["grads"][n]).max() + ATOL)), n) for n, p in model.named_parameters())
    measured("logits", _rel(logits, want["logits"]), RTOL)
    measured("worst gradient / bar", worst[0], 1.0, worst[1])
    assert _rel(logits, want["logits"]) <= RTOL
    assert abs(loss.item() - want["loss"]) <= RTOL * abs(want["loss"])
    assert _rel(qt.grad, want["dq"]) <= RTOL
    _check_alphas(model, want, V_LEN, RTOL, "mode %d %s" % (mode, head_form))
    assert model.alpha_dict["feature"].shape == (4, 2, 2048)
    assert worst[0] <= 1.0, worst


def test_cor2_bf16_with_counts_matches_the_bf16_aware_oracle_per_cut_sample(measured):
    """compute_dtype = bfloat16 against oracle/mixed_precision.py's restatement (it takes a [1, n, 2048] sample) run per cut sample,
    at tests/test_gpu_bf16.py's bars for that restatement"""
    from oracle import mixed_precision as MP
    from test_gpu_bf16 import RTOL_AWARE, RTOL_AWARE_ALL, RTOL_AWARE_MAX, _gradient_error, close_f32, npy
    from vqa_playground_pytorch_amd import CoR2Model
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], 2000, compute_dtype=torch.bfloat16), 0).eval().to(dev())
    aware = seeded.load_state(MP.CoR2MixedOracle(2000), 0).eval().double()
    v, q, a = _padded_inputs(4, V_LEN)
    got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev()),
                 "v_len": torch.tensor(V_LEN, dtype=torch.int32, device=dev())})                             # (device int32 counts)
    RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    want, alpha2 = [], []
    for b, L in enumerate(V_LEN):
        w = aware({"v": torch.from_numpy(v[b:b + 1, :L]).double(), "q": torch.from_numpy(q[b:b + 1]).double()})
        RF.kld_sum_loss(w, torch.from_numpy(a[b:b + 1]).double()).backward()
        want.append(w.detach())
        alpha2.append(torch.cat(aware.alpha_dict["alpha2"], 2).detach().numpy()[0])
    close_f32("logits", got, torch.cat(want).numpy(), RTOL_AWARE)
    got_a2 = torch.cat(model.alpha_dict["alpha2"], 2)
    for b, L in enumerate(V_LEN):
        assert not bool(got_a2[b, L:].any())
        close_f32("alpha2[%d]" % b, got_a2[b, :L], alpha2[b], RTOL_AWARE)
    params = dict(model.named_parameters())
    zero_grads = {"%s.list_linear1.%d.linear.bias" % (f, r) for f in ("fusion_vq1", "fusion_vq2") for r in range(2)} | \
        {"att1.conv_att.conv.bias", "att2.conv_att.conv.bias"}
    worst = (0.0, 0.0, 0.0, "")
    for (n, p), (_, po) in zip(model.named_parameters(), aware.named_parameters()):
        ref, g = po.grad.numpy().astype(np.float64), npy(p.grad)
        assert np.isfinite(g).all(), n
        if n in zero_grads:     # mathematically zero (a constant shift in front of a softmax): rounding noise on either side
            w_scale = np.abs(npy(params[n.replace(".bias", ".weight")].grad)).max()
            assert np.abs(g).max() <= 5e-2 * w_scale and np.abs(ref).max() <= 5e-2 * w_scale, n
            continue
        worst = max(worst, (*_gradient_error(g, ref), n))
        e_max, e_fro, e_all = _gradient_error(g, ref)
        print("  %-45s max-abs %.2e  Frobenius %.2e  whole %.2e" % (n, e_max, e_fro, e_all))
    measured("worst gradient max-abs", worst[0], RTOL_AWARE_MAX, worst[3])
    for (n, p), (_, po) in zip(model.named_parameters(), aware.named_parameters()):
        if n not in zero_grads:
            e_max, e_fro, e_all = _gradient_error(npy(p.grad), po.grad.numpy().astype(np.float64))
            assert e_max <= RTOL_AWARE_MAX and e_fro <= RTOL_AWARE and e_all <= RTOL_AWARE_ALL, (n, e_max, e_fro, e_all)


# ================================================================================================================================ E
def _train_step(model, v, q, a, v_len):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)                    # (the fused masks' seeds are drawn from torch's CPU generator)
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev()), "v_len": v_len})
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    return logits.detach().clone(), loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("dt,B,N", [(torch.float32, 64, 36), (torch.bfloat16, 16, 100)], ids=["f32-B64-N36", "bf16-B16-N100"])
def test_padding_is_invisible_to_a_training_step(dt, B, N):
    """train mode, the same dropout seeds twice: padded rows of zeros, then of N(0, 10^2) noise.  The padded rows only ever meet exact
    zeros (alpha, d_logits and with it every gradient row upstream), so logits, loss and EVERY parameter gradient are torch.equal;
    any difference is a leak.  fp32 at B = 64 reaches the fused relation / projection node, the grouped head and the unmasked
    kernels' fused-backward batch size."""
    from vqa_playground_pytorch_amd import CoR2Model
    nans = 300
    rs = np.random.RandomState(11)
    v_len = rs.randint(1, N + 1, size=B)
    v_len[3], v_len[B - 2] = 1, N
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans, compute_dtype=dt), 0).train().to(dev())
    lens_d = torch.from_numpy(v_len.astype(np.int32)).to(dev())
    runs = [_train_step(model, *_padded_inputs(B, v_len, N=N, nans=nans, seed=31, fill=fill), lens_d) for fill in ("zeros", "noise")]
    assert torch.equal(runs[0][0], runs[1][0]), "logits"
    assert torch.equal(runs[0][1], runs[1][1]), "loss"
    differ = [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
    assert not differ, differ
    assert all(bool(torch.isfinite(g).all()) for g in runs[1][2].values())


# ================================================================================================================================ F
def test_captured_step_reads_the_counts_of_every_batch():
    """DataParallelTrainer, graph path, B = 8 (eval mode: no dropout, both sides deterministic): the steps after the capture take
    three different v_len vectors through the same graph; losses and parameters follow the eager trainer fed the same batches
    (the bars of test_graph_replay_equals_eager_steps).  A last step with all counts 36 gives the loss of a step without the key,
    torch.equal, replayed or not."""
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    B, nans = 8, 300
    rs = np.random.RandomState(5)
    warm = DataParallelTrainer.EAGER_STEPS_BEFORE_CAPTURE
    lens = [rs.randint(1, 37, size=B) for _ in range(warm + 3)]
    out = {}
    for graph in (False, True):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans), 0).eval().to(dev())
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=graph)
        losses = []
        for step, v_len in enumerate(lens):
            v, q, a = (torch.from_numpy(x).to(dev()) for x in _padded_inputs(B, v_len, nans=nans, seed=40 + step))
            counts = torch.from_numpy(v_len) if step % 2 else torch.from_numpy(v_len.astype(np.int32)).to(dev())    # host int64 / device int32
            loss, norm = tr.step({"v": v, "q_idxes": q, "v_len": counts}, a)
            losses.append((loss.item(), norm.item()))
        if graph:
            assert tr._graph is not None and "v_len" in tr._graph["sample"], "the step was not captured with its counts"
        params = [p.detach().clone() for p in model.parameters()]
        # one more step with every count 36, against a step without the key from the same parameters (an eager trainer of its own:
        # the loss is computed before anything is updated, and at full length the masked forward carries the unmasked one's bits)
        v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(B, answers=nans, seed=77))
        full = tr.step({"v": v, "q_idxes": q, "v_len": torch.full((B,), 36, dtype=torch.int32)}, a)[0].detach().clone()
        plain_model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans), 0).eval().to(dev())
        plain_tr = DataParallelTrainer(plain_model, lr=2e-5, clip=0.25, graph=False)
        with torch.no_grad():
            for p, s_ in zip(plain_model.parameters(), params):
                p.copy_(s_)
        plain = plain_tr.step({"v": v, "q_idxes": q}, a)[0].detach().clone()
        assert torch.equal(full, plain), (graph, full, plain)
        out[graph] = (losses, params)
    for (l0, n0), (l1, n1) in zip(out[False][0], out[True][0]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6), (out[False][0], out[True][0])
    for p0, p1 in zip(out[False][1], out[True][1]):
        assert (p0 - p1).abs().max().item() <= 2e-3 * max(p0.abs().max().item(), 1e-3)


def test_full_counts_step_equals_a_step_without_the_key():
    """v_len all 36 against no v_len: the loss of an eager trainer step is torch.equal (the masked forward carries the unmasked one's
    bits at full length, and the loss is computed before anything is updated)"""
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    B, nans = 8, 300
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(B, answers=nans, seed=77))
    got = []
    for counts in (None, torch.full((B,), 36, dtype=torch.int64)):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans), 0).eval().to(dev())
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=False)
        sample = {"v": v, "q_idxes": q} if counts is None else {"v": v, "q_idxes": q, "v_len": counts}
        got.append(tr.step(sample, a)[0].detach().clone())
    assert torch.equal(got[0], got[1]), got


def test_evaluator_replays_the_forward_with_the_counts_of_each_batch():
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    B, nans = 8, 300
    rs = np.random.RandomState(9)
    batches = []
    for i in range(Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 2):
        v_len = rs.randint(1, 37, size=B)
        v, q, a = _padded_inputs(B, v_len, nans=nans, seed=60 + i)
        batches.append({"v": torch.from_numpy(v), "q_idxes": torch.from_numpy(q), "a": torch.from_numpy(a), "v_len": torch.from_numpy(v_len)})
    out = {}
    for graph in (False, True):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans), 0).to(dev())
        ev = Evaluator(model, graph=graph)
        out[graph] = [{k: t.clone() for k, t in ev.step(b).items() if t is not None} for b in batches]
        if graph:
            assert ev._graph is not None and "v_len" in ev._graph["inputs"], "the forward was not captured with its counts"
    for plain, replayed in zip(out[False], out[True]):
        assert torch.equal(plain["pred"], replayed["pred"]) and torch.equal(plain["top_idx"], replayed["top_idx"])
        assert torch.equal(plain["hits"], replayed["hits"])
    with pytest.raises(ValueError):
        Evaluator(model, graph=False).step(dict(batches[0], v_len=torch.zeros(B, dtype=torch.int64)))
