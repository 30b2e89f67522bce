"""Every launch form of the pairwise-relation kernels (csrc/pairwise_relation.hip: K1 and relation_apply) and of the attention-pool
kernels (csrc/attention_pool.hip: K3), through the C ABI, one dispatch form at a time.  tests/test_gpu_kernels.py and
tests/test_gpu_bf16.py reach these files at small shapes only; here every VQA_LAUNCH site of the two files is launched, the launch
log (kernel expression and grid in work-items) says that it was, and its result is compared whole.

  A  K1 and relation_apply with small-integer operands (|v|, |g|, |q|, |alpha|, |t|, |c2| <= 4; alpha NOT normalised, with zeros; p_drop
     0 or 0.5, keep factor exactly 2): every fp32 sum is an integer below 2^24, exact in any order.  The reference is int64 on the
     CPU (mode 0 by the closed form q1 sum_i a_i v_i + (sum a) q2 v_j, exact over integers); fp32 outputs equal it bit for bit (-0 is
     0), bf16 outputs equal ref.float().to(bfloat16) bit for bit.  Outputs sit in sentinel-filled buffers that are compared whole;
     alpha is read as glimpse 1 of a [B,N,3] tensor (alpha_stride = 3); D leaves the last column block partial.
  B  K3 with random operands against float64 (oracle/kernels_np.py), under the project's bar (Bars of
     tests/kernel_harness.py, reported here as one row per case): four times the error of the same formula in float32 with torch
     on the CPU plus one float32 ulp of the tensor's largest magnitude; a bf16 d_v gets 2^-8 |ref| on top.  Every case reports
     what it measured.
  C  non-finite isolation and refusals of K3.
  D  test_every_launch_site_is_declared (no GPU): every VQA_LAUNCH first argument of the two files is the form of some case below.

Dispatch form (as the launch log spells it) -> the test that launches it and asserts that it did:

  pairwise_fwd_reg_kernel<T>                       test_k1_forward_small_integers_are_exact [reg-*]
  (pairwise_fwd_stream_kernel<T,NT>)               test_k1_forward_small_integers_are_exact [stream-*] (N = 37, 300, 4096)
  pairwise_fwd_pairs_reg_kernel<T>                 ... [pairs-*]: small batch, bf16 at the large batch, B = 255 (one sample under
                                                   the reg2 threshold), VQA_K1_PAIRWISE_REG4
  pairwise_fwd_pairs_reg2_kernel                   ... [pairs2-*] (B D = 2^19), test_k1_forward_with_dropout_in_the_store (the
                                                   launch site of vqa_pairwise_relation_reduce_drop_fwd)
  (pairwise_fwd_kernel<T,128>)                     ... [lds128-*] (VQA_K1_PAIRWISE_LDS)
  (pairwise_fwd_kernel<T,64>)                      ... [lds64-*] (N = 37, and N = 144: 148 032 bytes of LDS)
  (pairwise_bwd_stream_kernel<T,NT,true|false,RS>) test_k1_backward_small_integers_are_exact [small-*]
  (pairwise_bwd_stream_kernel<T,NT,true|false,1>)  test_k1_backward_small_integers_are_exact [large-*],
                                                   test_k1_backward_threshold (B = 512 against B = 511)
  (relation_apply_fwd_kernel<T,NT>)                test_relation_apply_forward_small_integers_are_exact (zsplit 1 and ceil(N / 4))
  (relation_apply_bwd_kernel<T,NT,RS>), <T,NT,1>   test_relation_apply_backward_small_integers_are_exact, .._threshold
  relation_apply_bwd8_bf16_kernel<RS>              test_relation_apply_backward_small_integers_are_exact [bwd8-*]
  (attention_pool_fwd_kernel<T,NT,G>)              test_k3_forward_against_float64 (G = 1..8, N up to 1024)
  (attention_pool_bwd_fused_kernel<T,NT,G,2>)      test_k3_backward_fused_against_float64, test_k3_backward_lds_limits [fused-77KB]
  (attention_pool_bwd_stream_kernel<T,NT,G,RS>)    test_k3_backward_three_launches_against_float64 [rs4-*], .._fused_window_edges,
                                                   test_k3_backward_lds_limits (N G = 8192)
  (attention_pool_bwd_stream_kernel<T,NT,G,1>)     test_k3_backward_three_launches_against_float64 [rs1-*]
  attention_softmax_bwd_kernel                     with either stream form"""
import ctypes
import functools
import os

import pytest
import torch

import kernel_harness
from kernel_harness import (BF, EPS32, E_BADARG, E_UNSUPPORTED, F32, INF, NAN, PAD, _amax, _below_2_24, _call, _ceil, _d, _out, _ptr,
                            _same_bits, _sentinel, _untouched, _win, assert_exact, dev, launch_sites, ops)  # noqa: F401  (ops: the fixture)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AG, GL = 3, 1           # alpha is glimpse GL of a [B,N,AG] tensor: alpha_stride = AG
_dt_id = lambda dt: "bf16" if dt == BF else "f32"      # noqa: E731

# ---- the launch log's spelling of every dispatch form (blanks removed) -------------------------------------------------------
ZERO = "zero_fill_kernel"
K1_REG, K1_STREAM = "pairwise_fwd_reg_kernel<T>", "(pairwise_fwd_stream_kernel<T,NT>)"
K1_PAIRS, K1_PAIRS2 = "pairwise_fwd_pairs_reg_kernel<T>", "pairwise_fwd_pairs_reg2_kernel"
K1_LDS128, K1_LDS64 = "(pairwise_fwd_kernel<T,128>)", "(pairwise_fwd_kernel<T,64>)"
K1_BWD = {(dual, rs): "(pairwise_bwd_stream_kernel<T,NT,%s,%s>)" % ("true" if dual else "false", rs)
          for dual in (False, True) for rs in ("RS", "1")}
RA_FWD, RA_BWD4, RA_BWD1 = "(relation_apply_fwd_kernel<T,NT>)", "(relation_apply_bwd_kernel<T,NT,RS>)", "(relation_apply_bwd_kernel<T,NT,1>)"
RA_BWD8 = "relation_apply_bwd8_bf16_kernel<RS>"
K3_FWD, K3_FUSED = "(attention_pool_fwd_kernel<T,NT,G>)", "(attention_pool_bwd_fused_kernel<T,NT,G,2>)"
K3_STREAM4, K3_STREAM1 = "(attention_pool_bwd_stream_kernel<T,NT,G,RS>)", "(attention_pool_bwd_stream_kernel<T,NT,G,1>)"
K3_SOFTMAX = "attention_softmax_bwd_kernel"


def _sfx(dt):
    return "_bf16" if dt == BF else ""


def _ints(gen, *shape, amp=4):
    return torch.randint(-amp, amp + 1, shape, generator=gen)


# ======================================================================================================================= A: K1 forward
@functools.lru_cache(maxsize=2)
def k1_operands(B, N, D, amp=4):
    """int64 on the CPU: v [B,N,D] within +-amp; q1, q2 [B,D] and alpha [B,N,AG] within +-4, alpha with zeros"""
    gen = torch.Generator().manual_seed(1000003 * B + 1009 * N + D)
    v, q1, q2, alpha = _ints(gen, B, N, D, amp=amp), _ints(gen, B, D), _ints(gen, B, D), _ints(gen, B, N, AG)
    alpha[:, ::3, GL] = 0
    if N > 1:
        alpha[:, 1, GL] = 3         # (not all zero)
    return v, q1, q2, alpha


def k1_gradients(B, N, D, amp=4):
    """int64 on the CPU: the two gradients of v2, [B,N,D] within +-amp"""
    gen = torch.Generator().manual_seed(3000017 * B + 1019 * N + D)
    return _ints(gen, B, N, D, amp=amp), _ints(gen, B, N, D, amp=amp)


def k1_fwd_reference(v, q1, q2, alpha):
    """int64 closed form of both modes: v2_j = q1 sum_i a_i v_i + (sum_i a_i) q2 v_j"""
    a = alpha[:, :, GL]
    N = v.shape[1]
    # mode 0 adds N terms a_i (v_i q1 + v_j q2), each at most 2 * 4 * amax(v) * 4 in magnitude
    _below_2_24(N * 2 * _amax(a) * _amax(v) * max(_amax(q1), _amax(q2)))
    s = (a[:, :, None] * v).sum(1)
    return (q1 * s)[:, None, :] + (a.sum(1)[:, None] * q2)[:, None, :] * v


def run_k1_fwd(ops, dt, dv, B, N, D, mode):
    """dv: the operands on the GPU (v in dt) -> (rc, log, output buffer)"""
    v, q1, q2, alpha = dv
    buf = _out(B * N * D, dt)
    fn = getattr(ops._lib.lib(), "vqa_pairwise_relation_reduce_fwd" + _sfx(dt))
    rc, log = _call(ops, fn, _ptr(v), _ptr(q1), _ptr(q2), _ptr(alpha, GL), AG, _ptr(buf, PAD), B, N, D, mode)
    return rc, log, buf


# (id, kernel, threads per workgroup, elements per lane, dtypes, mode, B, N, D, knob)
K1_FWD_CASES = [
    ("reg-N1", K1_REG, 64, 4, (F32, BF), 1, 3, 1, 260, None),
    ("reg-N36", K1_REG, 64, 4, (F32, BF), 1, 3, 36, 260, None),
    ("stream-N37", K1_STREAM, 256, 4, (F32, BF), 1, 3, 37, 1028, None),
    ("stream-N300", K1_STREAM, 256, 4, (F32, BF), 1, 3, 300, 1028, None),
    ("stream-N4096", K1_STREAM, 256, 4, (F32, BF), 1, 1, 4096, 8, None),
    ("pairs-N1", K1_PAIRS, 64, 4, (F32, BF), 0, 3, 1, 260, None),
    ("pairs-N7", K1_PAIRS, 64, 4, (F32, BF), 0, 3, 7, 260, None),
    ("pairs-N36", K1_PAIRS, 64, 4, (F32, BF), 0, 3, 36, 260, None),
    ("pairs-reg4-B256", K1_PAIRS, 64, 4, (F32,), 0, 256, 5, 2048, "VQA_K1_PAIRWISE_REG4"),
    ("pairs-bf16-B256", K1_PAIRS, 64, 4, (BF,), 0, 256, 5, 2048, None),           # bf16 never takes reg2
    ("pairs-B255", K1_PAIRS, 64, 4, (F32,), 0, 255, 5, 2048, None),               # B D = 2^19 - 2048
    ("pairs2-N1", K1_PAIRS2, 64, 2, (F32,), 0, 256, 1, 2048, None),
    ("pairs2-N5", K1_PAIRS2, 64, 2, (F32,), 0, 256, 5, 2048, None),
    ("pairs2-N36", K1_PAIRS2, 64, 2, (F32,), 0, 256, 36, 2048, None),
    ("lds128-N5", K1_LDS128, 128, 4, (F32, BF), 0, 2, 5, 516, "VQA_K1_PAIRWISE_LDS"),
    ("lds128-N36", K1_LDS128, 128, 4, (F32, BF), 0, 2, 36, 516, "VQA_K1_PAIRWISE_LDS"),
    ("lds64-N37", K1_LDS64, 64, 4, (F32, BF), 0, 2, 37, 260, None),
    ("lds64-N144", K1_LDS64, 64, 4, (F32, BF), 0, 2, 144, 260, None),
]


@gpu
@pytest.mark.parametrize("case", K1_FWD_CASES, ids=lambda c: c[0])
def test_k1_forward_small_integers_are_exact(ops, lib_option, case):
    name, kernel, nt, per_lane, dtypes, mode, B, N, D, knob = case
    if knob:
        lib_option(knob, 1)
    v, q1, q2, alpha = k1_operands(B, N, D)
    ref = k1_fwd_reference(v, q1, q2, alpha)
    for dt in dtypes:
        dv = (_d(v, dt), _d(q1, F32), _d(q2, F32), _d(alpha, F32))
        rc, log, buf = run_k1_fwd(ops, dt, dv, B, N, D, mode)
        assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
        assert log == [(kernel, _ceil(D // per_lane, nt) * B * nt)], (name, _dt_id(dt), log)
        assert_exact("%s %s" % (name, _dt_id(dt)), _win(buf, (B, N, D), name), ref)


@gpu
@pytest.mark.parametrize("p", [0.0, 0.5])
def test_k1_forward_with_dropout_in_the_store(ops, p):
    """vqa_pairwise_relation_reduce_drop_fwd: the reg2 kernel with the consumer's dropout (the mask vqa_linear_dropout_mask exports
    for [B N, D]) in its store"""
    B, N, D, seed = 256, 5, 2048, 4242
    L = ops._lib.lib()
    assert L.vqa_pairwise_relation_reduce_drop_supported(B, N, D) == 1 and L.vqa_pairwise_relation_reduce_drop_supported(B - 1, N, D) == 0
    v, q1, q2, alpha = k1_operands(B, N, D)
    ref = k1_fwd_reference(v, q1, q2, alpha)
    if p:
        mask = ops.linear_dropout_mask(B * N, D, p, seed, dev()).cpu()
        assert set(torch.unique(mask).tolist()) == {0.0, 2.0}
        ref = ref * mask.view(B, N, D).long()
    buf = _out(B * N * D)
    v_d, q1_d, q2_d, alpha_d = _d(v, F32), _d(q1, F32), _d(q2, F32), _d(alpha, F32)
    rc, log = _call(ops, L.vqa_pairwise_relation_reduce_drop_fwd, _ptr(v_d), _ptr(q1_d), _ptr(q2_d), _ptr(alpha_d, GL), AG, _ptr(buf, PAD),
                    p, seed, None, B, N, D)
    assert rc == 0 and log == [(K1_PAIRS2, _ceil(D // 2, 64) * B * 64)], (rc, log)
    assert_exact("reg2 dropout p=%g" % p, _win(buf, (B, N, D), "reg2 dropout"), ref)


@gpu
@pytest.mark.parametrize("dt", [F32, BF], ids=_dt_id)
def test_k1_forward_refuses_past_its_limits(ops, dt):
    """mode 0: N = 145 is one row more than the LDS tile holds; mode 1: N = 4097.  VQA_E_UNSUPPORTED, no launch, v2 untouched"""
    for mode, B, N, D, word in ((0, 2, 145, 260, b"144"), (1, 1, 4097, 8, b"4096")):
        v, q1, q2, alpha = k1_operands(B, N, D)
        rc, log, buf = run_k1_fwd(ops, dt, (_d(v, dt), _d(q1, F32), _d(q2, F32), _d(alpha, F32)), B, N, D, mode)
        assert rc == E_UNSUPPORTED and log == [] and word in ops._lib.lib().vqa_last_error(), (mode, rc, log)
        assert _untouched(buf)


# ======================================================================================================================= A: K1 backward
def k1_bwd_reference(v, q1, q2, alpha, g, D):
    """int64: (d_alpha [B,N], d_q1, d_q2 [B,D], d_v [B,N,D]); g already holds the sum of the two gradients of a dual call"""
    a = alpha[:, :, GL]
    N = v.shape[1]
    gs, gvs = N * _amax(g), N * _amax(g) * _amax(v)                   # bounds of sum_j g_j and sum_j g_j v_j
    _below_2_24(D * (_amax(v) * _amax(q1) * gs + gvs * _amax(q2)),    # every partial sum of d_alpha
                N * _amax(a) * _amax(v) * gs, N * _amax(a) * gvs)     # d_q1, d_q2
    gsum, gv = g.sum(1), (g * v).sum(1)
    pooled, asum = (a[:, :, None] * v).sum(1), a.sum(1)
    u = q1 * gsum
    d_alpha = (v * u[:, None, :]).sum(2) + (gv * q2).sum(1)[:, None]
    d_v = a[:, :, None] * u[:, None, :] + (asum[:, None] * q2)[:, None, :] * g
    return d_alpha, pooled * gsum, asum[:, None] * gv, d_v


def run_k1_bwd(ops, dt, dv, B, N, D, dual, want_dv):
    """-> (log, d_alpha, d_q1, d_q2, d_v or None), every output taken whole out of its sentinel-filled buffer"""
    v, q1, q2, alpha, g, g_b = dv
    b_da, b_q1, b_q2 = _out(B * N), _out(B * D), _out(B * D)
    b_dv = _out(B * N * D, dt) if want_dv else None
    fn = getattr(ops._lib.lib(), "vqa_pairwise_relation_reduce_bwd" + _sfx(dt))
    rc, log = _call(ops, fn, _ptr(v), _ptr(q1), _ptr(q2), _ptr(alpha, GL), AG, _ptr(g), _ptr(g_b) if dual else None, _ptr(b_da, PAD),
                    _ptr(b_q1, PAD), _ptr(b_q2, PAD), _ptr(b_dv, PAD) if want_dv else None, B, N, D)
    assert rc == 0, (rc, ops._lib.lib().vqa_last_error())
    return (log, _win(b_da, (B, N), "d_alpha"), _win(b_q1, (B, D), "d_q1"), _win(b_q2, (B, D), "d_q2"),
            _win(b_dv, (B, N, D), "d_v") if want_dv else None)


def k1_bwd_log(B, N, D, dual):
    """the launches pairwise_bwd_impl makes: the row-split form below B D = 2^20"""
    if B * D // 4 < 4 * 65536:
        return [(ZERO, _ceil(B * N, 256) * 256), (K1_BWD[dual, "RS"], _ceil(D // 4, 64) * B * 256)]
    return [(ZERO, _ceil(B * N, 256) * 256), (K1_BWD[dual, "1"], _ceil(D // 4, 256) * B * 256)]


def check_k1_bwd(ops, name, host, B, N, D, form):
    """every (dual, d_v, T) of one shape; host: the int64 operands (the first B samples are used)"""
    v, q1, q2, alpha, g, g_b = (t[:B] for t in host)
    refs = {dual: k1_bwd_reference(v, q1, q2, alpha, g + g_b if dual else g, D) for dual in (False, True)}
    for dt in (F32, BF):
        dv = (_d(v, dt), _d(q1, F32), _d(q2, F32), _d(alpha, F32), _d(g, dt), _d(g_b, dt))
        for dual in (False, True):
            for want_dv in (False, True):
                what = "%s %s dual=%d d_v=%d" % (name, _dt_id(dt), dual, want_dv)
                log, *got = run_k1_bwd(ops, dt, dv, B, N, D, dual, want_dv)
                assert log == k1_bwd_log(B, N, D, dual) and log[1][0] == K1_BWD[dual, form], (what, log)
                for key, have, want in zip(("d_alpha", "d_q1", "d_q2", "d_v"), got, refs[dual]):
                    if have is not None:
                        assert_exact("%s %s" % (what, key), have, want)


# (id, form, B, N, D, amplitude of v and g)
K1_BWD_CASES = [("small-N1", "RS", 3, 1, 260, 4), ("small-N36", "RS", 3, 36, 260, 4), ("small-N300", "RS", 3, 300, 260, 2),
                ("large-D2048", "1", 512, 3, 2048, 4), ("large-D4100", "1", 256, 2, 4100, 4)]


@gpu
@pytest.mark.parametrize("case", K1_BWD_CASES, ids=lambda c: c[0])
def test_k1_backward_small_integers_are_exact(ops, case):
    name, form, B, N, D, amp = case
    check_k1_bwd(ops, name, k1_operands(B, N, D, amp) + k1_gradients(B, N, D, amp), B, N, D, form)


@gpu
def test_k1_backward_threshold(ops):
    """the inputs of [large-D2048] one sample short (B D = 2^20 - 2048): the row-split form, the same integers"""
    check_k1_bwd(ops, "B=511", k1_operands(512, 3, 2048, 4) + k1_gradients(512, 3, 2048, 4), 511, 3, 2048, "RS")


# ======================================================================================================================= A: relation_apply
@functools.lru_cache(maxsize=2)
def ra_operands(B, N, D):
    gen = torch.Generator().manual_seed(7000003 * B + 1013 * N + D)
    return _ints(gen, B, N, D), _ints(gen, B, N, D), _ints(gen, B, D), _ints(gen, B, D)     # v, g, t, c2


def ra_mask(ops, B, N, D, p, seed):
    if not p:
        return torch.ones(B, N, D, dtype=torch.int64)
    mask = ops.linear_dropout_mask(B * N, D, p, seed, dev()).cpu()
    assert set(torch.unique(mask).tolist()) == {0.0, 2.0}
    return mask.view(B, N, D).long()


# (id, B, N, D, grid z): zsplit = 1 when the batch alone gives 2048 workgroups; else ceil(N / 4) z-blocks of 4 rows, the last ragged
RA_FWD_CASES = [(RA_FWD, "zsplit1", 2048, 5, 8, 1), (RA_FWD, "zsplit-ragged", 1, 7, 1028, 2)]


@gpu
@pytest.mark.parametrize("case", RA_FWD_CASES, ids=lambda c: c[1])
def test_relation_apply_forward_small_integers_are_exact(ops, case):
    kernel, name, B, N, D, gz = case
    v, _, t, c2 = ra_operands(B, N, D)
    t_d, c2_d = _d(t, F32), _d(c2, F32)
    for dt in (F32, BF):
        v_d = _d(v, dt)
        for p in (0.0, 0.5):
            seed = 99 + int(p * 10)
            ref = ra_mask(ops, B, N, D, p, seed) * (t[:, None, :] + c2[:, None, :] * v)
            buf = _out(B * N * D, dt)
            fn = getattr(ops._lib.lib(), "vqa_relation_apply_fwd" + _sfx(dt))
            rc, log = _call(ops, fn, _ptr(v_d), _ptr(t_d), _ptr(c2_d), _ptr(buf, PAD), p, seed, None, B, N, D)
            assert rc == 0 and log == [(kernel, _ceil(D // 4, 256) * B * gz * 256)], (name, rc, log)
            assert_exact("relation_apply_fwd %s %s p=%g" % (name, _dt_id(dt), p), _win(buf, (B, N, D), name), ref)


def ra_bwd_log(dt, B, N, D, want_dv):
    """the launch relation_apply_bwd_impl makes"""
    small = B * D // 4 < 4 * 65536
    if dt == BF and not want_dv and D % 8 == 0 and small:
        return [(RA_BWD8, _ceil(D // 8, 32) * B * 256)]
    if small:
        return [(RA_BWD4, _ceil(D // 4, 64) * B * 256)]
    return [(RA_BWD1, _ceil(D // 4, 256) * B * 256)]


def check_ra_bwd(ops, name, host, B, N, D, kernel, dtypes, dvs):
    v, g, _, c2 = (t[:B] for t in host)
    _below_2_24(N * 2 * _amax(g) * _amax(v))
    for p in (0.0, 0.5):
        seed = 555 + int(p * 10)
        gk = g * ra_mask(ops, B, N, D, p, seed)
        refs = (gk.sum(1), (gk * v).sum(1), c2[:, None, :] * gk)
        for dt in dtypes:
            v_d, c2_d, g_d = _d(v, dt), _d(c2, F32), _d(g, dt)
            for want_dv in dvs:
                what = "relation_apply_bwd %s %s p=%g d_v=%d" % (name, _dt_id(dt), p, want_dv)
                b_t, b_c, b_v = _out(B * D), _out(B * D), _out(B * N * D, dt) if want_dv else None
                fn = getattr(ops._lib.lib(), "vqa_relation_apply_bwd" + _sfx(dt))
                rc, log = _call(ops, fn, _ptr(v_d), _ptr(c2_d), _ptr(g_d), _ptr(b_t, PAD), _ptr(b_c, PAD),
                                _ptr(b_v, PAD) if want_dv else None, p, seed, None, B, N, D)
                assert rc == 0 and log == ra_bwd_log(dt, B, N, D, want_dv) and log[0][0] == kernel, (what, rc, log)
                assert_exact(what + " d_t", _win(b_t, (B, D), what), refs[0])
                assert_exact(what + " d_c2", _win(b_c, (B, D), what), refs[1])
                if want_dv:
                    assert_exact(what + " d_v", _win(b_v, (B, N, D), what), refs[2])


# (id, kernel, B, N, D, dtypes, d_v asked for)
RA_BWD_CASES = [
    ("rs4", RA_BWD4, 5, 7, 260, (F32, BF), (False, True)),              # D % 8 != 0: bf16 without d_v takes the generic kernel too
    ("rs1", RA_BWD1, 512, 3, 2048, (F32, BF), (False, True)),
    ("bwd8-N1", RA_BWD8, 3, 1, 264, (BF,), (False,)),
    ("bwd8-N37", RA_BWD8, 3, 37, 264, (BF,), (False,)),
    ("bwd8-not-with-d_v", RA_BWD4, 3, 37, 264, (BF,), (True,)),
]


@gpu
@pytest.mark.parametrize("case", RA_BWD_CASES, ids=lambda c: c[0])
def test_relation_apply_backward_small_integers_are_exact(ops, case):
    name, kernel, B, N, D, dtypes, dvs = case
    check_ra_bwd(ops, name, ra_operands(B, N, D), B, N, D, kernel, dtypes, dvs)


@gpu
def test_relation_apply_backward_threshold(ops):
    """the inputs of [rs1] one sample short: the row-split kernel (bf16 without d_v: the 16-byte kernel), the same integers"""
    host = ra_operands(512, 3, 2048)
    check_ra_bwd(ops, "B=511", host, 511, 3, 2048, RA_BWD4, (F32,), (False, True))
    check_ra_bwd(ops, "B=511", host, 511, 3, 2048, RA_BWD4, (BF,), (True,))
    check_ra_bwd(ops, "B=511", host, 511, 3, 2048, RA_BWD8, (BF,), (False,))


# ======================================================================================================================= B: K3
class Bars(kernel_harness.Bars):
    """kernel_harness.Bars with one row per case instead of one per check(): close() hands the worst of the case, by err / bar, to
    `measured`, then fails if one missed its bar"""

    def report(self, name, err, bar):
        pass

    def close(self):
        _, err, bar, name = max((err / bar if bar else (INF if err else 0.0), err, bar, name) for err, bar, name, _ in self.rows)
        self.measured(self.case, err, bar, name)
        super().close()


def k3_mask(ops, B, G, D, p, seed):
    return ops.linear_dropout_mask(B * G, D, p, seed, dev()).cpu().view(B, G, D) if p else None


def k3_inputs(B, N, D, G, dt, seed):
    """CPU fp32: logits (with +-80 in sample 0), v (dt-exact values), d_pooled, d_first, d_alpha_ext"""
    gen = torch.Generator().manual_seed(seed)
    logits = 3.0 * torch.randn(B, N, G, generator=gen)
    logits[0, 0, :] = 80.0
    if N > 1:
        logits[0, N - 1, :] = -80.0
    v = torch.randn(B, N, D, generator=gen).to(dt).float()
    return logits, v, torch.randn(B, G, D, generator=gen), torch.randn(B, D, generator=gen), torch.randn(B, N, G, generator=gen)


def run_k3_fwd(ops, dt, logits_d, v_d, B, N, D, G, want_first, p, seed):
    """the plain entry point when neither `first` nor dropout is asked for, else the _drop one -> (rc, log, alpha, pooled, first buffers)"""
    L = ops._lib.lib()
    b_a, b_p, b_f = _out(B * N * G), _out(B * G * D), _out(B * D) if want_first else None
    if want_first or p:
        rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_drop_fwd" + _sfx(dt)), _ptr(logits_d), _ptr(v_d), _ptr(b_a, PAD),
                        _ptr(b_p, PAD), _ptr(b_f, PAD) if want_first else None, p, seed, None, B, N, D, G)
    else:
        rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_fwd" + _sfx(dt)), _ptr(logits_d), _ptr(v_d), _ptr(b_a, PAD),
                        _ptr(b_p, PAD), B, N, D, G)
    return rc, log, b_a, b_p, b_f


def k3_fwd_case(ops, bars, dt, B, N, D, G, want_first, p, seed):
    import oracle.kernels_np as knp
    logits, v, _, _, _ = k3_inputs(B, N, D, G, dt, seed)
    mask = k3_mask(ops, B, G, D, p, seed)
    rc, log, b_a, b_p, b_f = run_k3_fwd(ops, dt, logits.to(dev()), v.to(dt).to(dev()), B, N, D, G, want_first, p, seed)
    what = "fwd %s G=%d N=%d D=%d first=%d p=%g" % (_dt_id(dt), G, N, D, want_first, p)
    assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
    assert log == [(K3_FWD, _ceil(D // 4, 256) * B * 256)], (what, log)
    a64, p64 = (torch.from_numpy(x) for x in knp.softmax_attention_pool_fwd(logits.numpy(), v.numpy()))
    a32 = torch.softmax(logits, 1)
    p32 = torch.einsum("bng,bnd->bgd", a32, v)
    alpha = _win(b_a, (B, N, G), what)
    bars.check(what + " alpha", alpha, a64, a32)
    # rows sum to 1: a lane adds at most ceil(N / 64) terms, the wave tree 6 more levels, then one reciprocal and one product per
    # element; the float64 sum of the rounded alphas adds at most half an ulp
    assert float((alpha.double().sum(1).cpu() - 1.0).abs().max()) <= (_ceil(N, 64) + 10) * EPS32, what
    if want_first:
        bars.check(what + " first", _win(b_f, (B, D), what), p64[:, 0].contiguous(), p32[:, 0].contiguous())
    if mask is not None:
        p64, p32 = p64 * mask.double(), p32 * mask
    bars.check(what + " pooled", _win(b_p, (B, G, D), what), p64, p32)


K3_FWD_CASES = [(K3_FWD, dt, G) for dt in (F32, BF) for G in range(1, 9)]


@gpu
@pytest.mark.parametrize("case", K3_FWD_CASES, ids=lambda c: "%s-G%d" % (_dt_id(c[1]), c[2]))
def test_k3_forward_against_float64(ops, measured, case):
    """every G; N in {1, 100, 257} meets D in {8, 1028}, `first` and p in {0, 0.5, 0.25} in rotation; G = 8 also at N = 1024"""
    _, dt, G = case
    shapes = [(1, 8), (100, 1028), (257, 8), (1, 1028), (100, 8), (257, 1028)]
    runs = [(*shapes[(G + i) % 6], bool((G // 2 + i) % 2), (0.0, 0.5, 0.25)[(G + 2 * i) % 3]) for i in range(4)]
    if G == 8:
        runs += [(1024, 1028, True, 0.5), (1024, 8, False, 0.0)]
    for i, (N, D, want_first, p) in enumerate(runs):
        bars = Bars(measured, "fwd %s G%d N%d D%d f%d p%g" % (_dt_id(dt), G, N, D, want_first, p))
        k3_fwd_case(ops, bars, dt, 3, N, D, G, want_first, p, 31 * G + i)
        bars.close()


def k3_bwd_log(form, B, N, D, G):
    if form == K3_FUSED:
        return [(K3_FUSED, B * 256)]
    cols = 64 if form == K3_STREAM4 else 256
    return [(ZERO, min(_ceil(B * N * G, 256), 2048) * 256), (form, _ceil(D // 4, cols) * B * 256), (K3_SOFTMAX, B * 256)]


def k3_bwd_case(ops, bars, form, dt, B, N, D, G, ext, want_dv, first, p, seed, poison=None):
    """one backward call against float64.  alpha is an input: the float32 rounding of a float64 softmax.  poison: a sample whose
    d_pooled holds a NaN -- it is left out of the comparison and must be the only one whose d_logits is not finite"""
    import oracle.kernels_np as knp
    logits, v, d_pooled, d_first, d_ext = k3_inputs(B, N, D, G, dt, seed)
    alpha = torch.softmax(logits.double(), 1).float()
    mask = k3_mask(ops, B, G, D, p, seed)
    L = ops._lib.lib()
    b_l, b_v = _out(B * N * G), _out(B * N * D, dt) if want_dv else None
    dp_d = d_pooled.clone()
    if poison is not None:
        dp_d[poison, 0, 7] = NAN
    a_d, v_d, dp_d, df_d, de_d = alpha.to(dev()), v.to(dt).to(dev()), dp_d.to(dev()), d_first.to(dev()), d_ext.to(dev())
    if first or p:
        rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_drop_bwd" + _sfx(dt)), _ptr(a_d), _ptr(v_d), _ptr(dp_d),
                        _ptr(df_d) if first else None, _ptr(de_d) if ext else None, _ptr(b_l, PAD), _ptr(b_v, PAD) if want_dv else None,
                        p, seed, None, B, N, D, G)
    else:
        rc, log = _call(ops, getattr(L, "vqa_softmax_attention_pool_bwd" + _sfx(dt)), _ptr(a_d), _ptr(v_d), _ptr(dp_d),
                        _ptr(de_d) if ext else None, _ptr(b_l, PAD), _ptr(b_v, PAD) if want_dv else None, B, N, D, G)
    what = "bwd %s G=%d B=%d N=%d D=%d ext=%d d_v=%d first=%d p=%g" % (_dt_id(dt), G, B, N, D, ext, want_dv, first, p)
    assert rc == 0, (what, rc, L.vqa_last_error())
    assert log == k3_bwd_log(form, B, N, D, G), (what, log)
    dp = d_pooled if mask is None else d_pooled * mask
    if first:
        dp = dp.clone()
        dp[:, 0] += d_first
    dl64, dv64 = (torch.from_numpy(x) for x in knp.softmax_attention_pool_bwd(
        alpha.numpy(), v.numpy(), _dp64(d_pooled, mask, d_first if first else None), d_ext.numpy() if ext else None))
    dal32 = torch.einsum("bgd,bnd->bng", dp, v) + (d_ext if ext else 0.0)
    dl32 = alpha * (dal32 - (alpha * dal32).sum(1, keepdim=True))
    dv32 = torch.einsum("bng,bgd->bnd", alpha, dp)
    keep = [b for b in range(B) if b != poison]
    d_logits = _win(b_l, (B, N, G), what).cpu()
    if poison is not None:
        assert not bool(torch.isfinite(d_logits[poison]).all()), what
    bars.check(what + " d_logits", d_logits[keep], dl64[keep], dl32[keep])
    if want_dv:
        bars.check(what + " d_v", _win(b_v, (B, N, D), what).cpu()[keep], dv64[keep], dv32[keep])


def _dp64(d_pooled, mask, d_first):
    """float64 numpy: the gradient that reaches the pooled rows -- d_pooled through the forward's mask, d_first on glimpse 0"""
    dp = d_pooled.double() if mask is None else d_pooled.double() * mask.double()
    if d_first is not None:
        dp = dp.clone()
        dp[:, 0] += d_first.double()
    return dp.numpy()


K3_FUSED_CASES = [(K3_FUSED, dt, G) for dt in (F32, BF) for G in (1, 2, 4, 8)]


@gpu
@pytest.mark.parametrize("case", K3_FUSED_CASES, ids=lambda c: "%s-G%d" % (_dt_id(c[1]), c[2]))
def test_k3_backward_fused_against_float64(ops, lib_option, measured, case):
    """D in {1028, 2048} x d_alpha_ext x d_v x d_first x p in {0, 0.5, 0.25}; N = 37 (1028) and 20 (2048), B = 3"""
    form, dt, G = case
    lib_option("VQA_K3_FUSED_MIN_B", 1)
    i = 0
    for D, N in ((1028, 37), (2048, 20)):
        for ext in (False, True):
            for want_dv in (False, True):
                for first in (False, True):
                    for p in (0.0, 0.5, 0.25):
                        bars = Bars(measured, "fused %s G%d D%d e%d v%d f%d p%g" % (_dt_id(dt), G, D, ext, want_dv, first, p))
                        k3_bwd_case(ops, bars, form, dt, 3, N, D, G, ext, want_dv, first, p, 1000 * G + i)
                        bars.close()
                        i += 1


# (id, kernel, dtype, B, N, D, G, VQA_K3_FUSED_MIN_B or None): everything just outside the fused kernel's window
K3_EDGE_CASES = [
    ("D1024", K3_STREAM4, F32, 3, 37, 1024, 4, 1), ("D2052", K3_STREAM4, F32, 3, 37, 2052, 4, 1), ("G3", K3_STREAM4, F32, 3, 37, 2048, 3, 1),
    ("B63-default", K3_STREAM4, F32, 63, 2, 1028, 4, None), ("B64-default", K3_FUSED, F32, 64, 2, 1028, 4, None),
    ("B64-default-bf16", K3_STREAM4, BF, 64, 2, 1028, 4, None), ("huge-knob", K3_STREAM4, F32, 64, 2, 1028, 4, 1 << 30),
]


@gpu
@pytest.mark.parametrize("case", K3_EDGE_CASES, ids=lambda c: c[0])
def test_k3_backward_fused_window_edges(ops, lib_option, measured, case):
    name, form, dt, B, N, D, G, min_b = case
    lib_option("VQA_K3_FUSED_MIN_B", min_b)
    bars = Bars(measured, "edge %s" % name)
    k3_bwd_case(ops, bars, form, dt, B, N, D, G, True, True, True, 0.5, 77)
    bars.close()


# (id, kernel, B, N, D, G)
K3_THREE_CASES = ([("rs4-G%d-N%d" % (G, N), K3_STREAM4, 3, N, 260, G) for G in (3, 5, 6, 7) for N in (1, 100)]
                  + [("rs4-G%d-N100" % G, K3_STREAM4, 3, 100, 260, G) for G in (1, 2, 4, 8)]      # the butterfly branch of the row-split form
                  + [("rs1-D4096-G4", K3_STREAM1, 256, 3, 4096, 4), ("rs1-D1024-G3", K3_STREAM1, 1024, 2, 1024, 3)])


@gpu
@pytest.mark.parametrize("case", K3_THREE_CASES, ids=lambda c: c[0])
def test_k3_backward_three_launches_against_float64(ops, lib_option, measured, case):
    """zero + stream + softmax: d_logits adds up in float atomics and is held to the same bar as the fused form"""
    name, form, B, N, D, G = case
    lib_option("VQA_K3_FUSED_MIN_B", 1)          # (the window is missed by D or by G, not by the batch)
    for dt in (F32, BF):
        for i, (ext, want_dv, first, p) in enumerate([(False, True, False, 0.0), (True, False, True, 0.5), (True, True, True, 0.25)]):
            bars = Bars(measured, "%s %s e%d v%d f%d p%g" % (name, _dt_id(dt), ext, want_dv, first, p))
            k3_bwd_case(ops, bars, form, dt, B, N, D, G, ext, want_dv, first, p, 500 + i)
            bars.close()


# (id, kernel, B, N, D, G): the dynamic-LDS requests past 64 KiB.  N G = 8192: the softmax kernel asks for 65 568 bytes and the fused
# kernel would need 196 640 -- more than a CU has, so D = 2048 takes the three-launch form as well; N G = 3200: fused with 76 832
K3_LDS_CASES = [("three-launch-D260", K3_STREAM4, 2, 1024, 260, 8), ("fused-does-not-fit-D2048", K3_STREAM4, 2, 1024, 2048, 8),
                ("fused-77KB", K3_FUSED, 2, 400, 2048, 8)]


@gpu
@pytest.mark.parametrize("case", K3_LDS_CASES, ids=lambda c: c[0])
def test_k3_backward_lds_limits(ops, lib_option, measured, case):
    """accepted shapes (G <= 8, N <= 1024) whose dynamic-LDS request passes 64 KiB: VQA_OK and the bar of every other case.  The
    launcher raises the kernel's cap for them and keeps the fused form to requests that fit the 160 KB of a CU"""
    name, form, B, N, D, G = case
    lib_option("VQA_K3_FUSED_MIN_B", 1)
    for dt in (F32, BF):
        bars = Bars(measured, "lds %s %s" % (name, _dt_id(dt)))
        k3_bwd_case(ops, bars, form, dt, B, N, D, G, True, True, True, 0.5, 900)
        bars.close()


# ======================================================================================================================= C
@gpu
@pytest.mark.parametrize("dt", [F32, BF], ids=_dt_id)
def test_k3_non_finite_values_stay_in_their_sample(ops, lib_option, measured, dt):
    """a NaN logit: alpha and pooled of that sample only (the other samples bit for bit what a clean run gives); a NaN in d_pooled:
    d_logits of that sample only, in the fused and in the three-launch form"""
    B, N, D, G = 3, 37, 1028, 2
    logits, v, _, _, _ = k3_inputs(B, N, D, G, dt, 5)
    v_d = v.to(dt).to(dev())
    outs = []
    for poisoned in (False, True):
        lg = logits.clone()
        if poisoned:
            lg[1, 5, 0] = NAN
        rc, log, b_a, b_p, b_f = run_k3_fwd(ops, dt, lg.to(dev()), v_d, B, N, D, G, True, 0.0, 0)
        assert rc == 0 and log[0][0] == K3_FWD, (rc, log)
        outs.append((_win(b_a, (B, N, G), "alpha"), _win(b_p, (B, G, D), "pooled"), _win(b_f, (B, D), "first")))
    for clean, dirty in zip(*outs):
        assert _same_bits(clean[0], dirty[0]) and _same_bits(clean[2], dirty[2]), "the NaN of sample 1 reached another sample"
        assert bool(torch.isfinite(clean).all())
    alpha, pooled, first = outs[1]
    assert bool(torch.isnan(alpha[1, :, 0]).all()) and bool(torch.isnan(pooled[1, 0]).all()) and bool(torch.isnan(first[1]).all())
    assert _same_bits(alpha[1, :, 1], outs[0][0][1, :, 1]) and _same_bits(pooled[1, 1], outs[0][1][1, 1]), "the NaN left its glimpse"
    for form, D_ in ((K3_FUSED, 1028), (K3_STREAM4, 260)):
        lib_option("VQA_K3_FUSED_MIN_B", 1)
        bars = Bars(measured, "nan %s %s" % (_dt_id(dt), "fused" if form == K3_FUSED else "three"))
        k3_bwd_case(ops, bars, form, dt, B, N, D_, G, True, True, False, 0.0, 6, poison=1)
        bars.close()


@gpu
def test_k3_refusals_launch_nothing(ops):
    """G = 9, N = 1025, D % 4 != 0, a misaligned pooled / d_pooled, p = 1: the documented code, an error text, no launch, sentinels"""
    L = ops._lib.lib()
    src = torch.zeros(1 << 16, device=dev())
    outs = [_sentinel(1 << 16) for _ in range(3)]
    buf = (ctypes.c_ulonglong * 16)()

    def refused(code, fn, *args):
        L.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, args, L.vqa_last_error())
        assert L.vqa_last_error() and L.vqa_launch_log(buf, 16) == 0, "a refused call launched a kernel"

    def fwd(B=2, N=5, D=8, G=2, pooled=None, v=src):
        return (_ptr(src), _ptr(v), _ptr(outs[0]), pooled or _ptr(outs[1])), (B, N, D, G)

    def bwd(B=2, N=5, D=8, G=2, d_pooled=None, v=src):
        return (_ptr(src), _ptr(v), d_pooled or _ptr(src)), (_ptr(src), _ptr(outs[0]), _ptr(outs[1])), (B, N, D, G)

    for sfx, esz in (("", 4), ("_bf16", 2)):
        f, fd = getattr(L, "vqa_softmax_attention_pool_fwd" + sfx), getattr(L, "vqa_softmax_attention_pool_drop_fwd" + sfx)
        b, bd = getattr(L, "vqa_softmax_attention_pool_bwd" + sfx), getattr(L, "vqa_softmax_attention_pool_drop_bwd" + sfx)
        odd_v = ctypes.c_void_p(src.data_ptr() + esz)
        for kw in (dict(G=9), dict(N=1025), dict(D=6), dict(pooled=_ptr(outs[1], 1))):
            head, tail = fwd(**kw)
            refused(E_UNSUPPORTED, f, *head, *tail)
            refused(E_UNSUPPORTED, fd, *head, _ptr(outs[2]), 0.5, 0, None, *tail)
        for kw in (dict(G=9), dict(N=1025), dict(D=6), dict(d_pooled=_ptr(src, 1))):
            head, mid, tail = bwd(**kw)
            refused(E_UNSUPPORTED, b, *head, *mid, *tail)
            refused(E_UNSUPPORTED, bd, *head, _ptr(src), *mid, 0.5, 0, None, *tail)
        head, tail = fwd()
        refused(E_UNSUPPORTED, f, head[0], odd_v, *head[2:], *tail)                                   # a misaligned v
        refused(E_UNSUPPORTED, fd, *head, _ptr(outs[2], 1), 0.0, 0, None, *tail)                      # a misaligned first
        refused(E_BADARG, fd, *head, _ptr(outs[2]), 1.0, 0, None, *tail)                              # p = 1
        refused(E_BADARG, fd, *head, _ptr(outs[2]), -0.5, 0, None, *tail)
        refused(E_BADARG, f, *fwd(G=0)[0], *fwd(G=0)[1])
        refused(E_BADARG, f, None, *head[1:], *tail)
        head, mid, tail = bwd()
        refused(E_BADARG, bd, *head, _ptr(src), *mid, 1.0, 0, None, *tail)
        refused(E_UNSUPPORTED, bd, *head, _ptr(src, 1), *mid, 0.0, 0, None, *tail)                    # a misaligned d_first
        refused(E_BADARG, b, *head, mid[0], None, mid[2], *tail)                                      # d_logits = NULL
    torch.cuda.synchronize()
    for t in outs:
        assert _untouched(t)


# ======================================================================================================================= D
ALL_TABLES = [K1_FWD_CASES, RA_FWD_CASES, RA_BWD_CASES, K3_FWD_CASES, K3_FUSED_CASES, K3_EDGE_CASES, K3_THREE_CASES, K3_LDS_CASES]


def declared_forms():
    """every kernel expression a parametrised case above names (and asserts from the launch log)"""
    forms = {s for table in ALL_TABLES for case in table for s in case if isinstance(s, str) and "_kernel" in s}
    forms |= {K1_BWD[dual, form] for _, form, *_ in K1_BWD_CASES + [("threshold", "RS")] for dual in (False, True)}
    forms.add(K3_SOFTMAX)            # the third launch of every K3_STREAM4 / K3_STREAM1 case (k3_bwd_log)
    return forms


def test_every_launch_site_is_declared():
    """a launch site added to (or renamed in) either file without a case here fails; so does a case whose form no longer exists"""
    csrc = os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc")
    sites = launch_sites(os.path.join(csrc, "pairwise_relation.hip")) + launch_sites(os.path.join(csrc, "attention_pool.hip"))
    assert len(sites) == 20, sites
    declared = declared_forms()
    assert set(sites) - declared == set(), "launch sites that no case declares"
    assert declared - set(sites) == set(), "declared forms that no launch site has"
