"""Every launch form of the fp32 low-rank bilinear (Mutan) fusion, K4 (csrc/bilinear_fusion.hip, bilinear_folded.hip, bilinear_rt.hip,
bilinear_dw_rt.hip, bilinear_dw_split.hip), through the C ABI, one dispatch form at a time.  tests/test_gpu_kernels.py reaches these
files through autograd under a loose tolerance and never says which kernel ran; here every VQA_LAUNCH site is launched, the launch
log (kernel expression as the log spells it -- macro parameters substituted -- and grid in work-items, restated from B, N, L, H, R
and the dispatchers' arithmetic) says that it was, and its result is compared whole.

  A  small-integer operands (|x|, |w1|, |b1|, |h2|, |g| <= 3, with zeros; x >= 0 with about half its entries 0 under gate_dx = 1):
     every fp32 product and partial sum of every form is an integer below 2^24 (asserted per case from the operands' magnitudes, on
     the CPU as well: test_case_tables_stay_exact), so any order of summation gives the same bits -- on the fp32 MFMA engines and
     on the split engine, whose three-way bf16 split of such a value is exact.  The reference is the formula of
     oracle/kernels_np.py in float64 with torch on the CPU, chunked over b (exact for these integers; checked against the oracle
     itself in test_reference_is_the_oracle).  Outputs sit in sentinel-filled buffers that are compared whole, inputs in NaN-padded
     ones (ldx = L + 2 leaves a NaN gap behind every row of x), the workspace is exactly *_workspace_bytes long (restated here),
     pre-filled with NaN, with a sentinel fence behind it.  gate_dx = 1 gives the ungated d_x times (x > 0).
  B  random operands against float64 (oracle/kernels_np.py) under the project's bar (Bars of tests/kernel_harness.py):
     four times the error of the same formula in float32 with torch on the CPU plus one float32 ulp of the tensor's largest
     magnitude.  Every case reports what it measured.  The split engine reports against the same bar and is held to it or to the
     bar test_lowrank_bilinear_fusion_large_batch_against_torch_fp64 states for it (2e-5 of the largest magnitude).
  C  a NaN stays in its sample; refusals launch nothing and leave the outputs alone; gate_dx keeps d_x where x > 0, so a NaN x zeroes it.
  D  test_every_launch_site_is_declared (no GPU): every VQA_LAUNCH first argument of the five files is the form of some case below.

Not tested, on purpose: the VQA_K4_DW_TUNE site of bilinear_dw_rt.hip (a diagnostic build's stamps: it allocates and synchronises
inside the launch path); its spelling is listed for test D as declared and unlaunched.  VQA_K4_FOLD_DW_PF and VQA_K4_FOLD_DW_BK are
read per call like every other knob, so their cases ([pf2-*], [bk16-*]) run in this process under lib_option.

What this file found (fixed with it): the split engine writes four partial sums of d_h2 where the workspace held 2 ceil(L / 64), two
at L <= 64 ([split-L2], [split-L62], [split-L64] would have stored B R H floats past the workspace; folded_ws_bytes restates the
corrected figure); bilinear_dw_rt_kernel multiplied its columns past L + 1 with the next row of x, so a NaN in the first region of a
sample reached d_h2 of the sample before it (test_a_nan_stays_in_its_sample[dw_rt]); the gated entry launched the weight transpose
before it refused ldx != L (test_refusals_launch_nothing); VQA_K4_DW_FORM=1 at R = 1 chose the per-sample kernel's 4-rank form ([form1-R1]).

Dispatch form (as the source spells the launch site) -> the test that launches it and asserts that it did:

  (bilinear_fwd_kernel<BM_,BN_,BK_>)                 test_engine_forward_small_integers_are_exact [tile-*] (four tiles x PF 1, 2, 3 under
                                                     VQA_GEMM_TILE; partial row and column tiles; with and without h1), [N1], [R5], [R8], [ldx]
  bilinear_dh2_kernel                                the first launch of every test_engine_backward_small_integers_are_exact case
  (bilinear_dx_kernel<BM_,BN_,BK_>)                  ... [tile-*], [scaled-tile-*]; absent in [no-dx]
  (bilinear_dw_sample_kernel<BM_,BN_,PF_,R_>)        ... [tile-*] (R = 2, 3, 4), [sample-*], [form1-N17], [slabs-*-sample] (S = 1; 4 slabs for 9
                                                     samples: the last one empty), [lds-bound] (VQA_K4_DW_SPLITS=1 raised to 3), [ldx-sample]
  (bilinear_dw_kernel<BM_,BN_,BK_>)                  ... [scaled-tile-*] (VQA_K4_DW_FORM=0), [scaled-R1], [scaled-R5], [scaled-N17], [form0-N24],
                                                     [form1-R5], [form1-R1], [slabs-*-scaled], [ldx-scaled], [N1]
  bilinear_dw_reduce_kernel                          the last launch of every engine backward case
  (bilinear_folded_kernel<NB_,R_,H2_ROWS,W_,OB_>)    test_folded_small_integers_are_exact [lds-NB*-R*-W*-OB*]: every (NB, R, W) as a forward,
                                                     every (NB, R, W, OB) as a data gradient, gated and ungated (N = 112, R = 2, 8 waves: exactly
                                                     160 KB forward, 4 waves in the data gradient); [natural-*]; [rt-B255], [rt-N16], [rt-N49],
                                                     [rt-off], [rt-gated]
  fold_transpose_kernel                              the first launch of every folded backward that asks for d_x, absent otherwise
  (bilinear_fold_rt_kernel<FWD,S,IB,1>)              ... [rt-fwd-R1*], [rt-dx-R1]
  (bilinear_fold_rt_kernel<FWD,S,IB,2,2>), <..,2,4>, <..,2>   ... [rt-fwd-*], [rt-dx-*] (VQA_K4_FG = 2, 4, 1 and unset; H = 258 / L = 322: NO % 4 == 2)
  (bilinear_dw_rt_kernel<R_,NS_,D_>)                 ... [dwrt-*] ((R, N) in {1, 2} x {36, 100}; L = 258, 318; B = 65: three half-groups empty)
  (bilinear_dw_split_kernel<LBW_>)                   ... [split-L*] (VQA_K4_DW_SPLIT=1; LBW 1..5 on both sides of every block edge; B = 65: empty slabs)
  (bilinear_dw_dh2_kernel<64,64,PF_,R_,BK_>)         ... [dwdh2-*] (B = 1, 7, 65: S capped by B and by 64, the last slabs empty), [pf2-*], [bk16-*]
                                                     (VQA_K4_FOLD_DW_PF / _BK), [lds-*] (every folded backward with B < 64), the thresholds
                                                     [dwrt-L256], [dwrt-L320], [dwrt-B63], [dwrt-ldx], [dwrt-off], [dwrt-H770], [split-L320], ..
  bilinear_dw_dh2_reduce_kernel (three sites)        the last launch of every folded backward: after the split engine (16 slabs, 4 partial sums),
                                                     the register-tile form (8 and 2) and the LDS-tile form (S and 2 tiles_n)
  (bilinear_dw_rt_kernel<2,9,9,4>)                   declared, not launched (see above)"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from kernel_harness import (E_BADARG, E_UNSUPPORTED, F64, NAN, PAD, Bars, _below_2_24, _call, _ceil, _in, _out, _ptr, _sentinel, _untouched,
                            _win, assert_exact, dev, launch_sites, ops, set_knobs, spell)  # noqa: F401  (ops: the fixture)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc")
K4_FILES = ("bilinear_fusion.hip", "bilinear_folded.hip", "bilinear_rt.hip", "bilinear_dw_rt.hip", "bilinear_dw_split.hip")

# ---- the launch sites as the source spells them (blanks removed); a macro parameter (NAME_) arrives substituted in the log -------
S_FWD, S_DX, S_DW = "(bilinear_fwd_kernel<BM_,BN_,BK_>)", "(bilinear_dx_kernel<BM_,BN_,BK_>)", "(bilinear_dw_kernel<BM_,BN_,BK_>)"
S_DWS = "(bilinear_dw_sample_kernel<BM_,BN_,PF_,R_>)"
S_DH2, S_DWRED, S_RED = "bilinear_dh2_kernel", "bilinear_dw_reduce_kernel", "bilinear_dw_dh2_reduce_kernel"
S_DWDH2 = "(bilinear_dw_dh2_kernel<64,64,PF_,R_,BK_>)"
S_FOLD, S_TR = "(bilinear_folded_kernel<NB_,R_,H2_ROWS,W_,OB_>)", "fold_transpose_kernel"
S_RT1, S_RT22, S_RT24, S_RT2 = ("(bilinear_fold_rt_kernel<FWD,S,IB,1>)", "(bilinear_fold_rt_kernel<FWD,S,IB,2,2>)",
                                "(bilinear_fold_rt_kernel<FWD,S,IB,2,4>)", "(bilinear_fold_rt_kernel<FWD,S,IB,2>)")
S_DWRT, S_DWRT_TUNE = "(bilinear_dw_rt_kernel<R_,NS_,D_>)", "(bilinear_dw_rt_kernel<2,9,9,4>)"
S_SPLIT = "(bilinear_dw_split_kernel<LBW_>)"
MACRO_PARAMS = ("BM_", "BN_", "BK_", "PF_", "R_", "NB_", "W_", "OB_", "NS_", "LBW_")     # (D_ is a constant of the launcher, not a parameter)
spell = functools.partial(spell, params=MACRO_PARAMS)


def _pp(bufs, off=PAD):
    """host array of device pointers, one per rank"""
    return (ctypes.c_void_p * len(bufs))(*[b.data_ptr() + 4 * off for b in bufs])


# ======================================================================================================================= the dispatchers, restated
def _atoi(knobs, name, default=None):
    return int(knobs[name]) if name in knobs else default


def choose_tile(M, cols):
    """gemm_f32_mfma.hpp: fewest CU-rounds of padded work, mild preference for the larger tile"""
    best, pick = 1e300, (128, 128)
    for (bm, bn), pref in zip(((128, 128), (64, 128), (128, 64), (64, 64)), (1.35, 1.15, 1.25, 1.00)):
        cost = float(_ceil(_ceil(M, bm) * _ceil(cols, bn), 256)) * bm * bn * pref
        if cost < best:
            best, pick = cost, (bm, bn)
    return pick + (2,)


def tile_or(knobs, default):
    """tile_override_or: VQA_GEMM_TILE = BMxBN[xPF]"""
    e = knobs.get("VQA_GEMM_TILE")
    if e is not None:
        v = [int(s) for s in e.split("x")]
        if len(v) >= 2 and v[0] in (64, 128) and v[1] in (64, 128):
            return (v[0], v[1], v[2] if len(v) == 3 and 1 <= v[2] <= 3 else 2)
    return default


def dw_per_sample(N, R, knobs):
    if "VQA_K4_DW_FORM" in knobs:
        return int(knobs["VQA_K4_DW_FORM"]) != 0 and 2 <= R <= 4
    return 2 <= R <= 4 and N * 4 >= _ceil(N, 16) * 16 * 3


def max_samples_per_slab(R):
    return 65536 // (R * 64 * 4)


def engine_slabs(B, N, L, H, R, knobs):
    bm, bn, _ = tile_or(knobs, (64, 64, 2))
    tiles = _ceil(H, bm) * _ceil(L, bn)
    if dw_per_sample(N, R, knobs):
        s = min(_atoi(knobs, "VQA_K4_DW_SPLITS", _ceil(1280, tiles)), 64)
        per = max_samples_per_slab(R) * 64 // bm
        return max(min(max(s, _ceil(B, per)), B), 1)
    s = _atoi(knobs, "VQA_K4_DW_SPLITS", _ceil(1280, tiles * R))
    return max(min(s, _ceil(B * N, 256), 64), 1)


def engine_fwd_log(B, N, L, H, R, knobs):
    bm, bn, pf = tile_or(knobs, choose_tile(B * N, H))
    return [(S_FWD, spell(S_FWD, bm, bn, pf), _ceil(B * N, bm) * _ceil(H, bn) * 256)]


def engine_bwd_log(B, N, L, H, R, knobs, want_dx):
    M = B * N
    log = [(S_DH2, S_DH2, _ceil(H // 2, 64) * B * 256)]
    if want_dx:
        bm, bn, pf = tile_or(knobs, choose_tile(M, L))
        log.append((S_DX, spell(S_DX, bm, bn, pf), _ceil(M, bm) * _ceil(L, bn) * 256))
    bm, bn, pf = tile_or(knobs, (64, 64, 2))
    tiles, S = _ceil(H, bm) * _ceil(L, bn), engine_slabs(B, N, L, H, R, knobs)
    if dw_per_sample(N, R, knobs):
        log.append((S_DWS, spell(S_DWS, bm, bn, pf, R), tiles * S * 256))
    else:
        log.append((S_DW, spell(S_DW, bm, bn, pf), tiles * R * S * 256))
    return log + [(S_DWRED, S_DWRED, _ceil(H * L // 2, 256) * R * 256)]


def engine_ws_bytes(B, N, L, H, R, knobs):
    return engine_slabs(B, N, L, H, R, knobs) * R * H * (L + 1) * 4


def folded_lds_bytes(N, R, h2_rows, waves, ob=4):
    return 8 * (R * ob * 16 * 20 + waves * N * 20 + (0 if h2_rows else waves * R * 16))


def folded_config(B, N, O, R, h2_rows, knobs):
    """-> (waves, ob): the cost model's pick, then VQA_K4_FOLD_WAVES / _OB where the forced shape fits 160 KB of LDS"""
    best, pick = 1e30, (4, 4)
    for ob in (4, 5):
        if ob == 5 and (h2_rows or N > 48):
            continue
        for waves in (8, 4):
            lds = folded_lds_bytes(N, R, h2_rows, waves, ob)
            if lds > 160 * 1024:
                continue
            per_cu = min(160 * 1024 // lds, 16 // waves)
            per = _ceil(_ceil(O, ob * 16) * _ceil(B, waves), 256)
            cost = float(per * ob * waves)
            if min(per, per_cu) * waves < 8:
                cost *= 1.3
            if waves == 4:
                cost *= 1.05
            if waves == 8 and min(per, per_cu) == 1:
                cost *= 1.1
            if cost < best:
                best, pick = cost, (waves, ob)
    waves, ob = pick
    if _atoi(knobs, "VQA_K4_FOLD_WAVES") in (4, 8):
        waves = _atoi(knobs, "VQA_K4_FOLD_WAVES")
    eo = _atoi(knobs, "VQA_K4_FOLD_OB")
    if eo == 4 or (eo == 5 and not h2_rows and N <= 48):
        ob = eo
    return (waves, ob) if folded_lds_bytes(N, R, h2_rows, waves, ob) <= 160 * 1024 else pick


def region_blocks(N):
    return 1 if N <= 16 else 2 if N <= 32 else 3 if N <= 48 else 5 if N <= 80 else 7


def fold_entry(B, N, O, R, h2_rows, knobs):
    waves, ob = folded_config(B, N, O, R, h2_rows, knobs)
    nb = region_blocks(N)
    assert ob == 4 or (not h2_rows and nb <= 3)
    return (S_FOLD, spell(S_FOLD, nb, R, waves, ob), _ceil(O, ob * 16) * _ceil(B, waves) * 64 * waves)


def rt_ok(B, N, K, NO, R, ldx, ldw, ldo, knobs):
    return (not knobs.get("VQA_K4_RT", "").startswith("0") and 1 <= R <= 2 and 16 < N <= 48 and B >= 256 and K >= 32 and NO >= 64
            and ldx % 2 == 0 and ldw % 2 == 0 and ldo % 2 == 0 and B * N * max(ldx, ldo) * 4 < 2 ** 32 and NO * ldw * 4 < 2 ** 32)


def rt_entry(fwd, B, NO, R, knobs):
    S, IB = (4, 4) if fwd else (2, 5)
    fg = _atoi(knobs, "VQA_K4_FG", 4 if fwd else 2)
    site = S_RT1 if R == 1 else S_RT22 if fg == 2 else S_RT24 if fg == 4 else S_RT2
    return (site, site, _ceil(B, S) * _ceil(NO, 64 * IB) * 256)


def folded_fwd_log(B, N, L, H, R, ldx, knobs):
    return [rt_entry(True, B, H, R, knobs) if rt_ok(B, N, L, H, R, ldx, L, H, knobs) else fold_entry(B, N, H, R, True, knobs)]


def dw_fold_bk(N, R, knobs):
    return 40 if 32 < N <= 40 and R <= 2 and _atoi(knobs, "VQA_K4_FOLD_DW_BK", 0) != 16 else 16


def dw_fold_splits(B, N, H, L, R, knobs):
    resident = 2 if dw_fold_bk(N, R, knobs) == 40 else (3 if R <= 2 else 2)
    s = min(_atoi(knobs, "VQA_K4_DW_SPLITS", 256 * resident // (_ceil(H, 64) * _ceil(L, 64))), 64)
    return max(min(max(s, _ceil(B, max_samples_per_slab(R))), B), 1)


def dw_split_ok(B, N, L, H, R, ldx, knobs):
    lbw = (L + 64) // 64
    return (knobs.get("VQA_K4_DW_SPLIT", "").startswith("1") and R == 2 and N == 36 and ldx == L and L % 2 == 0 and L >= 2 and H % 2 == 0
            and 1 <= lbw <= 5 and H >= 16 and B >= 64 and _ceil(B, 16) <= 32)


def dw_rt_ok(B, N, L, H, R, ldx, knobs):
    return (not knobs.get("VQA_K4_DW_RT", "").startswith("0") and R in (1, 2) and N in (36, 100) and 256 < L < 320 and ldx == L
            and L % 2 == 0 and H >= 16 and B >= 64)


def folded_bwd_log(B, N, L, H, R, ldx, knobs, want_dx, gate):
    log = []
    if want_dx:
        log.append((S_TR, S_TR, _ceil(L, 32) * _ceil(H, 32) * R * 256))
        log.append(rt_entry(False, B, L, R, knobs) if not gate and rt_ok(B, N, H, L, R, H, H, L, knobs) else fold_entry(B, N, L, R, False, knobs))
    reduce_ = (S_RED, S_RED, (R * _ceil(H * L // 2, 256) + _ceil(B * R * H // 2, 256)) * 256)
    if dw_split_ok(B, N, L, H, R, ldx, knobs):
        return log + [(S_SPLIT, spell(S_SPLIT, (L + 64) // 64), 16 * 2 * _ceil(H, 64) * 256), reduce_]
    S = dw_fold_splits(B, N, H, L, R, knobs)
    if dw_rt_ok(B, N, L, H, R, ldx, knobs) and S >= 8:
        return log + [(S_DWRT, spell(S_DWRT, R, 9 if N == 36 else 25), _ceil(H, 16) * 8 * 256), reduce_]
    pf = 2 if _atoi(knobs, "VQA_K4_FOLD_DW_PF") == 2 else 1
    return log + [(S_DWDH2, spell(S_DWDH2, pf, R, dw_fold_bk(N, R, knobs)), _ceil(H, 64) * _ceil(L, 64) * S * 256), reduce_]


def folded_ws_bytes(B, N, L, H, R, knobs):
    """folded_bwd_floats: the transposes, S slabs of d_w1 and d_b1, then (from a multiple of 4 floats on) the partial sums of d_h2:
    two per 64-column tile, at least the four of the split engine where that form runs"""
    S, parts = dw_fold_splits(B, N, H, L, R, knobs), 2 * _ceil(L, 64)
    if dw_split_ok(B, N, L, H, R, L, knobs):
        S, parts = max(S, 16), max(parts, 4)
    return (_ceil(R * L * H + S * R * H * (L + 1), 4) * 4 + parts * B * R * H) * 4


# ======================================================================================================================= A: operands, reference
def bounds(B, N, L, H, R, a):
    """the largest sum of absolute values of the terms of an element of (out, d_x, d_w1, d_b1, d_h2); at a = 3: R (9 L + 3) 3, R H 27,
    B N 27, B N 9, N 3 (9 L + 3).  h1, an input of the engine backward, stays below the first"""
    return (R * (a * a * L + a) * a, R * H * a ** 3, B * N * a ** 3, B * N * a * a, N * a * (a * a * L + a))


def amplitude(B, N, L, H, R):
    """3, or the largest amplitude below it that keeps every sum of the case under 2^24"""
    for a in (3, 2, 1):
        if max(bounds(B, N, L, H, R, a)) < 2 ** 24:
            return a
    raise AssertionError("no amplitude keeps this shape exact")


@functools.lru_cache(maxsize=2)
def operands(B, N, L, H, R, amp, nonneg):
    """float64 integers on the CPU: x [B,N,L] (within [0, amp], about half of it 0, if nonneg), w1 [R,H,L], b1 [R,H], h2 [B,R,H], g [B,N,H]"""
    gen = torch.Generator().manual_seed(1000003 * B + 10007 * N + 101 * L + 13 * H + 7 * R + amp + 50 * nonneg)
    r = lambda lo, *shape: torch.randint(lo, amp + 1, shape, generator=gen).to(F64)      # noqa: E731
    x = r(0, B, N, L) * torch.randint(0, 2, (B, N, L), generator=gen).to(F64) if nonneg else r(-amp, B, N, L)
    return x, r(-amp, R, H, L), r(-amp, R, H), r(-amp, B, R, H), r(-amp, B, N, H)


def formulas(x, w1, b1, h2, g, backward=True, keep_h1=False):
    """oracle/kernels_np.py's lowrank_bilinear_fusion_fwd / _bwd in the operands' dtype, chunked over b
    -> dict out [B,N,H], h1 [B,N,R,H] (if kept), d_x [B,N,L], d_w1 [R,H,L], d_b1 [R,H], d_h2 [B,R,H]"""
    B, N, L = x.shape
    R, H, _ = w1.shape
    z = lambda *s: torch.zeros(*s, dtype=x.dtype)      # noqa: E731
    res = {"out": z(B, N, H), "h1": z(B, N, R, H) if keep_h1 else None}
    if backward:
        res.update(d_x=z(B, N, L), d_w1=z(R, H, L), d_b1=z(R, H), d_h2=z(B, R, H))
    chunk = max(1, (1 << 22) // (N * R * H))
    for b0 in range(0, B, chunk):
        s = slice(b0, min(B, b0 + chunk))
        h1 = torch.einsum("bnl,rhl->bnrh", x[s], w1) + b1[None, None]
        res["out"][s] = (h1 * h2[s, None]).sum(2)
        if keep_h1:
            res["h1"][s] = h1
        if backward:
            gh = g[s, :, None, :] * h2[s, None]
            res["d_x"][s] = torch.einsum("bnrh,rhl->bnl", gh, w1)
            res["d_w1"] += torch.einsum("bnrh,bnl->rhl", gh, x[s])
            res["d_b1"] += gh.sum((0, 1))
            res["d_h2"][s] = (g[s, :, None, :] * h1).sum(1)
    return res


@functools.lru_cache(maxsize=2)
def reference(B, N, L, H, R, amp, nonneg, backward=True, keep_h1=False):
    host = operands(B, N, L, H, R, amp, nonneg)
    bs = bounds(B, N, L, H, R, max(int(t.abs().max()) for t in host))
    _below_2_24(*(bs if backward else bs[:1]))
    return formulas(*host, backward=backward, keep_h1=keep_h1)


def test_reference_is_the_oracle():
    """the chunked torch restatement equals oracle/kernels_np.py on integers, bit for bit (both are exact)"""
    import oracle.kernels_np as knp
    B, N, L, H, R = 5, 7, 6, 4, 3
    host = operands(B, N, L, H, R, 3, False)
    res = formulas(*host, keep_h1=True)
    np_in = [t.numpy() for t in host]
    out, h1 = knp.lowrank_bilinear_fusion_fwd(*np_in[:4])
    for key, want in zip(("out", "h1", "d_x", "d_w1", "d_b1", "d_h2"), (out, h1) + tuple(knp.lowrank_bilinear_fusion_bwd(*np_in))):
        assert np.array_equal(res[key].numpy(), want), key
    assert float(res["d_x"].abs().max()) > 0 and float(operands(B, N, L, H, R, 3, True)[0].min()) == 0.0


# ======================================================================================================================= the calls
def to_dev(host, ldx):
    """the NaN-padded operand buffers on the GPU: x (rows at stride ldx), one buffer per rank of w1 and b1, h2, g"""
    x, w1, b1, h2, g = host
    return {"x": _in(x, ldx), "w1": [_in(w) for w in w1], "b1": [_in(b) for b in b1], "h2": _in(h2), "g": _in(g)}


def run_fwd(ops, entry, dv, B, N, L, H, R, ldx, want_h1=False):
    """-> (rc, log, out buffer, h1 buffer or None)"""
    Lb = ops._lib.lib()
    out, h1 = _out(B * N * H), _out(B * N * R * H) if want_h1 else None
    head = (_ptr(dv["x"], PAD), ldx, _pp(dv["w1"]), _pp(dv["b1"]), _ptr(dv["h2"], PAD), _ptr(out, PAD))
    if entry == "engine":
        rc, log = _call(ops, Lb.vqa_lowrank_bilinear_fusion_fwd, *head, _ptr(h1, PAD) if want_h1 else None, B, N, L, H, R)
    else:
        assert not want_h1
        rc, log = _call(ops, Lb.vqa_lowrank_bilinear_fusion_folded_fwd, *head, B, N, L, H, R)
    return rc, log, out, h1


def run_bwd(ops, entry, dv, B, N, L, H, R, ldx, knobs, want_dx=True, gate=None, h1=None):
    """-> (rc, log, {d_x, d_w1, d_b1, d_h2}), every output taken whole out of its sentinel-filled buffer; the workspace is exactly as
    long as the library asks for (the figure is restated), NaN-filled, and the sentinel behind it must survive.  gate None: the
    ungated folded entry; 0 / 1: the gated one"""
    Lb = ops._lib.lib()
    if entry == "engine":
        nbytes, want = Lb.vqa_lowrank_bilinear_fusion_bwd_workspace_bytes(B, N, L, H, R), engine_ws_bytes(B, N, L, H, R, knobs)
    else:
        nbytes, want = Lb.vqa_lowrank_bilinear_fusion_folded_bwd_workspace_bytes(B, N, L, H, R), folded_ws_bytes(B, N, L, H, R, knobs)
    assert nbytes == want, ("workspace bytes", nbytes, want)
    ws = _sentinel(nbytes // 4 + PAD)
    ws[:nbytes // 4] = NAN
    dx, dw, db, dh2 = _out(B * N * L) if want_dx else None, [_out(H * L) for _ in range(R)], [_out(H) for _ in range(R)], _out(B * R * H)
    tail = (_ptr(dv["g"], PAD), _ptr(dx, PAD) if want_dx else None, _pp(dw), _pp(db), _ptr(dh2, PAD), _ptr(ws), nbytes, B, N, L, H, R)
    if entry == "engine":
        rc, log = _call(ops, Lb.vqa_lowrank_bilinear_fusion_bwd, _ptr(dv["x"], PAD), ldx, _pp(dv["w1"]), _ptr(dv["h2"], PAD), _ptr(h1, PAD), *tail)
    else:
        head = (_ptr(dv["x"], PAD), ldx, _pp(dv["w1"]), _pp(dv["b1"]), _ptr(dv["h2"], PAD))
        if gate is None:
            rc, log = _call(ops, Lb.vqa_lowrank_bilinear_fusion_folded_bwd, *head, *tail)
        else:
            rc, log = _call(ops, Lb.vqa_lowrank_bilinear_fusion_folded_bwd_gated, *head, *tail, gate)
    if rc != 0:
        return rc, log, None
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    got = {"d_x": _win(dx, (B, N, L), "d_x") if want_dx else None, "d_h2": _win(dh2, (B, R, H), "d_h2"),
           "d_w1": torch.stack([_win(t, (H, L), "d_w1[%d]" % r) for r, t in enumerate(dw)]),
           "d_b1": torch.stack([_win(t, (H,), "d_b1[%d]" % r) for r, t in enumerate(db)])}
    return rc, log, got


def names(log):
    return [(name, grid) for _, name, grid in log]


def check_grads(what, got, ref, x=None):
    """x: the gate's operand (d_x must be the ungated gradient times (x > 0))"""
    for key in ("d_x", "d_w1", "d_b1", "d_h2"):
        if got[key] is None:
            continue
        want = ref[key] * (x > 0).to(F64) if key == "d_x" and x is not None else ref[key]
        assert_exact("%s %s" % (what, key), got[key], want)


# ======================================================================================================================= A: the engine
TILES = ((128, 128), (64, 128), (128, 64), (64, 64))


def _tile_knob(bm, bn, pf):
    return ("VQA_GEMM_TILE", "%dx%dx%d" % (bm, bn, pf))


# (id, B, N, L, H, R, ldx - L, knobs).  B N = 150 rows and H = 130 leave the last row and column tile of every tile shape partial
ENGINE_FWD_CASES = [("tile-%dx%dx%d" % (bm, bn, pf), 3, 50, 70, 130, 2, 0, (_tile_knob(bm, bn, pf),)) for bm, bn in TILES for pf in (1, 2, 3)]
ENGINE_FWD_CASES += [("tile-64x128-default-pf", 3, 50, 70, 130, 2, 0, (("VQA_GEMM_TILE", "64x128"),)), ("N1", 70, 1, 18, 34, 1, 0, ()),
                     ("R5", 3, 17, 18, 34, 5, 0, ()), ("R8", 2, 5, 18, 66, 8, 0, ()), ("ldx", 3, 50, 70, 130, 3, 2, ())]


@gpu
@pytest.mark.parametrize("case", ENGINE_FWD_CASES, ids=lambda c: c[0])
def test_engine_forward_small_integers_are_exact(ops, lib_option, case):
    """bilinear_fwd_kernel, without and with h1"""
    name, B, N, L, H, R, dl, knobs = case
    set_knobs(lib_option, knobs)
    amp = amplitude(B, N, L, H, R)
    ref = reference(B, N, L, H, R, amp, False, False, True)
    dv = to_dev(operands(B, N, L, H, R, amp, False), L + dl)
    for want_h1 in (False, True):
        rc, log, out, h1 = run_fwd(ops, "engine", dv, B, N, L, H, R, L + dl, want_h1)
        assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
        assert log == names(engine_fwd_log(B, N, L, H, R, dict(knobs))), (name, log)
        assert_exact(name + " out", _win(out, (B, N, H), "out"), ref["out"])
        if want_h1:
            assert_exact(name + " h1", _win(h1, (B, N, R, H), "h1"), ref["h1"])


FORM0, FORM1 = ("VQA_K4_DW_FORM", "0"), ("VQA_K4_DW_FORM", "1")
# (id, B, N, L, H, R, ldx - L, knobs, d_x asked for)
ENGINE_BWD_CASES = []
for _i, ((_bm, _bn), _pf) in enumerate((t, pf) for t in TILES for pf in (1, 2, 3)):
    ENGINE_BWD_CASES += [("tile-%dx%dx%d" % (_bm, _bn, _pf), 3, 50, 70, 130, 2 + _i % 3, 0, (_tile_knob(_bm, _bn, _pf),), True),
                         ("scaled-tile-%dx%dx%d" % (_bm, _bn, _pf), 3, 50, 70, 130, 1 + _i % 3, 0, (_tile_knob(_bm, _bn, _pf), FORM0), True)]
ENGINE_BWD_CASES += [
    ("sample-R3", 3, 24, 18, 34, 3, 0, (), True), ("sample-R4", 3, 36, 70, 66, 4, 0, (), True), ("sample-N24", 3, 24, 18, 34, 2, 0, (), True),
    # the scaled form by shape: ranks outside 2..4, and 17 regions in 32 padded rows (17 x 4 < 32 x 3; 24 x 4 = 32 x 3 is the per-sample form's)
    ("scaled-R1", 3, 24, 18, 34, 1, 0, (), True), ("scaled-R5", 3, 24, 18, 34, 5, 0, (), True), ("scaled-N17", 3, 17, 18, 34, 2, 0, (), True),
    ("form0-N24", 3, 24, 18, 34, 2, 0, (FORM0,), True), ("form1-N17", 3, 17, 18, 34, 2, 0, (FORM1,), True),
    ("form1-R5", 3, 24, 18, 34, 5, 0, (FORM1,), True), ("form1-R1", 3, 24, 18, 34, 1, 0, (FORM1,), True),
    # the slab count at both ends: one slab; four slabs for nine samples (3, 3, 3, 0); four slabs of the scaled form's 900 rows; one
    # slab asked for where 130 samples of 4 ranks need 3 to keep their question-side factors within 64 KB of LDS
    ("slabs-1-sample", 9, 24, 18, 34, 2, 0, (("VQA_K4_DW_SPLITS", "1"),), True), ("slabs-4-sample", 9, 24, 18, 34, 2, 0, (("VQA_K4_DW_SPLITS", "4"),), True),
    ("slabs-1-scaled", 9, 17, 18, 34, 2, 0, (("VQA_K4_DW_SPLITS", "1"),), False), ("slabs-4-scaled", 9, 100, 18, 34, 1, 0, (("VQA_K4_DW_SPLITS", "4"),), False),
    ("lds-bound", 130, 12, 18, 34, 4, 0, (("VQA_K4_DW_SPLITS", "1"),), False),
    ("ldx-sample", 3, 24, 18, 34, 2, 2, (), True), ("ldx-scaled", 3, 17, 18, 34, 2, 2, (), True), ("no-dx", 3, 24, 18, 34, 2, 0, (), False),
    ("N1", 70, 1, 18, 34, 2, 0, (), True),
]


@gpu
@pytest.mark.parametrize("case", ENGINE_BWD_CASES, ids=lambda c: c[0])
def test_engine_backward_small_integers_are_exact(ops, lib_option, case):
    """bilinear_dh2_kernel, bilinear_dx_kernel, one of the two weight-gradient kernels, bilinear_dw_reduce_kernel; h1 is the reference's"""
    name, B, N, L, H, R, dl, knobs, want_dx = case
    set_knobs(lib_option, knobs)
    amp = amplitude(B, N, L, H, R)
    ref = reference(B, N, L, H, R, amp, False, True, True)
    dv = to_dev(operands(B, N, L, H, R, amp, False), L + dl)
    rc, log, got = run_bwd(ops, "engine", dv, B, N, L, H, R, L + dl, dict(knobs), want_dx, h1=_in(ref["h1"]))
    assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
    assert log == names(engine_bwd_log(B, N, L, H, R, dict(knobs), want_dx)), (name, log)
    check_grads(name, got, ref)


# ======================================================================================================================= A: the folded entries
def _k(**kw):
    return tuple(("VQA_K4_" + k, str(v)) for k, v in kw.items())


# (id, B, N, L, H, R, ldx - L, knobs, calls): f the forward, b the backward with d_x, n the backward without, g the gated backward
# with d_x (ldx - L applies to f, b and n: the gate needs a dense x)
FOLDED_CASES = []
# the LDS-tile kernel: every (NB, R, W) forward, every (NB, R, W, OB) data gradient; B below the wave count and no multiple of it;
# L and H leave the last 64- (80-) wide output tile partial
_i = 0
for _nb, (_na, _nz) in ((1, (16, 16)), (2, (17, 32)), (3, (33, 48)), (5, (49, 80)), (7, (81, 112))):
    for _r in (1, 2, 3, 4) if _nb <= 3 else (1, 2):
        for _w in (4, 8):
            for _ob in (4, 5) if _nb <= 3 else (4,):
                _n = _na if (_w == 4) == (_ob == 4) else _nz
                _l, _h = (82, 66) if _i % 3 == 0 else (18, 34)
                FOLDED_CASES.append(("lds-NB%d-R%d-W%d-OB%d" % (_nb, _r, _w, _ob), 9 if _i % 2 == 0 else 3, _n, _l, _h, _r, 0,
                                     _k(FOLD_WAVES=_w, FOLD_OB=_ob), "fbg"))
                _i += 1
FOLDED_CASES += [
    ("natural-B512-N100", 512, 100, 18, 510, 2, 0, (), "f"), ("natural-small", 3, 36, 18, 34, 2, 0, (), "fbg"), ("lds-ldx", 9, 33, 82, 66, 2, 2, (), "fb"),
    # the register-tile forward (K = L >= 32, NO = H >= 64) and data gradient (K = H >= 32, NO = L >= 64): B = 256 and 257 (a group
    # of 4 / 2 samples past B), N = 17, 33, 48, R = 1, the fold bursts, a last column tile with NO % 4 == 2, a strided x
    ("rt-fwd-R1", 256, 17, 32, 64, 1, 0, (), "f"), ("rt-fwd-R2-B257", 257, 33, 32, 64, 2, 0, (), "f"), ("rt-fwd-fg1", 256, 48, 32, 64, 2, 0, _k(FG=1), "f"),
    ("rt-fwd-fg2", 256, 17, 32, 64, 2, 0, _k(FG=2), "f"), ("rt-fwd-fg4", 257, 33, 32, 64, 2, 0, _k(FG=4), "f"),
    ("rt-fwd-tail", 256, 17, 32, 258, 2, 0, (), "f"), ("rt-fwd-ldx", 257, 33, 32, 64, 2, 2, (), "f"), ("rt-fwd-R1-tail-ldx", 256, 48, 34, 66, 1, 2, (), "f"),
    ("rt-dx-R1", 256, 17, 66, 64, 1, 0, (), "b"), ("rt-dx-R2-B257", 257, 33, 66, 64, 2, 0, (), "b"), ("rt-dx-fg1", 256, 48, 66, 64, 2, 0, _k(FG=1), "b"),
    ("rt-dx-fg2", 256, 17, 66, 64, 2, 0, _k(FG=2), "b"), ("rt-dx-fg4", 257, 33, 66, 64, 2, 0, _k(FG=4), "b"), ("rt-dx-tail", 256, 17, 322, 64, 2, 0, (), "b"),
    # ... and its thresholds: the LDS-tile kernel on the other side of each
    ("rt-B255", 255, 17, 66, 64, 2, 0, (), "fb"), ("rt-N16", 256, 16, 66, 64, 2, 0, (), "fb"), ("rt-N49", 256, 49, 66, 64, 2, 0, (), "fb"),
    ("rt-off", 256, 17, 66, 64, 2, 0, _k(RT=0), "fb"), ("rt-gated", 256, 17, 66, 64, 2, 0, (), "g"),
    # the register-tile weight gradient: B = 65 gives 5 samples per half-group, three of the 16 half-groups empty
    ("dwrt-R1-N36", 64, 36, 258, 16, 1, 0, (), "n"), ("dwrt-R2-N36-B65", 65, 36, 318, 18, 2, 0, (), "n"), ("dwrt-R1-N100-B65", 65, 100, 318, 66, 1, 0, (), "n"),
    ("dwrt-R2-N100", 64, 100, 258, 16, 2, 0, (), "n"), ("dwrt-dx", 64, 36, 310, 66, 2, 0, (), "bg"),
    # ... and its thresholds: bilinear_dw_dh2_kernel on the other side of each (H = 770 at N = 36: 65 tiles leave 7 slabs, below the form's 8)
    ("dwrt-L256", 64, 36, 256, 16, 2, 0, (), "n"), ("dwrt-L320", 64, 36, 320, 16, 2, 0, (), "n"), ("dwrt-B63", 63, 36, 258, 16, 2, 0, (), "n"),
    ("dwrt-ldx", 64, 36, 258, 16, 2, 2, (), "b"), ("dwrt-off", 64, 36, 258, 16, 2, 0, _k(DW_RT=0), "n"), ("dwrt-H770", 64, 36, 258, 770, 2, 0, (), "n"),
    # the weight gradient's slab count: capped by B and by 64 (65 samples: 2 per slab, 31 slabs empty); one slab asked for where 130
    # samples of 4 ranks need 3
    ("dwdh2-lds-bound", 130, 36, 62, 64, 4, 0, _k(DW_SPLITS=1), "n"), ("dwdh2-ldx-N36", 7, 36, 62, 64, 2, 2, (), "b"), ("dwdh2-ldx-N17", 7, 17, 62, 64, 2, 2, (), "b"),
]
# bilinear_dw_dh2_kernel: one stage of 40 rows per sample at N = 33, 36, 40 with R <= 2, stages of 16 rows elsewhere
for _b in (1, 7, 65):
    FOLDED_CASES += [("dwdh2-B%d-N%d-R%d" % (_b, _n, _r), _b, _n, 62, 64, _r, 0, (), "n")
                     for _n, _r in ((33, 1), (36, 2), (40, 2), (16, 1), (17, 2), (32, 3), (41, 2), (48, 4), (112, 2), (36, 3), (36, 4))]
# two register sets in flight, and the three-stage 16-row form at N = 36
FOLDED_CASES += [("pf2-N36-R%d" % _r, 7, 36, 62, 64, _r, 0, _k(FOLD_DW_PF=2), "n") for _r in (1, 2, 3, 4)]
FOLDED_CASES += [("pf2-N17-R%d" % _r, 9, 17, 62, 64, _r, 0, _k(FOLD_DW_PF=2), "n") for _r in (1, 2, 3, 4)]
FOLDED_CASES += [("pf2-bk16-R%d" % _r, 7, 36, 62, 64, _r, 0, _k(FOLD_DW_PF=2, FOLD_DW_BK=16), "n") for _r in (1, 2)]
FOLDED_CASES += [("bk16-R%d" % _r, 7, 36, 62, 64, _r, 0, _k(FOLD_DW_BK=16), "n") for _r in (1, 2)]
# the split engine: LBW = ceil((L + 1) / 64) = 1..5 on both sides of every block edge (at L = 64, 128, 192, 256 the bias-gradient
# column L opens a block of its own); B = 65: 5 samples per slab, three of the 16 slabs empty; B = 512: the form's largest batch
SPLIT = _k(DW_SPLIT=1)
FOLDED_CASES += [("split-L%d" % _l, (64, 65, 512, 65, 64)[_i % 5], 36, _l, (16, 18, 66)[_i % 3], 2, 0, SPLIT, "b" if _i % 4 == 1 else "n")
                 for _i, _l in enumerate((2, 62, 64, 126, 128, 190, 192, 254, 256, 318))]
# ... and its thresholds: outside the form the fp32 kernels run
FOLDED_CASES += [("split-L320", 64, 36, 320, 16, 2, 0, SPLIT, "n"), ("split-B513", 513, 36, 62, 16, 2, 0, SPLIT, "n"),
                 ("split-N35", 64, 35, 62, 16, 2, 0, SPLIT, "n"), ("split-R1", 64, 36, 62, 16, 1, 0, SPLIT, "n"), ("split-ldx", 64, 36, 62, 16, 2, 2, SPLIT, "n")]
FOLDED_BY_ID = {c[0]: c for c in FOLDED_CASES}


def folded_calls(case):
    """-> [(call, ldx, expected log)] of a case"""
    name, B, N, L, H, R, dl, knobs, calls = case
    kn = dict(knobs)
    plan = []
    for c in calls:
        ldx = L if c == "g" else L + dl
        plan.append((c, ldx, folded_fwd_log(B, N, L, H, R, ldx, kn) if c == "f" else folded_bwd_log(B, N, L, H, R, ldx, kn, c != "n", c == "g")))
    return plan


@gpu
@pytest.mark.parametrize("case", FOLDED_CASES, ids=lambda c: c[0])
def test_folded_small_integers_are_exact(ops, lib_option, case):
    name, B, N, L, H, R, dl, knobs, calls = case
    assert len(FOLDED_BY_ID) == len(FOLDED_CASES)
    Lb = ops._lib.lib()
    set_knobs(lib_option, knobs)
    nonneg = "g" in calls
    amp = amplitude(B, N, L, H, R)
    host = operands(B, N, L, H, R, amp, nonneg)
    ref = reference(B, N, L, H, R, amp, nonneg, calls != "f", False)
    assert Lb.vqa_lowrank_bilinear_fusion_folded_supported(B, N, L, H, R) == 1
    bufs = {}
    for c, ldx, want_log in folded_calls(case):
        dv = bufs.setdefault(ldx, to_dev(host, ldx))
        what = "%s %s" % (name, c)
        if c == "f":
            rc, log, out, _ = run_fwd(ops, "folded", dv, B, N, L, H, R, ldx)
            assert rc == 0, (what, rc, Lb.vqa_last_error())
            assert log == names(want_log), (what, log)
            assert_exact(what + " out", _win(out, (B, N, H), "out"), ref["out"])
            continue
        # (the ungated call goes through the plain entry at an odd B and through the gated entry with gate_dx = 0 at an even one)
        gate = 1 if c == "g" else (None if B % 2 else 0)
        rc, log, got = run_bwd(ops, "folded", dv, B, N, L, H, R, ldx, dict(knobs), c != "n", gate)
        assert rc == 0, (what, rc, Lb.vqa_last_error())
        assert log == names(want_log), (what, log)
        check_grads(what, got, ref, host[0] if c == "g" else None)


def all_expected_logs():
    """every (site, spelled name, grid) that a section A case expects -- needs no GPU"""
    logs = []
    for name, B, N, L, H, R, dl, knobs in ENGINE_FWD_CASES:
        logs += engine_fwd_log(B, N, L, H, R, dict(knobs))
    for name, B, N, L, H, R, dl, knobs, want_dx in ENGINE_BWD_CASES:
        logs += engine_bwd_log(B, N, L, H, R, dict(knobs), want_dx)
    for case in FOLDED_CASES:
        for _, _, log in folded_calls(case):
            logs += log
    return logs


def test_case_tables_stay_exact():
    """every section A case: the chosen amplitude keeps every sum below 2^24 (3 wherever 3 does), and its shape is one the entry takes"""
    for case in ENGINE_FWD_CASES + ENGINE_BWD_CASES + FOLDED_CASES:
        B, N, L, H, R = case[1:6]
        a = amplitude(B, N, L, H, R)
        _below_2_24(*bounds(B, N, L, H, R, a))
        assert a == 3 or max(bounds(B, N, L, H, R, a + 1)) >= 2 ** 24
        assert L % 2 == 0 and H % 2 == 0 and case[6] % 2 == 0 and R <= 8
    assert bounds(2, 5, 10, 20, 2, 3) == (2 * 93 * 3, 2 * 20 * 27, 2 * 5 * 27, 2 * 5 * 9, 5 * 3 * 93)
    assert amplitude(512, 36, 310, 510, 2) == 3 and amplitude(8192, 100, 310, 510, 2) == 2
    for case in FOLDED_CASES:
        B, N, L, H, R = case[1:6]
        assert N <= 112 and R <= (4 if N <= 48 else 2)


def _log_of(cid, call):
    return [n for c, _, log in folded_calls(FOLDED_BY_ID[cid]) if c == call for _, n, _ in log]


def test_thresholds_have_both_sides():
    """what the case tables promise, checked on the restated dispatchers (the GPU tests check the restatement against the library)"""
    # the exact-160 KB workgroup: N = 112, R = 2, 8 waves fits the forward to the byte and not the data gradient
    assert folded_lds_bytes(112, 2, True, 8) == 160 * 1024 < folded_lds_bytes(112, 2, False, 8)
    assert _log_of("lds-NB7-R2-W8-OB4", "f") == ["(bilinear_folded_kernel<7,2,H2_ROWS,8,4>)"]
    assert _log_of("lds-NB7-R2-W8-OB4", "b")[1] == "(bilinear_folded_kernel<7,2,H2_ROWS,4,4>)"
    assert FOLDED_BY_ID["lds-NB7-R2-W8-OB4"][2] == 112
    # the natural picks
    assert _log_of("natural-B512-N100", "f") == ["(bilinear_folded_kernel<7,2,H2_ROWS,8,4>)"]
    assert _log_of("natural-small", "f") == ["(bilinear_folded_kernel<3,2,H2_ROWS,4,4>)"]
    # register-tile forward and data gradient against the LDS-tile kernel
    for cid, call, rt in (("rt-fwd-R2-B257", "f", True), ("rt-dx-R2-B257", "b", True), ("rt-B255", "f", False), ("rt-B255", "b", False),
                          ("rt-N16", "f", False), ("rt-N16", "b", False), ("rt-N49", "f", False), ("rt-N49", "b", False),
                          ("rt-off", "f", False), ("rt-off", "b", False), ("rt-gated", "g", False), ("rt-fwd-ldx", "f", True)):
        assert any("bilinear_fold_rt_kernel" in n for n in _log_of(cid, call)) == rt, (cid, call)
        assert any("bilinear_folded_kernel" in n for n in _log_of(cid, call)) != rt, (cid, call)
    assert _log_of("rt-fwd-R2-B257", "f") == [S_RT24] and _log_of("rt-dx-R2-B257", "b")[1] == S_RT22
    assert _log_of("rt-fwd-fg1", "f") == [S_RT2] and _log_of("rt-dx-fg1", "b")[1] == S_RT2 and _log_of("rt-dx-R1", "b")[1] == S_RT1
    # register-tile and split-engine weight gradient against bilinear_dw_dh2_kernel
    for cid, form in (("dwrt-R1-N36", "dw_rt"), ("dwrt-R2-N100", "dw_rt"), ("dwrt-L256", "dw_dh2"), ("dwrt-L320", "dw_dh2"), ("dwrt-B63", "dw_dh2"),
                      ("dwrt-ldx", "dw_dh2"), ("dwrt-off", "dw_dh2"), ("dwrt-H770", "dw_dh2"), ("split-L2", "dw_split"), ("split-L318", "dw_split"),
                      ("split-L320", "dw_dh2"), ("split-B513", "dw_dh2"), ("split-N35", "dw_dh2"), ("split-R1", "dw_dh2"), ("split-ldx", "dw_dh2")):
        call = FOLDED_BY_ID[cid][8][0]
        assert "bilinear_%s_kernel" % form in _log_of(cid, call)[-2], (cid, _log_of(cid, call))
    assert dw_fold_splits(64, 36, 770, 258, 2, {}) == 7 and dw_fold_splits(64, 36, 768, 258, 2, {}) == 8
    assert [(L + 64) // 64 for L in (2, 62, 64, 126, 128, 190, 192, 254, 256, 318)] == [1, 1, 2, 2, 3, 3, 4, 4, 5, 5]
    # slab counts: capped by B and by 64; raised by the 64 KB of question-side factors
    assert dw_fold_splits(65, 36, 64, 62, 2, {}) == 64 and dw_fold_splits(7, 36, 64, 62, 2, {}) == 7
    assert dw_fold_splits(130, 36, 64, 62, 4, {"VQA_K4_DW_SPLITS": "1"}) == 3 == engine_slabs(130, 12, 18, 34, 4, {"VQA_K4_DW_SPLITS": "1"})
    assert engine_slabs(9, 24, 18, 34, 2, {"VQA_K4_DW_SPLITS": "4"}) == 4 == engine_slabs(9, 100, 18, 34, 1, {"VQA_K4_DW_SPLITS": "4"})
    assert dw_per_sample(24, 2, {}) and not dw_per_sample(17, 2, {}) and not dw_per_sample(24, 1, {"VQA_K4_DW_FORM": "1"})


def test_case_tables_reach_every_instantiation():
    """beyond the launch sites: every template instantiation the dispatchers can pick is the spelled form of some case"""
    seen = {n for _, n, _ in all_expected_logs()}
    want = {spell(s, bm, bn, pf) for s in (S_FWD, S_DX, S_DW) for bm, bn in TILES for pf in (1, 2, 3)}
    want |= {spell(S_DWS, bm, bn, pf, 2 + i % 3) for i, ((bm, bn), pf) in enumerate((t, pf) for t in TILES for pf in (1, 2, 3))}
    want |= {spell(S_DWS, 64, 64, 2, r) for r in (2, 3, 4)}
    for nb in (1, 2, 3, 5, 7):
        for r in (1, 2, 3, 4) if nb <= 3 else (1, 2):
            # (forward and data gradient share the spelling: H2_ROWS is a template parameter of the launcher, not of the macro)
            want |= {spell(S_FOLD, nb, r, w, ob) for w in (4, 8) for ob in ((4, 5) if nb <= 3 else (4,))}
    want |= {spell(S_DWDH2, pf, r, bk) for pf in (1, 2) for r in (1, 2, 3, 4) for bk in ((16, 40) if r <= 2 else (16,))}
    want |= {spell(S_DWRT, r, ns) for r in (1, 2) for ns in (9, 25)} | {spell(S_SPLIT, lbw) for lbw in (1, 2, 3, 4, 5)}
    want |= {S_RT1, S_RT22, S_RT24, S_RT2, S_TR, S_DH2, S_DWRED, S_RED}
    assert want - seen == set(), "instantiations that no case launches"


# ======================================================================================================================= B
SPLIT_BAR = 2e-5      # test_lowrank_bilinear_fusion_large_batch_against_torch_fp64's bar for the split engine's gradients
# (id, entry, B, N, L, H, R, knobs, forward form, forms that must be in the backward's log)
RANDOM_CASES = [
    ("engine", "engine", 3, 50, 70, 130, 2, (), "bilinear_fwd_kernel", ("bilinear_dx_kernel", "bilinear_dw_sample_kernel")),
    ("engine-scaled", "engine", 9, 17, 70, 130, 3, (), "bilinear_fwd_kernel", ("bilinear_dx_kernel", "(bilinear_dw_kernel")),
    ("folded-lds", "folded", 9, 36, 82, 66, 2, (), "bilinear_folded_kernel", ("bilinear_folded_kernel", "bilinear_dw_dh2_kernel")),
    ("folded-lds-N100", "folded", 5, 100, 82, 66, 2, (), "bilinear_folded_kernel", ("bilinear_folded_kernel", "bilinear_dw_dh2_kernel")),
    ("rt", "folded", 256, 36, 66, 64, 2, (), "bilinear_fold_rt_kernel", ("bilinear_fold_rt_kernel", "bilinear_dw_dh2_kernel")),
    ("dw_rt", "folded", 64, 36, 310, 66, 2, (), "bilinear_folded_kernel", ("bilinear_dw_rt_kernel",)),
    ("dw_rt-N100-R1", "folded", 65, 100, 318, 18, 1, (), "bilinear_folded_kernel", ("bilinear_dw_rt_kernel",)),
    ("dw_split", "folded", 64, 36, 310, 66, 2, SPLIT, "bilinear_folded_kernel", ("bilinear_dw_split_kernel",)),
    ("dw_split-L62-B512", "folded", 512, 36, 62, 18, 2, SPLIT, "bilinear_folded_kernel", ("bilinear_dw_split_kernel",)),
    ("dw_dh2", "folded", 65, 36, 62, 64, 2, (), "bilinear_folded_kernel", ("bilinear_dw_dh2_kernel",)),
    ("dw_dh2-N17-R4", "folded", 7, 17, 62, 64, 4, (), "bilinear_folded_kernel", ("bilinear_dw_dh2_kernel",)),
]


@gpu
@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: c[0])
def test_random_operands_against_float64(ops, lib_option, measured, case):
    import oracle.kernels_np as knp
    name, entry, B, N, L, H, R, knobs, f_form, b_forms = case
    set_knobs(lib_option, knobs)
    gen = torch.Generator().manual_seed(7 * B + 11 * N + L + H + R)
    host = (torch.randn(B, N, L, generator=gen), torch.randn(R, H, L, generator=gen) / L ** 0.5, 0.1 * torch.randn(R, H, generator=gen),
            torch.randn(B, R, H, generator=gen), torch.randn(B, N, H, generator=gen))
    np_in = [t.numpy() for t in host]
    out64, h164 = knp.lowrank_bilinear_fusion_fwd(*np_in[:4])
    ref64 = dict(zip(("out", "h1", "d_x", "d_w1", "d_b1", "d_h2"), (torch.from_numpy(np.ascontiguousarray(a)) for a in
                                                                    (out64, h164) + tuple(knp.lowrank_bilinear_fusion_bwd(*np_in)))))
    ref32 = formulas(*host, keep_h1=True)
    dv = to_dev(host, L)
    rc, log, out, h1 = run_fwd(ops, entry, dv, B, N, L, H, R, L, entry == "engine")
    assert rc == 0 and len(log) == 1 and f_form in log[0][0], (name, rc, log)
    h1 = _win(h1, (B, N, R, H), "h1") if entry == "engine" else None
    rc, blog, got = run_bwd(ops, entry, dv, B, N, L, H, R, L, dict(knobs), True, None, _in(h1.cpu()) if h1 is not None else None)
    assert rc == 0 and all(any(f in n for n, _ in blog) for f in b_forms), (name, rc, blog)
    bars = Bars(measured, name)
    bars.check("out", _win(out, (B, N, H), "out"), ref64["out"], ref32["out"])
    if h1 is not None:
        bars.check("h1", h1, ref64["h1"], ref32["h1"])
    split = "dw_split" in name
    for key in ("d_x", "d_w1", "d_b1", "d_h2"):
        bars.check(key, got[key], ref64[key], ref32[key], SPLIT_BAR if split and key != "d_x" else None)
    bars.close()


# ======================================================================================================================= C
# (id, entry, B, N, L, H, R, knobs, the weight-gradient form that must run)
ISOLATION_CASES = [
    ("engine", "engine", 3, 24, 18, 34, 2, (), "bilinear_dw_sample_kernel"), ("engine-scaled", "engine", 3, 17, 18, 34, 2, (), "(bilinear_dw_kernel"),
    # 17 regions in two blocks of 16: the region blocks past N run on a duplicate of the last row, the one that holds the NaN
    ("folded-lds", "folded", 9, 17, 18, 34, 2, (), "bilinear_dw_dh2_kernel"), ("folded-lds-N49", "folded", 3, 49, 18, 34, 2, (), "bilinear_dw_dh2_kernel"),
    ("rt", "folded", 256, 17, 66, 64, 2, (), "bilinear_dw_dh2_kernel"), ("dw_rt", "folded", 64, 36, 258, 16, 2, (), "bilinear_dw_rt_kernel"),
    ("dw_split", "folded", 64, 36, 62, 16, 2, SPLIT, "bilinear_dw_split_kernel"),
]


@gpu
@pytest.mark.parametrize("case", ISOLATION_CASES, ids=lambda c: c[0])
def test_a_nan_stays_in_its_sample(ops, lib_option, case):
    """one NaN in the first region of x[1], one in its last region, then one in g[1]: out, d_x and d_h2 of every other sample are those
    of the clean run, bit for bit, and the NaN does arrive in its own sample (d_w1 and d_b1 sum over the samples and are not
    asserted).  The first row of a sample lies behind the last row of the one before: a kernel that reads a row past column L meets it"""
    name, entry, B, N, L, H, R, knobs, w_form = case
    set_knobs(lib_option, knobs)
    host = operands(B, N, L, H, R, 3, False)
    ref = reference(B, N, L, H, R, 3, False, True, True)
    h1 = _in(ref["h1"]) if entry == "engine" else None
    others = [b for b in range(B) if b != 1]
    for dirty, region in (("x", 0), ("x", N - 1), ("g", N - 1)):
        x, g = host[0].clone(), host[4].clone()
        (x if dirty == "x" else g)[1, region, 5] = NAN
        dv = to_dev((x,) + host[1:4] + (g,), L)
        rc, log, out, _ = run_fwd(ops, entry, dv, B, N, L, H, R, L)
        assert rc == 0 and len(log) == 1, (name, rc, log)
        rc, blog, got = run_bwd(ops, entry, dv, B, N, L, H, R, L, dict(knobs), True, None, h1)
        assert rc == 0 and any(w_form in n for n, _ in blog), (name, rc, blog)
        out = _win(out, (B, N, H), "out")
        for key, have in (("out", out), ("d_x", got["d_x"]), ("d_h2", got["d_h2"])):
            assert torch.equal(have[others].cpu().to(F64), ref[key][others]), "%s: the NaN in %s[1] reached %s of another sample" % (name, dirty, key)
        hit = out[1] if dirty == "x" else got["d_x"][1]
        assert bool(torch.isnan(hit).any()), "the NaN in %s[1] did not reach its own sample" % dirty
        # (the engine's d_h2 reads the saved h1, which is the clean one here)
        assert entry == "engine" and dirty == "x" or bool(torch.isnan(got["d_h2"][1]).any())


@gpu
def test_the_gate_zeroes_d_x_at_a_nan_x(ops):
    """gate_dx keeps d_x where x > 0: at x = NaN (and at x = 0 and x < 0) d_x is 0, everywhere else it is the ungated gradient -- on the
    LDS-tile kernel, the only one that gates"""
    B, N, L, H, R = 9, 17, 18, 34, 2
    host = operands(B, N, L, H, R, 3, False)
    ref = reference(B, N, L, H, R, 3, False, True, False)
    x = host[0].clone()
    x[2, 3, 4], x[0, 16, 17] = NAN, NAN
    assert float(ref["d_x"][2, 3, 4]) != 0.0 and float(ref["d_x"][0, 16, 17]) != 0.0 and bool((x < 0).any()) and bool((x == 0).any())
    rc, log, got = run_bwd(ops, "folded", to_dev((x,) + host[1:], L), B, N, L, H, R, L, {}, True, 1)
    assert rc == 0 and "bilinear_folded_kernel" in log[1][0], (rc, log)
    assert_exact("gated d_x", got["d_x"], ref["d_x"] * (x > 0).to(F64))
    assert bool(torch.isnan(got["d_h2"][2]).any()) and bool(torch.isfinite(got["d_h2"][[1, 3, 4, 5, 6, 7, 8]]).all())


@gpu
def test_refusals_launch_nothing(ops, lib_option):
    """null pointers, a rank pointer null or misaligned, a workspace one byte short: VQA_E_BADARG; sizes <= 0: VQA_E_BADARG from the engine
    entries, VQA_E_UNSUPPORTED from the folded ones (the shape is outside the folded form); odd L, H or ldx, ldx < L, R = 9, a misaligned
    tensor, the folded entries at N = 113, R = 5, N = 49 with R = 3, the gated entry with ldx != L when d_x is asked for:
    VQA_E_UNSUPPORTED.  An error text, no launch, the outputs untouched.  Every buffer is as large as the refused call would have needed"""
    Lb = ops._lib.lib()
    n = 1 << 18
    src = torch.zeros(n, device=dev())
    outs = [_sentinel(n) for _ in range(4)]
    ws = _sentinel(1 << 22)
    logbuf = (ctypes.c_ulonglong * 16)()
    E_WS, F_WS = Lb.vqa_lowrank_bilinear_fusion_bwd_workspace_bytes, Lb.vqa_lowrank_bilinear_fusion_folded_bwd_workspace_bytes

    def refused(code, fn, *args):
        Lb.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, args[-7:], Lb.vqa_last_error())
        assert Lb.vqa_last_error() and Lb.vqa_launch_log(logbuf, 16) == 0, ("a refused call launched a kernel", fn.__name__, args[-7:])

    def pp(t, R, bad=None, off=0):
        """R rank pointers into t; rank `bad` NULL (off = 0) or `off` bytes past an 8-byte boundary"""
        v = [t.data_ptr() + 4096 * r for r in range(max(R, 1))]
        if bad is not None:
            v[bad] = v[bad] + off if off else None
        return (ctypes.c_void_p * len(v))(*v)

    def fwd(folded, B=2, N=5, L=8, H=6, R=2, ldx=None, null=None, mis=None, rank=None):
        ldx = L if ldx is None else ldx
        ptrs = [_ptr(src), pp(src, R), pp(src, R), _ptr(src), _ptr(outs[0])]
        if rank is not None:
            ptrs[rank[0]] = pp(src, R, R - 1, rank[1])
        if null is not None:
            ptrs[null] = None
        if mis is not None:
            ptrs[mis] = ctypes.c_void_p(ptrs[mis].value + 4)
        if folded:
            return (Lb.vqa_lowrank_bilinear_fusion_folded_fwd, ptrs[0], ldx, *ptrs[1:], B, N, L, H, R)
        return (Lb.vqa_lowrank_bilinear_fusion_fwd, ptrs[0], ldx, *ptrs[1:], _ptr(outs[1]), B, N, L, H, R)

    def bwd(folded, B=2, N=5, L=8, H=6, R=2, ldx=None, null=None, mis=None, rank=None, short=0, gate=None):
        ldx = L if ldx is None else ldx
        # x, w1, (h2, h1 | b1, h2), g, d_x, d_w1, d_b1, d_h2, workspace
        ptrs = [_ptr(src), pp(src, R), _ptr(src), _ptr(src), _ptr(src), _ptr(outs[0]), pp(outs[1], R), pp(outs[2], R), _ptr(outs[3]), _ptr(ws)]
        if folded:
            ptrs[2] = pp(src, R)
        if rank is not None:
            ptrs[rank[0]] = pp(outs[1] if rank[0] == 6 else outs[2] if rank[0] == 7 else src, R, R - 1, rank[1])
        if null is not None:
            ptrs[null] = None
        if mis is not None:
            ptrs[mis] = ctypes.c_void_p(ptrs[mis].value + 4)
        need = (F_WS if folded else E_WS)(B, N, L, H, R)
        assert need <= 4 * ws.numel() and max(B * N * max(ldx, H), B * R * H, 1) <= n and H * L <= 1024
        args = (ptrs[0], ldx, *ptrs[1:], (need or 4 * ws.numel()) - short, B, N, L, H, R)
        if not folded:
            return (Lb.vqa_lowrank_bilinear_fusion_bwd, *args)
        return (Lb.vqa_lowrank_bilinear_fusion_folded_bwd, *args) if gate is None else (Lb.vqa_lowrank_bilinear_fusion_folded_bwd_gated, *args, gate)

    for folded in (False, True):
        for i in range(5):
            refused(E_BADARG, *fwd(folded, null=i))
        for i in (0, 1, 2, 3, 4, 6, 7, 8, 9):            # (5 is d_x, which may be NULL)
            refused(E_BADARG, *bwd(folded, null=i))
        for kw in (dict(B=0), dict(N=0), dict(L=0), dict(H=-2), dict(R=0), dict(B=-1)):
            refused(E_UNSUPPORTED if folded else E_BADARG, *fwd(folded, **kw))
            refused(E_UNSUPPORTED if folded else E_BADARG, *bwd(folded, **kw))
        for kw in (dict(L=7), dict(H=5), dict(ldx=9), dict(ldx=6), dict(R=9), dict(mis=0), dict(mis=3)):
            refused(E_UNSUPPORTED, *fwd(folded, **kw))
            refused(E_UNSUPPORTED, *bwd(folded, **kw))
        refused(E_UNSUPPORTED, *fwd(folded, mis=4))                              # out
        for i in (4, 5, 8, 9):                                                   # g, d_x, d_h2, the workspace (16 bytes)
            refused(E_UNSUPPORTED, *bwd(folded, mis=i))
        refused(E_BADARG, *fwd(folded, rank=(1, 0)))                             # w1[R - 1] NULL, then misaligned
        refused(E_BADARG, *fwd(folded, rank=(1, 4)))
        refused(E_BADARG, *fwd(folded, rank=(2, 0)))                             # b1[R - 1] NULL
        for i in (1, 6, 7):
            refused(E_BADARG, *bwd(folded, rank=(i, 0)))
            refused(E_BADARG, *bwd(folded, rank=(i, 4)))
        refused(E_BADARG, *bwd(folded, short=1))
    for kw in (dict(N=113), dict(R=5), dict(N=49, R=3)):
        assert Lb.vqa_lowrank_bilinear_fusion_folded_supported(2, kw.get("N", 5), 8, 6, kw.get("R", 2)) == 0
        assert F_WS(2, kw.get("N", 5), 8, 6, kw.get("R", 2)) == 0
        refused(E_UNSUPPORTED, *fwd(True, **kw))
        refused(E_UNSUPPORTED, *bwd(True, **kw))
        refused(E_UNSUPPORTED, *bwd(True, gate=1, **kw))
    assert Lb.vqa_lowrank_bilinear_fusion_folded_supported(2, 112, 8, 6, 2) == 1 and Lb.vqa_lowrank_bilinear_fusion_folded_supported(2, 48, 8, 6, 4) == 1
    assert E_WS(0, 5, 8, 6, 2) == 0 and E_WS(2, 5, 8, 6, 9) == 0 and F_WS(2, 5, 8, 5, 2) == 0
    # the gate needs a dense x when d_x is asked for -- and only then
    refused(E_UNSUPPORTED, *bwd(True, ldx=10, gate=1))
    torch.cuda.synchronize()
    for t in outs:
        assert _untouched(t)
    assert _untouched(ws)
    call = bwd(True, ldx=10, gate=1, null=5)
    Lb.vqa_launch_log_reset()
    assert call[0](*call[1:], None) == 0 and Lb.vqa_launch_log(logbuf, 16) == 2
    torch.cuda.synchronize()


# ======================================================================================================================= D
def test_every_launch_site_is_declared():
    """a launch site added to (or renamed in) one of the five files without a case here fails; so does a case whose site no longer
    exists.  The diagnostic VQA_K4_DW_TUNE site is declared and not launched"""
    sites = [s for f in K4_FILES for s in launch_sites(os.path.join(CSRC, f))]
    assert len(sites) == 19, sites
    assert sites.count(S_RED) == 3 and sites.count(S_DWRT_TUNE) == 1
    declared = {site for site, _, _ in all_expected_logs()} | {S_DWRT_TUNE}
    assert set(sites) - declared == set(), "launch sites that no case declares"
    assert declared - set(sites) == set(), "declared forms that no launch site has"
