"""Every launch form of the fused dropout-linear, K5 (csrc/linear_act.hip, linear_split.hip; engines in gemm_f32_mfma.hpp,
gemm_f32_rt.hpp, gemm_f32_split.hpp), through the C ABI, one dispatch form at a time.  tests/test_gpu_kernels.py reaches the LDS-tile
kernels up to M = 700 and the other engines at the workload's full shape only, under a loose relative bar, and never says which
kernel ran; here every VQA_LAUNCH site is launched, the launch log (kernel expression as the log spells it -- macro parameters
substituted -- and grid in work-items, restated from M, K, N, ldx, p, the knobs and the dispatchers' arithmetic) says that it was,
and its result is compared whole.

  A  small-integer operands (|x|, |w|, |b|, |gy|, |v|, |t|, |c2| <= 3, with zeros; p in {0, 0.5, 0.75}: scales 1, 2, 4): every fp32
     product and partial sum of every form is an integer below 2^24 (asserted per case from the operands' magnitudes, on the CPU as
     well: test_case_tables_stay_exact), so any order of summation, the K split over two waves, the slab reductions and the split
     engine's three bf16 planes give the same bits.  The reference is oracle/kernels_np.py's linear_act_fwd / linear_act_bwd formula
     in float64 with torch on the CPU (tied to the oracle in test_reference_is_the_oracle), fed the mask that vqa_linear_dropout_mask
     writes for the same (seed, M, K); the fused relation forms get t + c2 v formed in float64 first.  y is an exact integer, so the
     relu gate y > 0 is unambiguous.  Outputs sit in sentinel-filled buffers that are compared whole, inputs in NaN-padded ones
     (ldx > K leaves a NaN gap behind every row of x), the workspace is exactly *_workspace_bytes long (restated here), NaN-filled,
     with a sentinel fence behind it.  d_x = NULL, d_b = NULL, bias = NULL, gz_out present / absent each appear.
  B  random operands against float64 (oracle/kernels_np.py; the exported mask; the kernel's own y as the gate) under the project's
     bar (Bars of tests/kernel_harness.py): four times the error of the same formula in float32 with torch on the CPU
     plus one float32 ulp of the tensor's largest magnitude.  The split engine reports against the same bar and is held to it or to
     the bar tests/test_gpu_split.py states for it (2e-5 of the largest magnitude).  One case runs p = 0.3.
  C  a NaN in a row of x or gy stays in that row of y / d_x (rows at tile and split edges); a NaN in a DROPPED element of x: the
     register-tile and split engines mask by bit-and / select and never see it (y and d_w are the clean run's), the LDS-tile kernels
     multiply by 0 and hand the NaN on to the row of y and the column of d_w (pinned as it is); every VQA_REQUIRE of the ten entry
     points returns its code, launches nothing and leaves the outputs alone.
  D  no GPU: test_every_launch_site_is_declared (all 33 VQA_LAUNCH first arguments of the two files are the form of some case and
     the reverse), the restated dispatchers at hand-worked thresholds, empty splits exactly where a case says so.

What this file found:
  * rt::gemm_tn_kernel on an EMPTY row split (m_lo >= M; reachable through VQA_RT_DW_SPLITS only: the default never has S > 16 at
    M >= 4096) skipped its main loop and then ran its row tail from m_lo + 16 ((m_hi - m_lo) >> 4), below M: the last M % 16 rows
    were contracted once more per empty split into d_w and d_b ([rtdw-M4100-S64]: M = 4100, 64 splits asked for, 80 rows each, 12 of
    them empty).  Fixed on the host: vqa_linear_act_bwd caps S at ceil(M / rows_per_split) after rounding rows_per_split, so no
    empty split is launched (52 here); the workspace query keeps the larger figure.  Seen on the GPU before the fix, at both
    [rtdw-M4100-S64*] cases: d_w and d_b were off by exactly 12 times the contribution of the rows 4096..4099.
  * choose_tile(M, N, 1) cannot leave 64 x 64: a larger tile's preference factor (>= 1.15) always outweighs its fewer rounds (its
    tile count is at least a quarter / a half of the 64 x 64 one).  The issue's "choose_tile's own choice at a shape where it is not
    64 x 64" does not exist for K5; test_dispatchers_at_their_thresholds sweeps the arithmetic and says so.  The other tiles run
    under VQA_GEMM_TILE / VQA_LINEAR_DW_TILE.

Dispatch form (as the source spells the launch site) -> the test that launches it and asserts that it did:

  linear_act.hip
  (linear_fwd_kernel<BM_,BN_,PF_,false>), <..,true>   test_plain_small_integers_are_exact [tile-*] (four tiles x PF 1, 2, 3 under VQA_GEMM_TILE,
                                                      each without and with dropout, p = 0.5 and 0.75), [lds-*], the LDS side of the [rtf-*] thresholds
  (linear_dx_kernel<BM_,BN_,PF_,false>), <..,true>    ... the 'b' / 'z' call of [tile-*], [lds-*], [rtdw-dx*]
  (linear_dw_kernel<BM_,BN_,PF_,false>), <..,true>    ... [tile-*] (VQA_LINEAR_DW_TILE, another tile than the forward's), [lds-M256], [lds-M257],
                                                      [lds-S1], [lds-Scut], [lds-empty] (3 of 64 splits empty), [rtdw-M4095]
  linear_dw_reduce_kernel (LDS-tile site)             the last launch of those; N K / 2 = 256 ([lds-red256]) and 258 ([lds-red258])
  (rt::gemm_nt_kernel<9,5,1,2,2,false,EpiBiasAct>)    ... [rtf-M1152], [rtf-M1153], [rtf-K64], [rtf-K68], [rtf-K80], [rtf-N2], [rtf-N160], [rtf-N162]
  (rt::gemm_nt_kernel<9,5,1,2,2,true,EpiBiasAct>)     ... [rtf-K64-drop], [rtf-K96-drop], [rtf-ldx-drop], [rtf-M1153-drop]
  (rt::gemm_tn_kernel<5,2,true,true,true,1>)          ... [rtdw-gate-drop-share], [rtdw-M4100-S64], [rtdw-dx-drop]
  (rt::gemm_tn_kernel<5,2,false,true,true>)           ... [rtdw-drop-share]
  (rt::gemm_tn_kernel<5,2,true,true>)                 ... [rtdw-gate-drop-K96], [rtdw-gate-drop-noshare] (VQA_RT_SHARE_HASH=0)
  (rt::gemm_tn_kernel<5,2,true,false>)                ... [rtdw-gate], [rtdw-K132], [rtdw-N322]
  (rt::gemm_tn_kernel<5,2,false,true>)                ... [rtdw-drop-K96], [rtdw-drop-noshare]
  (rt::gemm_tn_kernel<5,2,false,false>)               ... [rtdw-M4096], [rtdw-M4100], [rtdw-N2], [rtdw-S1], [rtdw-red256]
  linear_dw_reduce_kernel (register-tile site)        the last launch of every [rtdw-*] but [rtdw-M4095]; N K / 2 = 256 in [rtdw-red256]
  linear_mask_kernel                                  test_mask_kernel, and the mask of every case with dropout

  linear_split.hip
  (sp::split_pack_kernel<false>) (two sites)          the first launch of every split forward [spf-*] and fused relation forward [rel-*]
  (sp::gemm_nt_kernel<9,5,1,2,2,false,SplitEpiBiasAct,0,3>), <..,true,..>   test_split_small_integers_are_exact [spf-*] / [spf-*-drop]
  (sp::gemm_nt_kernel<..,false,SplitEpiBiasAct,0,3,false,true>), <..,true,..>   test_relation_small_integers_are_exact [rel-*] 'f'
  (sp::pack_tn_kernel<true,true>), <true,false>, <false,false>   ... [spw-*] 'g' (gz_out compared whole), 'w' with act = 1, 'w' with act = 0
  (sp::gemm_tn_shared_kernel<NA,false>), <NA,true>    ... [spw-*] (the default)
  (sp::gemm_tn_kernel<NA,SPN,false>), <NA,SPN,true>   ... [spw-perwave], [spw-perwave-drop] (VQA_SPLIT_TN_SHARED=0)
  (sp::gemm_tn_shared_kernel<NA,false,0,true>), <NA,true,0,true>   test_relation_small_integers_are_exact [rel-*] 'w' / 'g'
  (sp::slab_sum_kernel)                               the last launch of every split weight gradient; S = 9, 10 (no multiple of 4), 1, 19"""
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
K5_FILES = ("linear_act.hip", "linear_split.hip")
SEED = 4242
AMP = 3                 # |operand| <= 3

# ---- the launch sites as the source spells them (blanks removed); a macro parameter (NAME_) arrives substituted in the log -------
S_FWD, S_FWD_D = "(linear_fwd_kernel<BM_,BN_,PF_,false>)", "(linear_fwd_kernel<BM_,BN_,PF_,true>)"
S_DX, S_DX_D = "(linear_dx_kernel<BM_,BN_,PF_,false>)", "(linear_dx_kernel<BM_,BN_,PF_,true>)"
S_DW, S_DW_D = "(linear_dw_kernel<BM_,BN_,PF_,false>)", "(linear_dw_kernel<BM_,BN_,PF_,true>)"
S_RED, S_MASK = "linear_dw_reduce_kernel", "linear_mask_kernel"
S_RTF, S_RTF_D = "(rt::gemm_nt_kernel<9,5,1,2,2,false,EpiBiasAct>)", "(rt::gemm_nt_kernel<9,5,1,2,2,true,EpiBiasAct>)"
# (gate, dropout, shared hash words) -> the register-tile weight-gradient form
S_RTDW = {(1, 1, 1): "(rt::gemm_tn_kernel<5,2,true,true,true,1>)", (0, 1, 1): "(rt::gemm_tn_kernel<5,2,false,true,true>)",
          (1, 1, 0): "(rt::gemm_tn_kernel<5,2,true,true>)", (1, 0, 0): "(rt::gemm_tn_kernel<5,2,true,false>)",
          (0, 1, 0): "(rt::gemm_tn_kernel<5,2,false,true>)", (0, 0, 0): "(rt::gemm_tn_kernel<5,2,false,false>)"}
S_PACKW = "(sp::split_pack_kernel<false>)"
S_SPF, S_SPF_D = ("(sp::gemm_nt_kernel<9,5,1,2,2,false,SplitEpiBiasAct,0,3>)", "(sp::gemm_nt_kernel<9,5,1,2,2,true,SplitEpiBiasAct,0,3>)")
S_REL, S_REL_D = ("(sp::gemm_nt_kernel<9,5,1,2,2,false,SplitEpiBiasAct,0,3,false,true>)",
                  "(sp::gemm_nt_kernel<9,5,1,2,2,true,SplitEpiBiasAct,0,3,false,true>)")
# (gate, gz_out) -> the pack of the output gradient
S_PACKG = {(1, 1): "(sp::pack_tn_kernel<true,true>)", (1, 0): "(sp::pack_tn_kernel<true,false>)", (0, 0): "(sp::pack_tn_kernel<false,false>)"}
S_TNS, S_TNS_D = "(sp::gemm_tn_shared_kernel<NA,false>)", "(sp::gemm_tn_shared_kernel<NA,true>)"
S_TNW, S_TNW_D = "(sp::gemm_tn_kernel<NA,SPN,false>)", "(sp::gemm_tn_kernel<NA,SPN,true>)"
S_TNR, S_TNR_D = "(sp::gemm_tn_shared_kernel<NA,false,0,true>)", "(sp::gemm_tn_shared_kernel<NA,true,0,true>)"
S_SUM = "(sp::slab_sum_kernel)"
MACRO_PARAMS = ("BM_", "BN_", "PF_")
spell = functools.partial(spell, params=MACRO_PARAMS)


def _round256(b):
    return (b + 255) & ~255


def names(log):
    return [(name, grid) for _, name, grid in log]


# ======================================================================================================================= the dispatchers, restated
def p8_of(p):
    """make_drop: round(p * 256) in float32, clamped to 0..255"""
    return min(255, max(0, int(np.float32(p) * np.float32(256.0) + np.float32(0.5))))


def scale_of(p):
    return 256.0 / (256.0 - p8_of(p))


def choose_tile(M, cols):
    """gemm_f32_mfma.hpp, one split: fewest CU-rounds of padded work, mild preference for the larger tile"""
    best, pick = 1e300, (128, 128)
    for (bm, bn), pref in zip(((128, 128), (64, 128), (128, 64), (64, 64)), (1.35, 1.15, 1.25, 1.00)):
        cost = float(_ceil(_ceil(M, bm) * _ceil(cols, bn), 256)) * bm * bn * pref
        if cost < best:
            best, pick = cost, (bm, bn)
    return pick + (2,)


def tile_override_or(kn, default):
    """VQA_GEMM_TILE = BMxBN[xPF]; a PF outside 1..3 reads as 2"""
    if "VQA_GEMM_TILE" in kn:
        v = [int(s) for s in kn["VQA_GEMM_TILE"].split("x")]
        if len(v) >= 2 and v[0] in (64, 128) and v[1] in (64, 128):
            return (v[0], v[1], v[2] if len(v) == 3 and 1 <= v[2] <= 3 else 2)
    return default


def linear_dw_tile(kn):
    """VQA_LINEAR_DW_TILE over VQA_GEMM_TILE over 64 x 64 x 2; with a PF outside 1..3 this knob is ignored"""
    t = tile_override_or(kn, (64, 64, 2))
    if "VQA_LINEAR_DW_TILE" in kn:
        v = [int(s) for s in kn["VQA_LINEAR_DW_TILE"].split("x")]
        if len(v) >= 2 and v[0] in (64, 128) and v[1] in (64, 128) and (len(v) == 2 or 1 <= v[2] <= 3):
            t = (v[0], v[1], v[2] if len(v) == 3 else 2)
    return t


def splits_for_linear_dw(M, K, N, tile, kn):
    s = _ceil(2560, _ceil(N, tile[0]) * _ceil(K, tile[1]))
    if "VQA_LINEAR_DW_SPLITS" in kn:
        s = int(kn["VQA_LINEAR_DW_SPLITS"])
    return max(min(s, _ceil(M, 256), 64), 1)


def rows_per_split(M, S):
    return _ceil(_ceil(M, S), 16) * 16


def rt_enabled(kn):
    return not kn.get("VQA_RT_ENGINE", "1").startswith("0")


def rt_fwd_ok(M, K, N, ldx, p8, kn):
    return (rt_enabled(kn) and M >= 1152 and K >= 64 and K % 4 == 0 and ldx % 4 == 0 and M * ldx * 4 < 2 ** 32 and N * K * 4 < 2 ** 32
            and (p8 == 0 or (p8 == 128 and K % 32 == 0)))


def rt_dw_ok(M, K, N, ldx, p8, kn):
    return (rt_enabled(kn) and M >= 4096 and K % 4 == 0 and ldx % 4 == 0 and M * ldx * 4 < 2 ** 32 and M * N * 4 < 2 ** 32 and M * K < 2 ** 32
            and p8 in (0, 128))


def rt_dw_splits(M, kn):
    """what the workspace query reserves"""
    s = int(kn["VQA_RT_DW_SPLITS"]) if "VQA_RT_DW_SPLITS" in kn else 16
    return max(min(s, max(M // 64, 1), 64), 1)


def rt_dw_launched(M, kn):
    """-> (S, rows per split) of the launch: no split of the rounded row count is empty"""
    rps = rows_per_split(M, rt_dw_splits(M, kn))
    return _ceil(M, rps), rps


def bwd_ws_bytes(M, K, N, kn):
    S = splits_for_linear_dw(M, K, N, linear_dw_tile(kn), kn)
    if rt_enabled(kn) and M >= 4096:
        S = max(S, rt_dw_splits(M, kn))
    return (S * N * K + S * N) * 4


def plain_fwd_log(M, K, N, ldx, p, kn):
    p8 = p8_of(p)
    if rt_fwd_ok(M, K, N, ldx, p8, kn):
        site = S_RTF_D if p8 else S_RTF
        return [(site, site, _ceil(M, 144) * _ceil(N, 160) * 256)]
    bm, bn, pf = tile_override_or(kn, choose_tile(M, N))
    site = S_FWD_D if p8 else S_FWD
    return [(site, spell(site, bm, bn, pf), _ceil(M, bm) * _ceil(N, bn) * 256)]


def plain_bwd_log(M, K, N, ldx, act, p, kn, want_dx):
    p8, log = p8_of(p), []
    if want_dx:
        bm, bn, pf = tile_override_or(kn, choose_tile(M, K))
        site = S_DX_D if p8 else S_DX
        log.append((site, spell(site, bm, bn, pf), _ceil(M, bm) * _ceil(K, bn) * 256))
    if rt_dw_ok(M, K, N, ldx, p8, kn):
        S, _ = rt_dw_launched(M, kn)
        share = int(p8 > 0 and K % 64 == 0 and not kn.get("VQA_RT_SHARE_HASH", "1").startswith("0"))
        site = S_RTDW[(int(act == 1), int(p8 > 0), share)]
        log.append((site, site, _ceil(N, 320) * _ceil(K, 128) * S * 256))
    else:
        bm, bn, pf = linear_dw_tile(kn)
        S = splits_for_linear_dw(M, K, N, (bm, bn, pf), kn)
        site = S_DW_D if p8 else S_DW
        log.append((site, spell(site, bm, bn, pf), _ceil(N, bm) * _ceil(K, bn) * S * 256))
    return log + [(S_RED, S_RED, _ceil(N * K // 2, 256) * 256)]


def lds_dw_empty_splits(M, K, N, kn):
    S = splits_for_linear_dw(M, K, N, linear_dw_tile(kn), kn)
    return S - _ceil(M, rows_per_split(M, S))


def split_shape_ok(M, K, N, ldx, p):
    return (M >= 1152 and K >= 128 and K % 64 == 0 and N >= 16 and N % 2 == 0 and _ceil(N, 16) <= 30 and ldx % 4 == 0 and ldx >= K
            and M * ldx * 4 < 2 ** 32 and M * N * 4 < 2 ** 32 and p8_of(p) in (0, 128))


def rel_lds_bytes(rps, K):
    return ((144 - 1) // rps + 2) * 2 * K * 4


def relation_linear_ok(B, Nr, D, L, p):
    return (B >= 1 and 8 <= Nr <= 1024 and split_shape_ok(B * Nr, D, L, D, p) and D % 128 == 0 and rel_lds_bytes(Nr, D) <= 96 * 1024
            and B * Nr * Nr < 2 ** 32)


def split_fwd_ws_bytes(K, N):
    return _round256(_ceil(N, 16) * (K // 32) * 3072)


def split_fwd_log(M, K, N, p, rel=False):
    drop = p8_of(p) > 0
    site = (S_REL_D if drop else S_REL) if rel else (S_SPF_D if drop else S_SPF)
    return [(S_PACKW, S_PACKW, _ceil(_ceil(N, 16) * (K // 32) * 64, 256) * 256), (site, site, _ceil(M, 144) * _ceil(N, 160) * 256)]


def tn_slabs(kn):
    return max(1, min(64, int(kn.get("VQA_SPLIT_DW_SLABS", 16))))


def tn_plan(M, want):
    """gemm_f32_split.hpp: -> (slabs, chunks of 32 rows per slab, an even count)"""
    chunks = _ceil(M, 32)
    S = min(max(want, 1), (chunks + 1) // 2)
    cps = (_ceil(chunks, S) + 1) & ~1
    return _ceil(chunks, cps), cps


def split_dw_ws_bytes(M, K, N, kn):
    slabs, cps = tn_plan(M, tn_slabs(kn))
    return _round256(slabs * cps * _ceil(N, 16) * 3072) + _round256(slabs * N * K * 4) + _round256(slabs * 36 * N * 4)


def slab_sum_blocks(NK, N):
    return _ceil(NK // 4, 256) + _ceil(N, 4)


def split_dw_log(M, K, N, act, p, kn, gz, rel=False):
    slabs, _ = tn_plan(M, tn_slabs(kn))
    drop = p8_of(p) > 0
    pack = S_PACKG[(int(act == 1), int(act == 1 and gz))]
    if rel:
        site = S_TNR_D if drop else S_TNR
    elif kn.get("VQA_SPLIT_TN_SHARED", "1").startswith("0"):
        site = S_TNW_D if drop else S_TNW
    else:
        site = S_TNS_D if drop else S_TNS
    grid = _ceil(_ceil(N, 16), 20) * _ceil(K, 128) * slabs * 256
    return [(pack, pack, slabs * 36 * 256), (site, site, grid), (S_SUM, S_SUM, slab_sum_blocks(N * K, N) * 256)]


# ======================================================================================================================= A: operands, reference
def bounds(M, K, N, scale, ax=AMP):
    """the largest sum of absolute values of the terms of an element of (y, d_x, d_w, d_b); ax: the layer input's amplitude (3, or
    3 + 3 * 3 = 12 for the fused relation forms)"""
    return (K * ax * AMP * scale + AMP, N * AMP * AMP * scale, M * AMP * ax * scale, M * AMP)


def _ints(gen, *shape):
    return torch.randint(-AMP, AMP + 1, shape, generator=gen).to(F64)


@functools.lru_cache(maxsize=4)
def operands(M, K, N):
    """float64 integers on the CPU: x [M,K], w [N,K], b [N], gy [M,N]"""
    gen = torch.Generator().manual_seed(1000003 * M + 10007 * K + 101 * N)
    return _ints(gen, M, K), _ints(gen, N, K), _ints(gen, N), _ints(gen, M, N)


@functools.lru_cache(maxsize=4)
def rel_operands(B, Nr, D, L):
    """v [B Nr, D], t [B, D], c2 [B, D], w [L, D], b [L], gy [B Nr, L]"""
    gen = torch.Generator().manual_seed(7 + 1000003 * B + 10007 * Nr + 101 * D + L)
    return _ints(gen, B * Nr, D), _ints(gen, B, D), _ints(gen, B, D), _ints(gen, L, D), _ints(gen, L), _ints(gen, B * Nr, L)


def relation_input(v, t, c2, Nr):
    """the relation step's output t + c2 v, in the operands' dtype"""
    return t.repeat_interleave(Nr, 0) + c2.repeat_interleave(Nr, 0) * v


def formulas(x, w, b, gy, act, mask, y=None):
    """oracle/kernels_np.py's linear_act_fwd / linear_act_bwd in the operands' dtype -> dict y, gz, d_x, d_w, d_b (the gate is the sign
    of `y` where one is given: the kernel's own output in section B)"""
    xd = x if mask is None else x * mask.to(x.dtype)
    z = xd @ w.T
    if b is not None:
        z = z + b
    out = torch.clamp(z, min=0.0) if act == 1 else z
    gate = out if y is None else y
    gz = gy * (gate > 0).to(gy.dtype) if act == 1 else gy
    dx = gz @ w
    return {"y": out, "gz": gz, "d_x": dx if mask is None else dx * mask.to(x.dtype), "d_w": gz.T @ xd, "d_b": gz.sum(0)}


def test_reference_is_the_oracle():
    """the torch restatement equals oracle/kernels_np.py on integers, bit for bit (both are exact)"""
    import oracle.kernels_np as knp
    M, K, N = 37, 10, 6
    x, w, b, gy = operands(M, K, N)
    mask = 2.0 * torch.randint(0, 2, (M, K), generator=torch.Generator().manual_seed(3)).to(F64)
    for act, m, bias in ((1, mask, b), (0, None, b), (1, None, None), (0, mask, None)):
        res = formulas(x, w, bias, gy, act, m)
        a = "relu" if act else None
        y = knp.linear_act_fwd(x.numpy(), w.numpy(), None if bias is None else bias.numpy(), a, None if m is None else m.numpy())
        assert np.array_equal(res["y"].numpy(), y)
        for key, want in zip(("d_x", "d_w", "d_b"), knp.linear_act_bwd(x.numpy(), w.numpy(), y, gy.numpy(), a, None if m is None else m.numpy())):
            assert np.array_equal(res[key].numpy(), want), key
        assert float(res["d_x"].abs().max()) > 0 and (act == 0 or bool((res["y"] == 0).any()))


_masks = {}


def mask_of(ops, p, M, K, seed=SEED):
    """the mask that vqa_linear_dropout_mask writes, float64 on the CPU (None at p = 0); kept for the module"""
    if p8_of(p) == 0:
        return None
    key = (p8_of(p), M, K, seed)
    if key not in _masks:
        if len(_masks) > 8:
            _masks.clear()
        buf = _out(M * K)
        rc, log = _call(ops, ops._lib.lib().vqa_linear_dropout_mask, _ptr(buf, PAD), p, seed, None, M, K)
        assert rc == 0 and log == [(S_MASK, _ceil(M * K // 2, 256) * 256)], (rc, log)
        _masks[key] = _win(buf, (M, K), "mask").cpu().to(F64)
        assert set(np.unique(_masks[key].numpy())) <= {0.0, float(np.float32(scale_of(p)))}      # (DropCfg.scale is a float)
    return _masks[key]


# ======================================================================================================================= the calls
def run_fwd(ops, engine, x, ldx, w, bias, M, K, N, act, p, seed=SEED):
    """engine 'plain' / 'split'; x, w, bias: device buffers from _in (bias may be None) -> (rc, log, y buffer)"""
    Lb = ops._lib.lib()
    y = _out(M * N)
    if engine == "plain":
        rc, log = _call(ops, Lb.vqa_linear_act_fwd, _ptr(x, PAD), ldx, _ptr(w, PAD), _ptr(bias, PAD), _ptr(y, PAD), M, K, N, act, p, seed, None)
        return rc, log, y
    nbytes = Lb.vqa_linear_act_fwd_split_workspace_bytes(K, N)
    assert nbytes == split_fwd_ws_bytes(K, N), ("workspace bytes", nbytes)
    ws = _workspace(nbytes)
    rc, log = _call(ops, Lb.vqa_linear_act_fwd_split, _ptr(x, PAD), ldx, _ptr(w, PAD), _ptr(bias, PAD), _ptr(y, PAD), _ptr(ws), nbytes,
                    M, K, N, act, p, seed, None)
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    return rc, log, y


def _workspace(nbytes):
    ws = _sentinel(nbytes // 4 + PAD)
    ws[:nbytes // 4] = NAN
    assert ws.data_ptr() % 16 == 0 and nbytes % 4 == 0
    return ws


def run_bwd(ops, x, ldx, w, y, gy, M, K, N, act, p, kn, want_dx=True, want_db=True, seed=SEED):
    """vqa_linear_act_bwd -> (rc, log, {d_x, d_w, d_b}), every output taken whole out of its sentinel-filled buffer; the workspace
    is exactly as long as the library asks for (the figure is restated), NaN-filled, and the sentinel behind it must survive"""
    Lb = ops._lib.lib()
    nbytes = Lb.vqa_linear_act_bwd_workspace_bytes(M, K, N)
    assert nbytes == bwd_ws_bytes(M, K, N, kn), ("workspace bytes", nbytes, bwd_ws_bytes(M, K, N, kn))
    ws = _workspace(nbytes)
    dx, dw, db = _out(M * K) if want_dx else None, _out(N * K), _out(N) if want_db else None
    rc, log = _call(ops, Lb.vqa_linear_act_bwd, _ptr(x, PAD), ldx, _ptr(w, PAD), _ptr(y, PAD), _ptr(gy, PAD), _ptr(dx, PAD) if want_dx else None,
                    _ptr(dw, PAD), _ptr(db, PAD) if want_db else None, _ptr(ws), nbytes, M, K, N, act, p, seed, None)
    if rc != 0:
        return rc, log, None
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    return rc, log, {"d_x": _win(dx, (M, K), "d_x") if want_dx else None, "d_w": _win(dw, (N, K), "d_w"),
                     "d_b": _win(db, (N,), "d_b") if want_db else None}


def run_dw_split(ops, x, ldx, y, gy, M, K, N, act, p, kn, want_db=True, want_gz=False, rel=None, seed=SEED):
    """vqa_linear_act_dw_split, or with rel = (t, c2, B, Nr) vqa_relation_linear_dw_split (x is v then) -> (rc, log, {d_w, d_b, gz})"""
    Lb = ops._lib.lib()
    nbytes = Lb.vqa_linear_act_dw_split_workspace_bytes(M, K, N)
    assert nbytes == split_dw_ws_bytes(M, K, N, kn), ("workspace bytes", nbytes, split_dw_ws_bytes(M, K, N, kn))
    ws = _workspace(nbytes)
    dw, db, gz = _out(N * K), _out(N) if want_db else None, _out(M * N) if want_gz else None
    outs = (_ptr(dw, PAD), _ptr(db, PAD) if want_db else None, _ptr(gz, PAD) if want_gz else None, _ptr(ws), nbytes)
    yp = _ptr(y, PAD) if y is not None else None
    if rel is None:
        rc, log = _call(ops, Lb.vqa_linear_act_dw_split, _ptr(x, PAD), ldx, yp, _ptr(gy, PAD), *outs, M, K, N, act, p, seed, None)
    else:
        t, c2, B, Nr = rel
        rc, log = _call(ops, Lb.vqa_relation_linear_dw_split, _ptr(x, PAD), _ptr(t, PAD), _ptr(c2, PAD), yp, _ptr(gy, PAD), *outs,
                        B, Nr, K, N, act, p, seed, None)
    if rc != 0:
        return rc, log, None
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    return rc, log, {"d_w": _win(dw, (N, K), "d_w"), "d_b": _win(db, (N,), "d_b") if want_db else None,
                     "gz": _win(gz, (M, N), "gz_out") if want_gz else None}


def run_rel_fwd(ops, v, t, c2, w, bias, B, Nr, D, L, act, p, seed=SEED):
    Lb = ops._lib.lib()
    nbytes = Lb.vqa_linear_act_fwd_split_workspace_bytes(D, L)
    assert nbytes == split_fwd_ws_bytes(D, L)
    ws, y = _workspace(nbytes), _out(B * Nr * L)
    rc, log = _call(ops, Lb.vqa_relation_linear_fwd_split, _ptr(v, PAD), _ptr(t, PAD), _ptr(c2, PAD), _ptr(w, PAD), _ptr(bias, PAD), _ptr(y, PAD),
                    _ptr(ws), nbytes, B, Nr, D, L, act, p, seed, None)
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    return rc, log, y


def check_grads(what, got, ref):
    for key in ("d_x", "d_w", "d_b", "gz"):
        if got.get(key) is not None:
            assert_exact("%s %s" % (what, key), got[key], ref[key])


# ======================================================================================================================= A: vqa_linear_act_fwd / _bwd
TILES = ((128, 128), (64, 128), (128, 64), (64, 64))
# (id, M, K, N, ldx - K, act, p, knobs, calls): f forward, F forward without bias, b backward with d_x and d_b, n backward without
# d_x, z backward without d_b
PLAIN_CASES = []
# the LDS-tile kernels: every (tile, PF) without and with dropout; (M, K, N) = (130, 50, 70) leaves the last row and column tile of
# every tile shape partial in all three GEMMs; the weight gradient runs another (tile, PF) under its own knob
for _i, ((_bm, _bn), _pf) in enumerate((t, pf) for t in TILES for pf in (1, 2, 3)):
    (_dm, _dn), _dpf = TILES[(_i // 3 + 1) % 4], _pf % 3 + 1
    for _p in (0.0, (0.5, 0.75)[_i % 2]):
        PLAIN_CASES.append(("tile-%dx%dx%d-p%g" % (_bm, _bn, _pf, _p), 130, 50, 70, 0, _i % 2, _p,
                            (("VQA_GEMM_TILE", "%dx%dx%d" % (_bm, _bn, _pf)), ("VQA_LINEAR_DW_TILE", "%dx%dx%d" % (_dm, _dn, _dpf))), "fb"))
_S = "VQA_LINEAR_DW_SPLITS"
PLAIN_CASES += [
    ("lds-70x18x34", 70, 18, 34, 0, 1, 0.75, (), "fFbz"), ("lds-1x2x2", 1, 2, 2, 0, 1, 0.5, (), "fbn"), ("lds-ldx", 130, 50, 70, 2, 1, 0.5, (), "fb"),
    ("lds-ldx-p0", 70, 18, 34, 2, 0, 0.0, (), "fFn"), ("lds-tile-default-pf", 130, 50, 70, 0, 1, 0.0, (("VQA_GEMM_TILE", "64x128"),), "fb"),
    # the weight gradient's row splits: S = ceil(M / 256) below 64; the knob, and the row cap that cuts it (8 asked for, 3 by rows:
    # 208 rows each, the last one 184 = 11 stages and a half); 257 rows in splits of 144: the second one ends 31 rows short
    ("lds-M256", 256, 18, 34, 0, 1, 0.5, (), "n"), ("lds-M257", 257, 18, 34, 0, 1, 0.5, (), "n"), ("lds-S1", 600, 18, 34, 0, 0, 0.0, ((_S, "1"),), "n"),
    ("lds-Scut", 600, 18, 34, 0, 1, 0.75, ((_S, "8"),), "nz"),
    # 64 splits of 272 rows cover 17408: the last three of 16400 rows are empty (d_w and d_b must get zeros from them)
    ("lds-empty", 16400, 18, 34, 0, 1, 0.75, (), "n"),
    # linear_dw_reduce_kernel: N K / 2 = 256 float2 lanes fill one block exactly, 258 need a second one
    ("lds-red256", 70, 32, 16, 0, 1, 0.0, (), "n"), ("lds-red258", 70, 86, 6, 0, 1, 0.5, (), "n"),
    # the register-tile forward: from M = 1152 (8 row tiles of 144; 1153: a ninth one of one row), K >= 64 and K % 4 == 0
    ("rtf-M1151", 1151, 64, 18, 0, 1, 0.0, (), "f"), ("rtf-M1152", 1152, 64, 18, 0, 1, 0.0, (), "fF"), ("rtf-M1153", 1153, 64, 18, 0, 0, 0.0, (), "f"),
    ("rtf-M1153-drop", 1153, 64, 18, 0, 1, 0.5, (), "fF"), ("rtf-K62", 1152, 62, 18, 0, 1, 0.0, (), "f"), ("rtf-K66", 1152, 66, 18, 0, 1, 0.5, (), "f"),
    # K = 64: two chunks per wave; 68: a K tail of 4 on the last wave; 80: five chunks, the second wave's a lone odd one; 96 with
    # dropout: 4 + 2 chunks; 80 with dropout: no whole hash words per row, the LDS tile
    ("rtf-K64", 1152, 64, 34, 0, 0, 0.0, (), "f"), ("rtf-K64-drop", 1152, 64, 34, 0, 1, 0.5, (), "f"), ("rtf-K68", 1152, 68, 18, 0, 1, 0.0, (), "f"),
    ("rtf-K80", 1152, 80, 18, 0, 1, 0.0, (), "f"), ("rtf-K96-drop", 1152, 96, 18, 0, 0, 0.5, (), "f"), ("rtf-K80-drop", 1152, 80, 18, 0, 1, 0.5, (), "f"),
    ("rtf-N2", 1152, 64, 2, 0, 1, 0.0, (), "f"), ("rtf-N160", 1152, 64, 160, 0, 1, 0.0, (), "f"), ("rtf-N162", 1153, 68, 162, 0, 1, 0.0, (), "fF"),
    # ldx = K + 4: the mask's counter is m K + k, not m ldx + k; ldx = K + 2 is no multiple of 4: the LDS tile
    ("rtf-ldx-drop", 1153, 64, 18, 4, 1, 0.5, (), "f"), ("rtf-ldx2", 1152, 64, 18, 2, 1, 0.0, (), "f"),
    ("rtf-off", 1152, 64, 18, 0, 1, 0.5, (("VQA_RT_ENGINE", "0"),), "f"), ("rtf-p75", 1152, 64, 18, 0, 1, 0.75, (), "f"),
    # the register-tile weight gradient: from M = 4096; gate x dropout, hash words shared at K % 64 == 0 unless VQA_RT_SHARE_HASH=0
    ("rtdw-M4095", 4095, 64, 18, 0, 0, 0.0, (), "n"), ("rtdw-M4096", 4096, 64, 18, 0, 0, 0.0, (), "fn"), ("rtdw-gate", 4096, 64, 18, 0, 1, 0.0, (), "n"),
    ("rtdw-gate-drop-share", 4096, 64, 18, 0, 1, 0.5, (), "n"), ("rtdw-drop-share", 4096, 128, 18, 0, 0, 0.5, (), "nz"),
    ("rtdw-gate-drop-K96", 4096, 96, 18, 0, 1, 0.5, (), "n"), ("rtdw-drop-K96", 4096, 96, 18, 0, 0, 0.5, (), "n"),
    ("rtdw-gate-drop-noshare", 4096, 64, 18, 0, 1, 0.5, (("VQA_RT_SHARE_HASH", "0"),), "n"),
    ("rtdw-drop-noshare", 4096, 64, 18, 0, 0, 0.5, (("VQA_RT_SHARE_HASH", "0"),), "n"),
    # K = 132: the second 128-column tile holds 4 columns, its spans are clamped to N2 - 4; N = 322: a second n1 tile of 2 rows;
    # M = 4100: 16 splits of 272 rows, the last one 20 = a chunk and a row tail of 4
    ("rtdw-K132", 4096, 132, 18, 0, 1, 0.0, (), "n"), ("rtdw-N2", 4096, 64, 2, 0, 0, 0.0, (), "n"), ("rtdw-N322", 4096, 64, 322, 0, 1, 0.0, (), "n"),
    ("rtdw-M4100", 4100, 64, 18, 0, 0, 0.0, (), "n"), ("rtdw-M4100-drop-ldx", 4100, 96, 18, 4, 1, 0.5, (), "nz"),
    ("rtdw-S1", 4096, 64, 18, 0, 0, 0.0, (("VQA_RT_DW_SPLITS", "1"),), "n"),
    # 64 splits asked for at M = 4100: 80 rows each, 52 cover M; the 12 empty ones are not launched (see the docstring)
    ("rtdw-M4100-S64", 4100, 64, 18, 0, 1, 0.5, (("VQA_RT_DW_SPLITS", "64"),), "n"),
    ("rtdw-M4100-S64-p0", 4100, 132, 34, 0, 0, 0.0, (("VQA_RT_DW_SPLITS", "64"),), "n"),
    ("rtdw-dx", 4096, 64, 18, 0, 1, 0.0, (), "b"), ("rtdw-dx-drop", 4100, 64, 18, 0, 1, 0.5, (), "b"), ("rtdw-red256", 4096, 64, 8, 0, 0, 0.0, (), "n"),
    ("rtdw-off", 4096, 64, 18, 0, 1, 0.5, (("VQA_RT_ENGINE", "0"),), "n"), ("rtdw-p75", 4096, 64, 18, 0, 1, 0.75, (), "n"),
]
PLAIN_BY_ID = {c[0]: c for c in PLAIN_CASES}


def plain_calls(case):
    """-> [(call, expected log)] of a case"""
    name, M, K, N, dl, act, p, knobs, calls = case
    kn = dict(knobs)
    return [(c, plain_fwd_log(M, K, N, K + dl, p, kn) if c in "fF" else plain_bwd_log(M, K, N, K + dl, act, p, kn, c in "bz")) for c in calls]


@gpu
@pytest.mark.parametrize("case", PLAIN_CASES, ids=lambda c: c[0])
def test_plain_small_integers_are_exact(ops, lib_option, case):
    """vqa_linear_act_fwd / vqa_linear_act_bwd on the LDS-tile and register-tile engines; the backward reads the reference's y"""
    name, M, K, N, dl, act, p, knobs, calls = case
    assert len(PLAIN_BY_ID) == len(PLAIN_CASES)
    Lb = ops._lib.lib()
    set_knobs(lib_option, knobs)
    _below_2_24(*bounds(M, K, N, scale_of(p)))
    x, w, b, gy = operands(M, K, N)
    mask = mask_of(ops, p, M, K)
    ref = formulas(x, w, b, gy, act, mask)
    ldx = K + dl
    dx_, dw_, db_, dgy = _in(x, ldx), _in(w), _in(b), _in(gy)
    dy = _in(ref["y"])
    for c, want_log in plain_calls(case):
        what = "%s %s" % (name, c)
        if c in "fF":
            rc, log, y = run_fwd(ops, "plain", dx_, ldx, dw_, db_ if c == "f" else None, M, K, N, act, p)
            assert rc == 0, (what, rc, Lb.vqa_last_error())
            assert log == names(want_log), (what, log, names(want_log))
            want = ref["y"] if c == "f" else formulas(x, w, None, gy, act, mask)["y"]
            assert_exact(what + " y", _win(y, (M, N), "y"), want)
            continue
        rc, log, got = run_bwd(ops, dx_, ldx, dw_, dy, dgy, M, K, N, act, p, dict(knobs), c in "bz", c != "z")
        assert rc == 0, (what, rc, Lb.vqa_last_error())
        assert log == names(want_log), (what, log, names(want_log))
        check_grads(what, got, ref)


# ======================================================================================================================= A: the split engine
# (id, M, K, N, ldx - K, act, p, knobs, calls): f / F forward with / without bias; w weight gradient; g with gz_out (act = 1); z
# without d_b
SPLIT_CASES = [
    ("spf-1152x128x16", 1152, 128, 16, 0, 1, 0.0, (), "fFw"), ("spf-1152x128x16-drop", 1152, 128, 16, 0, 1, 0.5, (), "fg"),
    # K = 192: the forward takes K % 64 == 0, the weight gradient needs K % 128 == 0 (refused: test_refusals_launch_nothing)
    ("spf-K192", 1152, 192, 16, 0, 0, 0.5, (), "f"), ("spf-N18", 1152, 128, 18, 0, 1, 0.0, (), "f"), ("spf-N162-drop", 1152, 128, 162, 0, 1, 0.5, (), "f"),
    ("spf-N480", 1152, 128, 480, 0, 0, 0.0, (), "f"), ("spf-M1153", 1153, 128, 18, 0, 1, 0.5, (), "fF"), ("spf-ldx", 1153, 128, 18, 4, 1, 0.5, (), "fw"),
    ("spf-ldx-p0", 1152, 128, 16, 4, 0, 0.0, (), "f"),
    # the weight gradient: 36 chunks of 32 rows in 9 slabs of 4 (1152) / 37 in 10 (1153: 31 zero-padded rows in the last chunk, 3
    # zero chunks behind it); the three packs; the shared and the per-wave TN kernel; 1 slab and 19 (64 asked for)
    ("spw-act0", 1152, 128, 16, 0, 0, 0.0, (), "wz"), ("spw-act0-drop", 1153, 128, 18, 0, 0, 0.5, (), "w"), ("spw-gate", 1153, 128, 18, 0, 1, 0.0, (), "wg"),
    ("spw-gate-drop", 1152, 256, 34, 0, 1, 0.5, (), "gz"),
    ("spw-perwave", 1153, 128, 18, 0, 1, 0.0, (("VQA_SPLIT_TN_SHARED", "0"),), "g"),
    ("spw-perwave-drop", 1152, 256, 34, 0, 0, 0.5, (("VQA_SPLIT_TN_SHARED", "0"),), "w"),
    ("spw-S1", 1153, 128, 18, 0, 1, 0.5, (("VQA_SPLIT_DW_SLABS", "1"),), "g"), ("spw-S64", 1153, 128, 18, 0, 1, 0.0, (("VQA_SPLIT_DW_SLABS", "64"),), "w"),
    ("spw-N322", 1152, 128, 322, 0, 1, 0.5, (), "g"),
]


def split_calls(case):
    name, M, K, N, dl, act, p, knobs, calls = case
    return [(c, split_fwd_log(M, K, N, p) if c in "fF" else split_dw_log(M, K, N, act, p, dict(knobs), c == "g")) for c in calls]


@gpu
@pytest.mark.parametrize("case", SPLIT_CASES, ids=lambda c: c[0])
def test_split_small_integers_are_exact(ops, lib_option, case):
    """vqa_linear_act_fwd_split / vqa_linear_act_dw_split: three bf16 planes of a small integer are that integer"""
    name, M, K, N, dl, act, p, knobs, calls = case
    Lb = ops._lib.lib()
    set_knobs(lib_option, knobs)
    _below_2_24(*bounds(M, K, N, scale_of(p)))
    ldx = K + dl
    assert split_shape_ok(M, K, N, ldx, p) and Lb.vqa_linear_split_supported(M, K, N, ldx, p) == 1
    x, w, b, gy = operands(M, K, N)
    mask = mask_of(ops, p, M, K)
    ref = formulas(x, w, b, gy, act, mask)
    dx_, dw_, db_, dgy, dy = _in(x, ldx), _in(w), _in(b), _in(gy), _in(ref["y"])
    for c, want_log in split_calls(case):
        what = "%s %s" % (name, c)
        if c in "fF":
            rc, log, y = run_fwd(ops, "split", dx_, ldx, dw_, db_ if c == "f" else None, M, K, N, act, p)
            assert rc == 0, (what, rc, Lb.vqa_last_error())
            assert log == names(want_log), (what, log, names(want_log))
            assert_exact(what + " y", _win(y, (M, N), "y"), ref["y"] if c == "f" else formulas(x, w, None, gy, act, mask)["y"])
            continue
        # (act = 0 never reads y: NULL)
        rc, log, got = run_dw_split(ops, dx_, ldx, dy if act == 1 else None, dgy, M, K, N, act, p, dict(knobs), c != "z", c == "g")
        assert rc == 0, (what, rc, Lb.vqa_last_error())
        assert log == names(want_log), (what, log, names(want_log))
        check_grads(what, got, ref)


# (id, B, Nr, D, L, act, p, knobs, calls): f forward, w weight gradient, g with gz_out
REL_CASES = [
    # Nr = 8: the smallest count, 18 samples per 144-row tile (19 staged); D = 640: 19 x 2 x 640 x 4 = 97280 bytes of (T, C2), the
    # largest D % 128 == 0 inside 96 KiB (768 is refused: test_refusals_launch_nothing)
    ("rel-Nr8", 144, 8, 128, 16, 1, 0.0, (), "fw"), ("rel-Nr8-drop", 144, 8, 128, 18, 1, 0.5, (), "fg"), ("rel-Nr8-D640", 144, 8, 640, 16, 0, 0.5, (), "fw"),
    # Nr = 36: four samples per tile; B = 33: a last tile of 36 rows
    ("rel-Nr36-B32", 32, 36, 128, 18, 1, 0.5, (), "fg"), ("rel-Nr36-B33", 33, 36, 128, 162, 1, 0.0, (), "fg"), ("rel-Nr36-B33-drop", 33, 36, 256, 18, 0, 0.5, (), "fw"),
    # Nr = 40: samples straddle every tile edge (144 = 3 x 40 + 24)
    ("rel-Nr40", 29, 40, 128, 18, 1, 0.5, (), "fg"),
]


def rel_calls(case):
    name, B, Nr, D, L, act, p, knobs, calls = case
    return [(c, split_fwd_log(B * Nr, D, L, p, True) if c == "f" else split_dw_log(B * Nr, D, L, act, p, dict(knobs), c == "g", True)) for c in calls]


@gpu
@pytest.mark.parametrize("case", REL_CASES, ids=lambda c: c[0])
def test_relation_small_integers_are_exact(ops, lib_option, case):
    """vqa_relation_linear_fwd_split / _dw_split: the layer input t + c2 v (|.| <= 12) is formed in registers; reference: in float64 first"""
    name, B, Nr, D, L, act, p, knobs, calls = case
    Lb = ops._lib.lib()
    set_knobs(lib_option, knobs)
    M = B * Nr
    _below_2_24(*bounds(M, D, L, scale_of(p), AMP + AMP * AMP))
    assert relation_linear_ok(B, Nr, D, L, p) and Lb.vqa_relation_linear_split_supported(B, Nr, D, L, p) == 1
    v, t, c2, w, b, gy = rel_operands(B, Nr, D, L)
    ref = formulas(relation_input(v, t, c2, Nr), w, b, gy, act, mask_of(ops, p, M, D))
    dv, dt, dc2, dw_, db_, dgy, dy = _in(v), _in(t), _in(c2), _in(w), _in(b), _in(gy), _in(ref["y"])
    for c, want_log in rel_calls(case):
        what = "%s %s" % (name, c)
        if c == "f":
            rc, log, y = run_rel_fwd(ops, dv, dt, dc2, dw_, db_, B, Nr, D, L, act, p)
            assert rc == 0, (what, rc, Lb.vqa_last_error())
            assert log == names(want_log), (what, log, names(want_log))
            assert_exact(what + " y", _win(y, (M, L), "y"), ref["y"])
            continue
        rc, log, got = run_dw_split(ops, dv, D, dy if act == 1 else None, dgy, M, D, L, act, p, dict(knobs), True, c == "g", (dt, dc2, B, Nr))
        assert rc == 0, (what, rc, Lb.vqa_last_error())
        assert log == names(want_log), (what, log, names(want_log))
        check_grads(what, got, ref)


@gpu
def test_mask_kernel(ops):
    """vqa_linear_dropout_mask: all ones at p = 0; values in {0, scale} at 0.5 (one bit per element) and 0.75 (one byte), about 1 - p
    of them kept; an odd count of pairs per block edge (M K / 2 = 257: two blocks), nothing outside the window"""
    Lb = ops._lib.lib()
    for M, K in ((1, 2), (257, 2), (70, 18)):
        for p, scale in ((0.0, 1.0), (0.5, 2.0), (0.75, 4.0)):
            buf = _out(M * K)
            rc, log = _call(ops, Lb.vqa_linear_dropout_mask, _ptr(buf, PAD), p, SEED, None, M, K)
            assert rc == 0 and log == [(S_MASK, _ceil(M * K // 2, 256) * 256)], (M, K, p, rc, log)
            m = _win(buf, (M, K), "mask").cpu()
            assert set(np.unique(m.numpy())) <= ({1.0} if p == 0 else {0.0, scale}), (M, K, p)
            if M * K > 1000:
                assert abs(float((m > 0).double().mean()) - (1 - p)) < 0.05, (M, K, p)
    # the mask is a function of (seed, element): another seed, another mask; the same seed, the same mask
    a, b = mask_of(ops, 0.5, 70, 18), mask_of(ops, 0.5, 70, 18, seed=SEED + 1)
    _masks.clear()
    assert not torch.equal(a, b) and torch.equal(a, mask_of(ops, 0.5, 70, 18))


# ======================================================================================================================= D (no GPU)
def all_expected_logs():
    """every (site, spelled name, grid) that a section A case expects -- needs no GPU"""
    logs = [(S_MASK, S_MASK, 256)]
    for case in PLAIN_CASES:
        for _, log in plain_calls(case):
            logs += log
    for case in SPLIT_CASES:
        for _, log in split_calls(case):
            logs += log
    for case in REL_CASES:
        for _, log in rel_calls(case):
            logs += log
    return logs


def test_case_tables_stay_exact():
    """every section A case: every sum stays below 2^24 at amplitude 3, and its shape is one the entry takes"""
    for name, M, K, N, dl, act, p, knobs, calls in PLAIN_CASES + SPLIT_CASES:
        _below_2_24(*bounds(M, K, N, scale_of(p)))
        assert K % 2 == 0 and N % 2 == 0 and dl % 2 == 0 and act in (0, 1) and p in (0.0, 0.5, 0.75), name
        assert scale_of(p) in (1.0, 2.0, 4.0)
    for name, M, K, N, dl, act, p, knobs, calls in SPLIT_CASES:
        assert split_shape_ok(M, K, N, K + dl, p) and (K % 128 == 0 or not set(calls) & set("wgz")) and ("g" not in calls or act == 1), name
    for name, B, Nr, D, L, act, p, knobs, calls in REL_CASES:
        _below_2_24(*bounds(B * Nr, D, L, scale_of(p), 12))
        assert relation_linear_ok(B, Nr, D, L, p) and ("g" not in calls or act == 1), name
    assert bounds(10, 20, 30, 2.0) == (20 * 9 * 2 + 3, 30 * 9 * 2, 10 * 9 * 2, 30) and bounds(10, 20, 30, 1.0, 12)[2] == 10 * 36
    assert (p8_of(0.5), p8_of(0.75), p8_of(0.3), p8_of(0.0)) == (128, 192, 77, 0) and scale_of(0.3) == 256.0 / 179.0


def _forms(table_by_id, plan, cid, call):
    return [n for c, log in plan(table_by_id[cid]) if c == call for _, n, _ in log]


def test_dispatchers_at_their_thresholds():
    """what the case tables promise, checked on the restated dispatchers at hand-worked values (the GPU tests check the restatement
    against the library)"""
    P = functools.partial(_forms, PLAIN_BY_ID, plain_calls)
    # choose_tile with one split never leaves 64 x 64 (see the docstring): a sweep over both sides of every round and tile edge
    for M in list(range(1, 400, 7)) + [1151, 1152, 4096, 16400, 18432, 65536]:
        for cols in list(range(2, 700, 6)) + [2048, 4096]:
            assert choose_tile(M, cols) == (64, 64, 2), (M, cols)
    assert tile_override_or({"VQA_GEMM_TILE": "64x128"}, (64, 64, 2)) == (64, 128, 2) == tile_override_or({"VQA_GEMM_TILE": "64x128x9"}, (64, 64, 3))
    assert tile_override_or({"VQA_GEMM_TILE": "32x128"}, (64, 64, 2)) == (64, 64, 2)
    assert linear_dw_tile({"VQA_GEMM_TILE": "128x128x3"}) == (128, 128, 3) and linear_dw_tile({"VQA_GEMM_TILE": "128x128x3", "VQA_LINEAR_DW_TILE": "64x128x1"}) == (64, 128, 1)
    assert linear_dw_tile({"VQA_LINEAR_DW_TILE": "64x128x4"}) == (64, 64, 2) and linear_dw_tile({"VQA_LINEAR_DW_TILE": "128x64"}) == (128, 64, 2)
    assert P("lds-tile-default-pf", "f") == ["(linear_fwd_kernel<64,128,2,false>)"]
    # the LDS weight gradient's row splits
    t = (64, 64, 2)
    assert [splits_for_linear_dw(M, 18, 34, t, {}) for M in (1, 256, 257, 512, 513, 16384, 16400)] == [1, 1, 2, 2, 3, 64, 64]
    assert splits_for_linear_dw(18432, 2048, 310, t, {}) == 16 and splits_for_linear_dw(600, 18, 34, t, {_S: "8"}) == 3
    assert splits_for_linear_dw(600, 18, 34, t, {_S: "1"}) == 1 and splits_for_linear_dw(600, 18, 34, t, {_S: "0"}) == 1
    assert rows_per_split(257, 2) == 144 and rows_per_split(600, 3) == 208 and rows_per_split(16400, 64) == 272
    # the register-tile forward
    for cid, rt in (("rtf-M1151", 0), ("rtf-M1152", 1), ("rtf-M1153", 1), ("rtf-K62", 0), ("rtf-K66", 0), ("rtf-K64", 1), ("rtf-K68", 1), ("rtf-K80", 1),
                    ("rtf-K96-drop", 1), ("rtf-K80-drop", 0), ("rtf-N2", 1), ("rtf-N162", 1), ("rtf-ldx-drop", 1), ("rtf-ldx2", 0), ("rtf-off", 0),
                    ("rtf-p75", 0), ("rtdw-M4096", 1)):
        assert ["rt::gemm_nt_kernel" in n for n in P(cid, "f")] == [bool(rt)], cid
    assert P("rtf-K96-drop", "f") == [S_RTF_D] and P("rtf-K80", "f") == [S_RTF] and P("rtf-K80-drop", "f") == ["(linear_fwd_kernel<64,64,2,true>)"]
    grid = lambda cid, call, i=0: [g for c, log in plain_calls(PLAIN_BY_ID[cid]) if c == call for _, _, g in log][i]      # noqa: E731
    assert grid("rtf-M1152", "f") == 8 * 256 and grid("rtf-M1153", "f") == 9 * 256 and grid("rtf-N160", "f") == 8 * 256 and grid("rtf-N162", "f") == 18 * 256
    # the register-tile weight gradient: its six forms, its splits
    for cid, form in (("rtdw-M4096", (0, 0, 0)), ("rtdw-gate", (1, 0, 0)), ("rtdw-gate-drop-share", (1, 1, 1)), ("rtdw-drop-share", (0, 1, 1)),
                      ("rtdw-gate-drop-K96", (1, 1, 0)), ("rtdw-drop-K96", (0, 1, 0)), ("rtdw-gate-drop-noshare", (1, 1, 0)), ("rtdw-drop-noshare", (0, 1, 0)),
                      ("rtdw-M4100-S64", (1, 1, 1)), ("rtdw-M4100-drop-ldx", (1, 1, 0))):
        assert P(cid, "n")[0] == S_RTDW[form], cid
    for cid in ("rtdw-M4095", "rtdw-off", "rtdw-p75"):
        assert "linear_dw_kernel" in P(cid, "n")[0], cid
    assert rt_dw_launched(4096, {}) == (16, 256) and rt_dw_launched(4100, {}) == (16, 272) and 15 * 272 + 16 + 4 == 4100
    assert rt_dw_launched(18432, {}) == (16, 1152) and rt_dw_launched(4096, {"VQA_RT_DW_SPLITS": "1"}) == (1, 4096)
    assert rt_dw_splits(4100, {"VQA_RT_DW_SPLITS": "64"}) == 64 and rt_dw_launched(4100, {"VQA_RT_DW_SPLITS": "64"}) == (52, 80) and 51 * 80 < 4100 <= 52 * 80
    assert grid("rtdw-K132", "n") == 2 * 16 * 256 and grid("rtdw-N322", "n") == 2 * 16 * 256 and grid("rtdw-M4100-S64", "n") == 52 * 256
    assert bwd_ws_bytes(4100, 64, 18, {"VQA_RT_DW_SPLITS": "64"}) == 64 * (18 * 64 + 18) * 4 and bwd_ws_bytes(4095, 64, 18, {}) == 16 * (18 * 64 + 18) * 4
    # both reduce sites on both sides of a block of 256 float2 lanes
    assert grid("lds-red256", "n", 1) == 256 and grid("lds-red258", "n", 1) == 512 and grid("rtdw-red256", "n", 1) == 256 and grid("rtdw-N2", "n", 1) == 256
    # the split engine
    assert split_shape_ok(1152, 128, 16, 128, 0.5) and not split_shape_ok(1151, 128, 16, 128, 0.5) and not split_shape_ok(1152, 64, 16, 64, 0.0)
    assert split_shape_ok(1152, 192, 16, 192, 0.0) and not split_shape_ok(1152, 160, 16, 160, 0.0) and not split_shape_ok(1152, 128, 14, 128, 0.0)
    assert split_shape_ok(1152, 128, 480, 128, 0.0) and not split_shape_ok(1152, 128, 482, 128, 0.0) and not split_shape_ok(1152, 128, 16, 130, 0.0)
    assert not split_shape_ok(1152, 128, 16, 128, 0.75) and not split_shape_ok(1152, 128, 16, 128, 0.3)
    assert split_fwd_ws_bytes(128, 16) == 4 * 3072 and split_fwd_ws_bytes(2048, 310) == 20 * 64 * 3072
    assert tn_plan(1152, 16) == (9, 4) and tn_plan(1153, 16) == (10, 4) and tn_plan(1153, 1) == (1, 38) and tn_plan(1153, 64) == (19, 2)
    assert tn_plan(18432, 16) == (16, 36) and tn_plan(1152, 64) == (18, 2)
    assert slab_sum_blocks(16 * 128, 16) == 2 + 4 and slab_sum_blocks(18 * 128, 18) == 3 + 5 and slab_sum_blocks(310 * 2048, 310) == 620 + 78
    assert split_dw_ws_bytes(1152, 128, 16, {}) == 9 * 4 * 3072 + 9 * 16 * 128 * 4 + _round256(9 * 36 * 16 * 4)
    # the fused relation forms: 96 KiB of staged (T, C2) rows
    assert rel_lds_bytes(8, 640) == 97280 <= 96 * 1024 < rel_lds_bytes(8, 768) and rel_lds_bytes(36, 2048) == 5 * 2 * 2048 * 4
    assert relation_linear_ok(144, 8, 640, 16, 0.5) and not relation_linear_ok(144, 8, 768, 16, 0.5) and not relation_linear_ok(165, 7, 128, 16, 0.0)
    assert not relation_linear_ok(144, 8, 192, 16, 0.0) and not relation_linear_ok(143, 8, 128, 16, 0.0)


def test_empty_splits_are_where_the_cases_say():
    """the LDS-tile weight gradient launches its empty splits (they write zeros): only [lds-empty] has any; the register-tile one
    launches none, and only the two [rtdw-M4100-S64*] cases ask for more splits than it launches; the split engine's plan never
    leaves a slab empty"""
    for name, M, K, N, dl, act, p, knobs, calls in PLAIN_CASES:
        kn = dict(knobs)
        if not set(calls) & set("bnz"):
            continue
        if rt_dw_ok(M, K, N, K + dl, p8_of(p), kn):
            S, rps = rt_dw_launched(M, kn)
            assert (S - 1) * rps < M <= S * rps and rps % 16 == 0, name
            assert (rt_dw_splits(M, kn) - S) == (12 if name.startswith("rtdw-M4100-S64") else 0), name
        else:
            assert lds_dw_empty_splits(M, K, N, kn) == (3 if name == "lds-empty" else 0), name
    for case in SPLIT_CASES + [(c[0], c[1] * c[2], c[3], c[4], 0) + c[5:] for c in REL_CASES]:
        slabs, cps = tn_plan(case[1], tn_slabs(dict(case[7])))
        assert (slabs - 1) * cps < _ceil(case[1], 32) <= slabs * cps and cps % 2 == 0, case[0]
    assert sorted({tn_plan(c[1], tn_slabs(dict(c[7])))[0] for c in SPLIT_CASES if set(c[8]) & set("wgz")}) == [1, 9, 10, 19]


def test_case_tables_reach_every_instantiation():
    """beyond the launch sites: every template instantiation the dispatchers can pick is the spelled form of some case"""
    seen = {n for _, n, _ in all_expected_logs()}
    want = {spell(s, bm, bn, pf) for s in (S_FWD, S_FWD_D, S_DX, S_DX_D, S_DW, S_DW_D) for bm, bn in TILES for pf in (1, 2, 3)}
    want |= set(S_RTDW.values()) | set(S_PACKG.values())
    want |= {S_RED, S_MASK, S_RTF, S_RTF_D, S_PACKW, S_SPF, S_SPF_D, S_REL, S_REL_D, S_TNS, S_TNS_D, S_TNW, S_TNW_D, S_TNR, S_TNR_D, S_SUM}
    assert want - seen == set(), "instantiations that no case launches"


def test_every_launch_site_is_declared():
    """a launch site added to (or renamed in) one of the two files without a case here fails; so does a case whose site no longer exists"""
    per_file = [launch_sites(os.path.join(CSRC, f)) for f in K5_FILES]
    assert [len(s) for s in per_file] == [17, 16], per_file
    sites = per_file[0] + per_file[1]
    assert sites.count(S_RED) == 2 and sites.count(S_PACKW) == 2 and len(set(sites)) == 31
    declared = {site for site, _, _ in all_expected_logs()}
    assert set(sites) - declared == set(), "launch sites that no case declares"
    assert declared - set(sites) == set(), "declared forms that no launch site has"


# ======================================================================================================================= B
SPLIT_BAR = 2e-5      # tests/test_gpu_split.py's bar for the split engine
# (id, entry, M | (B, Nr), K, N, act, p, knobs, forward form, forms that must be in the backward's log)
RANDOM_CASES = [
    ("lds-p0.3", "plain", 130, 50, 70, 1, 0.3, (), "linear_fwd_kernel", ("linear_dx_kernel", "linear_dw_kernel")),
    ("lds-splits", "plain", 600, 86, 34, 1, 0.0, (), "linear_fwd_kernel", ("linear_dx_kernel", "linear_dw_kernel")),
    ("rt-fwd", "plain", 1153, 68, 162, 1, 0.0, (), "rt::gemm_nt_kernel", ("linear_dw_kernel",)),
    ("rt-fwd-drop", "plain", 1153, 96, 34, 1, 0.5, (), "rt::gemm_nt_kernel", ("linear_dw_kernel",)),
    ("rt-dw", "plain", 4100, 132, 34, 1, 0.0, (), "rt::gemm_nt_kernel", ("linear_dx_kernel", "rt::gemm_tn_kernel<5,2,true,false>")),
    ("rt-dw-drop", "plain", 4100, 128, 34, 1, 0.5, (), "rt::gemm_nt_kernel", ("linear_dx_kernel", "rt::gemm_tn_kernel<5,2,true,true,true,1>")),
    ("split", "split", 1153, 128, 162, 1, 0.0, (), "sp::gemm_nt_kernel", ("sp::gemm_tn_shared_kernel",)),
    ("split-drop", "split", 1153, 256, 34, 1, 0.5, (), "sp::gemm_nt_kernel", ("sp::gemm_tn_shared_kernel",)),
    ("split-perwave", "split", 1153, 128, 34, 1, 0.5, (("VQA_SPLIT_TN_SHARED", "0"),), "sp::gemm_nt_kernel", ("sp::gemm_tn_kernel",)),
    ("rel", "rel", (33, 36), 256, 34, 1, 0.5, (), "sp::gemm_nt_kernel", ("sp::gemm_tn_shared_kernel<NA,true,0,true>",)),
]


@gpu
@pytest.mark.parametrize("case", RANDOM_CASES, ids=lambda c: c[0])
def test_random_operands_against_float64(ops, lib_option, measured, case):
    """forward, then the backward with the kernel's own y as the gate; the float64 reference is oracle/kernels_np.py itself"""
    import oracle.kernels_np as knp
    name, entry, M, K, N, act, p, knobs, f_form, b_forms = case
    set_knobs(lib_option, knobs)
    B, Nr = M if entry == "rel" else (0, 0)
    M = B * Nr if entry == "rel" else M
    gen = torch.Generator().manual_seed(7 * M + 11 * K + N)
    x, w, b, gy = (torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5, 0.1 * torch.randn(N, generator=gen),
                   torch.randn(M, N, generator=gen))
    mask = mask_of(ops, p, M, K)
    dw_, db_, dgy = _in(w), _in(b), _in(gy)
    if entry == "rel":
        t, c2 = torch.randn(B, K, generator=gen), torch.randn(B, K, generator=gen)
        dx_, dt, dc2 = _in(x), _in(t), _in(c2)
        x64, x32 = relation_input(x.double(), t.double(), c2.double(), Nr), relation_input(x, t, c2, Nr)
        rc, log, ybuf = run_rel_fwd(ops, dx_, dt, dc2, dw_, db_, B, Nr, K, N, act, p)
    else:
        dx_, x64, x32 = _in(x), x.double(), x
        rc, log, ybuf = run_fwd(ops, entry, dx_, K, dw_, db_, M, K, N, act, p)
    assert rc == 0 and f_form in log[-1][0], (name, rc, log)
    y = _win(ybuf, (M, N), "y")
    a, m64 = "relu" if act else None, None if mask is None else mask.numpy()
    y64 = torch.from_numpy(knp.linear_act_fwd(x64.numpy(), w.numpy(), b.numpy(), a, m64))
    g64 = [torch.from_numpy(np.ascontiguousarray(g)) for g in knp.linear_act_bwd(x64.numpy(), w.numpy(), y.cpu().numpy(), gy.numpy(), a, m64)]
    ref32 = formulas(x32, w, b, gy, act, None if mask is None else mask.float(), y.cpu())
    dy = _in(y.cpu())
    if entry == "plain":
        rc, blog, got = run_bwd(ops, dx_, K, dw_, dy, dgy, M, K, N, act, p, dict(knobs))
    else:
        rc, blog, got = run_dw_split(ops, dx_, K, dy, dgy, M, K, N, act, p, dict(knobs), True, True, (dt, dc2, B, Nr) if entry == "rel" else None)
    assert rc == 0 and all(any(f in n for n, _ in blog) for f in b_forms), (name, rc, blog)
    fb = None if entry == "plain" else SPLIT_BAR
    bars = Bars(measured, name)
    bars.check("y", y, y64, ref32["y"], fb)
    if got.get("d_x") is not None:
        bars.check("d_x", got["d_x"], g64[0], ref32["d_x"])
    bars.check("d_w", got["d_w"], g64[1], ref32["d_w"], fb)
    bars.check("d_b", got["d_b"], g64[2], ref32["d_b"], fb)
    bars.close()
    if got.get("gz") is not None:      # the gated gradient is a selection, not arithmetic: exact
        assert torch.equal(got["gz"].cpu(), ref32["gz"])


# ======================================================================================================================= C
# (id, M, K, N, p, the rows that carry the NaN): rows on both sides of a 64-row LDS tile / 144-row register tile edge, the last row
# (clamped loads of the rows past M repeat it), and for the data gradient's M the rows around a split edge of the weight gradient
ROW_CASES = [("lds", "plain", 130, 50, 70, 0.0, (63, 64, 129)), ("lds-drop", "plain", 130, 50, 70, 0.5, (0, 127, 128)),
             ("rt", "plain", 1153, 64, 18, 0.0, (143, 144, 1152)), ("rt-drop", "plain", 1153, 64, 18, 0.5, (287, 288, 1151)),
             ("rt-dw", "plain", 4100, 64, 18, 0.0, (271, 272, 4099)),
             # the split engine: the NaN's row comes back from the repair path (an fp32 dot product of the original operands)
             ("split", "split", 1153, 128, 18, 0.0, (143, 144, 1152)), ("split-drop", "split", 1153, 128, 18, 0.5, (0, 1007, 1008))]


@gpu
@pytest.mark.parametrize("case", ROW_CASES, ids=lambda c: c[0])
def test_a_nan_stays_in_its_row(ops, case):
    """act = 0 (relu's fmaxf would swallow the NaN).  A NaN in x[r]: y[r] is NaN, every other row of y is the clean run's, bit for
    bit.  A NaN in gy[r]: the same for d_x (d_w and d_b sum over the rows and are not asserted; the split engine has no d_x)"""
    name, entry, M, K, N, p, rows = case
    x, w, b, gy = operands(M, K, N)
    mask = mask_of(ops, p, M, K)
    ref = formulas(x, w, b, gy, 0, mask)
    dw_, db_, dy = _in(w), _in(b), _in(ref["y"])
    for r in rows:
        others = [i for i in range(M) if i != r]
        col = int((mask[r] > 0).nonzero()[0]) if mask is not None else 5      # (an element that is kept)
        xr = x.clone()
        xr[r, col] = NAN
        rc, log, ybuf = run_fwd(ops, entry, _in(xr), K, dw_, db_, M, K, N, 0, p)
        assert rc == 0 and ("rt::gemm_nt_kernel" in log[-1][0]) == name.startswith("rt") and ("sp::gemm_nt_kernel" in log[-1][0]) == (entry == "split"), (name, rc, log)
        y = _win(ybuf, (M, N), "y").cpu().to(F64)
        assert torch.equal(y[others], ref["y"][others]), "%s: the NaN in x[%d] reached another row of y" % (name, r)
        assert bool(torch.isnan(y[r]).all()), "%s: the NaN in x[%d] did not reach its own row" % (name, r)
        if entry == "split":
            continue
        gr = gy.clone()
        gr[r, 3] = NAN
        rc, blog, got = run_bwd(ops, _in(x), K, dw_, dy, _in(gr), M, K, N, 0, p, {})
        assert rc == 0 and ("rt::gemm_tn_kernel" in blog[1][0]) == (name == "rt-dw"), (name, rc, blog)
        dx = got["d_x"].cpu().to(F64)
        assert torch.equal(dx[others], ref["d_x"][others]), "%s: the NaN in gy[%d] reached another row of d_x" % (name, r)
        kept = (mask[r] > 0) if mask is not None else torch.ones(K, dtype=torch.bool)
        assert bool(torch.isnan(dx[r][kept]).all()), "%s: the NaN in gy[%d] did not reach its own row" % (name, r)


# (id, entry, M, K, N, the engine masks by bit-and / select)
DROPPED_CASES = [("lds", "plain", 130, 64, 18, False), ("rt-fwd", "plain", 1153, 64, 18, True), ("rt-dw", "plain", 4100, 64, 18, True),
                 ("rt-dw-noshare", "plain", 4100, 96, 18, True), ("split", "split", 1153, 128, 18, True)]


@gpu
@pytest.mark.parametrize("case", DROPPED_CASES, ids=lambda c: c[0])
def test_a_nan_in_a_dropped_element(ops, case):
    """p = 0.5, a NaN in dropped elements of x (one in a full chunk, one in the last row: the row tail of the last split).  The
    register-tile and split engines keep or clear the BITS of x: y and d_w are the clean run's.  The LDS-tile kernels multiply by the
    mask's 0: the NaN arrives in its row of y and its column of d_w, and nowhere else.  ([rt-fwd]: M < 4096, its d_w is the LDS tile's)"""
    name, entry, M, K, N, bitwise = case
    x, w, b, gy = operands(M, K, N)
    mask = mask_of(ops, 0.5, M, K)
    ref = formulas(x, w, b, gy, 1, mask)
    hits = [(r, int((mask[r] == 0).nonzero()[-1])) for r in (70, M - 1)]
    xr = x.clone()
    for r, c in hits:
        xr[r, c] = NAN
    dx_, dw_, db_, dgy, dy = _in(xr), _in(w), _in(b), _in(gy), _in(ref["y"])
    rc, log, ybuf = run_fwd(ops, entry, dx_, K, dw_, db_, M, K, N, 1, 0.5)
    assert rc == 0 and ("linear_fwd_kernel" in log[-1][0]) == (name == "lds"), (name, rc, log)
    y = _win(ybuf, (M, N), "y").cpu().to(F64)
    if entry == "plain":
        rc, blog, got = run_bwd(ops, dx_, K, dw_, dy, dgy, M, K, N, 1, 0.5, {}, False)
        assert rc == 0 and ("rt::gemm_tn_kernel" in blog[0][0]) == name.startswith("rt-dw"), (name, rc, blog)
    else:
        rc, blog, got = run_dw_split(ops, dx_, K, dy, dgy, M, K, N, 1, 0.5, {})
        assert rc == 0 and "sp::gemm_tn_shared_kernel" in blog[1][0], (name, rc, blog)
    d_w = got["d_w"].cpu().to(F64)
    if bitwise:
        assert torch.equal(y, ref["y"]), "%s: a dropped NaN reached y" % name
    else:
        rows = [r for r, _ in hits]
        clean = [i for i in range(M) if i not in rows]
        # (relu: fmaxf(NaN, 0) = 0, so the row reads 0 where the clean run may not)
        assert torch.equal(y[clean], ref["y"][clean]) and bool(((y[rows] == 0) | torch.isnan(y[rows])).all()) and not torch.equal(y[rows], ref["y"][rows])
    if bitwise and name != "rt-fwd":
        assert torch.equal(d_w, ref["d_w"]), "%s: a dropped NaN reached d_w" % name
    else:
        cols = sorted({c for _, c in hits})
        clean = [k for k in range(K) if k not in cols]
        assert torch.equal(d_w[:, clean], ref["d_w"][:, clean]), "%s: the NaN left its columns of d_w" % name
        # a column is NaN wherever a row of gz that meets the NaN is not dropped by the gate: gz * NaN, and 0 * NaN, are NaN
        assert bool(torch.isnan(d_w[:, cols]).all()), name
    assert torch.equal(got["d_b"].cpu().to(F64), ref["d_b"])


@gpu
def test_refusals_launch_nothing(ops, lib_option):
    """every VQA_REQUIRE of the ten entry points: null pointers, sizes <= 0, odd K / N / ldx, ldx < K, a bad act, p outside [0, 1),
    pointers off by 4 and by 8 bytes, a workspace one byte short, gz_out with act = 0, act = 1 without y, shapes outside
    *_supported.  Each returns its code and an error text, launches nothing and leaves the outputs alone.  Every buffer is as large
    as the refused call would have needed"""
    Lb = ops._lib.lib()
    n = 1 << 21
    src = torch.zeros(n, device=dev())
    outs = [_sentinel(n) for _ in range(3)]
    ws = _sentinel(1 << 22)
    logbuf = (ctypes.c_ulonglong * 16)()

    def refused(code, fn, *args):
        Lb.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, code, args, Lb.vqa_last_error())
        assert Lb.vqa_last_error() and Lb.vqa_launch_log(logbuf, 16) == 0, ("a refused call launched a kernel", fn.__name__, args)

    def ptrs(spec, null, mis, by):
        """spec: the pointer arguments' tensors, in order; `null`: index set to NULL; `mis`: index moved `by` bytes"""
        v = [_ptr(t) for t in spec]
        if null is not None:
            v[null] = None
        if mis is not None:
            v[mis] = ctypes.c_void_p(v[mis].value + by)
        return v

    def fwd(M=70, K=18, N=34, ldx=None, act=1, p=0.5, null=None, mis=None, by=4):
        x, w, b, y = ptrs((src, src, src, outs[0]), null, mis, by)
        return (Lb.vqa_linear_act_fwd, x, K if ldx is None else ldx, w, b, y, M, K, N, act, p, SEED, None)

    def bwd(M=70, K=18, N=34, ldx=None, act=1, p=0.5, null=None, mis=None, by=4, short=0):
        x, w, y, gy, dx, dw, db, wsp = ptrs((src, src, src, src, outs[0], outs[1], outs[2], ws), null, mis, by)
        need = Lb.vqa_linear_act_bwd_workspace_bytes(M, K, N)
        assert need <= 4 * ws.numel()
        return (Lb.vqa_linear_act_bwd, x, K if ldx is None else ldx, w, y, gy, dx, dw, db, wsp, (need or 1 << 20) - short, M, K, N, act, p, SEED, None)

    def fwd_split(M=1152, K=128, N=16, ldx=None, act=1, p=0.5, null=None, mis=None, by=4, short=0):
        x, w, b, y, wsp = ptrs((src, src, src, outs[0], ws), null, mis, by)
        need = Lb.vqa_linear_act_fwd_split_workspace_bytes(K, N) if K > 0 and N > 0 else 1 << 20
        return (Lb.vqa_linear_act_fwd_split, x, K if ldx is None else ldx, w, b, y, wsp, need - short, M, K, N, act, p, SEED, None)

    def dw_split(M=1152, K=128, N=16, ldx=None, act=1, p=0.5, null=None, mis=None, by=4, short=0, gz=True):
        x, y, gy, dw, db, gzp, wsp = ptrs((src, src, src, outs[0], outs[1], outs[2], ws), null, mis, by)
        need = Lb.vqa_linear_act_dw_split_workspace_bytes(M, K, N) if min(M, K, N) > 0 else 1 << 20
        assert need <= 4 * ws.numel()
        return (Lb.vqa_linear_act_dw_split, x, K if ldx is None else ldx, y, gy, dw, db, gzp if gz else None, wsp, need - short, M, K, N, act, p, SEED, None)

    def rel_fwd(B=144, Nr=8, D=128, L=16, act=1, p=0.5, null=None, mis=None, by=4, short=0):
        v, t, c2, w, b, y, wsp = ptrs((src, src, src, src, src, outs[0], ws), null, mis, by)
        need = Lb.vqa_linear_act_fwd_split_workspace_bytes(D, L) if D > 0 and L > 0 else 1 << 20
        return (Lb.vqa_relation_linear_fwd_split, v, t, c2, w, b, y, wsp, need - short, B, Nr, D, L, act, p, SEED, None)

    def rel_dw(B=144, Nr=8, D=128, L=16, act=1, p=0.5, null=None, mis=None, by=4, short=0, gz=True):
        v, t, c2, y, gy, dw, db, gzp, wsp = ptrs((src, src, src, src, src, outs[0], outs[1], outs[2], ws), null, mis, by)
        need = Lb.vqa_linear_act_dw_split_workspace_bytes(B * Nr, D, L) if min(B * Nr, D, L) > 0 else 1 << 20
        return (Lb.vqa_relation_linear_dw_split, v, t, c2, y, gy, dw, db, gzp if gz else None, wsp, need - short, B, Nr, D, L, act, p, SEED, None)

    # ---- vqa_linear_act_fwd / _bwd: bias, d_x and d_b may be NULL
    for i in (0, 1, 3):
        refused(E_BADARG, *fwd(null=i))
    for i in (0, 1, 2, 3, 5, 7):
        refused(E_BADARG, *bwd(null=i))
    for make in (fwd, bwd):
        for kw in (dict(M=0), dict(K=0), dict(N=-2), dict(act=2), dict(act=-1), dict(p=1.0), dict(p=-0.25), dict(p=1.5)):
            refused(E_BADARG, *make(**kw))
        for kw in (dict(K=17, ldx=18), dict(N=33), dict(ldx=19), dict(ldx=16), dict(mis=0), dict(mis=1)):
            refused(E_UNSUPPORTED, *make(**kw))
    refused(E_UNSUPPORTED, *fwd(mis=3))
    for i in (2, 3, 4, 5, 6):                        # y, gy, d_x, d_w, d_b by 4 bytes; the workspace by 4 and by 8 (it needs 16)
        refused(E_UNSUPPORTED, *bwd(mis=i))
    refused(E_UNSUPPORTED, *bwd(mis=7))
    refused(E_UNSUPPORTED, *bwd(mis=7, by=8))
    refused(E_BADARG, *bwd(short=1))
    lib_option("VQA_RT_DW_SPLITS", "64")             # (the query's larger figure is what the call asks for)
    refused(E_BADARG, *bwd(M=4100, K=64, N=18, short=1))
    lib_option("VQA_RT_DW_SPLITS", None)
    assert Lb.vqa_linear_act_bwd_workspace_bytes(0, 18, 34) == 0 == Lb.vqa_linear_act_bwd_workspace_bytes(70, 18, -1)
    # ---- vqa_linear_dropout_mask
    for args in ((None, 0.5, SEED, None, 70, 18), (_ptr(outs[0]), 0.5, SEED, None, 0, 18), (_ptr(outs[0]), 0.5, SEED, None, 70, 0),
                 (_ptr(outs[0]), 0.5, SEED, None, 70, 17), (_ptr(outs[0]), 1.0, SEED, None, 70, 18), (_ptr(outs[0]), -0.5, SEED, None, 70, 18)):
        refused(E_BADARG, Lb.vqa_linear_dropout_mask, *args)
    # ---- the split engine: 16 bytes for x, w, d_w and the workspace (off by 4 and by 8), 8 for y, gy, gz_out
    for i in (0, 1, 3, 4):
        refused(E_BADARG, *fwd_split(null=i))
    refused(E_BADARG, *fwd_split(act=2))
    refused(E_BADARG, *fwd_split(short=1))
    shapes = (dict(M=1151), dict(K=64), dict(K=160), dict(N=14), dict(N=17), dict(N=482), dict(ldx=130), dict(ldx=124), dict(p=0.75), dict(p=0.3),
              dict(M=0), dict(K=0, ldx=128), dict(N=0))
    for kw in shapes:
        assert Lb.vqa_linear_split_supported(kw.get("M", 1152), kw.get("K", 128), kw.get("N", 16), kw.get("ldx", kw.get("K", 128)), kw.get("p", 0.5)) == 0, kw
        refused(E_UNSUPPORTED, *fwd_split(**kw))
        refused(E_UNSUPPORTED, *dw_split(**kw))
    assert Lb.vqa_linear_split_supported(1152, 128, 480, 132, 0.5) == 1 == Lb.vqa_linear_split_supported(1152, 192, 16, 192, 0.0)
    refused(E_UNSUPPORTED, *dw_split(K=192))          # the forward's K % 64 == 0 is not enough for the weight gradient
    for i, by in ((0, 4), (0, 8), (1, 4), (1, 8), (3, 4), (4, 4), (4, 8)):
        refused(E_UNSUPPORTED, *fwd_split(mis=i, by=by))
    for i in (0, 2, 3, 6):                             # (y: asked for by act = 1, below; d_b and gz_out may be NULL)
        refused(E_BADARG, *dw_split(null=i))
    refused(E_BADARG, *dw_split(null=1))              # act = 1 without y
    refused(E_BADARG, *dw_split(act=0))               # gz_out with act = 0
    refused(E_BADARG, *dw_split(act=2, gz=False))
    refused(E_BADARG, *dw_split(mis=5))               # gz_out off by 4
    refused(E_BADARG, *dw_split(short=1))
    for i, by in ((0, 4), (0, 8), (1, 4), (2, 4), (3, 4), (3, 8), (6, 4), (6, 8)):
        refused(E_UNSUPPORTED, *dw_split(mis=i, by=by))
    # ---- the fused relation forms
    for i in (0, 1, 2, 3, 5, 6):
        refused(E_BADARG, *rel_fwd(null=i))
    for i in (0, 1, 2, 4, 5, 8):
        refused(E_BADARG, *rel_dw(null=i))
    refused(E_BADARG, *rel_dw(null=3))                # act = 1 without y
    refused(E_BADARG, *rel_dw(act=0))                 # gz_out with act = 0
    refused(E_BADARG, *rel_fwd(act=2))
    refused(E_BADARG, *rel_fwd(short=1))
    refused(E_BADARG, *rel_dw(short=1))
    for kw in (dict(B=0), dict(Nr=7, B=165), dict(Nr=1025, B=2), dict(B=143), dict(D=768), dict(D=192), dict(D=64), dict(L=14), dict(L=482), dict(p=0.75)):
        assert Lb.vqa_relation_linear_split_supported(kw.get("B", 144), kw.get("Nr", 8), kw.get("D", 128), kw.get("L", 16), kw.get("p", 0.5)) == 0, kw
        refused(E_UNSUPPORTED, *rel_fwd(**kw))
        refused(E_UNSUPPORTED, *rel_dw(**kw))
    assert Lb.vqa_relation_linear_split_supported(144, 8, 640, 16, 0.5) == 1 == Lb.vqa_relation_linear_split_supported(2, 1024, 128, 16, 0.0)
    for i, by in ((0, 4), (0, 8), (1, 4), (1, 8), (2, 4), (2, 8), (3, 4), (3, 8), (5, 4), (6, 4), (6, 8)):
        refused(E_UNSUPPORTED, *rel_fwd(mis=i, by=by))
    for i, by in ((0, 4), (0, 8), (1, 4), (1, 8), (2, 4), (2, 8), (3, 4), (4, 4), (5, 4), (5, 8), (8, 4), (8, 8)):
        refused(E_UNSUPPORTED, *rel_dw(mis=i, by=by))
    refused(E_BADARG, *rel_dw(mis=7))                 # gz_out off by 4
    torch.cuda.synchronize()
    for t in outs:
        assert _untouched(t)
    assert _untouched(ws)
    # ... and the same builders are accepted when nothing is wrong with them
    for call, launches in ((fwd(), 1), (bwd(), 3), (fwd_split(), 2), (dw_split(), 3), (rel_fwd(), 2), (rel_dw(), 3), (dw_split(act=0, gz=False, null=1), 3)):
        Lb.vqa_launch_log_reset()
        assert call[0](*call[1:], None) == 0 and Lb.vqa_launch_log(logbuf, 16) == launches, (call[0].__name__, Lb.vqa_last_error())
    torch.cuda.synchronize()
