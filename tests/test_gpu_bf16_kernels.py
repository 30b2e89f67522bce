"""The bf16 GEMM engine and the bf16 K4 kernels (csrc/bf16_path.hip, csrc/gemm_bf16_mfma.hpp, csrc/bilinear_fold_bf16.hip) pinned
to exact references, one dispatch form at a time.  tests/test_gpu_bf16.py holds the same kernels to 2e-2 / 2^-8 of a tensor's scale
at a handful of shapes; here

  A  small-integer operands (|v| <= 4: bf16 for matrices and gradients, fp32 for h2, biases, b1): every fp32 sum a kernel forms is
     an integer below 2^24, exact in any accumulation order, every bf16 store one rounding of an exact value.  The reference is
     int64 arithmetic on the CPU; fp32 outputs equal it bit for bit, bf16 outputs equal ref.float().to(bfloat16) bit for bit, and
     where a kernel reuses a rounded bf16 intermediate (h1 in the R-GEMM backward) the reference rounds at the same point.  An
     integer has one zero: a -0.0 of the kernel (0 * -3 summed with another -0) counts as the reference's 0, nothing else does.
     Outputs sit in sentinel-filled buffers that are compared whole, so a store outside the window fails the test.
       A1 vqa_gemm_bf16_nt / _nt_ex: tile shape x M x N x K, both store paths, bias / relu / gate, in-kernel dropout
       A2 vqa_gemm_bf16_tn / _tn_ex: tile choice x staging form x K (split counts, short and EMPTY last splits), groups, dropout
       A3 K4 as R GEMMs through the C ABI: fwd2 / generic forward, every prep kernel, gate_dx, d_x = NULL, phases 1 + 2 == 3
       A4 K4 rank-folded through the C ABI: every NB 1..8 and (LBW, NCH) instantiation, H % 256 != 0, empty and one-sample slabs
       A5 vqa_pack_bf16 / ShadowPlan.pack: plain, transposed (several 32 x 32 tiles, partial ones), offsets, both kinds, ties
  B  random bf16 operands against float64 with the project's bar (Bars: WorstBar of tests/kernel_harness.py): four times
     the error of the same formula in float32 with torch on the CPU plus one float32 ulp; bf16 outputs elementwise within
     2^-8 |ref| + that bar x scale.  The bf16 intermediates are REMOVED from the comparison: the R-GEMM backward's reference reads
     the kernel's own h1 and forms bf16(float32(g * h2)) as the kernel does; the fold draws h2 from +-{1/4 .. 4}, so that the folded
     weight bf16(float32 sum) computed on the CPU is the kernel's operand bit for bit.
  C  non-finite isolation (a NaN stays in its row / its sample) and refusals (documented code, no launch, outputs untouched).

Which launch each case makes is asserted from the library's launch log (kernel expression and grid), so a dispatch change that
would leave a form untested fails here.  Dispatch form -> the test that launches it (and asserts that it did):

  gemm_bf16_nt_kernel<BM,BN,BfNoTransform>   4 tile shapes x {16-byte image store, scalar store}: test_nt_small_integers_are_exact
      [tile-*] (N = 8 and N = 70, where ldc % 8 != 0: scalar only; N = 64, 72, 136: whole column tiles through the image, the last
      partial one scalar, in one launch; gate stride N + 3 and c one element off: the aligned path refused at run time); the
      default choice bm = 64 (M <= 64) / 128 in [tile-default],
      bn = 128 / 64 at N = 1024 in test_nt_default_choice_of_the_column_tile
  gemm_bf16_nt_kernel<BM,BN,BfDropHalf>      4 tile shapes (CA = 2 and 4): test_nt_dropout_small_integers_are_exact[tile-*]
  gemm_bf16_tn_kernel<BM,BN,BfNoTransform,TR>  64 / 128 on each side x TR in {true, false (perm)}: test_tn_small_integers_are_exact
      [N1-N2-staging-*], test_tn_tile_override_small_integers_are_exact (every shape on one product), S = 1, 2, 3;
      S = 64 with empty splits: test_tn_empty_splits_write_zero_slabs; 25 slabs: test_tn_random_operands_against_float64
  gemm_bf16_tn_kernel<BM,BN,BfDropHalf,TR>   BM in {64, 128} x BN in {64, 128} x both stagings: test_tn_dropout_small_integers_are_exact
  slab_reduce_kernel                         groups, crop, float2 tail: test_tn_groups_crop_into_their_windows; K4's bias job: A3
  bilinear_fwd2_bf16_kernel / bilinear_fwd_bf16_kernel<BM,BN>   test_k4_rgemm_small_integers_are_exact (K4_SHAPES names the
      kernel of each shape), test_k4_generic_forward_under_every_tile (<64,64>, <64,128>, <128,64>)
  bilinear_bwd_prep8_bf16_kernel<1..5>, bilinear_bwd_prep_bf16_kernel<16>, <4>   test_k4_rgemm_small_integers_are_exact, each at a
      shape with idle region slices (N = 7, N = 1) and at one where every slice works (N = 37, N = 4)
  fold_fwd_kernel<NB>, fold_dx_kernel<NB> (NB = 1..8), fold_dw_kernel<LBW,NCH> (5 x 4), fold_finish_kernel
      test_fold_small_integers_are_exact (FOLD_SHAPES; test_fold_shape_table_covers_every_instantiation counts them)
  pack_bf16_kernel, pack_many_kernel (plain and 32 x 32 transposed path)   test_pack_many_and_pack_bf16_round_to_even_into_their_windows"""
import ctypes
import functools

import pytest
import torch

from kernel_harness import (BF, E_BADARG, E_UNSUPPORTED, INF, NAN, SENT, WorstBar as Bars, _amax, _below_2_24, _dbf, _logged, _names, _ptr,
                            _ptrs, _same_bits, _sentinel, _take, _untouched, assert_exact, dev, ops)  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu
TILES = [None, "128x128", "128x64", "64x128", "64x64"]
_tile_id = lambda t: "tile-" + (t or "default")      # noqa: E731


def _ints(gen, *shape, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=gen)


def _df(t):
    return t.to(torch.float32).to(dev()).contiguous()


# ======================================================================================================================= A1: NT
@functools.lru_cache(maxsize=None)
def nt_operands(M, N, K):
    """int64 on the CPU: a [M,K], b [N,K], bias [N], gate [M,N+3] (float: integers, with 0, -0 and negative entries)"""
    gen = torch.Generator().manual_seed(10007 * M + 101 * N + K)
    a, b, bias = _ints(gen, M, K), _ints(gen, N, K), _ints(gen, N)
    gate = _ints(gen, M, N + 3).float()
    gate[::3, ::5] = -0.0
    gate[1::4, 2::3] = 0.0
    return a, b, bias, gate


def nt_reference(a, b, bias, act, gate, mask):
    """int64: act((a o mask) b^T + bias) o (gate > 0); mask holds the dropout's 0 / 2"""
    K = a.shape[1]
    _below_2_24((2 if mask is not None else 1) * _amax(a) * _amax(b) * K + (_amax(bias) if bias is not None else 0))
    ref = (a if mask is None else a * mask) @ b.T
    if bias is not None:
        ref = ref + bias
    if act:
        ref = ref.clamp_min(0)
    if gate is not None:
        ref = ref * (gate[:, :b.shape[0]] > 0)
    return ref


def run_nt(ops, a_d, b_d, M, N, K, ldc, bias_d=None, act=0, gate_d=None, ldg=0, p_drop=0.0, seed=0, c_off=0):
    """vqa_gemm_bf16_nt (or _nt_ex when a gate or dropout is asked for) with c inside a sentinel-filled [M + 3, ldc] buffer that
    starts c_off elements into its allocation -> (c [M,N], launch log)"""
    L = ops._lib.lib()
    buf = _sentinel((M + 3) * ldc + 8, dtype=BF)
    assert buf.data_ptr() % 16 == 0
    if gate_d is None and not p_drop:
        log = _logged(L, lambda: ops._launch("gemm_bf16_nt", (M, N, K, act), L.vqa_gemm_bf16_nt, _ptr(a_d), K, _ptr(b_d), K, _ptr(bias_d),
                                             _ptr(buf, c_off), ldc, M, N, K, act))
    else:
        log = _logged(L, lambda: ops._launch("gemm_bf16_nt", (M, N, K, act), L.vqa_gemm_bf16_nt_ex, _ptr(a_d), K, _ptr(b_d), K,
                                             _ptr(bias_d), _ptr(buf, c_off), ldc, M, N, K, act, _ptr(gate_d), ldg, float(p_drop),
                                             int(seed), None))
    torch.cuda.synchronize()
    assert len(log) == 1, log
    view = buf[c_off:c_off + (M + 3) * ldc].view(M + 3, ldc)
    got = view[:M, :N].clone()
    view[:M, :N] = SENT
    assert _untouched(buf), "gemm_bf16_nt M=%d N=%d K=%d ldc=%d: a store outside [M,N]" % (M, N, K, ldc)
    return got, log


def nt_tile(tile, M, N, K):
    """the tile shape launch_nt takes"""
    if tile:
        return tuple(int(v) for v in tile.split("x"))
    return (64 if M <= 64 else 128, 128 if (K <= 512 and N >= 1024) else 64)


# variant -> (bias, relu, gate stride - N or None, ldc - N, c offset).  N = 70: ldc % 8 != 0 either way, every store is scalar;
# N = 72 / 136: the first column tile(s) take the 16-byte LDS-image store, the last partial one the scalar path -- unless the
# gate's stride (N + 3) or c's offset (one element: 2 bytes) refuses the aligned path at run time.
NT_VARIANTS = [(False, False, None, 0, 0), (True, False, None, 8, 0), (True, True, None, 0, 0), (False, False, 0, 8, 0),
               (True, True, 3, 0, 0), (True, False, None, 8, 1)]
NT_MS, NT_NS = (1, 63, 64, 65, 129), (8, 64, 70, 72, 136)


@pytest.mark.parametrize("tile", TILES, ids=_tile_id)
def test_nt_small_integers_are_exact(ops, lib_option, tile):
    """every M meets every N under every tile shape, each pair in all six variants; K alternates between 64 (one stage) and 192
    (three: the odd tail stage)"""
    if tile:
        lib_option("VQA_BF16_TILE", tile)
    for im, M in enumerate(NT_MS):
        for jn, N in enumerate(NT_NS):
            for v, (with_bias, relu, gate_pad, ldc_pad, c_off) in enumerate(NT_VARIANTS):
                K = (64, 192)[(im + jn + v) % 2]
                a, b, bias, gate = nt_operands(M, N, K)
                ldg = N + gate_pad if gate_pad is not None else 0
                gate_d = _dbf(gate[:, :ldg]) if gate_pad is not None else None
                got, log = run_nt(ops, _dbf(a), _dbf(b), M, N, K, N + ldc_pad, _df(bias) if with_bias else None, int(relu), gate_d, ldg,
                                  c_off=c_off)
                bm, bn = nt_tile(tile, M, N, K)
                assert log[0][0] == "(gemm_bf16_nt_kernel<%d,%d,BfNoTransform>)" % (bm, bn), (log, M, N, K)
                assert log[0][1] == -(-M // bm) * -(-N // bn) * 256, (log, M, N, K)
                ref = nt_reference(a, b, bias if with_bias else None, relu, gate[:, :ldg] if gate_pad is not None else None, None)
                assert_exact("nt %s M=%d N=%d K=%d variant %d" % (_tile_id(tile), M, N, K, v), got, ref)


@pytest.mark.parametrize("K,bn", [(512, 128), (576, 64)])
def test_nt_default_choice_of_the_column_tile(ops, K, bn):
    """N >= 1024: K <= 512 lands on bn = 128, K = 576 on bn = 64; with ldc = N (image store) and ldc = N + 8"""
    M, N = 65, 1024
    a, b, bias, _ = nt_operands(M, N, K)
    ref = nt_reference(a, b, bias, True, None, None)
    for ldc in (N, N + 8):
        got, log = run_nt(ops, _dbf(a), _dbf(b), M, N, K, ldc, _df(bias), 1)
        assert log[0] == ("(gemm_bf16_nt_kernel<128,%d,BfNoTransform>)" % bn, (N // bn) * 256), log
        assert_exact("nt M=65 N=1024 K=%d ldc=%d" % (K, ldc), got, ref)


@pytest.mark.parametrize("tile", TILES, ids=_tile_id)
def test_nt_dropout_small_integers_are_exact(ops, lib_option, tile):
    """p = 0.5 inside the stager (BfDropHalf): the quad exchange of hash words with CA = 2 (64-row tiles) and CA = 4 (128-row
    tiles); M = 40 and 65 leave clamped rows in the tile; the mask is the one vqa_linear_dropout_mask exports"""
    if tile:
        lib_option("VQA_BF16_TILE", tile)
    for i, (M, N, K) in enumerate([(40, 64, 64), (40, 72, 192), (65, 64, 192), (65, 72, 64), (65, 136, 192)]):
        a, b, bias, _ = nt_operands(M, N, K)
        seed = 777 + 13 * i
        mask = ops.linear_dropout_mask(M, K, 0.5, seed, dev()).cpu()
        assert set(torch.unique(mask).tolist()) == {0.0, 2.0}
        got, log = run_nt(ops, _dbf(a), _dbf(b), M, N, K, N + 8 * (i % 2), _df(bias), i % 2, p_drop=0.5, seed=seed)
        assert log[0][0] == "(gemm_bf16_nt_kernel<%d,%d,BfDropHalf>)" % nt_tile(tile, M, N, K), log
        assert_exact("nt dropout %s M=%d N=%d K=%d" % (_tile_id(tile), M, N, K), got, nt_reference(a, b, bias, i % 2, None, mask.long()))


# ======================================================================================================================= A2: TN
@functools.lru_cache(maxsize=None)
def tn_operands(K, N1, N2):
    gen = torch.Generator().manual_seed(20011 * N1 + 211 * N2 + K)
    a, b = _ints(gen, K, N1), _ints(gen, K, N2)
    _below_2_24(2 * _amax(a) * _amax(b) * K)
    return a, b, a.T @ b


def run_tn(ops, a_d, b_d, K, N1, N2, window=None, p_drop=0.0, seed=0):
    """vqa_gemm_bf16_tn (window None: c dense [N1,N2], 16 elements into a sentinel-filled buffer) or vqa_gemm_bf16_tn_ex
    (window = (groups, out_rows, out_cols): every group into its own sentinel-filled [out_rows + 2, out_cols + 3] tensor); the
    workspace is NaN-filled, so a slab (or a part of one) that no workgroup writes poisons the sum -> (result, slabs, launch log)"""
    L = ops._lib.lib()
    ws_bytes = L.vqa_gemm_bf16_tn_workspace_bytes(K, N1, N2)
    assert ws_bytes > 0 and ws_bytes % (4 * N1 * N2) == 0
    ws = torch.full((ws_bytes // 4,), NAN, device=dev())
    if window is None:
        c = _sentinel(N1 * N2 + 32)
        log = _logged(L, lambda: ops._launch("gemm_bf16_tn", (K, N1, N2), L.vqa_gemm_bf16_tn, _ptr(a_d), N1, _ptr(b_d), N2, _ptr(c, 16),
                                             _ptr(ws), ws_bytes, K, N1, N2))
        torch.cuda.synchronize()
        got = _take(c, slice(16, 16 + N1 * N2), "gemm_bf16_tn").view(N1, N2)
    else:
        groups, out_rows, out_cols = window
        outs = [_sentinel(out_rows + 2, out_cols + 3) for _ in range(groups)]
        log = _logged(L, lambda: ops._launch("gemm_bf16_tn", (K, N1, N2), L.vqa_gemm_bf16_tn_ex, _ptr(a_d), N1, _ptr(b_d), N2, _ptrs(outs),
                                             groups, N1 // groups, out_rows, out_cols, out_cols + 3, _ptr(ws), ws_bytes, K, N1, N2,
                                             float(p_drop), int(seed), None))
        torch.cuda.synchronize()
        got = torch.stack([_take(o, (slice(0, out_rows), slice(0, out_cols)), "gemm_bf16_tn_ex group") for o in outs])
    assert len(log) == 2 and log[1][0] == "slab_reduce_kernel", log
    return got, ws_bytes // (4 * N1 * N2), log


def tn_kernel(N1, N2, xb, form):
    return "(gemm_bf16_tn_kernel<%d,%d,%s,%s>)" % (128 if N1 > 64 else 64, 128 if N2 > 64 else 64, xb, "false" if form == "perm" else "true")


def _set_form(lib_option, form):
    if form:
        lib_option("VQA_BF16_TN", form)


FORMS = [None, "perm"]
_form_id = lambda f: "staging-" + (f or "tr")      # noqa: E731


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("N1,N2", [(8, 8), (64, 72), (72, 64), (136, 392), (392, 136)], ids=lambda v: str(v))
def test_tn_small_integers_are_exact(ops, lib_option, N1, N2, form):
    """tile choices 64 / 128 on each side, tiles_m_fast on and off, partial tiles; K = 1 .. 65 is one split with a short stage,
    513 and 1025 are S = 2 and 3 with a last split of one row"""
    _set_form(lib_option, form)
    for K, S in ((1, 1), (63, 1), (64, 1), (65, 1), (513, 2), (1025, 3)):
        a, b, ref = tn_operands(K, N1, N2)
        got, slabs, log = run_tn(ops, _dbf(a), _dbf(b), K, N1, N2)
        tiles = -(-N1 // (128 if N1 > 64 else 64)) * -(-N2 // (128 if N2 > 64 else 64))
        assert slabs == S and log[0] == (tn_kernel(N1, N2, "BfNoTransform", form), tiles * S * 256), (K, slabs, log)
        assert_exact("tn K=%d N1=%d N2=%d %s" % (K, N1, N2, _form_id(form)), got, ref)


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
def test_tn_empty_splits_write_zero_slabs(ops, lib_option, form):
    """K = 33000 at N1 = N2 = 64: S is capped at 64 and the rows per split round up to 576, so splits 58 .. 63 start past the last
    row (k_lo > K).  They must stage nothing and write zero slabs (the workspace starts as NaN); twice, same bits."""
    _set_form(lib_option, form)
    K, N1, N2 = 33000, 64, 64
    a, b, ref = tn_operands(K, N1, N2)
    assert 57 * 576 < K < 58 * 576
    a_d, b_d = _dbf(a), _dbf(b)
    got, slabs, log = run_tn(ops, a_d, b_d, K, N1, N2)
    assert slabs == 64 and log[0] == (tn_kernel(N1, N2, "BfNoTransform", form), 64 * 256), (slabs, log)
    assert_exact("tn K=33000", got, ref)
    again, _, _ = run_tn(ops, a_d, b_d, K, N1, N2)
    assert _same_bits(got, again), "two runs of the split-K reduction differ"


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("groups,rpg,N2", [(2, 64, 72), (3, 72, 64), (2, 136, 136)])
def test_tn_groups_crop_into_their_windows(ops, lib_option, groups, rpg, N2, form):
    """_tn_ex: R = 2 and 3 groups, out_rows < rows_per_group, an odd out_cols < N2 (the float2 tail of the reduction)"""
    _set_form(lib_option, form)
    K, N1 = 130, groups * rpg
    out_rows, out_cols = rpg - 6, N2 - 5
    assert out_cols % 2 == 1
    a, b, ref = tn_operands(K, N1, N2)
    got, _, _ = run_tn(ops, _dbf(a), _dbf(b), K, N1, N2, (groups, out_rows, out_cols))
    assert_exact("tn_ex groups", got, ref.view(groups, rpg, N2)[:, :out_rows, :out_cols].contiguous())


@pytest.mark.parametrize("form", FORMS, ids=_form_id)
@pytest.mark.parametrize("N2", [32, 64, 160])
def test_tn_dropout_small_integers_are_exact(ops, lib_option, N2, form):
    """p = 0.5 on b while it is staged, BN = 64 (N2 = 32: half a tile, N2 = 64) and BN = 128 (N2 = 160: one whole and one partial
    tile), under BM = 64 and 128; K = 65 is one split with a one-row stage, K = 600 two splits"""
    _set_form(lib_option, form)
    for i, (K, N1) in enumerate([(65, 64), (600, 72), (600, 64)]):
        a, b, _ = tn_operands(K, N1, N2)
        seed = 4242 + 7 * i + N2
        mask = ops.linear_dropout_mask(K, N2, 0.5, seed, dev()).cpu()
        assert set(torch.unique(mask).tolist()) == {0.0, 2.0}
        got, slabs, log = run_tn(ops, _dbf(a), _dbf(b), K, N1, N2, (1, N1, N2), 0.5, seed)
        assert slabs == (1 if K < 512 else 2) and log[0][0] == tn_kernel(N1, N2, "BfDropHalf", form), (slabs, log)
        assert_exact("tn dropout K=%d N1=%d N2=%d" % (K, N1, N2), got[0], a.T @ (b * mask.long()))


def test_tn_tile_override_small_integers_are_exact(ops, lib_option):
    """VQA_BF16_TILE reaches the TN launcher too: every shape on a product whose edges are partial under each of them"""
    K, N1, N2 = 513, 136, 72
    a, b, ref = tn_operands(K, N1, N2)
    for tile in TILES[1:]:
        lib_option("VQA_BF16_TILE", tile)
        for form in FORMS:
            lib_option("VQA_BF16_TN", form)
            got, _, log = run_tn(ops, _dbf(a), _dbf(b), K, N1, N2)
            bm, bn = (int(v) for v in tile.split("x"))
            assert log[0][0] == "(gemm_bf16_tn_kernel<%d,%d,BfNoTransform,%s>)" % (bm, bn, "false" if form else "true"), log
            assert_exact("tn %s %s" % (tile, _form_id(form)), got, ref)


# ======================================================================================================================= A3: K4 as R GEMMs
def pad_h2(h2, H):
    out = h2.new_zeros(h2.shape[0], h2.shape[1], H)
    out[..., :h2.shape[2]] = h2
    return out


@functools.lru_cache(maxsize=None)
def k4_operands(shape):
    """int64 on the CPU: x [B,N,L], w1 [R,H,L], b1 [R,H], h2 [B,R,H_in], g [B,N,H]; H_in = H - 6 and L_out = L - 3 are the
    master shape.  The pads hold values like everything else: the kernels' contract is the arithmetic over the padded shapes with
    h2 zero past H_in, and a column that leaks shows."""
    B, N, L, H, R = shape
    gen = torch.Generator().manual_seed(30011 * B + 307 * N + L + H + 7 * R)
    return {"x": _ints(gen, B, N, L), "w1": _ints(gen, R, H, L), "b1": _ints(gen, R, H), "h2": _ints(gen, B, R, H - 6),
            "g": _ints(gen, B, N, H), "Hin": H - 6, "Lout": L - 3}


def k4_device(case):
    w1 = case["w1"]
    R, H, L = w1.shape
    return {"x": _dbf(case["x"]), "w1": _dbf(w1), "b1": _df(case["b1"]), "h2": _df(case["h2"]), "g": _dbf(case["g"]),
            "w1t": _dbf(w1.permute(2, 0, 1).reshape(L, R * H))}


def bf_round_int(t):
    """int64 -> the integer its bf16 rounding holds"""
    _below_2_24(_amax(t))
    return t.float().to(BF).float().to(torch.int64)


@functools.lru_cache(maxsize=None)
def k4_rgemm_reference(shape):
    """int64: out, h1 (before its rounding), and the backward formed from bf16(h1) as the kernel forms it"""
    B, N, L, H, R = shape
    c = k4_operands(shape)
    x, w1, b1, g, Hin, Lout = c["x"], c["w1"], c["b1"], c["g"], c["Hin"], c["Lout"]
    h2 = pad_h2(c["h2"], H)
    _below_2_24(R * 4 * (16 * L + 4), 4 * N * (16 * L + 4), 64 * R * H, 64 * B * N, 16 * N * B)
    hv = torch.einsum("bnl,rhl->bnrh", x, w1) + b1
    out = (hv * h2[:, None]).sum(2)
    h1 = bf_round_int(hv)
    gs = g[:, :, None, :] * h2[:, None]                                # <= 16: exact in bf16
    d_x = torch.einsum("bnrh,rhl->bnl", gs, w1)
    return {"out": out, "h1": hv, "d_h2": torch.einsum("bnh,bnrh->brh", g, h1)[..., :Hin].contiguous(), "d_x": d_x,
            "d_x_gated": d_x * (x > 0), "d_w1": torch.einsum("bnrh,bnl->rhl", gs, x)[:, :Hin, :Lout].contiguous(),
            "d_b1": torch.einsum("brh,bh->rh", h2, g.sum(1))[:, :Hin].contiguous()}


def k4_fwd(ops, d, shape, Hin, want_h1=True):
    """-> out [B,N,H], h1 [B,N,R,H] (both behind two sentinel rows), launch log"""
    B, N, L, H, R = shape
    L_ = ops._lib.lib()
    M = B * N
    out, h1 = _sentinel(M + 2, H, dtype=BF), (_sentinel(M + 2, R * H, dtype=BF) if want_h1 else None)
    log = _logged(L_, lambda: ops._launch("lowrank_bilinear_fusion_fwd_bf16", shape, L_.vqa_lowrank_bilinear_fusion_fwd_bf16, _ptr(d["x"]),
                                          _ptr(d["w1"]), _ptr(d["b1"]), _ptr(d["h2"]), _ptr(out), _ptr(h1), B, N, L, H, R, Hin))
    torch.cuda.synchronize()
    assert len(log) == 1, log
    got_h1 = _take(h1, slice(0, M), "K4 forward h1").view(B, N, R, H) if want_h1 else None
    return _take(out, slice(0, M), "K4 forward out").view(B, N, H), got_h1, log


def k4_bwd(ops, d, shape, Hin, Lout, h1_d, gate_dx, with_dx=True, phases=(3,)):
    """-> {d_x [B,N,L] or None, d_h2 [B,R,H_in], d_w1 [R,H_in,L_out], d_b1 [R,H_in]}, launch log.  d_w1[r] / d_b1[r] are
    master-shaped tensors with sentinel rows / elements behind them; `phases`: the calls made, in order, into one workspace."""
    B, N, L, H, R = shape
    L_ = ops._lib.lib()
    M = B * N
    ws_bytes = L_.vqa_lowrank_bilinear_fusion_bwd_bf16_workspace_bytes(B, N, L, H, R)
    ws = torch.full((ws_bytes // 4 + 64,), NAN, device=dev())
    assert ws.data_ptr() % 256 == 0
    d_x = _sentinel(M + 2, L, dtype=BF) if with_dx else None
    d_h2 = _sentinel(B * R * Hin + 16)
    d_w1, d_b1 = [_sentinel(Hin + 2, Lout) for _ in range(R)], [_sentinel(Hin + 8) for _ in range(R)]
    log = []
    for ph in phases:
        log += _logged(L_, lambda: ops._launch("lowrank_bilinear_fusion_bwd_bf16", shape, L_.vqa_lowrank_bilinear_fusion_bwd_bf16,
                                               _ptr(d["x"]), _ptr(d["w1t"]) if with_dx else None, _ptr(d["h2"]), _ptr(h1_d), _ptr(d["g"]),
                                               _ptr(d_x), _ptrs(d_w1), _ptrs(d_b1), _ptr(d_h2), _ptr(ws), ws_bytes, B, N, L, H, R, Hin, Lout,
                                               int(gate_dx), ph))
    torch.cuda.synchronize()
    return {"d_x": _take(d_x, slice(0, M), "K4 d_x").view(B, N, L) if with_dx else None,
            "d_h2": _take(d_h2, slice(0, B * R * Hin), "K4 d_h2").view(B, R, Hin),
            "d_w1": torch.stack([_take(t, slice(0, Hin), "K4 d_w1") for t in d_w1]),
            "d_b1": torch.stack([_take(t, slice(0, Hin), "K4 d_b1") for t in d_b1])}, log


# (B, N, L, H, R) -> (forward kernel, prep kernel)
K4_SHAPES = {
    (70, 2, 64, 256, 2): ("bilinear_fwd2_bf16_kernel", "bilinear_bwd_prep8_bf16_kernel<2>"),       # fwd2 at N = 2: the largest h2 overlay
    (22, 3, 128, 256, 2): ("bilinear_fwd2_bf16_kernel", "bilinear_bwd_prep8_bf16_kernel<2>"),      # M = 66: a sample straddles the tile edge
    (21, 3, 64, 256, 2): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep8_bf16_kernel<2>"),    # M = 63: generic at R = 2
    (3, 36, 320, 512, 2): ("bilinear_fwd2_bf16_kernel", "bilinear_bwd_prep8_bf16_kernel<2>"),      # the config's proportions
    (5, 7, 64, 256, 1): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep8_bf16_kernel<1>"),
    (5, 7, 64, 256, 3): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep8_bf16_kernel<3>"),
    (5, 7, 64, 256, 4): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep8_bf16_kernel<4>"),
    (5, 7, 64, 256, 5): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep8_bf16_kernel<5>"),
    (5, 7, 64, 256, 6): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep_bf16_kernel<16>"),
    (5, 7, 64, 256, 8): ("(bilinear_fwd_bf16_kernel<64,64>)", "bilinear_bwd_prep_bf16_kernel<16>"),
    (1024, 1, 64, 256, 6): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep_bf16_kernel<4>"),   # B * H = 2^18
    # the prep kernels split a sample's regions over 16 slices (prep<4>: 4) that meet in LDS: at N = 7 (N = 1) most slices are
    # idle and a lost slice would not show.  N = 37 = 2 * 16 + 5 keeps every slice busy, unevenly; N = 4 all four of prep<4>
    (3, 37, 64, 256, 1): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep8_bf16_kernel<1>"),
    (3, 37, 64, 256, 3): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep8_bf16_kernel<3>"),
    (3, 37, 64, 256, 4): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep8_bf16_kernel<4>"),
    (3, 37, 64, 256, 5): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep8_bf16_kernel<5>"),
    (3, 37, 64, 256, 6): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep_bf16_kernel<16>"),
    (3, 37, 64, 256, 8): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep_bf16_kernel<16>"),
    (1024, 4, 64, 256, 6): ("(bilinear_fwd_bf16_kernel<128,64>)", "bilinear_bwd_prep_bf16_kernel<4>"),
}
_k4_id = lambda s: "B%dN%dL%dH%dR%d" % s      # noqa: E731


@pytest.mark.parametrize("shape", list(K4_SHAPES), ids=_k4_id)
def test_k4_rgemm_small_integers_are_exact(ops, shape):
    """every output of the forward and the backward: out, h1, d_x (gated, plain, NULL), d_h2, every d_w1[r] and d_b1[r]; phases 1
    then 2 into one workspace leave the bits of phases = 3"""
    B, N, L, H, R = shape
    case, ref = k4_operands(shape), k4_rgemm_reference(shape)
    d, Hin, Lout = k4_device(case), case["Hin"], case["Lout"]
    fwd_kernel, prep_kernel = K4_SHAPES[shape]
    out, h1, log = k4_fwd(ops, d, shape, Hin)
    assert log[0][0] == fwd_kernel, log
    assert_exact("out", out, ref["out"])
    assert_exact("h1", h1, ref["h1"])
    out_only, _, _ = k4_fwd(ops, d, shape, Hin, want_h1=False)
    assert _same_bits(out, out_only), "out depends on whether h1 is stored"
    h1_d = h1.contiguous()

    def check(tag, got, dx_key):
        if dx_key is not None:
            assert_exact(tag + " d_x", got["d_x"], ref[dx_key])
        assert_exact(tag + " d_h2", got["d_h2"], ref["d_h2"])
        for r in range(R):
            assert_exact("%s d_w1[%d]" % (tag, r), got["d_w1"][r], ref["d_w1"][r])
            assert_exact("%s d_b1[%d]" % (tag, r), got["d_b1"][r], ref["d_b1"][r])

    gated, log = k4_bwd(ops, d, shape, Hin, Lout, h1_d, True)
    assert [k for k in _names(log) if "prep" in k] == [prep_kernel], log
    assert len(log) == 4 and "gemm_bf16_nt_kernel" in log[1][0] and "gemm_bf16_tn_kernel" in log[2][0] and log[3][0] == "slab_reduce_kernel", log
    check("gate_dx", gated, "d_x_gated")
    plain, _ = k4_bwd(ops, d, shape, Hin, Lout, h1_d, False)
    check("plain", plain, "d_x")
    no_dx, log = k4_bwd(ops, d, shape, Hin, Lout, h1_d, False, with_dx=False)
    assert len(log) == 3 and not any("gemm_bf16_nt_kernel" in k for k in _names(log)), log
    check("d_x = NULL", no_dx, None)
    split, log = k4_bwd(ops, d, shape, Hin, Lout, h1_d, True, phases=(1, 2))
    assert len(log) == 4, log
    for k in ("d_x", "d_h2", "d_w1", "d_b1"):
        assert _same_bits(split[k], gated[k]), "phases 1 + 2 differ from phases = 3 in %s" % k


@pytest.mark.parametrize("shape", [(21, 3, 64, 256, 2), (5, 7, 64, 256, 3), (43, 3, 64, 256, 5)], ids=_k4_id)
def test_k4_generic_forward_under_every_tile(ops, lib_option, shape):
    """the generic forward takes VQA_BF16_TILE (128x128 becomes 128x64: the per-rank accumulators); M = 63 and 35 leave clamped rows
    in every tile, M = 129 a second row tile of one row under the 128-row shapes"""
    case, ref = k4_operands(shape), k4_rgemm_reference(shape)
    d = k4_device(case)
    for tile in TILES[1:]:
        lib_option("VQA_BF16_TILE", tile)
        out, h1, log = k4_fwd(ops, d, shape, case["Hin"])
        bm, bn = (int(v) for v in tile.split("x"))
        assert log[0][0] == "(bilinear_fwd_bf16_kernel<%d,%d>)" % (bm, 64 if (bm, bn) == (128, 128) else bn), log
        assert_exact("out " + tile, out, ref["out"])
        assert_exact("h1 " + tile, h1, ref["h1"])


# ======================================================================================================================= A4: K4 rank-folded
# (B, N, L, H): N gives NB = ceil(N/16) = 1..8 and NCH = ceil(N/32) = 1..4 with one N on each block edge; each of the 20 (LBW = L/64,
# NCH) weight-gradient instantiations occurs once; H in {64, 192, 256}; B in {1, 15, 16, 17, 33}: 16 sample slabs with 15 empty, one
# empty, one sample each, two per slab with seven empty, three per slab with a last slab of three
FOLD_SHAPES = [(33, 1, 64, 64), (17, 33, 64, 192), (1, 65, 64, 256), (15, 97, 64, 64),
               (16, 16, 128, 192), (1, 49, 128, 256), (15, 81, 128, 64), (16, 113, 128, 192),
               (33, 17, 192, 256), (17, 33, 192, 64), (1, 65, 192, 192), (1, 128, 192, 256),
               (17, 1, 256, 64), (16, 49, 256, 192), (1, 81, 256, 256), (15, 97, 256, 64),
               (33, 16, 320, 192), (15, 33, 320, 256), (16, 65, 320, 64), (1, 113, 320, 192)]
_fold_id = lambda s: "B%dN%dL%dH%d" % s      # noqa: E731


def test_fold_shape_table_covers_every_instantiation():
    assert {-(-N // 16) for _, N, _, _ in FOLD_SHAPES} == set(range(1, 9))
    assert {(L // 64, -(-N // 32)) for _, N, L, _ in FOLD_SHAPES} == {(lbw, nch) for lbw in range(1, 6) for nch in range(1, 5)}
    assert {N for _, N, _, _ in FOLD_SHAPES} == {1, 16, 17, 33, 49, 65, 81, 97, 113, 128}
    assert {B for B, _, _, _ in FOLD_SHAPES} == {1, 15, 16, 17, 33} and {H for _, _, _, H in FOLD_SHAPES} == {64, 192, 256}


def fold_reference(case, H, to=torch.int64, wb=None):
    """the fold's closed forms in `to` arithmetic from the folded weight Wb [B,H,L] (given, or formed here)"""
    x, w1, b1, g, Hin, Lout = (case[k].to(to) if isinstance(case[k], torch.Tensor) else case[k] for k in ("x", "w1", "b1", "g", "Hin", "Lout"))
    h2 = pad_h2(case["h2"].to(to), H)
    if wb is None:
        wb = torch.einsum("brh,rhl->bhl", h2, w1)
    gsum = g.sum(1)
    P = torch.einsum("bnh,bnl->bhl", g, x)
    d_x = torch.einsum("bnh,bhl->bnl", g, wb)
    return {"out": torch.einsum("bnl,bhl->bnh", x, wb) + torch.einsum("brh,rh->bh", h2, b1)[:, None], "d_x": d_x,
            "d_x_gated": d_x * (x > 0), "d_w1": torch.einsum("brh,bhl->rhl", h2, P)[:, :Hin, :Lout].contiguous(),
            "d_h2": (torch.einsum("bhl,rhl->brh", P, w1) + b1[None] * gsum[:, None])[..., :Hin].contiguous(),
            "d_b1": torch.einsum("brh,bh->rh", h2, gsum)[:, :Hin].contiguous()}


def fold_fwd(ops, d, shape5, Hin):
    B, N, L, H, R = shape5
    L_ = ops._lib.lib()
    out = _sentinel(B * N + 2, H, dtype=BF)
    log = _logged(L_, lambda: ops._launch("bilinear_fold_fwd_bf16", shape5, L_.vqa_bilinear_fold_fwd_bf16, _ptr(d["x"]), _ptr(d["w1"]),
                                          _ptr(d["b1"]), _ptr(d["h2"]), _ptr(out), B, N, L, H, R, Hin))
    torch.cuda.synchronize()
    return _take(out, slice(0, B * N), "fold forward out").view(B, N, H), log


def fold_bwd(ops, d, shape5, Hin, Lout, gate_dx, with_dx=True):
    B, N, L, H, R = shape5
    L_ = ops._lib.lib()
    M = B * N
    ws_bytes = L_.vqa_bilinear_fold_bwd_bf16_workspace_bytes(B, N, L, H, R)
    ws = torch.full((ws_bytes // 4 + 64,), NAN, device=dev())
    assert ws_bytes > 0 and ws.data_ptr() % 256 == 0
    d_x = _sentinel(M + 2, L, dtype=BF) if with_dx else None
    d_h2 = _sentinel(B * R * Hin + 16)
    d_w1, d_b1 = [_sentinel(Hin + 2, Lout) for _ in range(R)], [_sentinel(Hin + 8) for _ in range(R)]
    log = _logged(L_, lambda: ops._launch("bilinear_fold_bwd_bf16", shape5, L_.vqa_bilinear_fold_bwd_bf16, _ptr(d["x"]), _ptr(d["w1"]),
                                          _ptr(d["w1t"]) if with_dx else None, _ptr(d["b1"]), _ptr(d["h2"]), _ptr(d["g"]), _ptr(d_x), _ptrs(d_w1),
                                          _ptrs(d_b1), _ptr(d_h2), _ptr(ws), ws_bytes, B, N, L, H, R, Hin, Lout, int(gate_dx)))
    torch.cuda.synchronize()
    return {"d_x": _take(d_x, slice(0, M), "fold d_x").view(B, N, L) if with_dx else None,
            "d_h2": _take(d_h2, slice(0, B * R * Hin), "fold d_h2").view(B, R, Hin),
            "d_w1": torch.stack([_take(t, slice(0, Hin), "fold d_w1") for t in d_w1]),
            "d_b1": torch.stack([_take(t, slice(0, Hin), "fold d_b1") for t in d_b1])}, log


@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=_fold_id)
def test_fold_small_integers_are_exact(ops, shape):
    """the folded weight sum_r h2_r W1_r (<= 32) is exact in bf16, so out, d_x (gated, plain, NULL), d_h2, d_w1[r], d_b1[r] are all
    integer sums; H_in = H - 6 < H"""
    B, N, L, H = shape
    shape5 = (B, N, L, H, 2)
    L_ = ops._lib.lib()
    assert L_.vqa_bilinear_fold_bf16_supported(*shape5) == 1
    assert L_.vqa_bilinear_fold_bf16_supported(B, 129, L, H, 2) == 0 and L_.vqa_bilinear_fold_bf16_supported(B, N, 384, H, 2) == 0
    assert L_.vqa_bilinear_fold_bf16_supported(B, N, L, H, 3) == 0
    case = k4_operands(shape5)
    Hin, Lout = case["Hin"], case["Lout"]
    _below_2_24(32 * 4 * L + 32, 32 * 4 * H, 16 * N * 4 * B, 16 * N * 4 * L + 16 * N, 16 * N * B)
    ref = fold_reference(case, H)
    assert _amax(torch.einsum("brh,rhl->bhl", pad_h2(case["h2"], H), case["w1"])) <= 256      # the folded weight: exact in bf16
    d = k4_device(case)
    NB, lbw, nch = -(-N // 16), L // 64, -(-N // 32)
    out, log = fold_fwd(ops, d, shape5, Hin)
    assert _names(log) == ["(fold_fwd_kernel<%d>)" % NB], log
    assert_exact("out", out, ref["out"])

    def check(tag, got, dx_key):
        if dx_key is not None:
            assert_exact(tag + " d_x", got["d_x"], ref[dx_key])
        for k in ("d_h2", "d_w1", "d_b1"):
            assert_exact("%s %s" % (tag, k), got[k], ref[k])

    gated, log = fold_bwd(ops, d, shape5, Hin, Lout, True)
    assert _names(log) == ["(fold_dx_kernel<%d>)" % NB, "(fold_dw_kernel<%d,%d>)" % (lbw, nch), "fold_finish_kernel"], log
    check("gate_dx", gated, "d_x_gated")
    plain, _ = fold_bwd(ops, d, shape5, Hin, Lout, False)
    check("plain", plain, "d_x")
    no_dx, log = fold_bwd(ops, d, shape5, Hin, Lout, False, with_dx=False)
    assert len(log) == 2, log
    check("d_x = NULL", no_dx, None)


# ======================================================================================================================= A5: packing
@functools.lru_cache(maxsize=None)
def pack_master(rows, cols):
    """fp32 [rows, cols]: a third exact ties between two neighbouring bf16 values (half an ulp above a bf16 value, both parities
    of its last bit: round-to-even goes down and up), random fp32 in between, and +-0, +-inf"""
    gen = torch.Generator().manual_seed(50021 * rows + cols)
    w = torch.randn(rows, cols, generator=gen)
    flat = w.view(-1)
    ties = (flat[::3].to(BF).float().view(torch.int32) + 0x8000).view(torch.float32)
    assert bool(((ties.view(torch.int32) & 0xFFFF) == 0x8000).all())
    flat[::3] = ties
    flat[1], flat[4], flat[7], flat[10] = 0.0, -0.0, INF, -INF
    even = (flat[::3].view(torch.int32) >> 16) & 1
    assert 0 < int(even.sum()) < even.numel()
    return w


def test_pack_many_and_pack_bf16_round_to_even_into_their_windows(ops):
    """one ShadowPlan of seven jobs over [70,33] and [33,70] masters and a [70] vector: plain, transposed (3 x 2 and 2 x 3 tiles of
    32 x 32, the last of each partial), offsets, bf16 and fp32 destinations; the jobs start at 0, 3072, 9216, 12288, 18432, 19456 and
    25600.  Every destination is compared whole against tensor.to(bfloat16) placed in a sentinel-filled copy; vqa_pack_bf16 fills
    the same layouts with the same bits."""
    w_a, w_b = pack_master(70, 33).to(dev()), pack_master(33, 70).to(dev())
    vec = pack_master(1, 70).view(70).to(dev())
    jobs = [  # (src, dst shape, dtype, row stride, col stride, offset, expected placement)
        (w_a, (72, 64), BF, 64, 1, 0, lambda e, s: e[:70, :33].copy_(s)),
        (w_a, (40, 72), BF, 1, 72, 3 + 2 * 72, lambda e, s: e.view(-1)[3 + 2 * 72:].as_strided((70, 33), (1, 72)).copy_(s)),
        (w_b, (40, 80), torch.float32, 80, 1, 5, lambda e, s: e.view(-1)[5:].as_strided((33, 70), (80, 1)).copy_(s)),
        (w_b, (72, 40), BF, 1, 40, 1, lambda e, s: e.view(-1)[1:].as_strided((33, 70), (1, 40)).copy_(s)),
        (vec, (2, 80), torch.float32, 80, 1, 80 + 4, lambda e, s: e.view(-1)[84:84 + 70].copy_(s)),
        (w_b, (70, 40), torch.float32, 1, 40, 2, lambda e, s: e.view(-1)[2:].as_strided((33, 70), (1, 40)).copy_(s)),
        (w_a, (70, 33), BF, 33, 1, 0, lambda e, s: e.copy_(s)),
    ]
    plan = ops.ShadowPlan()
    dsts, wants = [], []
    for src, shape, dtype, rs, cs, off, place in jobs:
        dst = _sentinel(*shape, dtype=dtype)
        plan.add(src, dst, rs, cs, offset=off)
        want = _sentinel(*shape, dtype=dtype)
        place(want, src.to(dtype))
        dsts.append(dst)
        wants.append(want)
    plan.pack()
    torch.cuda.synchronize()
    assert [int(r[7]) for r in plan._table.cpu().tolist()] == [0, 3072, 9216, 12288, 18432, 19456, 25600]
    for i, (dst, want) in enumerate(zip(dsts, wants)):
        assert _same_bits(dst, want), "pack_many job %d" % i
    for i, (src, shape, dtype, rs, cs, off, _) in enumerate(jobs):
        if dtype != BF:
            continue
        dst = _sentinel(*shape, dtype=BF)
        ops.pack_bf16(src, dst, 0, rs, cs, zero_fill=False, offset=off)
        assert _same_bits(dst, wants[i]), "pack_bf16 job %d" % i
    both = torch.stack([w_a, w_a.flip(0)])                     # a batch of two, the second behind the first's padded rows
    dst = _sentinel(2, 72, 64, dtype=BF)
    ops.pack_bf16(both, dst, 72 * 64, 64, 1, zero_fill=False)
    want = _sentinel(2, 72, 64, dtype=BF)
    want[:, :70, :33] = both.to(BF)
    assert _same_bits(dst, want)
    filled = ops.pack_bf16(both, _sentinel(2, 72, 64, dtype=BF), 72 * 64, 64, 1)       # zero_fill: the pads become +0
    want = torch.zeros(2, 72, 64, device=dev(), dtype=BF)
    want[:, :70, :33] = both.to(BF)
    assert _same_bits(filled, want)


# ======================================================================================================================= B: float64
def _rand_bf(gen, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=gen)).to(BF).float()


def test_nt_random_operands_against_float64(ops, measured):
    M, N, K = 300, 320, 320
    gen = torch.Generator().manual_seed(61)
    a, b, bias = _rand_bf(gen, M, K), _rand_bf(gen, N, K, scale=K ** -0.5), torch.randn(N, generator=gen)
    got, _ = run_nt(ops, _dbf(a), _dbf(b), M, N, K, N, _df(bias), 0)
    bars = Bars()
    bars.check_bf16("nt c", got, a.double() @ b.double().T + bias.double(), a @ b.T + bias)
    bars.report(measured, "gemm_bf16_nt 300x320x320")


@pytest.mark.parametrize("K,N1,N2", [(1000, 320, 128), (12800, 128, 64)])
def test_tn_random_operands_against_float64(ops, measured, K, N1, N2):
    """(12800, 128, 64): one tile, 25 slabs"""
    gen = torch.Generator().manual_seed(62 + K)
    a, b = _rand_bf(gen, K, N1), _rand_bf(gen, K, N2)
    got, slabs, _ = run_tn(ops, _dbf(a), _dbf(b), K, N1, N2)
    assert slabs == (2 if K == 1000 else 25), slabs
    bars = Bars()
    bars.check("tn c", got, a.double().T @ b.double(), a.T @ b)
    bars.report(measured, "gemm_bf16_tn K=%d %dx%d (%d slabs)" % (K, N1, N2, slabs))


def k4_random_case(shape, fold):
    B, N, L, H, R = shape
    gen = torch.Generator().manual_seed(63 + int(fold))
    Hin = H - 6
    if fold:        # powers of two: h2_r * W1_r is exact, the sum of the two one float32 rounding however it is contracted
        h2 = torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])[torch.randint(0, 5, (B, R, Hin), generator=gen)]
        h2 = h2 * (2.0 * torch.randint(0, 2, (B, R, Hin), generator=gen) - 1.0)
    else:
        h2 = torch.randn(B, R, Hin, generator=gen)
    return {"x": _rand_bf(gen, B, N, L), "w1": _rand_bf(gen, R, H, L, scale=L ** -0.5), "b1": 0.1 * torch.randn(R, H, generator=gen), "h2": h2,
            "g": _rand_bf(gen, B, N, H), "Hin": Hin, "Lout": L - 3}


def test_k4_rgemm_random_operands_against_float64(ops, measured):
    """out and h1 as bf16 roundings of the float64 values; the backward with the kernel's OWN h1 and gs = bf16(float32(g * h2)) on
    both sides, so that d_x (one rounding), d_w1, d_h2 and d_b1 differ from float64 by fp32 accumulation only"""
    shape = (3, 36, 320, 512, 2)
    B, N, L, H, R = shape
    case = k4_random_case(shape, False)
    d, Hin, Lout = k4_device(case), case["Hin"], case["Lout"]
    out, h1, _ = k4_fwd(ops, d, shape, Hin)
    bars = Bars()

    def forward(t):
        x, w1, b1, h2 = case["x"].to(t), case["w1"].to(t), case["b1"].to(t), pad_h2(case["h2"].to(t), H)
        hv = torch.einsum("bnl,rhl->bnrh", x, w1) + b1
        return (hv * h2[:, None]).sum(2), hv

    (out64, hv64), (out32, hv32) = forward(torch.float64), forward(torch.float32)
    bars.check_bf16("out", out, out64, out32)
    bars.check_bf16("h1", h1, hv64, hv32)
    got, _ = k4_bwd(ops, d, shape, Hin, Lout, h1.contiguous(), False)
    h1_own = h1.float().cpu()
    gs = (case["g"][:, :, None, :] * pad_h2(case["h2"], H)[:, None]).to(BF).float()       # one float32 multiply, one rounding

    def backward(t):
        x, w1, g, h2 = case["x"].to(t), case["w1"].to(t), case["g"].to(t), pad_h2(case["h2"].to(t), H)
        return {"d_x": torch.einsum("bnrh,rhl->bnl", gs.to(t), w1), "d_h2": torch.einsum("bnh,bnrh->brh", g, h1_own.to(t))[..., :Hin],
                "d_w1": torch.einsum("bnrh,bnl->rhl", gs.to(t), x)[:, :Hin, :Lout], "d_b1": torch.einsum("brh,bh->rh", h2, g.sum(1))[:, :Hin]}

    r64, r32 = backward(torch.float64), backward(torch.float32)
    bars.check_bf16("d_x", got["d_x"], r64["d_x"], r32["d_x"])
    for k in ("d_h2", "d_w1", "d_b1"):
        bars.check(k, got[k], r64[k], r32[k])
    bars.report(measured, "K4 rgemm B3 N36 L320 H512 R2")


def test_fold_random_operands_against_float64(ops, measured):
    shape = (3, 36, 320, 512, 2)
    B, N, L, H, R = shape
    case = k4_random_case(shape, True)
    d, Hin, Lout = k4_device(case), case["Hin"], case["Lout"]
    h2, w1 = pad_h2(case["h2"], H), case["w1"]
    prod = h2[:, :, :, None] * w1[None]                                       # float32 [B,R,H,L]
    assert torch.equal(prod.double(), h2.double()[:, :, :, None] * w1.double()[None]), "a product of the fold is not exact in float32"
    wb = (prod[:, 0] + prod[:, 1]).to(BF).float()                              # the kernel's operand, bit for bit
    out, _ = fold_fwd(ops, d, shape, Hin)
    got, _ = fold_bwd(ops, d, shape, Hin, Lout, False)
    r64, r32 = fold_reference(case, H, torch.float64, wb.double()), fold_reference(case, H, torch.float32, wb)
    bars = Bars()
    bars.check_bf16("out", out, r64["out"], r32["out"])
    bars.check_bf16("d_x", got["d_x"], r64["d_x"], r32["d_x"])
    for k in ("d_h2", "d_w1", "d_b1"):
        bars.check(k, got[k], r64[k], r32[k])
    bars.report(measured, "K4 fold B3 N36 L320 H512")


# ======================================================================================================================= C: non-finites
def _rows_equal(a, b, keep):
    return _same_bits(a[keep].contiguous(), b[keep].contiguous())


@pytest.mark.parametrize("tile", [None, "64x128"], ids=_tile_id)
def test_nt_non_finites_stay_in_their_row_and_column(ops, lib_option, tile):
    """M = 77, N = 72: the stager clamps tile rows 77 .. 127 to row 76 and weight rows 72 .. 127 to row 71, so a NaN / inf there is
    multiplied into the tile's padding; only the store bounds keep it out (run_nt compares the sentinel border)"""
    if tile:
        lib_option("VQA_BF16_TILE", tile)
    M, N, K = 77, 72, 128
    gen = torch.Generator().manual_seed(71)
    a, b = _rand_bf(gen, M, K), _rand_bf(gen, N, K)
    b[b == 0] = 1.0
    a[a == 0] = 1.0
    for ldc in (N, N + 3):
        clean, _ = run_nt(ops, a.to(BF).to(dev()), b.to(BF).to(dev()), M, N, K, ldc)
        bad = a.clone()
        bad[M - 1, 17] = NAN
        got, _ = run_nt(ops, bad.to(BF).to(dev()), b.to(BF).to(dev()), M, N, K, ldc)
        assert bool(torch.isnan(got[M - 1]).all()) and _rows_equal(got, clean, slice(0, M - 1))
        bad = b.clone()
        bad[N - 1, 5] = INF
        got, _ = run_nt(ops, a.to(BF).to(dev()), bad.to(BF).to(dev()), M, N, K, ldc)
        assert bool(torch.isinf(got[:, N - 1]).all()) and _same_bits(got[:, :N - 1].contiguous(), clean[:, :N - 1].contiguous())


K4_NAN_SHAPES = [((21, 3, 64, 256, 2), "generic"), ((22, 3, 128, 256, 2), "fwd2"), ((22, 3, 128, 256, 2), "fold")]


@pytest.mark.parametrize("shape,form", K4_NAN_SHAPES, ids=lambda v: v if isinstance(v, str) else _k4_id(v))
def test_k4_non_finites_stay_in_their_row_and_sample(ops, shape, form):
    """forward: a NaN in one region of x stays in that output row, a NaN in h2[b] in sample b; backward: a NaN in g of sample b
    reaches d_x[b] and d_h2[b] only (the weight gradients sum over the samples and may be NaN)"""
    B, N, L, H, R = shape
    case = k4_random_case(shape, False)
    Hin, Lout = case["Hin"], case["Lout"]
    fold = form == "fold"

    def fwd(c):
        d = k4_device_any(c)
        if fold:
            return fold_fwd(ops, d, shape, Hin)[0], None, d
        out, h1, log = k4_fwd(ops, d, shape, Hin)
        assert ("fwd2" in log[0][0]) == (form == "fwd2"), log
        return out, h1, d

    def bwd(d, h1):
        if fold:
            return fold_bwd(ops, d, shape, Hin, Lout, False)[0]
        return k4_bwd(ops, d, shape, Hin, Lout, h1.contiguous(), False)[0]

    clean_out, clean_h1, d = fwd(case)
    clean = bwd(d, clean_h1)
    b_bad, n_bad = B - 2, 1
    others = [b for b in range(B) if b != b_bad]
    bad = dict(case, x=case["x"].clone())
    bad["x"][b_bad, n_bad, 7] = NAN
    out, _, _ = fwd(bad)
    flat, flat_clean = out.view(B * N, H), clean_out.view(B * N, H)
    keep = [m for m in range(B * N) if m != b_bad * N + n_bad]
    assert bool(torch.isnan(flat[b_bad * N + n_bad, :Hin]).all()) and _rows_equal(flat, flat_clean, keep)
    bad = dict(case, h2=case["h2"].clone())
    bad["h2"][b_bad, 1, 5] = NAN
    out, _, _ = fwd(bad)
    assert bool(torch.isnan(out[b_bad, :, 5]).all()) and _rows_equal(out, clean_out, others)
    bad = dict(case, g=case["g"].clone())
    bad["g"][b_bad, n_bad, 9] = NAN
    got = bwd(k4_device_any(bad), clean_h1)
    assert bool(torch.isnan(got["d_x"][b_bad, n_bad]).all()) and bool(torch.isnan(got["d_h2"][b_bad, :, 9]).all())
    assert _rows_equal(got["d_x"], clean["d_x"], others) and _rows_equal(got["d_h2"], clean["d_h2"], others)


def k4_device_any(case):
    """k4_device for operands that are bf16 values but may hold a NaN"""
    w1 = case["w1"]
    R, H, L = w1.shape
    to_bf = lambda t: t.to(BF).to(dev()).contiguous()      # noqa: E731
    return {"x": to_bf(case["x"]), "w1": to_bf(w1), "b1": _df(case["b1"]), "h2": _df(case["h2"]), "g": to_bf(case["g"]),
            "w1t": to_bf(w1.permute(2, 0, 1).reshape(L, R * H))}


# ======================================================================================================================= C: refusals
def test_refusals_launch_nothing(ops):
    """every VQA_REQUIRE of the bf16 entry points: the documented code, an error text, no launch, every output still the sentinel"""
    L = ops._lib.lib()
    a = torch.zeros(128, 128, device=dev(), dtype=BF)
    c, c32 = _sentinel(128, 128, dtype=BF), _sentinel(128, 128)
    ws = _sentinel(1 << 18)
    h2 = torch.zeros(4 * 8 * 256, device=dev())
    outs = [c32, _sentinel(128, 128)]
    buf = (ctypes.c_ulonglong * 16)()

    def refused(code, fn, *args):
        L.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, args, L.vqa_last_error())
        assert L.vqa_last_error() and L.vqa_launch_log(buf, 16) == 0, "a refused call launched a kernel"

    def nt(M=64, N=64, K=64, lda=64, ldb=64, ldc=64, act=0, a_=a, b_=a, c_=c):
        return (_ptr(a_), lda, _ptr(b_), ldb, None, _ptr(c_), ldc, M, N, K, act)

    for args in (nt(K=72, lda=72, ldb=72), nt(K=32, lda=32, ldb=32), nt(lda=68), nt(ldb=68), nt(a_=a.view(-1)[4:]), nt(b_=a.view(-1)[1:]),
                 nt(lda=56), nt(ldc=56)):
        refused(E_UNSUPPORTED, L.vqa_gemm_bf16_nt, *args)
        refused(E_UNSUPPORTED, L.vqa_gemm_bf16_nt_ex, *args, None, 0, 0.0, 0, None)
    for args in (nt(M=0), nt(N=0), nt(K=0), nt(act=2), nt(a_=None), nt(c_=None)):
        refused(E_BADARG, L.vqa_gemm_bf16_nt, *args)
        refused(E_BADARG, L.vqa_gemm_bf16_nt_ex, *args, None, 0, 0.0, 0, None)
    refused(E_BADARG, L.vqa_gemm_bf16_nt_ex, *nt(), _ptr(a), 56, 0.0, 0, None)                       # gate stride < N
    refused(E_UNSUPPORTED, L.vqa_gemm_bf16_nt_ex, *nt(), None, 0, 0.25, 0, None)                     # p_drop not 0 / 0.5
    refused(E_UNSUPPORTED, L.vqa_gemm_bf16_nt_ex, *nt(lda=128), None, 0, 0.5, 0, None)               # dropout needs lda == K

    def tn(K=64, N1=64, N2=64, lda=64, ldb=64, a_=a, b_=a, ws_=ws, ws_bytes=4 * 64 * 64):
        return (_ptr(a_), lda, _ptr(b_), ldb), (_ptr(ws_), ws_bytes, K, N1, N2)

    def tn_plain(**kw):
        head, tail = tn(**kw)
        return (*head, _ptr(c32), *tail)

    def tn_ex(groups=2, rpg=32, out_rows=30, out_cols=61, out_ld=64, p_drop=0.0, o=None, **kw):
        head, tail = tn(**kw)
        return (*head, _ptrs(outs) if o is None else o, groups, rpg, out_rows, out_cols, out_ld, *tail, p_drop, 0, None)

    for kw in (dict(N1=60), dict(N2=60), dict(lda=68), dict(ldb=68), dict(lda=56), dict(a_=a.view(-1)[4:]), dict(b_=a.view(-1)[4:])):
        refused(E_UNSUPPORTED, L.vqa_gemm_bf16_tn, *tn_plain(**kw))
        refused(E_UNSUPPORTED, L.vqa_gemm_bf16_tn_ex, *tn_ex(**kw))
    assert L.vqa_gemm_bf16_tn_workspace_bytes(64, 64, 64) == 4 * 64 * 64
    for kw in (dict(ws_bytes=4 * 64 * 64 - 4), dict(ws_=None), dict(ws_=ws[1:]), dict(K=0), dict(a_=None)):
        refused(E_BADARG, L.vqa_gemm_bf16_tn, *tn_plain(**kw))
        refused(E_BADARG, L.vqa_gemm_bf16_tn_ex, *tn_ex(**kw))
    for kw in (dict(rpg=31), dict(rpg=33), dict(groups=0), dict(groups=9, rpg=8), dict(out_rows=33), dict(out_cols=65, out_ld=65), dict(out_ld=60),
               dict(o=(ctypes.c_void_p * 2)(c32.data_ptr(), None))):
        refused(E_BADARG, L.vqa_gemm_bf16_tn_ex, *tn_ex(**kw))
    refused(E_UNSUPPORTED, L.vqa_gemm_bf16_tn_ex, *tn_ex(p_drop=0.25))
    refused(E_UNSUPPORTED, L.vqa_gemm_bf16_tn_ex, *tn_ex(p_drop=0.5, N2=8, ldb=8, out_cols=7, out_ld=8))      # dropout needs ldb % 32 == 0

    d_w1, d_b1 = [_sentinel(64, 64) for _ in range(9)], [_sentinel(64) for _ in range(9)]
    d_h2, d_x = _sentinel(4 * 9 * 256), _sentinel(128, 128, dtype=BF)

    def fwd(B=2, N=3, L_=64, H=256, R=2, Hin=250, x=a, out=c):
        return (_ptr(x), _ptr(a), _ptr(h2), _ptr(h2), _ptr(out), _ptr(d_x), B, N, L_, H, R, Hin)

    def bwd(B=2, N=3, L_=64, H=256, R=2, Hout=250, Lout=60, phases=3, x=a, w1t=a, ws_bytes=4 << 18, ws_=ws, dx=d_x):
        return (_ptr(x), _ptr(w1t), _ptr(h2), _ptr(a), _ptr(a), _ptr(dx), _ptrs(d_w1[:max(R, 1)]), _ptrs(d_b1[:max(R, 1)]), _ptr(d_h2), _ptr(ws_),
                ws_bytes, B, N, L_, H, R, Hout, Lout, 0, phases)

    assert L.vqa_lowrank_bilinear_fusion_bwd_bf16_workspace_bytes(2, 3, 64, 256, 2) <= 4 << 18
    for kw in (dict(R=9), dict(H=320), dict(H=128), dict(L_=96), dict(x=a.view(-1)[4:])):
        refused(E_UNSUPPORTED, L.vqa_lowrank_bilinear_fusion_fwd_bf16, *fwd(**kw))
        refused(E_UNSUPPORTED, L.vqa_lowrank_bilinear_fusion_bwd_bf16, *bwd(**kw))
    refused(E_UNSUPPORTED, L.vqa_lowrank_bilinear_fusion_bwd_bf16, *bwd(ws_=ws[4:]))
    for kw in (dict(B=0), dict(R=0), dict(x=None)):
        refused(E_BADARG, L.vqa_lowrank_bilinear_fusion_fwd_bf16, *fwd(**kw))
        refused(E_BADARG, L.vqa_lowrank_bilinear_fusion_bwd_bf16, *bwd(**kw))
    refused(E_BADARG, L.vqa_lowrank_bilinear_fusion_fwd_bf16, *fwd(Hin=257))
    refused(E_BADARG, L.vqa_lowrank_bilinear_fusion_fwd_bf16, *fwd(Hin=0))
    for kw in (dict(phases=0), dict(phases=4), dict(w1t=None), dict(Hout=257), dict(Lout=65), dict(Lout=0), dict(ws_bytes=1024), dict(ws_=None)):
        refused(E_BADARG, L.vqa_lowrank_bilinear_fusion_bwd_bf16, *bwd(**kw))

    def fold_fwd_args(B=2, N=3, L_=64, H=64, R=2, Hin=60, x=a):
        return (_ptr(x), _ptr(a), _ptr(h2), _ptr(h2), _ptr(c), B, N, L_, H, R, Hin)

    def fold_bwd_args(B=2, N=3, L_=64, H=64, R=2, Hout=60, Lout=60, x=a, w1t=a, ws_bytes=4 << 18, ws_=ws):
        return (_ptr(x), _ptr(a), _ptr(w1t), _ptr(h2), _ptr(h2), _ptr(a), _ptr(d_x), _ptrs(d_w1[:2]), _ptrs(d_b1[:2]), _ptr(d_h2), _ptr(ws_), ws_bytes,
                B, N, L_, H, R, Hout, Lout, 0)

    assert 0 < L.vqa_bilinear_fold_bwd_bf16_workspace_bytes(2, 3, 64, 64, 2) <= 4 << 18
    for kw in (dict(R=3), dict(R=1), dict(N=129), dict(L_=384), dict(L_=96), dict(H=96), dict(x=a.view(-1)[4:])):
        refused(E_UNSUPPORTED, L.vqa_bilinear_fold_fwd_bf16, *fold_fwd_args(**kw))
        refused(E_UNSUPPORTED, L.vqa_bilinear_fold_bwd_bf16, *fold_bwd_args(**kw))
    refused(E_BADARG, L.vqa_bilinear_fold_fwd_bf16, *fold_fwd_args(Hin=65))
    refused(E_BADARG, L.vqa_bilinear_fold_fwd_bf16, *fold_fwd_args(x=None))
    for kw in (dict(w1t=None), dict(Hout=65), dict(Lout=65), dict(ws_bytes=1024), dict(x=None)):
        refused(E_BADARG, L.vqa_bilinear_fold_bwd_bf16, *fold_bwd_args(**kw))

    src = torch.zeros(4, 4, device=dev())
    refused(E_BADARG, L.vqa_pack_bf16, _ptr(src), 1, 4, 4, _ptr(c), 0, 64, 1, 3 * 64 + 3, 0)        # destination one element short
    refused(E_BADARG, L.vqa_pack_bf16, _ptr(src), 1, 4, 4, _ptr(c), 0, 0, 1, 1 << 14, 0)
    refused(E_BADARG, L.vqa_pack_bf16, None, 1, 4, 4, _ptr(c), 0, 64, 1, 1 << 14, 0)
    refused(E_BADARG, L.vqa_pack_many, None, 1, 16)
    refused(E_BADARG, L.vqa_pack_many, _ptr(ws), 0, 16)
    refused(E_UNSUPPORTED, L.vqa_pack_many, _ptr(ws, 1), 1, 16)
    torch.cuda.synchronize()
    for t in [c, c32, ws, d_h2, d_x, *outs, *d_w1, *d_b1]:
        assert _untouched(t), "a refused call wrote to an output"
