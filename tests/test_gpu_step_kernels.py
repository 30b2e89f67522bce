"""Kernel-level checks of the kernels that finish every training step -- the column sums (csrc/reduce.hip), the batched
layers' bias_act / act_bwd_colsum (csrc/epilogue.hip), the clip norm and coefficient and the fused Adam pass
(csrc/optimizer.hip) -- against references made on the CPU, at the sizes where the launch geometry changes path.

Two kinds of assertion:

  EXACT    inputs are small integers, so every fp32 partial sum in any order is exact (|partial| < 2**24, asserted when the
           case is built) and the result must equal the int64 reference bit for bit: any dropped, duplicated or misplaced
           element shows.
  ROUNDED  real-valued inputs against float64.  The bar is not invented: `rounded_bar` evaluates the same formula in plain
           numpy float32 on the CPU, measures that evaluation's error against float64, and allows the kernel 4x of it (FMA
           contraction, another summation order), with a floor of one fp32 ulp of the output's largest magnitude.  Where the
           project already holds a bar it stays as a second assertion: 1e-6 relative on the norm, 2e-6 absolute on a
           parameter, 1e-6 of the maximum on a state buffer.  Both the value and the bar go through `measured`.

Paths, by section:

  1  column sums.  Short kernel (M <= 1024): M over the 16-row slices and the 128-row stride, N over the 16-column block.
     Tall kernel: the short/tall boundary; trailing slabs without rows (ceil(M/S) * (S-1) >= M); vec 4 / 2 / 1 in fp32 and
     bf16, chosen by N, by ld (`cols=` with ld > N, a sentinel behind the summed columns) and by the base pointer's alignment;
     the finish kernel's tail-only loop (S <= 12) and its unrolled loop with a remainder (S = 17, 33); S == 1 (no workspace,
     no finish kernel); a reused and a NaN-filled `out`; one inf and one NaN.  Each tall case restates column_slabs /
     column_vec in Python (`slabs`, `vec_of`) and holds the launch log to the grid that restatement predicts, so a retune
     cannot move a case off its path unseen.  Rounded: [18432, 310] normal and +-1e4 + normal (cancellation), error relative
     to the column's sum of |x|.
  2  bias_act / act_bwd_colsum through the C ABI: B across the 16-row slice and the 128-row stride of the row loop, A across
     the 16-column block, G in {1, 3}, both layouts; exact for act none / relu (out, gz in [G,B,A], d_bias); sigmoid rounded
     with +-30 and +-100 among the inputs; d_bias = NULL; bias / d_bias strides larger than A with a sentinel in the gaps; no
     bias.
  3  clip norm and coefficient.  Exact by indicator vectors (the norm of k ones is float32(sqrt(float64(k))) bit for bit) with
     the ones on the first / last element, the scalar tail, the last float4, the first and last float4 of every grid-stride
     sweep and ~1000 strided positions; n up to 2**24 + 2**20 + 3, the first size whose threads run 17 iterations: the spill
     of the fp32 run into float64 at 16 and the reset of its counter.  Dense integers in [-3, 3] at that size.  Dense normal
     gradients at 1e-6 relative.  The coefficient: 1.0 exactly for max_norm = 0, a norm below the cap, an all-zero gradient;
     else the fp32 formula from the kernel's own norm, bit for bit.  A NaN-filled workspace changes nothing.
  4  Adam.  p, m and v after five steps against torch.optim.Adam in float64 (the hyper-parameters are the float32 values the
     C ABI receives, widened), with the clip coefficient and with norm_and_coef = None (coef_ptr == nullptr); from p0 = 0
     (error relative to lr); gradients around eps (|g| in [1e-12, 1e-6]), where sqrt(v)/sqrt(bc2) + eps is told from every
     misplacement of eps or of the correction; g = m = v = 0 leaves the bits alone; step in {1, 2, 1000} from non-zero
     moments; the static and the `dyn` form bitwise equal (scalars computed as trainer._set_step_scalars does, from the
     float32 lr and betas the static form is handed); [x, 1.0] bitwise the None form; [x, 0.37] against float64.
  5  refusals: every call here is refused on the host (ValueError) or by a VQA_REQUIRE ahead of the launch
     (VqaLibraryError), and the library's launch log stays empty."""
import ctypes
import math

import numpy as np
import pytest
import torch

from kernel_harness import dev
from vqa_playground_pytorch_amd import _lib, ops

pytestmark = pytest.mark.gpu

F32 = np.float32
SENT = 2.0 ** 25                 # exact in fp32 and bf16; one of them in a sum of |entries| <= 8 cannot go unseen
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099, 2 ** 20 + 3]        # as tests/test_gpu_loss_optim_kernels.py


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def ulp(x):
    """One fp32 ulp at the largest magnitude of x."""
    return float(np.spacing(F32(np.abs(np.asarray(x, dtype=np.float64)).max())))


def rounded_bar(ref64, plain32):
    """4 x the error of the plain numpy float32 evaluation against float64, at least one fp32 ulp of the largest output."""
    e_np = float(np.abs(np.asarray(plain32, dtype=np.float64) - ref64).max())
    return max(4.0 * e_np, ulp(ref64)), e_np


def launch_log():
    h = _lib.lib()
    buf = (ctypes.c_ulonglong * 16)()
    n = h.vqa_launch_log(buf, 16)
    return [(int(buf[i]), (h.vqa_launch_log_kernel(i) or b"").decode()) for i in range(min(n, 16))]


# ---- 1. column sums -----------------------------------------------------------------------------------------------------------
COL_SHORT_M = 1024


def slabs(M, N, vec):
    """column_slabs of csrc/reduce.hip: aim at 512 workgroups, keep 64 rows a slab."""
    col_blocks = -(-N // (64 * vec))
    return max(1, min(-(-512 // col_blocks), (M + 63) // 64))


def vec_of(N, ld, byte_offset, esize):
    """column_vec of csrc/reduce.hip, for a base `byte_offset` behind a 16-byte aligned allocation."""
    for vec in (4, 2):
        if N % vec == 0 and ld % vec == 0 and byte_offset % (vec * esize) == 0:
            return vec
    return 1


def expected_launches(M, N, vec, S):
    """Grids in work-items of the launches column_sum makes."""
    if M <= COL_SHORT_M:
        return [-(-N // 16) * 256]
    return [-(-N // (64 * vec)) * S * 256] + ([-(-N // 64) * 256] if S > 1 else [])


_int_mats = {}


def int_matrix(M, ld, N):
    """[M, ld] integers in [-8, 8] (columns from N on: the sentinel) and the int64 sums of the first N columns, made once."""
    key = (M, ld, N)
    if key not in _int_mats:
        g = torch.Generator().manual_seed(M * 100003 + ld * 17 + N)
        x = torch.randint(-8, 9, (M, ld), generator=g, dtype=torch.int8)
        want = x[:, :N].sum(0, dtype=torch.int64)
        assert int(x[:, :N].abs().sum(0, dtype=torch.int64).max()) < 2 ** 24           # every partial sum is an exact fp32
        xf = x.float()
        xf[:, N:] = SENT
        _int_mats[key] = (xf, want)
    return _int_mats[key]


def check_exact_column_sum(M, ld, N, dtype, offset=0, vec=None, S=None):
    """column_sum of the integer case equals the int64 reference bit for bit and launches the grids of (vec, S)."""
    xf, want = int_matrix(M, ld, N)
    esize = 2 if dtype == torch.bfloat16 else 4
    buf = torch.full((offset + M * ld + 8,), SENT, dtype=dtype, device=dev())
    assert buf.data_ptr() % 16 == 0
    xd = buf[offset:offset + M * ld].view(M, ld)
    xd.copy_(xf)
    assert xd.is_contiguous() and xd.data_ptr() == buf.data_ptr() + offset * esize
    if M > COL_SHORT_M:
        assert vec_of(N, ld, offset * esize, esize) == vec and slabs(M, N, vec) == S, (vec_of(N, ld, offset * esize, esize), slabs(M, N, vec))
    _lib.lib().vqa_launch_log_reset()
    got = ops.column_sum(xd, cols=None if N == ld else N)
    log = launch_log()
    assert [g for g, _ in log] == expected_launches(M, N, vec, S), log
    if M > COL_SHORT_M:
        assert "%d>" % vec in log[0][1], log
    assert got.dtype == torch.float32 and got.shape == (N,)
    assert torch.equal(got.cpu().double(), want.double()), "M=%d ld=%d N=%d %s offset %d" % (M, ld, N, dtype, offset)
    return got


DTYPES = [torch.float32, torch.bfloat16]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 127, 128, 129, 1024])
def test_column_sum_short_kernel_is_exact(M, dtype):
    """M <= 1024: 16 row slices, 8 rows in flight (stride 128); N across the 16-column block."""
    for N in (1, 15, 16, 17, 33):
        check_exact_column_sum(M, N, N, dtype)


# (id, M, ld, N, vec, S): every case names the path it exists for
TALL = [
    ("short-tall-boundary_vec4_finish-unrolled-S17", 1025, 4, 4, 4, 17),
    ("finish-unrolled-with-remainder-S33", 2100, 4, 4, 4, 33),
    ("empty-trailing-slabs-S512", 40000, 4, 4, 4, 512),
    ("vec4_half-filled-last-column-block", 1100, 260, 260, 4, 18),
    ("vec2", 1100, 310, 310, 2, 18),
    ("vec1", 1100, 155, 155, 1, 18),
    ("ld320-cols310_vec2", 1100, 320, 310, 2, 18),
    ("ld320-cols308_vec4", 1100, 320, 308, 4, 18),
    ("ld320-cols155_vec1", 1100, 320, 155, 1, 18),
    ("finish-tail-only-S8", 1025, 16384, 16384, 4, 8),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("case", TALL, ids=[c[0] for c in TALL])
def test_column_sum_tall_kernel_is_exact(case, dtype):
    _, M, ld, N, vec, S = case
    if S == 512:                                                    # slabs 507 .. 511 hold no row
        rows = -(-M // S)
        assert rows == 79 and rows * 507 >= M > rows * 506
    check_exact_column_sum(M, ld, N, dtype, vec=vec, S=S)


@pytest.mark.parametrize("dtype,offset,vec", [(torch.float32, 1, 1), (torch.bfloat16, 1, 1), (torch.bfloat16, 2, 2)],
                         ids=["f32-off1-vec1", "bf16-off1-vec1", "bf16-off2-vec2"])
def test_column_sum_alignment_fallback(dtype, offset, vec):
    """A contiguous [1100, 8] view that starts `offset` elements into its buffer: N and ld allow vec 4, the base does not."""
    check_exact_column_sum(1100, 8, 8, dtype, offset=offset, vec=vec, S=slabs(1100, 8, vec))


def test_column_sum_single_slab_writes_out_directly():
    """S == 1 (M = 1025, N = 32769: 513 column blocks at vec 1): no workspace, no finish kernel."""
    M, N = 1025, 32769
    assert slabs(M, N, 1) == 1 and vec_of(N, N, 0, 4) == 1
    check_exact_column_sum(M, N, N, torch.float32, vec=1, S=1)
    xf, want = _int_mats.pop((M, N, N))                             # 134 MB: not kept for the rest of the session
    # and through the C ABI with no workspace at all: out is written by the one kernel
    xd, out = xf.to(dev()), torch.full((N,), float("nan"), device=dev())
    _lib.lib().vqa_launch_log_reset()
    _lib.check(_lib.lib().vqa_column_sum(ptr(xd), N, ptr(out), None, 0, M, N, None), "column_sum")
    assert [g for g, _ in launch_log()] == expected_launches(M, N, 1, 1)
    assert torch.equal(out.cpu().double(), want.double())


def test_column_sum_single_slab_asks_for_no_workspace():
    """vqa_column_sum_workspace_bytes sizes for the vector widths column_vec can choose for this N (N % vec == 0): an odd N
    runs at vec 1, S == 1 here, and no workspace is asked for.  (It used to take the maximum over vec 1, 2, 4 whatever N and
    answered 524304 = 4 slabs of 32769 floats.)  An even N of the same size still gets the larger widths' slabs."""
    h = _lib.lib()
    assert slabs(1025, 32769, 1) == 1
    assert h.vqa_column_sum_workspace_bytes(1025, 32769) == 0
    assert h.vqa_column_sum_workspace_bytes(1025, 32768) == slabs(1025, 32768, 4) * 32768 * 4
    assert h.vqa_column_sum_workspace_bytes(1100, 310) == slabs(1100, 310, 2) * 310 * 4
    assert h.vqa_column_sum_workspace_bytes(1100, 155) == slabs(1100, 155, 1) * 155 * 4
    assert h.vqa_column_sum_workspace_bytes(1024, 32769) == 0                                  # the short kernel


@pytest.mark.parametrize("M", [100, 1100])
def test_column_sum_out_is_reused_and_fully_overwritten(M):
    xf, want = int_matrix(M, 310, 310)
    xd = xf.to(dev())
    out = torch.full((310,), float("nan"), device=dev())
    got = ops.column_sum(xd, out=out)
    assert got.data_ptr() == out.data_ptr()
    first = bits(out).clone()
    assert torch.equal(out.cpu().double(), want.double())           # no NaN left
    got = ops.column_sum(xd, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(bits(out), first)


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("M", [100, 1100])
def test_column_sum_non_finite_stays_in_its_column(M, dtype):
    xf, want = int_matrix(M, 40, 40)
    x = xf.clone()
    x[5, 3] = float("inf")
    x[M - 1, 20] = float("nan")
    got = ops.column_sum(x.to(dev()).to(dtype)).cpu()
    assert got[3].item() == float("inf") and math.isnan(got[20].item())
    keep = [n for n in range(40) if n not in (3, 20)]
    assert torch.equal(got[keep].double(), want[keep].double())


_real_mats = {}


def real_matrix(kind):
    if kind not in _real_mats:
        g = torch.Generator().manual_seed(18432)
        x = torch.randn(18432, 310, generator=g)
        if kind == "cancel":
            x = x + torch.where(torch.rand(18432, 310, generator=g) < 0.5, -1e4, 1e4)
        _real_mats[kind] = x
    return _real_mats[kind]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["normal", "cancel"])
def test_column_sum_rounded(kind, dtype, measured):
    """[18432, 310] (the product's tall shape, vec 2): error per column relative to its sum of |x|."""
    x = real_matrix(kind).to(dtype)                                  # bf16: the inputs are rounded first
    x32 = x.float().numpy()
    ref = x32.astype(np.float64).sum(0)
    sumabs = np.abs(x32).astype(np.float64).sum(0)
    plain = x32.sum(0, dtype=np.float32)
    e_np = float((np.abs(plain.astype(np.float64) - ref) / sumabs).max())
    got = ops.column_sum(x.to(dev())).cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    name = "colsum %s %s err/sum|x|" % (kind, "bf16" if dtype == torch.bfloat16 else "f32")
    measured(name, float((err / sumabs).max()), 4 * e_np, "numpy fp32: %.3e" % e_np)
    assert (err <= np.maximum(4 * e_np * sumabs, ulp(ref))).all(), name


# ---- 2. bias_act / act_bwd_colsum ---------------------------------------------------------------------------------------------
NONE, RELU, SIGMOID = 0, 1, 2
GUARD = 8
AS, GS = (1, 15, 16, 17, 510), (1, 3)


def guarded(data):
    """The array on the device with GUARD sentinels behind it."""
    t = torch.full((data.size + GUARD,), SENT, device=dev())
    t[:data.size].copy_(torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32)).flatten())
    return t


def strided_rows(rows, stride):
    """[G, A] rows `stride` apart in a sentinel-filled buffer -> (device buffer, mask of the gaps)."""
    G, A = rows.shape
    host = np.full((G, stride), SENT, np.float32)
    host[:, :A] = rows
    gaps = np.ones((G, stride), bool)
    gaps[:, :A] = False
    return torch.from_numpy(host).to(dev()), gaps


def bias_act(y, bias, bias_stride, G, B, A, act, group_first):
    """y [G,B,A] numpy -> out numpy, [G,B,A] or [B,G,A]; the guard behind out must survive."""
    yd = guarded(y)
    out = torch.full((G * B * A + GUARD,), SENT, device=dev())
    _lib.check(_lib.lib().vqa_bias_act(ptr(yd), ptr(bias), bias_stride, ptr(out), G, B, A, act, int(group_first), None), "bias_act")
    res = out.cpu().numpy()
    assert (res[G * B * A:] == SENT).all(), "bias_act wrote behind out"
    return res[:G * B * A].reshape((G, B, A) if group_first else (B, G, A))


def act_bwd(gy, out, d_bias, d_bias_stride, G, B, A, act, group_first):
    """gy / out numpy in the layout of `group_first` -> gz [G,B,A] numpy; d_bias (a device buffer or None) is written in place."""
    gz = torch.full((G * B * A + GUARD,), SENT, device=dev())
    gyd, outd = guarded(gy), guarded(out)                             # (held here: the call takes addresses)
    _lib.check(_lib.lib().vqa_act_bwd_colsum(ptr(gyd), ptr(outd), ptr(gz), ptr(d_bias), d_bias_stride, G, B, A, act,
                                             int(group_first), None), "act_bwd_colsum")
    res = gz.cpu().numpy()
    assert (res[G * B * A:] == SENT).all(), "act_bwd_colsum wrote behind gz"
    return res[:G * B * A].reshape(G, B, A)


def to_layout(x_gba, group_first):
    return x_gba if group_first else np.ascontiguousarray(x_gba.transpose(1, 0, 2))


@pytest.mark.parametrize("B", [1, 16, 127, 128, 129, 300])
def test_bias_act_and_act_bwd_colsum_are_exact(B):
    """Integers, act none and relu (about half of out exactly zero), bias and d_bias rows 3 resp. 5 floats apart in
    sentinel-filled buffers: out, gz [G,B,A] and d_bias equal the integer reference; the gaps keep their sentinel."""
    for A in AS:
        for G in GS:
            rng = np.random.default_rng(B * 1000 + A * 10 + G)
            y = rng.integers(-8, 9, (G, B, A))
            bias = rng.integers(-4, 5, (G, A))
            gy = rng.integers(-8, 9, (G, B, A))
            for act in (NONE, RELU):
                z = y + bias[:, None, :]
                want_out = np.maximum(z, 0) if act == RELU else z
                want_gz = gy * (want_out > 0) if act == RELU else gy
                want_db = want_gz.sum(1)
                assert np.abs(want_gz).sum(1).max() < 2 ** 24
                if act == RELU and A >= 15 and B >= 16:
                    assert 0.3 < (want_out == 0).mean() < 0.7
                for group_first in (True, False):
                    what = "B=%d A=%d G=%d act=%d group_first=%d" % (B, A, G, act, group_first)
                    bd, bgaps = strided_rows(bias, A + 3)
                    out = bias_act(y, bd, A + 3, G, B, A, act, group_first)
                    assert np.array_equal(out, to_layout(want_out, group_first).astype(np.float32)), what
                    db, dgaps = strided_rows(np.full((G, A), SENT), A + 5)
                    gz = act_bwd(to_layout(gy, group_first), out, db, A + 5, G, B, A, act, group_first)
                    assert np.array_equal(gz, want_gz.astype(np.float32)), what
                    dbh = db.cpu().numpy()
                    assert np.array_equal(dbh[:, :A], want_db.astype(np.float32)), what
                    assert (dbh[dgaps] == SENT).all() and (bd.cpu().numpy()[bgaps] == SENT).all(), what
                    gz_only = act_bwd(to_layout(gy, group_first), out, None, 0, G, B, A, act, group_first)   # d_bias = NULL
                    assert np.array_equal(gz_only, gz), what
            out = bias_act(y, None, 0, G, B, A, RELU, True)                                                   # no bias
            assert np.array_equal(out, np.maximum(y, 0).astype(np.float32))


@pytest.mark.parametrize("B", [1, 16, 127, 128, 129, 300])
def test_sigmoid_forward_and_backward_rounded(B, measured):
    """act = sigmoid with +-30 and +-100 among the inputs: out against a float64 logistic, gz against g * s * (1 - s) in float64
    from the kernel's own fp32 out."""
    worst = {"out": (0.0, 0.0), "gz": (0.0, 0.0)}
    for A in AS:
        for G in GS:
            rng = np.random.default_rng(B * 1000 + A * 10 + G + 7)
            y = (rng.standard_normal((G, B, A)) * 4).astype(np.float32)
            flat = y.reshape(-1)
            flat[:min(4, flat.size)] = np.array([30.0, -30.0, 100.0, -100.0], np.float32)[:flat.size]
            bias = rng.standard_normal((G, A)).astype(np.float32)
            flat[:min(4, flat.size)] -= np.broadcast_to(bias[:, None, :], y.shape).reshape(-1)[:min(4, flat.size)]
            gy = rng.standard_normal((G, B, A)).astype(np.float32)
            z32 = y + bias[:, None, :]
            with np.errstate(over="ignore"):
                plain = F32(1) / (F32(1) + np.exp(-z32))
                ref = 1.0 / (1.0 + np.exp(-(y.astype(np.float64) + bias[:, None, :].astype(np.float64))))
            bar, _ = rounded_bar(ref, plain)
            for group_first in (True, False):
                what = "B=%d A=%d G=%d group_first=%d" % (B, A, G, group_first)
                out = bias_act(y, torch.from_numpy(bias).to(dev()), A, G, B, A, SIGMOID, group_first)
                assert np.isfinite(out).all() and out.min() >= 0.0 and out.max() <= 1.0, what
                e = float(np.abs(out.astype(np.float64) - to_layout(ref, group_first)).max())
                assert e <= bar, (what, e, bar)
                worst["out"] = max(worst["out"], (e / bar, e))
                o_gba = out if group_first else np.ascontiguousarray(out.transpose(1, 0, 2))
                o64, g64 = o_gba.astype(np.float64), gy.astype(np.float64)
                ref_gz = g64 * o64 * (1.0 - o64)
                bar_gz, _ = rounded_bar(ref_gz, gy * o_gba * (F32(1) - o_gba))
                gz = act_bwd(to_layout(gy, group_first), out, None, 0, G, B, A, SIGMOID, group_first)
                e = float(np.abs(gz.astype(np.float64) - ref_gz).max())
                assert e <= bar_gz, (what, e, bar_gz)
                worst["gz"] = max(worst["gz"], (e / bar_gz, e))
    for k, (ratio, e) in worst.items():
        measured("sigmoid %s worst err/bar B=%d" % (k, B), ratio, 1.0, "abs %.3e" % e)


# ---- 3. clip norm and coefficient ---------------------------------------------------------------------------------------------
NORM_SIZES = SIZES + [2 ** 20 + 4 * 1024 * 256 + 7, 2 ** 24 + 2 ** 20 + 3]
NORM_BLOCKS = 1024


def sweep_float4s(n):
    """float4s one grid-stride sweep of sumsq_partial_kernel covers (vqa_grad_norm_clip_coef's grid x 256 threads)."""
    need = (n // 4 + 255) // 256
    return min(NORM_BLOCKS, max(need, 1)) * 256


def indicator_positions(n):
    """The positions P named in the module docstring, at most 4096 of them, all inside [0, n)."""
    n4 = n // 4
    P = {0, n - 1}
    P.update(range(n - n % 4, n))                                   # the scalar tail
    if n4:
        P.update(range(4 * (n4 - 1), 4 * n4))                       # the last full float4
        sweep = sweep_float4s(n)
        for first in range(0, n4, sweep):                           # first and last float4 of every sweep
            last = min(first + sweep, n4) - 1
            P.update((4 * first, 4 * first + 3, 4 * last, 4 * last + 3))
    stride = (n // 1000) | 1                                        # odd: coprime to 4 * 1024 * 256 = 2**20
    assert math.gcd(stride, 4 * 1024 * 256) == 1
    P.update((j * stride) % n for j in range(min(1000, n)))
    assert 0 < len(P) <= 4096 and min(P) >= 0 and max(P) < n
    return sorted(P)


def clip(g, max_norm, fill=float("nan")):
    """(norm, coef) as fp32 numpy scalars from vqa_grad_norm_clip_coef with a workspace that held `fill`."""
    out = torch.full((2,), float("nan"), device=dev())
    ws = torch.full((NORM_BLOCKS,), fill, device=dev(), dtype=torch.float64)
    ops.grad_norm_clip_coef(g, max_norm, out, ws)
    got = out.cpu().numpy()
    return got[0], got[1]


def coef_fp32(norm, max_norm):
    return min(F32(1), F32(max_norm) / (F32(norm) + F32(1e-6))) if max_norm > 0 else F32(1)


_dense = {}


def dense_normal(n):
    if n not in _dense:
        _dense.clear()                                              # one large buffer at a time
        _dense[n] = torch.randn(n, generator=torch.Generator().manual_seed(n))
    return _dense[n]


@pytest.mark.parametrize("n", NORM_SIZES)
def test_clip_norm_of_indicator_vectors_is_exact(n):
    """k ones among zeros: the norm is float32(sqrt(float64(k))) bit for bit, whatever a NaN- or zero-filled workspace held."""
    P = indicator_positions(n)
    sweep = sweep_float4s(n)
    iterations = -(-(n // 4) // sweep)
    assert iterations == {2 ** 20 + 3: 1, 2 ** 20 + 4 * 1024 * 256 + 7: 3, 2 ** 24 + 2 ** 20 + 3: 17}.get(n, iterations)
    g = torch.zeros(n, device=dev())
    g[torch.tensor(P, device=dev())] = 1.0
    want = F32(np.sqrt(np.float64(len(P))))
    norm, coef = clip(g, 0.25)
    assert norm.tobytes() == want.tobytes(), (n, len(P), norm, want)
    assert coef.tobytes() == coef_fp32(norm, 0.25).tobytes()
    norm0, coef0 = clip(g, 0.25, fill=0.0)
    assert (norm0.tobytes(), coef0.tobytes()) == (norm.tobytes(), coef.tobytes())
    if len(P) > 1:                                                  # fp32 tells sqrt(k) from sqrt(k -+ 1) for k <= 4096
        assert F32(np.sqrt(np.float64(len(P) - 1))) != want != F32(np.sqrt(np.float64(len(P) + 1)))


def test_clip_norm_of_dense_integers_is_exact_past_the_spill():
    """n = 2**24 + 2**20 + 3 (17 iterations a thread: the fp32 run is moved to float64 at 16, the counter restarts), integers in
    [-3, 3]: a thread's fp32 run stays below 16 * 4 * 9, so the sum of squares is exact and the norm is the float32 of its root."""
    n = NORM_SIZES[-1]
    gi = torch.randint(-3, 4, (n,), generator=torch.Generator().manual_seed(5), dtype=torch.int8)
    ss = int((gi.to(torch.int32) ** 2).sum(dtype=torch.int64))
    assert ss < 2 ** 53
    norm, coef = clip(gi.float().to(dev()), 0.25)
    assert norm.tobytes() == F32(np.sqrt(np.float64(ss))).tobytes()
    assert coef.tobytes() == coef_fp32(norm, 0.25).tobytes()


@pytest.mark.parametrize("n", NORM_SIZES)
def test_clip_norm_of_dense_normal_gradients(n, measured):
    g = dense_normal(n)
    want = torch.linalg.vector_norm(g.double()).item()
    norm, coef = clip(g.to(dev()), 0.25)
    e = abs(float(norm) - want) / want
    measured("norm rel n=%d" % n, e, 1e-6, "fp32 ulp/2 = 6.0e-08")
    assert e <= 1e-6
    assert coef.tobytes() == coef_fp32(norm, 0.25).tobytes()


@pytest.mark.parametrize("n", [1, 5, 1025, 2 ** 20 + 3])
def test_clip_coefficient(n):
    g = dense_normal(n).to(dev()) + 2.0                              # (n = 1: never zero)
    norm, coef = clip(g, 0.0)
    assert norm > 0 and coef.tobytes() == F32(1).tobytes()           # max_norm = 0: no clipping
    norm, coef = clip(g, -1.0)
    assert coef.tobytes() == F32(1).tobytes()
    norm, coef = clip(g, float(norm) * 2)
    assert coef.tobytes() == F32(1).tobytes()                        # a norm below the cap
    norm, coef = clip(g, float(norm) / 3)
    assert coef < 1 and coef.tobytes() == coef_fp32(norm, float(norm) / 3).tobytes()
    norm, coef = clip(torch.zeros(n, device=dev()), 0.25)
    assert norm.tobytes() == F32(0).tobytes() and coef.tobytes() == F32(1).tobytes()


# ---- 4. Adam ------------------------------------------------------------------------------------------------------------------
def c_float(x):
    """What a C `float` parameter holds of the Python number, widened again."""
    return float(F32(x))


def step_scalars(lr, b1, b2, t):
    """{lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} in Python floats, as trainer._set_step_scalars computes them, from the float32 lr
    and betas vqa_adam_step receives; rounded to fp32 as the copy into the device words does."""
    lr, b1, b2 = c_float(lr), c_float(b1), c_float(b2)
    return F32(lr / (1.0 - b1 ** t)), F32(1.0 / math.sqrt(1.0 - b2 ** t))


def adam_plain32(p, g, m, v, coef, t, lr=LR):
    """One step of adam_kernel's formula in numpy float32, operation by operation."""
    b1, b2, eps, one = F32(B1), F32(B2), F32(EPS), F32(1)
    step_size, inv_sqrt_bc2 = step_scalars(lr, B1, B2, t)
    gs = g * F32(coef)
    m = b1 * m + (one - b1) * gs
    v = b2 * v + (one - b2) * gs * gs
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + eps)
    return p, m, v


def adam_ref64(p0, m0, v0, first_step, lr=LR):
    """torch.optim.Adam in float64 on the CPU with the hyper-parameters the C ABI receives, its state set to (m0, v0) after
    first_step - 1 steps."""
    rp = p0.double().clone().requires_grad_()
    opt = torch.optim.Adam([rp], lr=c_float(lr), betas=(c_float(B1), c_float(B2)), eps=c_float(EPS))
    opt.state[rp] = {"step": torch.tensor(float(first_step - 1)), "exp_avg": m0.double().clone(), "exp_avg_sq": v0.double().clone()}
    return rp, opt


def check_adam(label, got, ref, plain, measured, scale=1.0):
    """got / ref / plain: (p, m, v) of the kernel, of float64, of numpy float32.  The rounded rule on all three, then the project's
    bars (2e-6 absolute on p, 1e-6 of the maximum on m and v)."""
    for name, a, r, q in zip("pmv", got, ref, plain):
        r = r.detach().numpy()
        e = float(np.abs(a.cpu().numpy().astype(np.float64) - r).max())
        bar, e_np = rounded_bar(r, q)
        measured("adam %s %s" % (name, label), e / scale, bar / scale, "numpy fp32: %.3e" % (e_np / scale))
        assert e <= bar, (label, name, e, bar)
        if name == "p":
            assert e <= 2e-6, (label, e)
        elif np.abs(r).max() > 0:
            assert e <= 1e-6 * np.abs(r).max(), (label, name, e)


def run_adam(p0, grads, clip_norm, measured, label, lr=LR, m0=None, v0=None, first_step=1, scale=1.0):
    """len(grads) steps of vqa_adam_step from (p0, m0, v0) against float64 and against the numpy float32 evaluation."""
    n = p0.numel()
    m0 = torch.zeros(n) if m0 is None else m0
    v0 = torch.zeros(n) if v0 is None else v0
    p, m, v = p0.to(dev()), m0.to(dev()), v0.to(dev())
    nc = torch.zeros(2, device=dev()) if clip_norm else None          # None: the coef_ptr == nullptr form
    ws = torch.empty(NORM_BLOCKS, device=dev(), dtype=torch.float64)
    rp, opt = adam_ref64(p0, m0, v0, first_step, lr)
    q = (p0.numpy().copy(), m0.numpy().copy(), v0.numpy().copy())
    for k, gi in enumerate(grads):
        gd = gi.to(dev())
        coef = F32(1)
        if clip_norm:
            ops.grad_norm_clip_coef(gd, clip_norm, nc, ws)
            coef = coef_fp32(F32(torch.linalg.vector_norm(gi.double()).item()), clip_norm)
        ops.adam_step(p, gd, m, v, nc, lr, B1, B2, EPS, first_step + k)
        rp.grad = gi.double()
        if clip_norm:
            torch.nn.utils.clip_grad_norm_([rp], clip_norm)
        opt.step()
        q = adam_plain32(*q[:1], gi.numpy(), *q[1:], coef, first_step + k, lr)
    st = opt.state[rp]
    check_adam(label, (p, m, v), (rp, st["exp_avg"], st["exp_avg_sq"]), q, measured, scale)
    return p, m, v


@pytest.mark.parametrize("clip_norm", [0.25, None])
@pytest.mark.parametrize("n", SIZES)
def test_adam_matches_torch_adam_in_float64(n, clip_norm, measured):
    """Five steps with growing gradients: p, m and v; with the clip coefficient and with norm_and_coef = None."""
    g0 = torch.Generator().manual_seed(n)
    p0, grad = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    run_adam(p0, [grad * s for s in range(1, 6)], clip_norm, measured, "n=%d clip=%s" % (n, clip_norm))


def test_adam_from_zero_parameters(measured):
    """p0 = 0: the parameter's own rounding no longer hides the update's arithmetic; errors are reported relative to lr."""
    n = 4099
    grad = torch.randn(n, generator=torch.Generator().manual_seed(11))
    run_adam(torch.zeros(n), [grad * s for s in range(1, 6)], None, measured, "p0=0 /lr", scale=LR)


@pytest.mark.parametrize("steps", [1, 3])
def test_adam_with_gradients_around_eps(steps, measured):
    """|g| log-uniform in [1e-12, 1e-6], mixed signs, no clip, from p0 = 0: sqrt(v_hat) and eps = 1e-8 are comparable, so eps
    inside the root, eps ahead of the bias correction or a missing correction of v each move p by a large fraction of lr."""
    n = 4099
    g0 = torch.Generator().manual_seed(steps)
    mag = 10.0 ** (torch.rand(n, generator=g0, dtype=torch.float64) * 6 - 12)
    grad = (mag * torch.where(torch.rand(n, generator=g0) < 0.5, -1.0, 1.0)).float()
    assert 1e-12 <= grad.abs().min() and grad.abs().max() <= 1.0001e-6
    assert float(grad.abs().min()) ** 2 * (1 - B2) > 1.2e-38          # g^2 (1 - b2) is a normal float
    p, _, _ = run_adam(torch.zeros(n), [grad * s for s in range(1, steps + 1)], None, measured, "g~eps steps=%d /lr" % steps, scale=LR)
    assert 0.05 * LR < p.abs().max().item() <= 1.01 * LR * steps      # the updates are of the order of lr, not lost


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_static_step_from_nonzero_moments(step, measured):
    n = 4099
    g0 = torch.Generator().manual_seed(100 + step)
    p0, grad = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    m0, v0 = torch.randn(n, generator=g0) * 0.1, torch.rand(n, generator=g0) * 0.01
    run_adam(p0, [grad], None, measured, "step=%d" % step, m0=m0, v0=v0, first_step=step)


@pytest.mark.parametrize("n", [5, 1025])
def test_adam_zero_gradient_and_moments_change_nothing(n):
    p0 = torch.randn(n, generator=torch.Generator().manual_seed(n))
    p, g, m, v = p0.to(dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev()), torch.zeros(n, device=dev())
    ops.adam_step(p, g, m, v, None, LR, B1, B2, EPS, 1)
    assert torch.equal(bits(p), bits(p0)) and not bits(m).any() and not bits(v).any()      # not even a -0.0


@pytest.mark.parametrize("n", [5, 1025, 2 ** 20 + 3])
def test_adam_static_dyn_and_coefficient_forms(n, measured):
    """adam_step and adam_step_dyn are one kernel: bitwise the same p, m, v over three steps when the device scalars are the
    static form's own.  norm_and_coef = [x, 1.0] is bitwise the None form; [x, 0.37] scales the gradient."""
    g0 = torch.Generator().manual_seed(n + 1)
    p0, grad = torch.randn(n, generator=g0), torch.randn(n, generator=g0)
    m0, v0 = torch.randn(n, generator=g0) * 0.1, torch.rand(n, generator=g0) * 0.01
    nc = torch.tensor([3.0, 0.37], device=dev())

    def run(form, coef):
        p, m, v, gd = p0.to(dev()), m0.to(dev()), v0.to(dev()), grad.to(dev())
        for t in (1, 2, 3):
            if form == "dyn":
                ops.adam_step_dyn(p, gd, m, v, coef, torch.tensor(step_scalars(LR, B1, B2, t), device=dev()), B1, B2, EPS)
            else:
                ops.adam_step(p, gd, m, v, coef, LR, B1, B2, EPS, t)
        return p, m, v
    static, dyn = run("static", nc), run("dyn", nc)
    assert not torch.equal(static[0], p0.to(dev()))
    for a, b in zip(static, dyn):
        assert torch.equal(bits(a), bits(b))
    none, one = run("static", None), run("static", torch.tensor([123.0, 1.0], device=dev()))
    for a, b, c in zip(none, one, run("dyn", None)):
        assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c))
    # [x, 0.37]: float64 on the gradient scaled by the float32 coefficient
    rp, opt = adam_ref64(p0, m0, v0, 1)
    q = (p0.numpy().copy(), m0.numpy().copy(), v0.numpy().copy())
    for t in (1, 2, 3):
        rp.grad = grad.double() * c_float(0.37)
        opt.step()
        q = adam_plain32(q[0], grad.numpy(), q[1], q[2], 0.37, t)
    st = opt.state[rp]
    check_adam("coef=0.37 n=%d" % n, static, (rp, st["exp_avg"], st["exp_avg_sq"]), q, measured)


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """Every call below is refused on the host (ValueError from ops.py) or by a VQA_REQUIRE ahead of the launch
    (VqaLibraryError: the alignment checks of vqa_adam_step / vqa_adam_step_dyn / vqa_grad_norm_clip_coef come before
    VQA_LAUNCH); the launch log stays empty and no buffer changes."""
    h = _lib.lib()
    n = 16
    d = dev()
    p, g, m, v = (torch.full((n,), float(k + 1), device=d) for k in range(4))
    nc, sc = torch.tensor([1.0, 0.5], device=d), torch.tensor([1e-3, 1.0], device=d)
    out = torch.full((2,), 7.0, device=d)
    ws = torch.zeros(NORM_BLOCKS, device=d, dtype=torch.float64)
    assert ws.numel() * 8 == h.vqa_grad_norm_workspace_bytes()
    odd = torch.zeros(n + 4, device=d)[1:n + 1]                     # contiguous, n long, 4 bytes off 16-byte alignment
    assert odd.is_contiguous() and odd.data_ptr() % 16 == 4
    x2 = torch.ones(1100, 8, device=d)
    buf = (ctypes.c_ulonglong * 16)()

    def refused(exc, fn, *args, **kw):
        h.vqa_launch_log_reset()
        with pytest.raises(exc):
            fn(*args, **kw)
        assert h.vqa_launch_log(buf, 16) == 0, "a refused call launched a kernel"

    E, L = ValueError, _lib.VqaLibraryError
    tail = (LR, B1, B2, EPS, 1)
    for fn, rest in ((ops.adam_step, tail), (ops.adam_step_dyn, (sc, B1, B2, EPS))):
        refused(E, fn, p, g, m[:n - 1], v, nc, *rest)               # an m shorter than p
        refused(E, fn, p, g[:n - 1], m, v, nc, *rest)
        refused(E, fn, p, g, m, torch.zeros(n + 1, device=d), nc, *rest)
        refused(E, fn, p, g.double(), m, v, nc, *rest)              # a float64 g
        refused(E, fn, p.double(), g, m, v, nc, *rest)
        refused(E, fn, p, g, m, torch.zeros(2 * n, device=d)[::2], nc, *rest)      # not contiguous
        refused(E, fn, p[:0], g[:0], m[:0], v[:0], nc, *rest)       # empty
        refused(E, fn, p, g, m, v, nc[:1], *rest)                   # a one-element norm_and_coef
        refused(E, fn, p, g, m, v, nc.double(), *rest)
        refused(E, fn, p, g, m, v, nc.cpu(), *rest)
        refused(L, fn, p, odd, m, v, nc, *rest)                     # g not 16-byte aligned: the library's VQA_REQUIRE
    refused(E, ops.adam_step, p, g, m, v, nc, LR, B1, B2, EPS, 0)   # step counts from 1
    refused(E, ops.adam_step_dyn, p, g, m, v, nc, sc[:1], B1, B2, EPS)
    refused(E, ops.adam_step_dyn, p, g, m, v, nc, sc.double(), B1, B2, EPS)
    refused(E, ops.adam_step_dyn, p, g, m, v, nc, sc.cpu(), B1, B2, EPS)
    refused(E, ops.adam_step_dyn, p, g, m, v, nc, None, B1, B2, EPS)
    refused(E, ops.grad_norm_clip_coef, g, 0.25, out[:1], ws)
    refused(E, ops.grad_norm_clip_coef, g, 0.25, out.double(), ws)
    refused(E, ops.grad_norm_clip_coef, g, 0.25, out, ws[:NORM_BLOCKS - 1])        # workspace too small
    refused(E, ops.grad_norm_clip_coef, g, 0.25, out, ws.cpu())
    refused(E, ops.grad_norm_clip_coef, g.double(), 0.25, out, ws)
    refused(E, ops.grad_norm_clip_coef, g[:0], 0.25, out, ws)
    refused(L, ops.grad_norm_clip_coef, odd, 0.25, out, ws)
    refused(E, ops.column_sum, x2, cols=0)
    refused(E, ops.column_sum, x2, cols=9)
    refused(E, ops.column_sum, x2, cols=-1)
    refused(E, ops.column_sum, x2.view(100, 11, 8))                 # a 3-D input
    torch.cuda.synchronize()
    for k, t in enumerate((p, g, m, v)):
        assert bool((t == float(k + 1)).all())
    assert out.tolist() == [7.0, 7.0] and nc.tolist() == [1.0, 0.5]
    # ... and the accepted forms launch: one kernel for Adam with and without a coefficient, two for the norm
    for call in (lambda: ops.adam_step(p, g, m, v, None, *tail), lambda: ops.adam_step_dyn(p, g, m, v, nc, sc, B1, B2, EPS)):
        h.vqa_launch_log_reset()
        call()
        assert h.vqa_launch_log(buf, 16) == 1
    h.vqa_launch_log_reset()
    ops.grad_norm_clip_coef(g, 0.25, out, ws)
    assert h.vqa_launch_log(buf, 16) == 2
    torch.cuda.synchronize()
