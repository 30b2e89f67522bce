"""Kernel-level tests of the question encoder's HIP kernels (csrc/gru_gemm.hip: vqa_split_weights_pack and
vqa_gemm_nt_split_batched; csrc/gru.hip: vqa_gru_gates_fwd / _bwd) and of ops.GruSequence's choice between the batched kernel
and the grouped fallback, at the shapes, strides and values where such kernels go wrong:

  1  the batched NT GEMM against float64 over a shape table (production shapes of both weight images, every tile edge of M, N
     and K, strides, one shared A, grids that are not a multiple of the 8 XCDs), stores confined to the G [M,N] windows
  2  the weight image is an exact three-way split, in both orientations (one-hot and small-integer operands: bit for bit)
  3  operands at the edges of fp32, and non-finite values where a padded load reaches but the product must not
  4  the gate kernels against float64: every output, every history slot, null and given optional operands, saturated gates;
     refusals (no GPU needed: the checks precede the launch)
  5  BayesianGRU's GPU form against the step-by-step float64 form at the batch sizes the shipped configs train with

All operands are seeded and built on the CPU; every reference is a float64 restatement written here.  The GEMM bars are the
split engine's own (tests/test_gpu_split.py: error / sum_k |a_k||w_k| <= 4e-6, rms within 2x of the fp32 MFMA engine on the same
operands); the gate and sequence bars derive from what the same formulas make in float32 with torch on the CPU."""
import ctypes

import pytest
import torch

from kernel_harness import (EPS32, E_BADARG, E_UNSUPPORTED, INF, NAN, SENT, _bits, _ptr, _same_bits, _sentinel, _untouched, dev,
                            ops, spy_launches)  # noqa: F401  (ops: the fixture)
from vqa_playground_pytorch_amd.encoder import BayesianGRU

gpu = pytest.mark.gpu
MAX_BAR, RMS_FACTOR = 4e-6, 2.0          # tests/test_gpu_split.py::_compare_with_engine


def _classes(t):
    """0 finite, 1 +Inf, 2 -Inf, 3 NaN"""
    return torch.where(torch.isnan(t), 3, torch.where(torch.isposinf(t), 1, torch.where(torch.isneginf(t), 2, 0)))


def _dev(t):
    """t on the GPU with the strides it has (a padded row stride survives; .to() would pack the rows)"""
    if t is None:
        return None
    out = torch.empty_strided(t.shape, t.stride(), device=dev(), dtype=t.dtype)
    out.copy_(t)
    return out


# ---- 1. the batched NT GEMM ------------------------------------------------------------------------------------------------------
class Case:
    """G problems C_g [M,N] = A_g [M,K] W_g^T (+ bias_g).  A_g starts a_off + g * a_gs floats into a flat tensor, rows lda apart
    (a_gs = 0: one shared A; a_gs < lda: the problems interleave as batched_linear's [B,G,K] input does); W [G,N,K], or [G,K,N]
    when transposed, rows wpad floats longer than they need be; C_g starts c_off + g * c_gs floats into a sentinel-filled flat
    tensor, rows ldc apart; bias [G,N] rows of stride N + 4."""

    def __init__(self, G, M, N, K, lda=None, a_gs=None, a_off=8, ldc=None, c_gs=None, c_off=3, bias=False, transposed=False, wpad=0):
        self.G, self.M, self.N, self.K = G, M, N, K
        self.lda = K if lda is None else lda
        self.a_gs = M * self.lda + 8 if a_gs is None else a_gs
        self.a_off, self.c_off = a_off, c_off
        self.ldc = N if ldc is None else ldc
        self.c_gs = M * self.ldc if c_gs is None else c_gs
        self.bias, self.transposed, self.wpad = bias, transposed, wpad
        assert self.lda % 4 == 0 and self.lda >= K and self.a_gs % 4 == 0 and a_off % 4 == 0 and self.ldc >= N

    def __repr__(self):
        return "G%d M%d N%d K%d lda%d ags%d ldc%d cgs%d%s%s" % (self.G, self.M, self.N, self.K, self.lda, self.a_gs, self.ldc, self.c_gs,
                                                                " bias" if self.bias else "", " T" if self.transposed else "")

    def a_size(self):
        return self.a_off + (self.G - 1) * self.a_gs + self.M * self.lda + 64

    def a_view(self, flat):
        return flat.as_strided((self.G, self.M, self.K), (self.a_gs, self.lda, 1), self.a_off)

    def c_size(self):
        return self.c_off + (self.G - 1) * self.c_gs + self.M * self.ldc + 64

    def c_view(self, flat):
        return flat.as_strided((self.G, self.M, self.N), (self.c_gs, self.ldc, 1), self.c_off)

    def w_logical(self, w):
        """[G,N,K] view of the weights, whichever way they are stored"""
        return w.transpose(1, 2) if self.transposed else w


def draw_operands(case, gen, ints=False):
    """(flat A storage, W, bias or None) on the CPU.  The gaps of the A storage hold finite garbage."""
    c = case
    if ints:
        rnd = lambda *s: torch.randint(-8, 9, s, generator=gen).float()      # noqa: E731
    else:
        rnd = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    flat = rnd(c.a_size())
    rows, cols = (c.K, c.N) if c.transposed else (c.N, c.K)
    w = rnd(c.G, rows, cols + c.wpad)
    w = (w if ints else w / c.K ** 0.5)[:, :, :cols]          # (a view: the rows keep their stride of cols + wpad)
    bias = rnd(c.G, c.N + 4)[:, :c.N] if c.bias else None
    return flat, w, bias


def grid_of(case, rb=None):
    """(row blocks, tiles_m, tiles_n, workgroups) of the launch: vqa_gemm_nt_split_batched's choice restated"""
    c = case
    tiles_n = (c.N + 159) // 160
    if rb is None:
        rb = 9
        if c.M <= 1024:
            best = 1e30
            for cand in (9, 8, 7):
                wgs = ((c.M + 16 * cand - 1) // (16 * cand)) * tiles_n * c.G
                cost = ((wgs + 255) // 256) * cand
                if cost < best - 1e-9:
                    best, rb = cost, cand
    tiles_m = (c.M + 16 * rb - 1) // (16 * rb)
    return rb, tiles_m, tiles_n, tiles_m * tiles_n * c.G


def pack_image(ops, case, w):
    """vqa_split_weights_pack into an image of exactly vqa_split_weights_bytes with a sentinel tail behind it"""
    c, L = case, ops._lib.lib()
    nbytes = L.vqa_split_weights_bytes(c.G, c.N, c.K)
    assert nbytes % 16 == 0
    img = torch.full((nbytes // 4 + 64,), SENT, device=dev(), dtype=torch.float32)
    ops._launch("split_weights_pack", (c.G, c.N, c.K, c.transposed), L.vqa_split_weights_pack, _ptr(w), w.stride(0), w.stride(1),
                int(c.transposed), _ptr(img), nbytes, c.G, c.N, c.K)
    assert bool((img[nbytes // 4:] == SENT).all()), "%r: the pack wrote behind its image" % c
    return img


def run_split(ops, case, flat, w, bias, rb=None):
    """The kernel under test on device operands -> [G,M,N]; nothing outside the G windows of the output buffer was written, and
    the launch had the workgroups of `rb` row blocks per tile (None: the cost model's choice) -- a forced VQA_GRU_GEMM_RB was
    honoured."""
    c, L = case, ops._lib.lib()
    assert ops.gemm_nt_split_batched_ok(c.M, c.N, c.K, c.lda, flat, w) and c.a_off % 4 == 0
    assert ops._lib.lib().vqa_gemm_nt_split_batched_supported(c.M, c.N, c.K, c.lda, c.ldc) == 1
    img = pack_image(ops, c, w)
    cbuf = torch.full((c.c_size(),), SENT, device=dev(), dtype=torch.float32)
    L.vqa_launch_log_reset()
    ops.gemm_nt_split_batched(flat, c.a_off, c.a_gs, c.lda, img, c.c_view(cbuf), bias, w, c.transposed, c.G, c.M, c.N, c.K,
                              c_gs=c.c_gs, ldc=c.ldc)
    log = (ctypes.c_ulonglong * 16)()
    assert L.vqa_launch_log(log, 16) == 1 and int(log[0]) == grid_of(c, rb)[3] * 256, (c, rb, int(log[0]), grid_of(c, rb))
    got = c.c_view(cbuf).clone()
    c.c_view(cbuf).fill_(SENT)
    untouched = _bits(cbuf) == _bits(torch.full((1,), SENT, device=dev()))
    assert bool(untouched.all()), "%r: %d stores outside the [M,N] windows, first at flat index %d" % (
        c, int((~untouched).sum()), int((~untouched).nonzero()[0]))
    return got


def run_twin(ops, case, flat, w, bias):
    """The same products on the fp32 MFMA engine: the K6 grouped kernel forced to fp32 MFMA, NT against W [N,K], NN against
    W [K,N], as GruSequence's fallback calls it.  That engine takes even extents only, so the operands are copied with one zero
    column / row appended where K or N is odd (an exact zero term; the spare output column is dropped); the bias is added in
    fp32 afterwards, one rounding as in the kernel's store."""
    from vqa_playground_pytorch_amd import head
    c = case
    Ke, Ne = c.K + c.K % 2, c.N + c.N % 2
    a = torch.zeros(c.G, c.M, Ke, device=dev())
    a[:, :, :c.K] = c.a_view(flat)
    if c.transposed:
        we = torch.zeros(c.G, Ke, Ne, device=dev())
        we[:, :c.K, :c.N] = w
        form, ldb = head.NN, Ne
    else:
        we = torch.zeros(c.G, Ne, Ke, device=dev())
        we[:, :c.N, :c.K] = w
        form, ldb = head.NT, Ke
    out = torch.empty(c.G, c.M, Ne, device=dev())
    ops._grouped_products("encoder_kernel_twin", [(form, a, g * c.M * Ke, Ke, we, g * Ke * Ne, ldb, c.M, Ne, Ke, out[g]) for g in range(c.G)],
                          engine="mfma")
    out = out[:, :, :c.N]
    return out + bias[:, None, :] if bias is not None else out.contiguous()


def reference64(case, flat, w, bias, device):
    """(a[:, :K].double() @ W.double().T + bias, sum_k |a_k||w_k| + |bias|) on `device`"""
    c = case
    a64 = c.a_view(flat).to(device).double()
    w64 = c.w_logical(w).to(device).double()
    ref, scale = a64 @ w64.transpose(1, 2), a64.abs() @ w64.abs().transpose(1, 2)
    if bias is not None:
        b64 = bias.to(device).double()
        ref, scale = ref + b64[:, None, :], scale + b64.abs()[:, None, :]
    return ref, scale


def compare(name, got_s, got_m, ref64, scale64, finite_everywhere):
    """tests/test_gpu_split.py::_compare_with_engine restated, returning what it measured: non-finite outputs have the same
    class on both engines; -> (max, rms of the split engine's error / sum|a||w| over the finite outputs, the fp32 MFMA engine's
    rms, number of non-finite outputs)."""
    cs, cm = _classes(got_s), _classes(got_m)
    if not torch.equal(cs, cm):
        first = tuple((cs != cm).nonzero()[0].tolist())
        raise AssertionError("%s: %d outputs differ in class (finite / +Inf / -Inf / NaN) between the engines; first at %s: split %s, "
                             "mfma %s" % (name, int((cs != cm).sum()), first, got_s[first].item(), got_m[first].item()))
    fin = (cm == 0) & torch.isfinite(ref64) & torch.isfinite(scale64)
    if finite_everywhere:
        assert bool((cm == 0).all()), "%s: the fp32 MFMA engine itself is not finite here -- the case is mis-built" % name
    unit = scale64.clamp_min(1e-300)
    es = ((got_s.double() - ref64).abs() / unit)[fin]
    em = ((got_m.double() - ref64).abs() / unit)[fin]
    rs, rm = es.pow(2).mean().sqrt().item(), em.pow(2).mean().sqrt().item()
    print("[%s] finite outputs %d of %d; error / sum|a||w|: split max %.2e rms %.2e, mfma max %.2e rms %.2e"
          % (name, int(fin.sum()), fin.numel(), es.max().item(), rs, em.max().item(), rm))
    return es.max().item(), rs, rm, int((cm != 0).sum())


class Worst:
    """the worst of each figure over the cases of one test"""

    def __init__(self):
        self.mx, self.ratio, self.rs, self.rm = (0.0, ""), (0.0, ""), 0.0, 0.0

    def add(self, name, mx, rs, rm):
        if mx >= self.mx[0]:
            self.mx = (mx, name)
        ratio = rs / (RMS_FACTOR * rm + 1e-9)
        if ratio >= self.ratio[0]:
            self.ratio, self.rs, self.rm = (ratio, name), rs, rm

    def report(self, measured, tag):
        measured("%s max err/sum|a||w|" % tag, self.mx[0], MAX_BAR, self.mx[1])
        measured("%s rms (bar 2x mfma's)" % tag, self.rs, RMS_FACTOR * self.rm + 1e-9, self.ratio[1])


def check_against_float64(ops, case, gen, worst, ref_device="cpu", tag="", rb=None):
    c = case
    flat, w, bias = draw_operands(c, gen)
    ref, scale = reference64(c, flat, w, bias, ref_device)
    assert bool(torch.isfinite(ref).all())
    flat, w, bias = flat.to(dev()), _dev(w), _dev(bias)
    got_s = run_split(ops, c, flat, w, bias, rb)
    got_m = run_twin(ops, c, flat, w, bias)
    mx, rs, rm, _ = compare("%r%s" % (c, tag), got_s.to(ref.device), got_m.to(ref.device), ref, scale, True)
    worst.add("%r%s" % (c, tag), mx, rs, rm)
    assert mx <= MAX_BAR, (c, tag, mx)
    assert rs <= RMS_FACTOR * rm + 1e-9, (c, tag, rs, rm)
    return got_s


# M around every tile edge (16 x 7 = 112, 16 x 9 = 144 rows per workgroup), the minimum, and where the row-block choice changes
M_EDGES = [Case(3, M, 176, 128, lda=132, ldc=180, c_gs=M * 180 + 20, bias=(M % 2 == 1)) for M in (64, 65, 111, 112, 113, 143, 144, 145)]
M_EDGES += [Case(3, 64, 176, 128, transposed=True), Case(3, 145, 161, 96, transposed=True, wpad=4, ldc=164)]
M_LARGE = [Case(7, 1024, 620, 64), Case(1, 1024, 160, 64), Case(1, 1025, 160, 64, bias=True), Case(3, 1024, 161, 64, transposed=True), Case(3, 1025, 176, 96, lda=100)]
N_EDGES = [Case(G, 130, N, 96, bias=b, transposed=t, ldc=N + 5)
           for N, G, b, t in ((16, 1, True, False), (17, 3, False, False), (159, 7, True, False), (160, 3, False, True), (161, 1, True, True),
                              (176, 7, False, False), (620, 3, True, False), (17, 7, True, True), (159, 1, False, True))]
K_EDGES = [Case(3, 130, 176, 64), Case(1, 130, 176, 64, transposed=True, bias=True), Case(3, 130, 176, 65, lda=68), Case(3, 130, 176, 65, lda=68, transposed=True),
           Case(3, 130, 176, 67, lda=68, bias=True), Case(7, 70, 33, 67, lda=68, transposed=True, wpad=1), Case(3, 130, 176, 96, lda=128),
           Case(1, 130, 176, 128, lda=256, wpad=8), Case(3, 130, 176, 620), Case(3, 130, 17, 620, lda=624, transposed=True, bias=True)]
LAYOUTS = [Case(3, 130, 176, 100, lda=104, a_gs=0), Case(7, 65, 176, 128, a_gs=0, transposed=True, bias=True),          # one shared A
           Case(3, 130, 176, 100, lda=3 * 104, a_gs=104, bias=True),                                                   # interleaved A ([B,G,K])
           Case(3, 130, 100, 176, c_gs=100, ldc=300, c_off=0, transposed=True),                                        # interleaved C ([B,G,K])
           Case(1, 64, 16, 64, a_off=0, c_off=0), Case(7, 64, 16, 64, ldc=16, c_gs=64 * 16 + 1, a_gs=64 * 64)]
SMALL = M_EDGES + M_LARGE + N_EDGES + K_EDGES + LAYOUTS


def test_the_small_shape_table_covers_what_it_claims():
    """(no GPU needed) the table holds every edge it is meant to: grids that are and are not a multiple of 8, all three
    row-block choices, both tile orders, K % 4 != 0, lda > K, a shared A, K = 64, all G."""
    grids = [grid_of(c) for c in SMALL]
    assert sum(1 for g in grids if g[3] % 8) >= 2 and sum(1 for g in grids if g[3] % 8 == 0) >= 1
    assert {g[0] for g in grids} == {7, 8, 9}
    assert any(g[1] <= 8 for g in grids) and any(g[1] > 8 for g in grids)          # col_major iff tiles_m <= 8
    assert {c.G for c in SMALL} == {1, 3, 7}
    assert {16, 17, 159, 160, 161, 176, 620} <= {c.N for c in SMALL} and {64, 65, 67, 96, 128, 620} <= {c.K for c in SMALL}
    assert {64, 65, 111, 112, 113, 143, 144, 145, 1024, 1025} <= {c.M for c in SMALL}
    assert any(c.K % 4 for c in SMALL) and any(c.lda > c.K for c in SMALL) and any(c.a_gs == 0 for c in SMALL)
    assert any(c.bias for c in SMALL) and any(not c.bias for c in SMALL) and any(c.transposed for c in SMALL)
    assert all(c.K <= 128 or c.M <= 130 for c in SMALL)


@gpu
def test_batched_nt_small_shapes_against_float64(ops, measured):
    """Every small case of the table with the kernel's own choice of row blocks and tile order."""
    worst = Worst()
    for i, c in enumerate(SMALL):
        check_against_float64(ops, c, torch.Generator().manual_seed(1000 + i), worst)
    worst.report(measured, "small shapes")


@gpu
@pytest.mark.parametrize("rb", [7, 8, 9])
def test_batched_nt_tile_edges_with_forced_row_blocks(ops, lib_option, measured, rb):
    """M around the tile edges and across the cost model's range with VQA_GRU_GEMM_RB forced: every row-block variant runs
    every ragged last row tile, not only the ones the cost model would hand it."""
    lib_option("VQA_GRU_GEMM_RB", rb)
    worst = Worst()
    for i, c in enumerate(M_EDGES + M_LARGE[3:] + K_EDGES[:3]):
        check_against_float64(ops, c, torch.Generator().manual_seed(2000 + i), worst, tag=" rb%d" % rb, rb=rb)
    worst.report(measured, "rb=%d" % rb)


def _production_cases():
    out = []
    for B in (100, 256, 512):       # the recurrent step as GruSequence passes it: slot t = 1 of a [3,T,B,H] history, T = 2
        for tr in (False, True):
            out.append(Case(3, B, 2400, 2400, a_off=B * 2400, a_gs=2 * B * 2400, c_off=0, transposed=tr))
    # the input projections as batched_linear passes them: x [B*T,3,620] interleaved, bias in the store; and their data gradient
    # against the transposed image, written into the consumer's [B*T,3,620] layout
    out.append(Case(3, 13312, 2400, 620, lda=3 * 620, a_gs=620, a_off=0, c_off=0, bias=True))
    out.append(Case(3, 13312, 620, 2400, a_off=0, a_gs=13312 * 2400, c_gs=620, ldc=1860, c_off=0, transposed=True))
    return out


@gpu
@pytest.mark.parametrize("case", _production_cases(), ids=repr)
def test_batched_nt_production_shapes_against_float64(ops, measured, case):
    """The shapes the encoder launches at the batch sizes the configs train with (config/CoR2.py 100, config/ODA.py 256,
    bench.py 512), both weight images.  The float64 products of these run on the GPU (torch's float64 matmul)."""
    worst = Worst()
    check_against_float64(ops, case, torch.Generator().manual_seed(case.M + case.N), worst, ref_device=dev())
    worst.report(measured, "production")


@gpu
def test_batched_nt_tile_order_does_not_change_a_bit(ops, lib_option):
    """VQA_GRU_GEMM_ORDER=c and =r: one workgroup owns an element and the chunk split depends only on Kp and the wave, so the
    order in which tiles are dealt out cannot change any element's arithmetic."""
    for i, c in enumerate((Case(3, 145, 176, 128, lda=132, bias=True), Case(3, 1025, 161, 64, transposed=True))):
        assert grid_of(c)[1] > 1 and grid_of(c)[2] > 1
        flat, w, bias = (_dev(t) for t in draw_operands(c, torch.Generator().manual_seed(3000 + i)))
        got = {}
        for order in ("c", "r"):
            lib_option("VQA_GRU_GEMM_ORDER", order)
            got[order] = run_split(ops, c, flat, w, bias)
        assert _same_bits(got["c"], got["r"]), (c, (got["c"] - got["r"]).abs().max().item())


@gpu
def test_batched_nt_row_block_variants_side_by_side(ops, lib_option, measured):
    """The row-block variants 7 / 8 / 9 on the same operands agree BIT FOR BIT: an element's chunk range depends only on Kp and
    its pair of waves, the load ring (which differs between the variants) decides when a chunk is loaded and not the order of
    the MFMAs into an accumulator, and the two halves are added the same way.  (Each variant is held to the float64 bars in
    test_batched_nt_tile_edges_with_forced_row_blocks as well.)"""
    for i, c in enumerate((Case(3, 145, 176, 128, lda=132, bias=True), Case(3, 130, 176, 620, transposed=True))):
        flat, w, bias = (_dev(t) for t in draw_operands(c, torch.Generator().manual_seed(3100 + i)))
        got = {}
        for rb in (7, 8, 9):
            lib_option("VQA_GRU_GEMM_RB", rb)
            got[rb] = run_split(ops, c, flat, w, bias, rb)
        for rb in (7, 8):
            differ = int((_bits(got[rb]) != _bits(got[9])).sum())
            measured("elements differing rb%d vs rb9" % rb, differ, 0, repr(c))
            assert differ == 0, (c, rb, differ, (got[rb] - got[9]).abs().max().item())


# ---- 2. the weight image is exact ----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("transposed", [False, True])
def test_weight_image_is_an_exact_split(ops, transposed):
    """A one-hot (A[m, m % K] = 1, K = 100 is not a multiple of 64, every k up to K - 1 is selected by some row) against weights
    with full 24-bit mantissas and magnitudes over 2^-20 .. 2^20: C[m, :] must equal W[:, m % K] BIT FOR BIT.  1.0 splits into
    (1, 0, 0); the three planes of w sum to w exactly and every partial sum of them is representable in fp32, in any order; all
    other terms are exact zeros.  A dropped plane, a swapped k, a wrong ldw / w_gs or a transposed-index slip fails by many ulp."""
    c = Case(2, 128, 176, 100, ldc=180, transposed=transposed, wpad=4)
    gen = torch.Generator().manual_seed(41 + transposed)
    rows, cols = (c.K, c.N) if transposed else (c.N, c.K)
    shape = (c.G, rows, cols + c.wpad)
    mant = 1.0 + torch.randint(0, 1 << 23, shape, generator=gen).double() / (1 << 23)
    sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
    w = (sign * mant * torch.exp2(torch.randint(-20, 20, shape, generator=gen).double())).float()[:, :, :cols]
    assert bool((w.abs() >= 2.0 ** -20).all()) and bool((w.abs() < 2.0 ** 20).all())
    assert bool(((_bits(w) & 0xFF) != 0).float().mean() > 0.9)         # the low mantissa byte (the third plane) is in use
    flat = torch.zeros(c.a_size())
    a = c.a_view(flat)
    for g in range(c.G):
        a[g, torch.arange(c.M), torch.arange(c.M) % c.K] = 1.0
    got = run_split(ops, c, flat.to(dev()), _dev(w), None).cpu()
    # ops.split_weights (contiguous rows, another ldw) builds the same image
    L = ops._lib.lib()
    words = L.vqa_split_weights_bytes(c.G, c.N, c.K) // 4
    assert _same_bits(ops.split_weights(w.contiguous().to(dev()), transposed)[:words], pack_image(ops, c, _dev(w))[:words])
    want = c.w_logical(w)[:, :, torch.arange(c.M) % c.K].transpose(1, 2)          # [G,M,N]: W_g[:, m % K]
    assert not torch.equal(want[0], want[1])
    diff = _bits(got) != _bits(want)
    assert not bool(diff.any()), "%d of %d elements differ, first at (g, m, n) = %s: got %r, W holds %r" % (
        int(diff.sum()), diff.numel(), diff.nonzero()[0].tolist(), got[tuple(diff.nonzero()[0])].item(), want[tuple(diff.nonzero()[0])].item())


@gpu
@pytest.mark.parametrize("transposed", [False, True])
def test_small_integer_products_are_exact(ops, transposed):
    """Integer operands with |values| <= 8 over K = 128 (and an integer bias): every product, partial sum and plane is exact in
    fp32, so the result equals the float64 one cast to float32 bit for bit."""
    c = Case(3, 130, 176, 128, lda=132, ldc=180, bias=True, transposed=transposed)
    flat, w, bias = draw_operands(c, torch.Generator().manual_seed(43 + transposed), ints=True)
    ref, _ = reference64(c, flat, w, bias, "cpu")
    got = run_split(ops, c, flat.to(dev()), _dev(w), _dev(bias)).cpu()
    assert float(ref.abs().max()) > 100 and torch.equal(got.double(), ref)
    assert _same_bits(got, (ref + 0.0).float())


# ---- 3. edge values ------------------------------------------------------------------------------------------------------------
def _edge_case(transposed, interleaved=False):
    if interleaved:
        return Case(3, 130, 176, 100, lda=3 * 104, a_gs=104, ldc=180, transposed=transposed)
    return Case(3, 130, 176, 100, lda=104, ldc=180, transposed=transposed)


def _explicit_reference64(case, flat, w):
    """The products summed term by term in float64, no BLAS: the class (finite / +Inf / -Inf / NaN) of every output is what
    IEEE arithmetic gives (an Inf times an exact zero is NaN, Inf - Inf is NaN), whatever a GEMM library does with such terms."""
    a64, w64 = case.a_view(flat).double(), case.w_logical(w).double()
    ref = (a64[:, :, None, :] * w64[:, None, :, :]).sum(-1)
    scale = (a64[:, :, None, :].abs() * w64[:, None, :, :].abs()).sum(-1)
    return ref, scale


def _poison(n, i0=0):
    return torch.tensor([(INF, -INF, NAN)[(i0 + i) % 3] for i in range(n)])


def _run_edge(ops, c, flat, w):
    ref, scale = _explicit_reference64(c, flat, w)
    flat, w = flat.to(dev()), _dev(w)
    return run_split(ops, c, flat, w, None).cpu(), run_twin(ops, c, flat, w, None).cpu(), ref, scale


@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("kind", ["flt_max", "spread"])
def test_batched_nt_edge_values_finite(ops, measured, kind, transposed):
    """Operands next to FLT_MAX (their leading bf16 plane rounds to Inf: the repair path recomputes those outputs) and with
    exponents spread over 2^-40 .. 2^40: finite everywhere in float64, so the bars of the shape table hold."""
    c = _edge_case(transposed)
    gen = torch.Generator().manual_seed(51 + transposed)
    flat, w, _ = draw_operands(c, gen)
    a, wl = c.a_view(flat), c.w_logical(w)
    fmax = torch.finfo(torch.float32).max
    if kind == "flt_max":
        for i, (g, m, k) in enumerate([(0, 0, 0), (0, 5, 17), (1, 111, 99), (1, 112, 31), (2, 129, 64), (2, 129, 99), (2, 64, 96)]):
            a[g, m, k] = fmax * (1.0 if i % 2 == 0 else -1.0) * (1.0 - 2.0 ** -(9 + i))
            wl[g, :, k] *= 2.0 ** -30
        for g, n, k in [(0, 3, 40), (2, 175, 98)]:
            wl[g, n, k] = -fmax * (1.0 - 2.0 ** -12)
            a[g, :, k] *= 2.0 ** -40
    else:
        a *= torch.exp2(torch.randint(-40, 41, a.shape, generator=gen).float())
        wl *= torch.exp2(torch.randint(-40, 41, wl.shape, generator=gen).float())
    got_s, got_m, ref, scale = _run_edge(ops, c, flat, w)
    assert bool(torch.isfinite(ref).all())
    mx, rs, rm, _ = compare("%s %r" % (kind, c), got_s, got_m, ref, scale, True)
    measured("%s max err/sum|a||w|" % kind, mx, MAX_BAR)
    measured("%s rms (bar 2x mfma's)" % kind, rs, RMS_FACTOR * rm + 1e-9)
    assert bool(torch.isfinite(got_s).all())
    assert mx <= MAX_BAR and rs <= RMS_FACTOR * rm + 1e-9, (mx, rs, rm)
    if kind == "flt_max":
        assert float(got_s.abs().max()) > 1e7          # the large operands did take part


@gpu
@pytest.mark.parametrize("transposed", [False, True])
def test_batched_nt_edge_values_nonfinite(ops, measured, transposed):
    """+-Inf / NaN at real positions of A and W: every output has the class (finite / +Inf / -Inf / NaN) of the float64
    reference cast to float32 AND of the fp32 MFMA engine; the finite ones meet the bars.  The repair path re-reads the fp32
    weights through strides that differ between the two images."""
    c = _edge_case(transposed)
    flat, w, _ = draw_operands(c, torch.Generator().manual_seed(53 + transposed))
    a, wl = c.a_view(flat), c.w_logical(w)
    a[0, 1, 3], a[0, 120, 99], a[1, 121, 99], a[1, 64, 0], a[2, 129, 99] = INF, -INF, NAN, INF, NAN
    a[2, 70, 10], a[2, 70, 11] = INF, -INF          # Inf - Inf in one row
    wl[0, 5, 9], wl[1, 170, 50], wl[2, 17, 99], wl[2, 175, 0] = INF, NAN, -INF, INF
    wl[0, 40, 3] = 0.0                               # a[0, 1, 3] = Inf meets an exact zero: NaN on any engine
    got_s, got_m, ref, scale = _run_edge(ops, c, flat, w)
    mx, rs, rm, n_bad = compare("nonfinite %r" % c, got_s, got_m, ref, scale, False)
    want = _classes(ref.float())
    assert torch.equal(_classes(got_s), want), "%d outputs differ in class from float64; first at %s" % (
        int((_classes(got_s) != want).sum()), (_classes(got_s) != want).nonzero()[0].tolist())
    assert n_bad > 0 and 0 < int((want != 0).sum()) < want.numel() // 4          # the case reaches the outputs, and not all of them
    measured("nonfinite max err/sum|a||w|", mx, MAX_BAR)
    measured("nonfinite rms (bar 2x mfma's)", rs, RMS_FACTOR * rm + 1e-9)
    assert mx <= MAX_BAR and rs <= RMS_FACTOR * rm + 1e-9, (mx, rs, rm)


@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("interleaved", [False, True])
def test_batched_nt_nonfinite_neighbour(ops, measured, interleaved, transposed):
    """+-Inf / NaN ONLY where a padded load can reach but the product must not: the contraction is padded 100 -> 128, so row m's
    loads run over the lda - K gap columns into what follows.  Every float of the A storage that is no operand element is
    poisoned -- the gap columns of every row, the floats between the problems (behind the last row of each), the floats in front
    of the first and behind the last problem (inside the allocation).  The float64 reference does not see them, so it is finite
    everywhere, and so must EVERY output be, at the bars of the shape table: a non-finite accumulator has to be recomputed over
    the real contraction.  (What a row reaches: rows 0 .. M - 2 of a problem read their gap columns and the 24 floats behind
    them through the repair path's trigger; the LAST row's padded loads fall behind the extent the kernel hands the buffer
    descriptor, ((M - 1) lda + K) floats, and return zeros -- the poison behind each problem's last row pins that range check.)
    (The first values of row m + 1 -- and, when problems interleave, of the next problem's row -- are real operand elements: an
    Inf there makes that row's own outputs non-finite by right.  That half of the case, the row in front staying clean, is
    test_batched_nt_nonfinite_next_row.)"""
    c = _edge_case(transposed, interleaved)
    flat, w, _ = draw_operands(c, torch.Generator().manual_seed(55 + transposed + 2 * interleaved))
    real = torch.zeros(c.a_size(), dtype=torch.bool)
    c.a_view(real).fill_(True)
    assert int(real.sum()) == c.G * c.M * c.K and int((~real).sum()) >= c.G * c.M * 4
    flat[~real] = _poison(int((~real).sum()))
    assert bool(torch.isfinite(c.a_view(flat)).all()) and not bool(torch.isfinite(flat[c.a_off + c.K:c.a_off + c.K + 4]).any())
    got_s, got_m, ref, scale = _run_edge(ops, c, flat, w)
    assert bool(torch.isfinite(ref).all())
    assert bool(torch.isfinite(got_s).all()), "%d outputs are not finite; first at (g, m, n) = %s" % (
        int((~torch.isfinite(got_s)).sum()), (~torch.isfinite(got_s)).nonzero()[0].tolist())
    mx, rs, rm, n_bad = compare("neighbour %r" % c, got_s, got_m, ref, scale, True)
    measured("neighbour max err/sum|a||w|", mx, MAX_BAR)
    measured("neighbour rms (bar 2x mfma's)", rs, RMS_FACTOR * rm + 1e-9)
    assert n_bad == 0 and mx <= MAX_BAR and rs <= RMS_FACTOR * rm + 1e-9, (mx, rs, rm)


@gpu
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("interleaved", [False, True])
def test_batched_nt_nonfinite_next_row(ops, measured, interleaved, transposed):
    """+-Inf / NaN in the first values of a few rows (the contraction is padded by Kp - K = 28, of which lda - K = 4 fall into
    the gap and 24 into what follows): the padded loads of the row in front (the same row of the
    problem in front, when problems interleave) pick them up against zero planes.  The rows that own such a value are non-finite
    by right -- the class of every output equals float64's and the fp32 MFMA engine's -- and every other row, the neighbours
    included, is finite and meets the bars.  (Owners in row 0 of problems 1 and 2: when the problems do not interleave, the
    row in front of them is the last row of the problem before, whose padded loads end at its own extent -- the range check, not
    the repair path, keeps those out.)"""
    c = _edge_case(transposed, interleaved)
    flat, w, _ = draw_operands(c, torch.Generator().manual_seed(57 + transposed + 2 * interleaved))
    a = c.a_view(flat)
    owners = [(0, 1, 0), (0, 17, 5), (1, 64, 23), (1, 112, 1), (2, 129, 2), (2, 113, 20), (1, 0, 0), (2, 0, 3)]
    for i, (g, m, k) in enumerate(owners):
        a[g, m, k] = (INF, -INF, NAN)[i % 3]
    got_s, got_m, ref, scale = _run_edge(ops, c, flat, w)
    mx, rs, rm, n_bad = compare("next row %r" % c, got_s, got_m, ref, scale, False)
    want = _classes(ref.float())
    assert torch.equal(_classes(got_s), want), "first difference from float64's classes at %s" % (_classes(got_s) != want).nonzero()[0].tolist()
    bad_rows = {(g, m) for g, m in (~torch.isfinite(got_s)).any(2).nonzero().tolist()}
    assert bad_rows == {(g, m) for g, m, _ in owners}, sorted(bad_rows)
    measured("next row max err/sum|a||w|", mx, MAX_BAR)
    measured("next row rms (bar 2x mfma's)", rs, RMS_FACTOR * rm + 1e-9)
    assert n_bad == len(owners) * c.N and mx <= MAX_BAR and rs <= RMS_FACTOR * rm + 1e-9, (n_bad, mx, rs, rm)


# ---- 4. the gate kernels -------------------------------------------------------------------------------------------------------
def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def gates_fwd_ref(gi_t, a, hp, masks, af):
    """csrc/gru.hip's forward formulas in the dtype of the operands (gi_t = gi[:, :, t]) -> h', [hm_r, hm_i, hm_n], r, i, n, a_n"""
    r = _sig(gi_t[0] + a[0])
    i = _sig(gi_t[1] + a[1])
    z = gi_t[2] + r * a[2]
    n = torch.relu(z) if af == 1 else torch.tanh(z)
    hn = (1.0 - i) * n + i * hp
    return {"h_new": hn, "hm": torch.stack([hn * masks[g] if masks is not None else hn for g in range(3)]),
            "r": r, "i": i, "n": n, "a_n": a[2].clone()}


def gates_bwd_ref(d_out, carry, dhm, masks, r, i, n, an, hp, af):
    """csrc/gru.hip's backward formulas -> gz [dzr, dzi, dan], d_gi [dzr, dzi, dzn], carry_out"""
    dh = d_out.clone() if d_out is not None else torch.zeros_like(r)
    if carry is not None:
        dh = dh + carry
    if dhm is not None:
        for g in range(3):
            dh = dh + (dhm[g] * masks[g] if masks is not None else dhm[g])
    grad = (n > 0).to(n.dtype) if af == 1 else 1.0 - n * n
    dn = dh * (1.0 - i) * grad
    dzr = dn * an * r * (1.0 - r)
    dzi = dh * (hp - n) * i * (1.0 - i)
    return {"gz": torch.stack([dzr, dzi, dn * r]), "d_gi": torch.stack([dzr, dzi, dn]), "carry_out": dh * i}


def _both(fn, args):
    """fn on the float32 operands in float64 and in float32 (torch on the CPU)"""
    cast = lambda x, dt: x.to(dt) if isinstance(x, torch.Tensor) else x      # noqa: E731
    return fn(*[cast(x, torch.float64) for x in args]), fn(*[cast(x, torch.float32) for x in args])


class GateBars:
    """kernel error against float64, relative to the tensor's largest magnitude; bar: four times the error of the same formulas
    in float32 with torch on the CPU, plus one float32 ulp of that magnitude"""

    def __init__(self):
        self.worst = (-1.0, 0.0, 0.0, "")

    def check(self, name, got, ref64, ref32):
        got = got.cpu()
        assert got.shape == ref64.shape, (name, got.shape, ref64.shape)
        assert bool(torch.isfinite(got).all()), name
        mag = float(ref64.abs().max())
        if mag == 0.0:
            assert not bool(got.any()), name
            return
        err = float((got.double() - ref64).abs().max()) / mag
        e32 = float((ref32.double() - ref64).abs().max()) / mag
        bar = 4.0 * e32 + EPS32
        print("[%s] kernel %.3e  float32 torch %.3e  bar %.3e" % (name, err, e32, bar))
        if err / bar > self.worst[0]:
            self.worst = (err / bar, err, bar, name)
        assert err <= bar, (name, err, e32, bar)

    def report(self, measured, tag):
        measured("%s err / max|ref|" % tag, self.worst[1], self.worst[2], self.worst[3])


def _steps(T):
    return sorted({0, T // 2, T - 1})


GATE_SHAPES = [(1, 1, 4), (3, 5, 20), (7, 4, 324), (100, 26, 2400)]
HIST_PAD = 8           # floats between the groups of a history beyond T*B*H: hist_group_stride is its own argument


def run_gates_fwd(ops, gi, a, hp, masks, B, T, H, t, af, with_next):
    """vqa_gru_gates_fwd on sentinel-filled [T,...] buffers the way ops.GruSequence passes them -> the outputs of slot t;
    asserts that nothing but slot t (and slot t + 1 of the history's three groups) was written."""
    L = ops._lib.lib()
    BH, gs = B * H, T * B * H + HIST_PAD
    out, saved, hist = _sentinel(T, B, H), _sentinel(4, T, B, H), _sentinel(3, gs)
    d = lambda x: x.to(dev()).contiguous() if x is not None else None      # noqa: E731
    gi_d, a_d, hp_d, m_d = d(gi), d(a), d(hp), d(masks)
    ops._launch("gru_gates_fwd", (B, T, H), L.vqa_gru_gates_fwd, _ptr(gi_d), _ptr(a_d), _ptr(hp_d), _ptr(m_d) if m_d is not None else None,
                _ptr(out[t]), _ptr(hist, (t + 1) * BH) if with_next else None, gs, _ptr(saved[0, t]), _ptr(saved[1, t]), _ptr(saved[2, t]),
                _ptr(saved[3, t]), B, T, H, t, af)
    torch.cuda.synchronize()
    got = {"h_new": out[t].clone(), "r": saved[0, t].clone(), "i": saved[1, t].clone(), "n": saved[2, t].clone(), "a_n": saved[3, t].clone()}
    out[t].fill_(SENT)
    saved[:, t].fill_(SENT)
    if with_next:
        slot = hist[:, (t + 1) * BH:(t + 2) * BH]
        got["hm"] = slot.reshape(3, B, H).clone()
        slot.fill_(SENT)
    assert _untouched(out), "h' went to another slot than t = %d" % t
    assert _untouched(saved), "r / i / n / a_n went to another slot than t = %d" % t
    assert _untouched(hist), "a masked copy went outside slot t + 1 = %d of the history (null hm_next: %s)" % (t + 1, not with_next)
    return got


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "B%dT%dH%d" % s)
def test_gru_gates_fwd_against_float64(ops, measured, shape, af, with_masks):
    """h', the three masked copies, r, i, n, a_n at t = 0, mid, T - 1 (hm_next null at the last step and, once, earlier)."""
    B, T, H = shape
    gen = torch.Generator().manual_seed(61 + B + af)
    gi, a, hp = torch.randn(3, B, T, H, generator=gen), torch.randn(3, B, H, generator=gen), torch.randn(B, H, generator=gen)
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    bars = GateBars()
    for t in _steps(T):
        for with_next in ([True, False] if (t == 0 and T > 1) else [t + 1 < T]):
            ref64, ref32 = _both(gates_fwd_ref, (gi[:, :, t], a, hp, masks, af))
            got = run_gates_fwd(ops, gi, a, hp, masks, B, T, H, t, af, with_next)
            for k in got:
                bars.check("fwd %s t=%d" % (k, t), got[k], ref64[k], ref32[k])
            assert _same_bits(got["a_n"].cpu(), a[2])
            if with_next and masks is not None:          # a dropped unit is an exact zero, a kept one h' * (1 / 0.75) in fp32
                assert torch.equal(got["hm"].cpu(), got["h_new"].cpu()[None] * masks)
            elif with_next:
                assert all(_same_bits(got["hm"][g], got["h_new"]) for g in range(3))
    bars.report(measured, "gates fwd")


def run_gates_bwd(ops, d_out, carry, dhm, masks, r, i, n, an, hp, B, T, H, t, af):
    L = ops._lib.lib()
    BH, gs = B * H, T * B * H + HIST_PAD
    gz, d_gi, co = _sentinel(3, gs), _sentinel(3, B, T, H), _sentinel(B, H)
    d = lambda x: x.to(dev()).contiguous() if x is not None else None      # noqa: E731
    ins = [d(x) for x in (d_out, carry, dhm, masks, r, i, n, an, hp)]
    ops._launch("gru_gates_bwd", (B, T, H), L.vqa_gru_gates_bwd, *[_ptr(x) if x is not None else None for x in ins], _ptr(gz, t * BH), gs,
                _ptr(d_gi), _ptr(co), B, T, H, t, af)
    torch.cuda.synchronize()
    slot = gz[:, t * BH:(t + 1) * BH]
    got = {"gz": slot.reshape(3, B, H).clone(), "d_gi": d_gi[:, :, t].clone(), "carry_out": co.clone()}
    slot.fill_(SENT)
    d_gi[:, :, t].fill_(SENT)
    assert _untouched(gz), "gz went outside slot t = %d of its history" % t
    assert _untouched(d_gi), "d_gi went to another step than t = %d" % t
    return got


@gpu
@pytest.mark.parametrize("with_masks,last", [(True, False), (False, False), (True, True)], ids=["masks-carry", "nomasks-carry", "nullcarry"])
@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "B%dT%dH%d" % s)
def test_gru_gates_bwd_against_float64(ops, measured, shape, af, with_masks, last):
    """gz (third group: dan), d_gi (third group: dzn), carry_out at t = 0, mid, T - 1; carry_in / dhm null (the last step's
    call: the kernel reads the masks only next to dhm, so that case runs once, masks given as GruSequence gives them) or given."""
    B, T, H = shape
    gen = torch.Generator().manual_seed(71 + B + af)
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    r, i, an, hp, d_out = torch.sigmoid(rn(B, H)), torch.sigmoid(rn(B, H)), rn(B, H), rn(B, H), rn(B, H)
    n = torch.relu(rn(B, H)) if af == 1 else torch.tanh(rn(B, H))
    carry, dhm = (None, None) if last else (rn(B, H), rn(3, B, H))
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    bars = GateBars()
    ref64, ref32 = _both(gates_bwd_ref, (d_out, carry, dhm, masks, r, i, n, an, hp, af))
    for t in _steps(T):
        got = run_gates_bwd(ops, d_out, carry, dhm, masks, r, i, n, an, hp, B, T, H, t, af)
        for k in got:
            bars.check("bwd %s t=%d" % (k, t), got[k], ref64[k], ref32[k])
        assert _same_bits(got["gz"][:2], got["d_gi"][:2])          # dzr, dzi are written twice
    if not last:       # d_out null as well: dh = carry + sum_g dhm[g] * m_g
        ref64, ref32 = _both(gates_bwd_ref, (None, carry, dhm, masks, r, i, n, an, hp, af))
        got = run_gates_bwd(ops, None, carry, dhm, masks, r, i, n, an, hp, B, T, H, T - 1, af)
        for k in got:
            bars.check("bwd %s (no d_out)" % k, got[k], ref64[k], ref32[k])
    bars.report(measured, "gates bwd")


@gpu
@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
def test_gru_gates_saturated(ops, measured, af):
    """Pre-activations of +-30 and +-1e4: r and i are exactly 0 or 1 wherever float64 rounds to that in float32, every output is
    finite, and a gradient is exactly 0 where the float64 one rounds to 0 in float32."""
    B, T, H, t = 7, 4, 324, 1
    gen = torch.Generator().manual_seed(81 + af)
    pick = lambda *s: torch.tensor([30.0, -30.0, 1e4, -1e4])[torch.randint(0, 4, s, generator=gen)]      # noqa: E731
    gi = torch.randn(3, B, T, H, generator=gen)
    a = torch.randn(3, B, H, generator=gen)
    gi[:, :, t] = pick(3, B, H) - a                  # the sums the kernel forms are +-30 / +-1e4 up to one rounding
    gi[2, :, t] = pick(B, H)                         # (n's pre-activation is gi_n + r * a_n: r is 0 or 1, a_n of order 1)
    hp = torch.randn(B, H, generator=gen)
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75
    bars = GateBars()
    ref64, ref32 = _both(gates_fwd_ref, (gi[:, :, t], a, hp, masks, af))
    got = run_gates_fwd(ops, gi, a, hp, masks, B, T, H, t, af, True)
    for k in got:
        bars.check("saturated fwd %s" % k, got[k], ref64[k], ref32[k])
    for k in ("r", "i"):
        want = ref64[k].float()
        exact = (want == 0) | (want == 1)
        assert float(exact.float().mean()) > 0.6 and torch.equal(got[k].cpu()[exact], want[exact]), k
        assert bool(((got[k].cpu() >= 0) & (got[k].cpu() <= 1)).all())
    # backward on the kernel's own saved values (r, i in {0, 1, 9.4e-14}; n = +-1 under tanh, 0 or large under relu)
    r, i, n, an = (got[k].cpu() for k in ("r", "i", "n", "a_n"))
    d_out, carry, dhm = torch.randn(B, H, generator=gen), torch.randn(B, H, generator=gen), torch.randn(3, B, H, generator=gen)
    ref64, ref32 = _both(gates_bwd_ref, (d_out, carry, dhm, masks, r, i, n, an, hp, af))
    gotb = run_gates_bwd(ops, d_out, carry, dhm, masks, r, i, n, an, hp, B, T, H, t, af)
    for k in gotb:
        bars.check("saturated bwd %s" % k, gotb[k], ref64[k], ref32[k])
        zero = ref64[k].float() == 0
        assert int(zero.sum()) > 0 and not bool(gotb[k].cpu()[zero].any()), k
    bars.report(measured, "gates saturated")


def test_encoder_kernels_refuse_what_they_cannot_run():
    """(no GPU needed: every check precedes the launch, so aligned non-null addresses that are never dereferenced suffice)"""
    from vqa_playground_pytorch_amd import _lib
    L = _lib.lib()
    p, odd = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    L.vqa_launch_log_reset()

    def fwd(B=2, T=3, H=8, t=1, af=1, gi=p, h_new=p):
        return L.vqa_gru_gates_fwd(gi, p, p, None, h_new, None, T * B * H, p, p, p, p, B, T, H, t, af, None)

    def bwd(B=2, T=3, H=8, t=1, af=3, r_s=p, carry_out=p):
        return L.vqa_gru_gates_bwd(None, None, None, None, r_s, p, p, p, p, p, T * B * H, p, carry_out, B, T, H, t, af, None)

    for call in (fwd, bwd):
        assert call(H=6) == E_UNSUPPORTED and b"H % 4" in L.vqa_last_error()
        assert call(af=2) == E_BADARG and call(af=0) == E_BADARG
        assert call(t=3) == E_BADARG and call(t=-1) == E_BADARG
        assert call(B=0) == E_BADARG and call(T=0) == E_BADARG and call(H=0) == E_BADARG
    assert fwd(gi=None) == E_BADARG and fwd(h_new=None) == E_BADARG and b"null pointer" in L.vqa_last_error()
    assert bwd(r_s=None) == E_BADARG and bwd(carry_out=None) == E_BADARG and b"null pointer" in L.vqa_last_error()

    ok = L.vqa_gemm_nt_split_batched_supported
    assert ok(64, 16, 64, 64, 16) == 1
    assert ok(63, 16, 64, 64, 16) == 0 and ok(64, 15, 64, 64, 15) == 0 and ok(64, 16, 63, 64, 16) == 0
    assert ok(64, 16, 64, 66, 16) == 0 and ok(64, 16, 64, 68, 16) == 1          # lda % 4
    assert ok(64, 16, 128, 124, 16) == 0 and ok(64, 16, 128, 128, 16) == 1      # lda >= K
    assert ok(64, 16, 64, 64, 15) == 0 and ok(64, 17, 64, 64, 17) == 1          # ldc >= N

    def gemm(a=p, a_gs=64 * 64, G=1, image=p, c=p, M=64):
        return L.vqa_gemm_nt_split_batched(a, a_gs, 64, image, c, M * 16, 16, None, 0, p, 16 * 64, 64, 1, G, M, 16, 64, None)

    assert gemm(G=0) == E_BADARG and gemm(G=4097) == E_BADARG and b"G out of range" in L.vqa_last_error()
    assert gemm(a=None) == E_BADARG and gemm(image=None) == E_BADARG and gemm(c=None) == E_BADARG
    assert gemm(M=63) == E_UNSUPPORTED
    assert gemm(a=odd) == E_UNSUPPORTED and b"16-byte aligned" in L.vqa_last_error()
    assert gemm(a_gs=6) == E_UNSUPPORTED and gemm(image=odd) == E_UNSUPPORTED

    nbytes = L.vqa_split_weights_bytes(2, 176, 100)
    assert nbytes == 2 * L.vqa_split_weights_bytes(1, 176, 100) and nbytes >= 2 * 3 * 176 * 128 * 2      # three bf16 planes, K padded to 128
    assert L.vqa_split_weights_pack(p, 176 * 100, 100, 0, p, nbytes - 1, 2, 176, 100, None) == E_BADARG
    assert L.vqa_split_weights_pack(p, 176 * 100, 100, 0, ctypes.c_void_p(0x10008), nbytes, 2, 176, 100, None) == E_BADARG
    assert L.vqa_split_weights_pack(None, 176 * 100, 100, 0, p, nbytes, 2, 176, 100, None) == E_BADARG
    assert L.vqa_split_weights_pack(p, 176 * 100, 100, 0, p, nbytes, 0, 176, 100, None) == E_BADARG
    assert L.vqa_launch_log((ctypes.c_ulonglong * 16)(), 16) == 0, "a refused call launched a kernel"


# ---- 5. the sequence at the configs' batch sizes -------------------------------------------------------------------------------
def _sequence_case(ops, monkeypatch, measured, B, T, K, H, af, train, tag):
    """BayesianGRU's GPU form against the step-by-step CPU form in float64 -- y, all hidden states, d_x, every parameter
    gradient -- with the same masks and lengths; per tensor the bar is max(2e-5, 4 x e32), e32 being the error of the float32
    CPU step-by-step form against the float64 one.  -> the names of the launches and the shapes of the torch.bmm calls seen."""
    torch.manual_seed(5 + B)
    c64 = BayesianGRU(K, H, dropout=0.25, af=af).double()
    c32, g32 = BayesianGRU(K, H, dropout=0.25, af=af), BayesianGRU(K, H, dropout=0.25, af=af)
    state = {k: v.float() for k, v in c64.state_dict().items()}
    c32.load_state_dict(state)
    g32.load_state_dict(state)
    g32.to(dev())
    gen = torch.Generator().manual_seed(12 + B)
    masks = [(torch.rand(B, 1, K, generator=gen) > 0.25).float() / 0.75 for _ in range(3)] + \
            [(torch.rand(B, H, generator=gen) > 0.25).float() / 0.75 for _ in range(3)]
    for m, device, dt in ((c64, "cpu", torch.float64), (c32, "cpu", torch.float32), (g32, dev(), torch.float32)):
        m.train(train)
        if train:
            queue = [t.to(device=device, dtype=dt) for t in masks]
            m._mask = lambda like, q=queue: q.pop(0)
    x = torch.randn(B, T, K, generator=gen)
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    gy = torch.randn(B, H, generator=gen)
    x64, x32, xg = x.double().requires_grad_(), x.clone().requires_grad_(), x.clone().to(dev()).requires_grad_()
    bmms, bmm = [], torch.bmm
    with monkeypatch.context() as m:
        seen = spy_launches(m, ops)
        m.setattr(torch, "bmm", lambda *a, **k: (bmms.append(tuple(a[0].shape) + tuple(a[1].shape)), bmm(*a, **k))[1])
        yg = g32(xg, lengths.to(dev()))
        yg.backward(gy.to(dev()))
        torch.cuda.synchronize()
    y64 = c64(x64, lengths)
    y64.backward(gy.double())
    y32 = c32(x32, lengths)
    y32.backward(gy)

    def rel(a, b):
        return float((a.detach().cpu().double() - b.detach()).abs().max() / b.detach().abs().max().clamp_min(1e-30))
    triples = {"y": (yg, y32, y64), "hidden": (g32.all_hiddens, c32.all_hiddens, c64.all_hiddens), "d_x": (xg.grad, x32.grad, x64.grad)}
    for (n, p64), (_, p32), (_, pg) in zip(c64.named_parameters(), c32.named_parameters(), g32.named_parameters()):
        triples["d_" + n.replace("gru_cell.", "")] = (pg.grad, p32.grad, p64.grad)
    assert len(triples) == 3 + 9
    rows = {k: (rel(g, r64), rel(r32, r64)) for k, (g, r32, r64) in triples.items()}
    bars = {k: max(2e-5, 4.0 * e32) for k, (_, e32) in rows.items()}
    worst = max(rows, key=lambda k: rows[k][0] / bars[k])
    print("[%s] " % tag + "  ".join("%s gpu %.2e e32 %.2e" % (k, *v) for k, v in rows.items()))
    measured("%s worst rel err vs float64" % tag, rows[worst][0], bars[worst], "%s (e32 %.2e)" % (worst, rows[worst][1]))
    for k in rows:
        assert rows[k][0] <= bars[k], (k, rows[k], bars[k])
    return seen, bmms


def _assert_path(seen, bmms, B, T, batched):
    """Which kernels formed the recurrent products.  (The input projections are batched_linear's: the batched split kernel from
    1152 rows on, the batched library GEMM below -- three torch.bmm calls with B*T rows each, forward, d_x and d_w -- as
    ops.BatchedLinearFn documents; none may have B rows, which is what a recurrent product would have.)"""
    names = [n for n, _ in seen]
    phases = [s[0] for n, s in seen if n in ("grouped_gemm", "grouped_gemm_split")]
    # (which side of batched_linear's own row threshold the input projections fell on is read off what it launched, not restated)
    projections = [s for n, s in seen if n == "gemm_nt_split_batched" and s[1] == B * T]
    if projections:
        assert len(projections) == 2 and not bmms, "the encoder issued a library GEMM: %s" % bmms
    else:
        assert len(bmms) == 3 and all(B * T in s and s.count(B) == 0 for s in bmms), bmms
    recurrent = [s for n, s in seen if n == "gemm_nt_split_batched" and s[1] == B]
    packs = [s for n, s in seen if n == "split_weights_pack" and s[1] == s[2]]          # the [H,H] recurrent weights' images
    if batched:
        assert len(recurrent) == 2 * (T - 1) and "gru_step_fwd" not in phases and "gru_step_bwd" not in phases, (len(recurrent), phases)
        assert sorted(s[3] for s in packs) == [False, True], packs          # W for the forward, W^T for the data gradients: once each
    else:
        assert not recurrent and not packs, (recurrent, packs)
        assert phases.count("gru_step_fwd") == T - 1 and phases.count("gru_step_bwd") == T - 1, phases
    assert names.count("gemm_nt_split_batched") == len(recurrent) + len(projections), names
    assert names.count("gru_gates_fwd") == T and names.count("gru_gates_bwd") == T


@gpu
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("af", ["relu", "tanh"])
@pytest.mark.parametrize("B", [63, 64, 100, 130, 256])
def test_gru_sequence_next_to_the_threshold_and_at_the_configs_batch_sizes(ops, monkeypatch, measured, B, af, train):
    """128 -> 324 (N = 324 has a ragged column tile, the contraction pads 324 -> 384), T = 9: B = 63 takes the grouped fallback,
    B >= 64 the batched kernel (ops.GruSequence: fast = gemm_nt_split_batched_ok, M >= 64), and no recurrent product is a
    library GEMM either way."""
    seen, bmms = _sequence_case(ops, monkeypatch, measured, B, 9, 128, 324, af, train, "B=%d %s %s" % (B, af, "train" if train else "eval"))
    _assert_path(seen, bmms, B, 9, batched=B >= 64)


@gpu
def test_gru_sequence_at_full_width_and_length(ops, monkeypatch, measured):
    """620 -> 2400, B = 100 (config/CoR2.py), T = 26 (the encoder's real sequence length), tanh, training mode: the rounding of 26
    recurrent steps compounds, which the float32 CPU form measures on the same inputs and masks."""
    seen, bmms = _sequence_case(ops, monkeypatch, measured, 100, 26, 620, 2400, "tanh", True, "B=100 T=26 full width")
    _assert_path(seen, bmms, 100, 26, batched=True)
    assert [n for n, _ in seen].count("gemm_tn_split") == 6


# ---- 6. the launches of one sequence, in order ----------------------------------------------------------------------------------
def _launch_steps(first, product, gate, T):
    """[first, gate] + [product, gate] * (T - 1): what is prepared once per pass, then a gate launch per step with the step's
    product in front of all but the first"""
    return [first, gate] + [product, gate] * (T - 1)


# Recorded from the fp32 and the bf16 autograd Function as they stood before the two shared one loop body (today both are
# ops.GruSequence); forward then backward, relu, masks given, d_w wanted; (compute_dtype, B, T, H) -> names handed to ops._launch.  fp32: B = 2 takes the grouped fallback (every
# product one direct-output grouped launch), B = 64, H = 324 the batched kernel (the smallest such case of section 5; 324 is outside
# of vqa_gemm_tn_split: d_w is a grouped launch on the split engine with its epilogue).  bf16 has one path; H = 328 is 324 rounded
# up to the multiple of 8 it needs.
GRU_LAUNCHES = {
    (None, 2, 3, 8): ["gru_gates_fwd", "grouped_gemm", "gru_gates_fwd", "grouped_gemm", "gru_gates_fwd",
                      "gru_gates_bwd", "grouped_gemm", "gru_gates_bwd", "grouped_gemm", "gru_gates_bwd", "grouped_gemm"],
    (None, 64, 9, 324): _launch_steps("split_weights_pack", "gemm_nt_split_batched", "gru_gates_fwd", 9)
    + _launch_steps("split_weights_pack", "gemm_nt_split_batched", "gru_gates_bwd", 9) + ["grouped_gemm_split", "grouped_epilogue"],
    ("bf16", 2, 3, 8): ["pack_bf16", "gru_gates_fwd_bf16", "gru_gemm_bf16", "gru_gates_fwd_bf16", "gru_gemm_bf16", "gru_gates_fwd_bf16",
                        "pack_bf16", "gru_gates_bwd_bf16", "gru_gemm_bf16", "gru_gates_bwd_bf16", "gru_gemm_bf16", "gru_gates_bwd_bf16",
                        "gemm_bf16_tn", "gemm_bf16_tn", "gemm_bf16_tn"],
    ("bf16", 64, 9, 328): _launch_steps("pack_bf16", "gru_gemm_bf16", "gru_gates_fwd_bf16", 9)
    + _launch_steps("pack_bf16", "gru_gemm_bf16", "gru_gates_bwd_bf16", 9) + ["gemm_bf16_tn"] * 3,
}


@gpu
@pytest.mark.parametrize("case", list(GRU_LAUNCHES), ids=lambda c: "%s-B%dT%dH%d" % (c[0] or "f32", *c[1:]))
def test_gru_sequence_issues_the_recorded_launches_in_order(ops, monkeypatch, case):
    dtype, B, T, H = case
    gen = torch.Generator().manual_seed(B + H)
    gi = (0.5 * torch.randn(3, B, T, H, generator=gen)).to(dev()).requires_grad_()
    w = (torch.randn(3, H, H, generator=gen) / H ** 0.5).to(dev()).requires_grad_()
    masks = ((torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75).to(dev())
    with monkeypatch.context() as m:
        launches = spy_launches(m, ops)
        out = ops.gru_sequence(gi, w, masks, "relu", compute_dtype=dtype)
        out.backward(torch.randn(T, B, H, generator=gen).to(dev()))
        torch.cuda.synchronize()
    seen = [name for name, _ in launches]
    assert seen == GRU_LAUNCHES[case], seen
    assert all(bool(torch.isfinite(t).all()) for t in (out, gi.grad, w.grad))
