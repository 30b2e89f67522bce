"""The question encoder's mixed-precision INPUT side on the GPU (csrc/encoder_input_bf16.hip, ops.EncoderInputBf16):

  kernel level    vqa_embed_pack_bf16 bit for bit against torch's (table[idx] * m).to(bfloat16), pads and further planes untouched;
                  vqa_gemm_bf16_nt_f32_bias exact on small integers, against float64 on random bf16 operands, bit-equal to
                  vqa_gru_gemm_bf16 without a bias, a shared `a` plane, stores confined to [M,N], row isolation of a NaN, refusals;
                  vqa_embed_grad exact on small integers under any order of the atomics (a B*T-way collision included), against
                  float64 on random values, the dense form exact and run-to-run bit-equal
  function level  ops.encoder_input_bf16 against a float64 emulation of the contract written here, its launches, run-to-run bits
  module level    BayesianGRU / SkipThoughts(input_dtype=bfloat16) with both values of compute_dtype
  model level     CoR2 with encoder_input_dtype=bf16: eval logits next to the fp32 encoder's, the graph-replayed train step, the
                  evaluator

Bars: fp32 results of one kernel: four times the error of the same formulas in float32 with torch on the CPU plus one float32 ulp
(`Bars`: WorstBar of tests/kernel_harness.py); results that pass through a bf16 intermediate: 2e-2 of the tensor's
scale (RTOL_MID of tests/test_gpu_bf16.py)."""
import ctypes
import functools

import pytest
import torch

from kernel_harness import (BF, E_BADARG, E_UNSUPPORTED, SENT, WorstBar as Bars, _ptr, _same_bits, _sentinel, _untouched, dev,
                            ops, spy_launches)  # noqa: F401  (ops: the fixture)

gpu = pytest.mark.gpu
RTOL_MID = 2e-2


def _d(x):
    return x.to(dev()).contiguous() if x is not None else None


def pad64(n):
    return (n + 63) // 64 * 64


def pad8(n):
    return (n + 7) // 8 * 8


def _token_ids(M, V, gen, same=None):
    """ids with 0 (PAD), a repeat and V - 1 among them as far as M allows"""
    if same is not None:
        return torch.full((M,), same, dtype=torch.int64)
    ids = torch.randint(0, V, (M,), generator=gen)
    if M >= 4:
        ids[0], ids[1], ids[2], ids[M - 1] = 0, V - 1, V - 1, 0
    return ids


# ---- 1. vqa_embed_pack_bf16 -------------------------------------------------------------------------------------------------------
PACK_SHAPES = [(7, 1, 1, 8, 64), (11, 3, 4, 20, 64), (50, 5, 7, 620, 640)]      # (V, B, T, K, ld)


def run_pack(ops, table_or_x, ids, masks, B, T, K, ld, V):
    """-> the planes the kernel was asked for, [planes, M, K] bf16; asserts that nothing else of a 4-plane sentinel buffer (the
    columns [K, ld) of every row, the further planes, the words between the planes) was written"""
    M, L = B * T, ops._lib.lib()
    plane = M * ld + 8
    xb = _sentinel(4 * plane, dtype=BF)
    src, idx_d, m_d = _d(table_or_x), _d(ids), _d(masks)
    ops._launch("embed_pack_bf16", (B, T, K), L.vqa_embed_pack_bf16, _ptr(src), _ptr(idx_d), _ptr(m_d), _ptr(xb), plane, ld, M, K, T, V, 3)
    torch.cuda.synchronize()
    planes = 3 if masks is not None else 1
    view = xb.view(4, plane)[:planes, :M * ld].view(planes, M, ld)
    got = view[:, :, :K].clone()
    view[:, :, :K] = SENT
    assert _untouched(xb), "the kernel wrote a pad column, a plane it was not asked for, or between the planes"
    return got


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("with_idx", [True, False], ids=["idx", "dense"])
@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "V%dB%dT%dK%dld%d" % s)
def test_embed_pack_is_torchs_gather_mask_round_bit_for_bit(ops, shape, with_idx, with_masks):
    V, B, T, K, ld = shape
    M = B * T
    gen = torch.Generator().manual_seed(41 + V + K)
    masks = (torch.rand(B, 3, K, generator=gen) > 0.25).float() * (4.0 / 3.0) if with_masks else None
    mrow = masks.repeat_interleave(T, 0).transpose(0, 1) if with_masks else None      # [3, M, K]: row m uses b = m / T
    if with_idx:
        table = torch.randn(V, K, generator=gen)
        cases = [_token_ids(M, V, gen)] if M >= 4 else [torch.full((M,), 0, dtype=torch.int64), torch.full((M,), V - 1, dtype=torch.int64)]
        for ids in cases:
            e = table[ids]
            want = (e[None] * mrow).to(BF) if with_masks else e[None].to(BF)
            assert _same_bits(run_pack(ops, table, ids, masks, B, T, K, ld, V).cpu(), want)
    else:
        x = torch.randn(M, K, generator=gen)
        want = (x[None] * mrow).to(BF) if with_masks else x[None].to(BF)
        assert _same_bits(run_pack(ops, x, None, masks, B, T, K, ld, 0).cpu(), want)


@gpu
def test_embed_pack_clamps_an_id_outside_the_table(ops):
    V, B, T, K, ld = 11, 3, 4, 20, 64
    gen = torch.Generator().manual_seed(43)
    table = torch.randn(V, K, generator=gen)
    ids = _token_ids(B * T, V, gen)
    ids[3], ids[4], ids[5] = -3, V, V + 1000
    got = run_pack(ops, table, ids, None, B, T, K, ld, V)
    assert _same_bits(got.cpu(), table[ids.clamp(0, V - 1)][None].to(BF))


# ---- 2. vqa_gemm_bf16_nt_f32_bias ---------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(3, 1, 72, 64), (3, 5, 72, 20), (2, 130, 200, 64), (3, 77, 2400, 620), (1, 512, 2400, 620)]      # (G, M, N, K)
_ids = lambda s: "G%dM%dN%dK%d" % s      # noqa: E731


@functools.lru_cache(maxsize=None)
def gemm_operands(shape, ints):
    """(a [G,M,K], w [G,N,K], bias [G,N]) fp32 on the CPU, a and w holding bf16-exact values; the float64 result [G,M,N] and the
    float32 one; computed once per shape and shared (never modified)"""
    G, M, N, K = shape
    gen = torch.Generator().manual_seed(1000 * M + N + K + G + int(ints))
    if ints:
        a, w = (torch.randint(-8, 9, s, generator=gen).float() for s in ((G, M, K), (G, N, K)))
        bias = torch.randint(-8, 9, (G, N), generator=gen).float()
    else:
        a, w = (torch.randn(*s, generator=gen).to(BF).float() for s in ((G, M, K), (G, N, K)))
        bias = torch.randn(G, N, generator=gen)
    ref64 = torch.bmm(a.double(), w.double().transpose(1, 2)) + bias.double()[:, None]
    return a, w, bias, ref64, torch.bmm(a, w.transpose(1, 2)) + bias[:, None]


def run_gemm(ops, shape, a, w, bias, shared_a=False, entry="nt_f32_bias"):
    """The product the way ops.EncoderInputBf16 calls it: `a` in zero-padded bf16 planes (ONE plane and a_gs = 0 with shared_a),
    the weights' shadow packed by vqa_pack_bf16, the bias rows bias_gs = N + 3 apart, c inside a larger sentinel buffer (ldc > N,
    rows past M) -> c [G,M,N].  entry 'gru': vqa_gru_gemm_bf16 on the same operands (K rounded up to 8: the pads are zero)."""
    G, M, N, K = shape
    Kp, L = pad64(K), ops._lib.lib()
    a_d = torch.zeros(1 if shared_a else G, M, Kp, device=dev(), dtype=BF)
    a_d[:, :, :K] = a[:1].to(dev()) if shared_a else a.to(dev())
    shadow = torch.zeros(G, N, Kp, device=dev(), dtype=BF)
    ops.pack_bf16(w.to(dev()), shadow, N * Kp, Kp, 1, zero_fill=False)
    assert not bool(shadow[:, :, K:].any()) and torch.equal(shadow[:, :, :K].float().cpu(), w)
    b_d = None
    if bias is not None:
        b_d = _sentinel(G, N + 3)
        b_d[:, :N] = bias.to(dev())
    ldc, rows = N + 5, M + 3
    c = _sentinel(G, rows, ldc)
    if entry == "gru":
        ops._launch("gru_gemm_bf16", shape, L.vqa_gru_gemm_bf16, _ptr(a_d), 0 if shared_a else M * Kp, Kp, _ptr(shadow), N * Kp, Kp,
                    _ptr(c), rows * ldc, ldc, G, M, N, pad8(K))
    else:
        ops._launch("gemm_bf16_nt_f32_bias", shape, L.vqa_gemm_bf16_nt_f32_bias, _ptr(a_d), 0 if shared_a else M * Kp, Kp, _ptr(shadow),
                    N * Kp, Kp, _ptr(b_d), N + 3, _ptr(c), rows * ldc, ldc, G, M, N, K)
    torch.cuda.synchronize()
    got = c[:, :M, :N].clone()
    c[:, :M, :N] = SENT
    assert _untouched(c), "the kernel wrote outside [M,N] of a c_g"
    return got


@gpu
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_ids)
def test_gemm_small_integers_and_an_integer_bias_are_exact(ops, shape):
    """|v| <= 8: every partial sum stays below 64 * 640 + 8 < 2^24, so any accumulation order is exact in fp32."""
    a, w, bias, ref64, _ = gemm_operands(shape, True)
    assert float(ref64.abs().max()) < 2 ** 24
    got = run_gemm(ops, shape, a, w, bias)
    assert torch.equal(got.cpu().double(), ref64)


@gpu
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_ids)
def test_gemm_random_operands_against_float64(ops, measured, shape):
    a, w, bias, ref64, ref32 = gemm_operands(shape, False)
    bars = Bars()
    bars.check("gemm %s" % _ids(shape), run_gemm(ops, shape, a, w, bias), ref64, ref32)
    bars.report(measured, "gemm_bf16_nt_f32_bias")
    measured("gemm_bf16_nt_f32_bias err / bar", bars.worst[0], 1.0)


@gpu
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_ids)
def test_gemm_without_a_bias_is_gru_gemm_bf16_bit_for_bit(ops, shape):
    a, w, _, _, _ = gemm_operands(shape, False)
    assert _same_bits(run_gemm(ops, shape, a, w, None), run_gemm(ops, shape, a, w, None, entry="gru"))


@gpu
@pytest.mark.parametrize("shape", [s for s in GEMM_SHAPES if s[0] > 1], ids=_ids)
def test_gemm_shared_a_plane_is_three_copies_of_it(ops, shape):
    a, w, bias, _, _ = gemm_operands(shape, False)
    copies = a[:1].expand_as(a).contiguous()
    assert _same_bits(run_gemm(ops, shape, a, w, bias, shared_a=True), run_gemm(ops, shape, copies, w, bias))


@gpu
@pytest.mark.parametrize("row", [76, 63])
def test_gemm_a_nan_stays_in_its_row(ops, row):
    """M = 77: the last row is the one the clamped loads of rows 77 .. 127 re-read; row 63 is the last of the first wave pair."""
    shape = (3, 77, 136, 620)
    a, w, bias, _, _ = gemm_operands(shape, False)
    clean = run_gemm(ops, shape, a, w, bias)
    bad = a.clone()
    bad[:, row, 17] = float("nan")
    got = run_gemm(ops, shape, bad, w, bias)
    assert bool(torch.isnan(got[:, row]).all())
    keep = [m for m in range(77) if m != row]
    assert _same_bits(got[:, keep], clean[:, keep])


# ---- refusals (no GPU needed: every check precedes the launch) -----------------------------------------------------------------------
def test_encoder_input_kernels_refuse_what_they_cannot_run():
    from vqa_playground_pytorch_amd import _lib
    L = _lib.lib()
    p, odd = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    L.vqa_launch_log_reset()

    def gemm(a=p, w=p, c=p, bias=p, G=3, M=5, N=72, K=20, lda=64, ldw=64, ldc=72, a_gs=5 * 64):
        return L.vqa_gemm_bf16_nt_f32_bias(a, a_gs, lda, w, 72 * 64, ldw, bias, 72, c, M * 72, ldc, G, M, N, K, None)

    assert gemm(a=None) == E_BADARG and gemm(w=None) == E_BADARG and gemm(c=None) == E_BADARG
    assert gemm(G=0) == E_BADARG and gemm(M=0) == E_BADARG and gemm(K=0) == E_BADARG and gemm(a_gs=-8) == E_BADARG
    assert gemm(a=odd) == E_UNSUPPORTED and b"16-byte" in L.vqa_last_error()                    # a misaligned a
    assert gemm(a_gs=5 * 64 + 4) == E_UNSUPPORTED
    assert gemm(K=65) == E_UNSUPPORTED and b"multiple of 64" in L.vqa_last_error()            # lda = 64 < K padded to 64 = 128
    assert gemm(lda=32) == E_UNSUPPORTED and gemm(ldw=56) == E_UNSUPPORTED and gemm(lda=68) == E_UNSUPPORTED
    assert gemm(N=76, ldc=76) == E_UNSUPPORTED and gemm(ldc=64) == E_UNSUPPORTED               # N % 8, ldc >= N

    def pack(src=p, idx=p, masks=p, xb=p, plane=12 * 64, ld=64, M=12, K=20, T=4, V=11, G=3):
        return L.vqa_embed_pack_bf16(src, idx, masks, xb, plane, ld, M, K, T, V, G, None)

    assert pack(src=None) == E_BADARG and pack(xb=None) == E_BADARG and pack(M=0) == E_BADARG and pack(T=5) == E_BADARG
    assert pack(V=0) == E_BADARG and pack(ld=16) == E_BADARG and pack(plane=11 * 64) == E_BADARG
    assert pack(K=22) == E_UNSUPPORTED and b"K % 4" in L.vqa_last_error()
    assert pack(ld=68, plane=12 * 68) == E_UNSUPPORTED and pack(xb=odd) == E_UNSUPPORTED and pack(masks=odd) == E_UNSUPPORTED

    def grad(dxm=p, gs=12 * 24, ldx=24, masks=p, idx=p, out=p, M=12, K=20, T=4, V=11, G=3):
        return L.vqa_embed_grad(dxm, gs, ldx, masks, idx, 0, out, M, K, T, V, G, None)

    assert grad(dxm=None) == E_BADARG and grad(out=None) == E_BADARG and grad(M=0) == E_BADARG and grad(T=5) == E_BADARG
    assert grad(V=0) == E_BADARG and grad(ldx=16) == E_BADARG and grad(gs=11 * 24) == E_BADARG
    assert grad(K=22) == E_UNSUPPORTED and grad(ldx=22, gs=12 * 22) == E_UNSUPPORTED and grad(dxm=odd) == E_UNSUPPORTED
    assert L.vqa_launch_log((ctypes.c_ulonglong * 16)(), 16) == 0, "a refused call launched a kernel"


# ---- 3. vqa_embed_grad ----------------------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(7, 1, 1, 8, 8), (11, 3, 4, 20, 24), (50, 5, 7, 620, 624)]      # (V, B, T, K, ldx)
_gid = lambda s: "V%dB%dT%dK%dldx%d" % s      # noqa: E731
JUNK = 77.0          # what the columns [K, ldx) of dxm hold: never read


def run_grad(ops, dxm, masks, ids, B, T, K, ldx, V, padding_idx=0):
    """dxm [3,M,K] on the CPU -> d_table [V,K] (ids given) or d_x [M,K]; dxm sits in planes of row stride ldx, `out` inside a
    zero-filled buffer whose tail holds a sentinel"""
    M, L = B * T, ops._lib.lib()
    dxm_d = torch.full((3, M, ldx), JUNK, device=dev())
    dxm_d[:, :, :K] = dxm.to(dev())
    rows = V if ids is not None else M
    buf = _sentinel(rows * K + 16)
    buf[:rows * K] = 0.0
    m_d, idx_d = _d(masks), _d(ids)
    ops._launch("embed_grad", (B, T, K), L.vqa_embed_grad, _ptr(dxm_d), M * ldx, ldx, _ptr(m_d), _ptr(idx_d), padding_idx,
                _ptr(buf), M, K, T, V if ids is not None else 0, 3)
    torch.cuda.synchronize()
    assert _untouched(buf[rows * K:]), "the kernel wrote past the gradient"
    return buf[:rows * K].view(rows, K).clone()


def grad_reference(dxm, masks, ids, T, V, dtype, padding_idx=0):
    d = dxm.to(dtype)
    if masks is not None:
        d = d * masks.to(dtype).repeat_interleave(T, 0).transpose(0, 1)
    d_e = d[0] + d[1] + d[2]
    if ids is None:
        return d_e
    keep = (ids != padding_idx).to(dtype).unsqueeze(1)
    return torch.zeros(V, dxm.shape[2], dtype=dtype).index_add_(0, ids, d_e * keep)


@gpu
@pytest.mark.parametrize("collide", [False, True], ids=["mixed-ids", "one-id"])
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=_gid)
def test_embed_grad_small_integers_are_exact_in_any_order(ops, shape, with_masks, collide):
    """|dxm| <= 8, masks in {0, 2}: every partial sum is an integer below 2^24, so the atomics may arrive in any order."""
    V, B, T, K, ldx = shape
    M = B * T
    gen = torch.Generator().manual_seed(53 + V)
    dxm = torch.randint(-8, 9, (3, M, K), generator=gen).float()
    masks = (torch.rand(B, 3, K, generator=gen) > 0.25).float() * 2.0 if with_masks else None
    ids = _token_ids(M, V, gen, same=V - 2 if collide else None)      # one-id: a B*T-way collision on every element of a row
    if M == 1 and not collide:
        ids[0] = 0                                                    # the PAD id alone: nothing is added anywhere
    got = run_grad(ops, dxm, masks, ids, B, T, K, ldx, V).cpu()
    assert torch.equal(got.double(), grad_reference(dxm, masks, ids, T, V, torch.float64))
    unused = sorted(set(range(V)) - set(ids.tolist()) | {0})
    assert not bool(got[unused].any()), "a row of an unused id or the PAD row is not exactly zero"
    if collide:
        assert bool(got[V - 2].any())


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=_gid)
def test_embed_grad_random_values_against_float64(ops, measured, shape, with_masks):
    V, B, T, K, ldx = shape
    M = B * T
    gen = torch.Generator().manual_seed(59 + V)
    dxm = torch.randn(3, M, K, generator=gen)
    masks = (torch.rand(B, 3, K, generator=gen) > 0.25).float() * (4.0 / 3.0) if with_masks else None
    ids = _token_ids(M, V, gen) if M > 1 else torch.full((1,), V - 1, dtype=torch.int64)
    bars = Bars()
    bars.check("embed_grad %s" % _gid(shape), run_grad(ops, dxm, masks, ids, B, T, K, ldx, V),
               grad_reference(dxm, masks, ids, T, V, torch.float64), grad_reference(dxm, masks, ids, T, V, torch.float32))
    bars.report(measured, "embed_grad")


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("shape", GRAD_SHAPES, ids=_gid)
def test_embed_grad_dense_form_is_exact_and_reproducible(ops, shape, with_masks):
    V, B, T, K, ldx = shape
    M = B * T
    gen = torch.Generator().manual_seed(61 + V)
    masks = (torch.rand(B, 3, K, generator=gen) > 0.25).float() * 2.0 if with_masks else None
    dxm = torch.randint(-8, 9, (3, M, K), generator=gen).float()
    got = run_grad(ops, dxm, masks, None, B, T, K, ldx, V).cpu()
    assert torch.equal(got.double(), grad_reference(dxm, masks, None, T, V, torch.float64))
    rnd = torch.randn(3, M, K, generator=gen)
    m43 = masks * (2.0 / 3.0) if with_masks else None
    assert _same_bits(run_grad(ops, rnd, m43, None, B, T, K, ldx, V), run_grad(ops, rnd, m43, None, B, T, K, ldx, V))


# ---- the float64 emulation of the contract ----------------------------------------------------------------------------------------
def bf(x):
    return x.to(torch.float32).to(BF).to(torch.float64)


def same(x):
    return x


def emulate_input_fwd(e, mx, w, b, rnd=bf):
    """e [B,T,K], mx [B,3,K] or None, w [3,H,K], b [3,H], float64 -> gi [3,B,T,H] and what the backward needs"""
    B, T, K = e.shape
    m = mx.transpose(0, 1)[:, :, None, :] if mx is not None else torch.ones(3, B, 1, K, dtype=torch.float64)
    xb, wb = rnd(e[None] * m), rnd(w)                                     # xb_g = bf(e * mx_g), Wb_g = bf(W_ig)
    gi = torch.einsum("gbtk,ghk->gbth", xb, wb) + b[:, None, None, :]
    return gi, (xb, wb, m)


def emulate_input_bwd(saved, d_gi, rnd=bf):
    """-> d_w [3,H,K], d_b [3,H], d_e [B,T,K]"""
    xb, wb, m = saved
    dgb = rnd(d_gi)                                                        # dgb = bf(d_gi)
    d_w = torch.einsum("gbth,gbtk->ghk", dgb, xb)
    d_b = d_gi.sum((1, 2))                                                 # the UNROUNDED d_gi
    d_e = (torch.einsum("gbth,ghk->gbtk", dgb, wb) * m).sum(0)
    return d_w, d_b, d_e


def scatter(d_e, ids, V, padding_idx=0):
    flat = ids.reshape(-1)
    keep = (flat != padding_idx).double().unsqueeze(1)
    return torch.zeros(V, d_e.shape[-1], dtype=torch.float64).index_add_(0, flat, d_e.reshape(flat.numel(), -1) * keep)


def emulate_sequence(gi, w, masks, af, d_out, rnd):
    """The recurrent part in float64 (tests/test_gpu_encoder_bf16.py); rnd = bf for compute_dtype=bfloat16, `same` for fp32."""
    _, B, T, H = gi.shape
    m = masks if masks is not None else torch.ones(3, B, H, dtype=torch.float64)
    wb = rnd(w)
    h = torch.zeros(B, H, dtype=torch.float64)
    hs, hms, rs, is_, ns, ans, pres = [], [], [], [], [], [], []
    for t in range(T):
        hm = rnd(h[None] * m) if t else torch.zeros(3, B, H, dtype=torch.float64)
        a = torch.einsum("gbk,gnk->gbn", hm, wb)
        r = torch.sigmoid(gi[0, :, t] + a[0])
        i = torch.sigmoid(gi[1, :, t] + a[1])
        pre = gi[2, :, t] + r * a[2]
        n = torch.relu(pre) if af == "relu" else torch.tanh(pre)
        hs.append(h)
        h = (1 - i) * n + i * h
        for lst, v in ((hms, hm), (rs, r), (is_, i), (ns, n), (ans, a[2]), (pres, pre)):
            lst.append(v)
    out = torch.stack(hs[1:] + [h])
    d_gi, d_w = torch.zeros_like(gi), torch.zeros_like(w)
    carry, dhm = torch.zeros(B, H, dtype=torch.float64), None
    for t in range(T - 1, -1, -1):
        dh = d_out[t] + carry
        if dhm is not None:
            dh = dh + (dhm * m).sum(0)
        r, i, n, an = rs[t], is_[t], ns[t], ans[t]
        dn = dh * (1 - i) * ((n > 0).double() if af == "relu" else 1 - n * n)
        dzr, dzi = dn * an * r * (1 - r), dh * (hs[t] - n) * i * (1 - i)
        d_gi[0, :, t], d_gi[1, :, t], d_gi[2, :, t] = dzr, dzi, dn
        gzb = rnd(torch.stack([dzr, dzi, dn * r]))
        d_w += torch.einsum("gbn,gbk->gnk", gzb, hms[t])
        dhm = torch.einsum("gbn,gnk->gbk", gzb, wb)
        carry = dh * i
    return out, d_gi, d_w, float(torch.stack(pres).abs().min())


# ---- 4. ops.encoder_input_bf16 -----------------------------------------------------------------------------------------------------
FN_SHAPES = [(5, 4, 20, 72, 11), (33, 6, 620, 520, 50), (70, 3, 620, 2400, 200)]      # (B, T, K, H, V)
_fid = lambda s: "B%dT%dK%dH%dV%d" % s      # noqa: E731


@functools.lru_cache(maxsize=None)
def fn_case(shape, with_masks):
    B, T, K, H, V = shape
    gen = torch.Generator().manual_seed(67 + B + H)
    table = torch.randn(V, K, generator=gen)
    ids = _token_ids(B * T, V, gen).view(B, T)
    mx = (torch.rand(B, 3, K, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    w, b = torch.randn(3, H, K, generator=gen) / K ** 0.5, torch.randn(3, H, generator=gen)
    d_gi = torch.randn(3, B, T, H, generator=gen)
    gi64, saved = emulate_input_fwd(table[ids].double(), mx.double() if with_masks else None, w.double(), b.double())
    dw64, db64, de64 = emulate_input_bwd(saved, d_gi.double())
    return table, ids, mx, w, b, d_gi, {"gi": gi64, "d_w": dw64, "d_b": db64, "d_table": scatter(de64, ids, V), "d_x": de64}


def run_fn(ops, table, ids, mx, w, b, d_gi, dense=False):
    src = _d(table[ids] if dense else table).requires_grad_()
    w_d, b_d = _d(w).requires_grad_(), _d(b).requires_grad_()
    gi = ops.encoder_input_bf16(src, None if dense else _d(ids), _d(mx), w_d, b_d, None if dense else 0)
    gi.backward(_d(d_gi))
    torch.cuda.synchronize()
    return {"gi": gi.detach(), "d_w": w_d.grad, "d_b": b_d.grad, "d_x" if dense else "d_table": src.grad}


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("shape", FN_SHAPES, ids=_fid)
def test_encoder_input_bf16_against_the_float64_emulation(ops, monkeypatch, measured, shape, with_masks):
    B, T, K, H, V = shape
    table, ids, mx, w, b, d_gi, want = fn_case(shape, with_masks)
    bmms, bmm = [], torch.bmm
    with monkeypatch.context() as m:
        seen = spy_launches(m, ops)
        m.setattr(torch, "bmm", lambda *a, **k: (bmms.append(1), bmm(*a, **k))[1])
        got = run_fn(ops, table, ids, mx, w, b, d_gi)
    names = [n for n, _ in seen]
    assert names.count("embed_pack_bf16") == 1 and names.count("gemm_bf16_nt_f32_bias") == 1 and names.count("embed_grad") == 1, seen
    assert names.count("gemm_bf16_tn") == 3 and names.count("gru_gemm_bf16") == 1 and names.count("column_sum") == 3, seen
    assert not bmms and not [s for n, s in seen if n in ("gemm_nt_split_batched", "gemm_tn_split") and B * T in s], seen
    assert not {"bias_act", "act_bwd_colsum", "grouped_gemm", "grouped_gemm_split"} & set(names), seen
    tag = "%s %s" % (_fid(shape), "masks" if with_masks else "nomasks")
    for name in ("gi", "d_w", "d_b", "d_table"):
        g, r = got[name], want[name]
        assert g.dtype == torch.float32 and bool(torch.isfinite(g).all()), name
        err = float((g.cpu().double() - r).abs().max()) / float(r.abs().max())
        measured("%s %s err / scale" % (tag, name), err, RTOL_MID)
        assert err <= RTOL_MID, (name, err)
    assert not bool(got["d_table"][0].any()), "the PAD row of the table's gradient is not exactly zero"
    again = run_fn(ops, table, ids, mx, w, b, d_gi)
    for name in ("gi", "d_w", "d_b"):
        assert _same_bits(got[name], again[name]), "%s differs between two runs from the same inputs" % name


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
def test_encoder_input_bf16_dense_form(ops, measured, with_masks):
    """idx = None: the caller's x [B,T,K]; the same gi as the lookup of the same rows bit for bit, d_x by plain stores"""
    shape = FN_SHAPES[1]
    table, ids, mx, w, b, d_gi, want = fn_case(shape, with_masks)
    got, tok = run_fn(ops, table, ids, mx, w, b, d_gi, dense=True), run_fn(ops, table, ids, mx, w, b, d_gi)
    for name in ("gi", "d_w", "d_b"):
        assert _same_bits(got[name], tok[name]), name
    err = float((got["d_x"].cpu().double() - want["d_x"]).abs().max()) / float(want["d_x"].abs().max())
    measured("%s %s d_x err / scale" % (_fid(shape), "masks" if with_masks else "nomasks"), err, RTOL_MID)
    assert err <= RTOL_MID, err
    assert _same_bits(got["d_x"], run_fn(ops, table, ids, mx, w, b, d_gi, dense=True)["d_x"])


@gpu
def test_encoder_input_bf16_names_its_limits(ops):
    w = torch.zeros(3, 16, 12, device=dev())
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.encoder_input_bf16(torch.zeros(2, 3, 10, device=dev()), None, None, torch.zeros(3, 16, 10, device=dev()))
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.encoder_input_bf16(torch.zeros(2, 3, 12, device=dev()), None, None, torch.zeros(3, 12, 12, device=dev()))
    with pytest.raises(ValueError, match="mx must be"):
        ops.encoder_input_bf16(torch.zeros(2, 3, 12, device=dev()), None, torch.ones(2, 12, device=dev()), w)
    with pytest.raises(ValueError, match="table"):
        ops.encoder_input_bf16(torch.zeros(2, 3, 12, device=dev()), torch.zeros(2, 3, dtype=torch.long, device=dev()), None, w)
    assert ops.encoder_input_bf16(torch.zeros(2, 3, 12, device=dev()), None, None, w).shape == (3, 2, 3, 16)


# ---- 5. the modules ------------------------------------------------------------------------------------------------------------------
MOD_SHAPES = [(5, 4, 20, 72, 11), (33, 6, 620, 520, 50)]      # (B, T, K, H, V)
NAMES = ("r", "i", "n")


@functools.lru_cache(maxsize=None)
def module_case(shape, af, compute_dtype):
    """A BayesianGRU(K, H), token ids, a table, the six masks and a grad_output, with the float64 emulation of the module's forward
    and backward (input side rounded; the recurrent side rounded when compute_dtype is bfloat16)"""
    from vqa_playground_pytorch_amd.encoder import BayesianGRU
    B, T, K, H, V = shape
    torch.manual_seed(71 + H)
    ref = BayesianGRU(K, H, dropout=0.25, af=af)
    gen = torch.Generator().manual_seed(73 + B + (af == "relu"))
    c = ref.gru_cell
    if af == "relu":       # no relu decision on a knife edge (tests/test_encoder_bf16.py)
        with torch.no_grad():
            sign = torch.where(torch.rand(H, generator=gen) < 0.5, -1.0, 1.0)
            c.weight_in.bias.copy_(sign * (0.5 + torch.randn(H, generator=gen).abs()))
            c.weight_in.weight.copy_(0.05 * torch.randn(H, K, generator=gen) / K ** 0.5)       # (x 4/3 masks: sigma 0.06 per sum)
            c.weight_hn.weight.copy_(0.1 * torch.randn(H, H, generator=gen) / H ** 0.5)
    table = torch.randn(V, K, generator=gen)
    ids = _token_ids(B * T, V, gen).view(B, T)
    lengths = torch.randint(1, T + 1, (B,), generator=gen)
    gy = torch.randn(B, H, generator=gen)
    masks = [(torch.rand(B, 1, K, generator=gen) > 0.25).float() / 0.75 for _ in range(3)] + \
            [(torch.rand(B, H, generator=gen) > 0.25).float() / 0.75 for _ in range(3)]
    d = {k: v.double() for k, v in ref.state_dict().items()}
    mx = torch.cat(masks[:3], 1).double()                                     # [B,3,K]
    w_in = torch.stack([d["gru_cell.weight_i%s.weight" % n] for n in NAMES])
    b_in = torch.stack([d["gru_cell.weight_i%s.bias" % n] for n in NAMES])
    gi, saved = emulate_input_fwd(table[ids].double(), mx, w_in, b_in)
    idx = (lengths - 1) % T
    d_out = torch.zeros(T, B, H, dtype=torch.float64)
    d_out[idx, torch.arange(B)] = gy.double()
    w_h = torch.stack([d["gru_cell.weight_h%s.weight" % n] for n in NAMES])
    out, d_gi, d_wh, min_pre = emulate_sequence(gi, w_h, torch.stack(masks[3:]).double(), af, d_out, bf if compute_dtype == BF else same)
    d_wi, d_bi, d_e = emulate_input_bwd(saved, d_gi)
    want = {"y": out[idx, torch.arange(B)], "d_x": d_e, "d_table": scatter(d_e, ids, V)}
    for g, n in enumerate(NAMES):
        want["d_gru_cell.weight_h%s.weight" % n] = d_wh[g]
        want["d_gru_cell.weight_i%s.weight" % n] = d_wi[g]
        want["d_gru_cell.weight_i%s.bias" % n] = d_bi[g]
    return ref, table, ids, lengths, gy, masks, want, min_pre


def run_module(ref, table, ids, lengths, gy, masks, af, tokens, **dtypes):
    from vqa_playground_pytorch_amd.encoder import BayesianGRU
    m = BayesianGRU(ref.input_size, ref.hidden_size, dropout=0.25, af=af, **dtypes)
    m.load_state_dict(ref.state_dict())
    m = m.to(dev()).train()
    queue = [_d(x) for x in masks]
    m._mask = lambda like: queue.pop(0)
    if tokens:
        src = _d(table).requires_grad_()
        y = m(_d(ids), _d(lengths), table=src, padding_idx=0)
    else:
        src = _d(table[ids]).requires_grad_()
        y = m(src, _d(lengths))
    y.backward(_d(gy))
    torch.cuda.synchronize()
    assert not queue, "the module did not draw six masks"
    res = {"y": y.detach(), "d_table" if tokens else "d_x": src.grad}
    res.update({"d_" + n: p.grad for n, p in m.named_parameters()})
    return res


@gpu
@pytest.mark.parametrize("tokens", [True, False], ids=["tokens", "float-x"])
@pytest.mark.parametrize("compute_dtype", [None, BF], ids=["rec-f32", "rec-bf16"])
@pytest.mark.parametrize("af", ["tanh", "relu"])
@pytest.mark.parametrize("shape", MOD_SHAPES, ids=_fid)
def test_bayesian_gru_input_bf16_against_the_float64_emulation(ops, measured, shape, af, compute_dtype, tokens):
    ref, table, ids, lengths, gy, masks, want, min_pre = module_case(shape, af, compute_dtype)
    if af == "relu":
        assert min_pre >= 0.05, min_pre
    got = run_module(ref, table, ids, lengths, gy, masks, af, tokens, input_dtype=BF, compute_dtype=compute_dtype)
    off = run_module(ref, table, ids, lengths, gy, masks, af, False, compute_dtype=compute_dtype)
    assert len(got) == 2 + 9
    tag = "%s %s %s %s" % (_fid(shape), af, "rec-bf16" if compute_dtype == BF else "rec-f32", "tokens" if tokens else "x")
    for k, g in got.items():
        r = want[k]
        assert bool(torch.isfinite(g).all()), k
        err = float((g.cpu().double() - r).abs().max()) / float(r.abs().max())
        measured("%s %s err / scale" % (tag, k.replace("gru_cell.weight_", "")), err, RTOL_MID)
        assert err <= RTOL_MID, (k, err)
    assert not torch.equal(got["y"], off["y"]), "the bf16 input mode returned the fp32 input side's result"
    assert not torch.equal(got["d_gru_cell.weight_ir.weight"], off["d_gru_cell.weight_ir.weight"])


VOCAB = ["PAD", "UNK"] + ["w%d" % i for i in range(38)]
ANSWERS, MB, MT = 20, 8, 5


def _questions(gen, unique=False):
    if unique:      # left-aligned token ids, 0 = PAD, no word twice: the table's gradient then has no atomics that meet
        q = (1 + torch.randperm(len(VOCAB) - 1, generator=gen))[:MB * MT - 1]
        q = torch.cat([q, q.new_zeros(1)]).view(MB, MT)
    else:
        q = torch.randint(1, len(VOCAB), (MB, MT), generator=gen)
    q[1, 3:] = 0
    q[4, 1:] = 0
    return q


def _skipthoughts_run(q, gy, **kw):
    from vqa_playground_pytorch_amd.encoder import SkipThoughts
    torch.manual_seed(29)
    enc = SkipThoughts(VOCAB, af="tanh", **kw).to(dev()).train()
    torch.manual_seed(31)                       # the six masks
    y = enc(q)
    y.backward(gy)
    torch.cuda.synchronize()
    return [y.detach()] + [p.grad for _, p in enc.named_parameters()]


@gpu
@pytest.mark.parametrize("compute_dtype", [None, BF], ids=["rec-f32", "rec-bf16"])
def test_skipthoughts_input_dtype_none_is_not_passing_the_keyword(ops, measured, compute_dtype):
    gen = torch.Generator().manual_seed(37)
    q, gy = _questions(gen, unique=True).to(dev()), torch.randn(MB, 2400, generator=gen).to(dev())
    plain = _skipthoughts_run(q, gy, compute_dtype=compute_dtype)
    for spelled in (None, torch.float32):
        again = _skipthoughts_run(q, gy, compute_dtype=compute_dtype, input_dtype=spelled)
        assert len(plain) == len(again) == 1 + 10 and all(_same_bits(a, b) for a, b in zip(plain, again)), spelled
    mixed = _skipthoughts_run(q, gy, compute_dtype=compute_dtype, input_dtype=BF)
    assert all(bool(torch.isfinite(t).all()) for t in mixed)
    assert not torch.equal(mixed[0], plain[0]) and not torch.equal(mixed[1], plain[1]), "the mode on returned the fp32 input side's bits"
    # same masks (drawn in the fp32 path's order from the same seed), so the two modes sit next to each other
    err = float((mixed[0] - plain[0]).abs().max() / plain[0].abs().max())
    measured("SkipThoughts output, bf16 input side vs fp32 input side", err, RTOL_MID)
    assert err <= RTOL_MID, err
    assert not bool(mixed[1][0].any()), "the PAD row of the embedding gradient is not exactly zero"


# ---- 6. the model --------------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from vqa_playground_pytorch_amd import cor2
    torch.manual_seed(17)
    return cor2.Model(VOCAB, ANSWERS, seq2vec="skipthoughts", **kw).to(dev())


def _batch():
    gen = torch.Generator().manual_seed(19)
    v = torch.randn(MB, 36, 2048, generator=gen).abs()
    q = _questions(gen)
    a = torch.softmax(2.0 * torch.randn(MB, ANSWERS, generator=gen), dim=1)
    return {"v": v.to(dev()), "q_idxes": q.to(dev())}, a.to(dev())


@gpu
@pytest.mark.parametrize("encoder_dtype", [None, BF], ids=["rec-f32", "rec-bf16"])
def test_cor2_eval_logits_with_the_bf16_input_side(measured, encoder_dtype):
    sample, _ = _batch()
    f32, b16 = _model().eval(), _model(encoder_input_dtype=BF, encoder_dtype=encoder_dtype).eval()
    assert b16.seq2vec.input_dtype == BF and f32.seq2vec.input_dtype == torch.float32
    for (k, x), (_, y) in zip(f32.state_dict().items(), b16.state_dict().items()):
        assert torch.equal(x, y), k
    with torch.no_grad():
        want, got = f32(sample), b16(sample)
    err = float((got - want).abs().max() / want.abs().max())
    measured("CoR2 eval logits, bf16 input side vs fp32 encoder", err, RTOL_MID)
    assert bool(torch.isfinite(got).all()) and err <= RTOL_MID and not torch.equal(got, want), err


@gpu
def test_cor2_trains_and_evaluates_under_graph_replay_with_the_bf16_input_side():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    sample, a = _batch()
    model = _model(encoder_input_dtype=BF, encoder_dtype=BF).train()
    torch.manual_seed(23)
    tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
    table_before = model.seq2vec.embedding.weight.detach().clone()
    for _ in range(3):
        loss, norm = tr.step(sample, a)
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(norm))
    torch.cuda.synchronize()
    assert tr._graph is not None, "the step was not captured"
    assert all(c.get("memset", 0) == 0 for c in tr.graph_nodes.values()), tr.graph_nodes
    table = model.seq2vec.embedding.weight.detach()
    used = sorted(set(sample["q_idxes"].flatten().tolist()) - {0})
    assert torch.equal(table[0], table_before[0]), "the PAD row of the table moved"
    assert not torch.equal(table[used], table_before[used]), "the embedding was not trained"
    ev = Evaluator(model, graph=True)
    out = ev.step(dict(sample, a=a))
    torch.cuda.synchronize()
    assert out["pred"].shape == (MB,) and bool(((out["pred"] >= 0) & (out["pred"] < ANSWERS)).all())
