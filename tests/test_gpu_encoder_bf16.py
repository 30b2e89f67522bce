"""The question encoder's mixed-precision recurrent path on the GPU (csrc/gru_bf16.hip, csrc/gru.hip, ops.GruSequence(bf16=True)):

  kernel level    vqa_gru_gemm_bf16 exact on small integers (any accumulation order is exact below 2^24) in both uses -- the
                  forward's shadow and the transposed shadow of the data gradient --, against float64 on random bf16 operands,
                  row isolation of a NaN, stores confined to [M,N]; vqa_gru_gates_{fwd,bwd}_bf16 against float64, their bf16
                  histories bit for bit from the kernel's own fp32 outputs; refusals
  sequence level  ops.gru_sequence(..., compute_dtype=torch.bfloat16) against a float64 emulation of the contract written here,
                  the launches it makes, run-to-run bits, and the untouched fp32 default
  model level     CoR2 with the bf16 encoder: eval logits next to the fp32 encoder's, the graph-replayed train step, the evaluator

Bars: fp32 results of one kernel: four times the error of the same formulas in float32 with torch on the CPU plus one float32
ulp (WorstBar of tests/kernel_harness.py, the rule of tests/test_gpu_encoder_kernels.py::GateBars); results that pass through a
bf16 intermediate: 2e-2 of the tensor's scale (RTOL_MID of tests/test_gpu_bf16.py)."""
import ctypes
import functools

import pytest
import torch

from kernel_harness import (BF, EPS_BF16, E_BADARG, E_UNSUPPORTED, SENT, WorstBar as Bars, _ptr, _same_bits, _sentinel, _untouched, dev,
                            ops, spy_launches)  # noqa: F401  (ops: the fixture)

gpu = pytest.mark.gpu
RTOL_F32 = 2e-4
RTOL_MID = 2e-2


def pad64(n):
    return (n + 63) // 64 * 64


# ---- 1-3. the GEMM -------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(3, 1, 72, 72), (3, 5, 72, 72), (2, 130, 200, 64), (3, 64, 136, 520), (3, 77, 2400, 2400), (1, 512, 2400, 2400)]
_ids = lambda s: "G%dM%dN%dK%d" % s      # noqa: E731


@functools.lru_cache(maxsize=None)
def gemm_operands(shape, ints):
    """(a [G,M,K], w [G,N,K]) fp32 on the CPU holding bf16-exact values, their float64 product [G,M,N] and the float32 one"""
    G, M, N, K = shape
    gen = torch.Generator().manual_seed(1000 * M + N + K + G + int(ints))
    if ints:
        a, w = (torch.randint(-8, 9, s, generator=gen).float() for s in ((G, M, K), (G, N, K)))
    else:
        a, w = (torch.randn(*s, generator=gen).to(BF).float() for s in ((G, M, K), (G, N, K)))
    ref64 = torch.bmm(a.double(), w.double().transpose(1, 2))
    return a, w, ref64, torch.bmm(a, w.transpose(1, 2))


def run_gemm(ops, shape, a, w, transposed):
    """vqa_gru_gemm_bf16 the way ops.GruSequence calls it: `a` in a zero-padded bf16 history slot, the weights' bf16 shadow
    packed from fp32 masters by vqa_pack_bf16 -- [N,K] masters as they are (the forward), or [K,N] masters into the transposed
    shadow (the data gradient) -- and c inside a larger sentinel-filled buffer (ldc > N, rows past M) -> c [G,M,N]."""
    G, M, N, K = shape
    Kp, L = pad64(K), ops._lib.lib()
    a_d = torch.zeros(G, M, Kp, device=dev(), dtype=BF)
    a_d[:, :, :K] = a.to(dev())
    shadow = torch.zeros(G, N, Kp, device=dev(), dtype=BF)
    if transposed:
        ops.pack_bf16(w.transpose(1, 2).contiguous().to(dev()), shadow, N * Kp, 1, Kp, zero_fill=False)
    else:
        ops.pack_bf16(w.to(dev()), shadow, N * Kp, Kp, 1, zero_fill=False)
    assert not bool(shadow[:, :, K:].any()) and torch.equal(shadow[:, :, :K].float().cpu(), w)
    ldc, rows = N + 5, M + 3
    c = _sentinel(G, rows, ldc)
    assert L.vqa_gru_gemm_bf16_supported(M, N, K, Kp, Kp, ldc) == 1
    ops._launch("gru_gemm_bf16", shape, L.vqa_gru_gemm_bf16, _ptr(a_d), M * Kp, Kp, _ptr(shadow), N * Kp, Kp, _ptr(c), rows * ldc, ldc,
                G, M, N, K)
    torch.cuda.synchronize()
    got = c[:, :M, :N].clone()
    c[:, :M, :N] = SENT
    assert _untouched(c), "the kernel wrote outside [M,N] of a c_g"
    return got


@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["shadow", "transposed-shadow"])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_ids)
def test_gemm_small_integers_are_exact(ops, shape, transposed):
    """|v| <= 8: every partial sum stays below 64 * 2400 < 2^24, so any accumulation order is exact in fp32 (and the float64
    matmul the reference is formed with is the integer product)."""
    a, w, ref64, _ = gemm_operands(shape, True)
    assert float(ref64.abs().max()) < 2 ** 24
    got = run_gemm(ops, shape, a, w, transposed)
    assert torch.equal(got.cpu().to(torch.int64), ref64.to(torch.int64)) and torch.equal(got.cpu().double(), ref64)


@gpu
@pytest.mark.parametrize("transposed", [False, True], ids=["shadow", "transposed-shadow"])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=_ids)
def test_gemm_random_operands_against_float64(ops, measured, shape, transposed):
    a, w, ref64, ref32 = gemm_operands(shape, False)
    bars = Bars()
    bars.check("gemm %s" % _ids(shape), run_gemm(ops, shape, a, w, transposed), ref64, ref32)
    bars.report(measured, "gru_gemm_bf16")
    measured("gru_gemm_bf16 err / bar", bars.worst[0], 1.0)


@gpu
@pytest.mark.parametrize("row", [76, 63])
def test_gemm_a_nan_stays_in_its_row(ops, row):
    """M = 77: the last row is the one the clamped loads of rows 77 .. 127 re-read; row 63 is the last of the first wave pair."""
    shape = (3, 77, 136, 520)
    a, w, _, _ = gemm_operands(shape, False)
    clean = run_gemm(ops, shape, a, w, False)
    bad = a.clone()
    bad[:, row, 17] = float("nan")
    got = run_gemm(ops, shape, bad, w, False)
    assert bool(torch.isnan(got[:, row]).all())
    keep = [m for m in range(77) if m != row]
    assert _same_bits(got[:, keep], clean[:, keep])


# ---- 4. the gate kernels ----------------------------------------------------------------------------------------------------------
def _sig(z):
    return 1.0 / (1.0 + torch.exp(-z))


def gates_fwd_ref(gi_t, a, hp, af):
    r = _sig(gi_t[0] + a[0])
    i = _sig(gi_t[1] + a[1])
    z = gi_t[2] + r * a[2]
    n = torch.relu(z) if af == 1 else torch.tanh(z)
    return {"h_new": (1.0 - i) * n + i * hp, "r": r, "i": i, "n": n, "a_n": a[2].clone()}


def gates_bwd_ref(d_out, carry, dhm, masks, r, i, n, an, hp, af):
    dh = d_out + carry
    for g in range(3):
        dh = dh + (dhm[g] * masks[g] if masks is not None else dhm[g])
    grad = (n > 0).to(n.dtype) if af == 1 else 1.0 - n * n
    dn = dh * (1.0 - i) * grad
    dzr = dn * an * r * (1.0 - r)
    dzi = dh * (hp - n) * i * (1.0 - i)
    return {"dan": dn * r, "d_gi": torch.stack([dzr, dzi, dn]), "carry_out": dh * i}


def _both(fn, args):
    cast = lambda x, dt: x.to(dt) if isinstance(x, torch.Tensor) else x      # noqa: E731
    return fn(*[cast(x, torch.float64) for x in args]), fn(*[cast(x, torch.float32) for x in args])


GATE_SHAPES = [(1, 1, 8), (3, 5, 24), (7, 4, 328), (100, 26, 2400)]
LD_EXTRA, HIST_PAD = 8, 16      # ld = H + 8; bf16 elements between the groups of a history beyond T*B*ld


def _steps(T):
    return sorted({0, T // 2, T - 1})


def _d(x):
    return x.to(dev()).contiguous() if x is not None else None


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "B%dT%dH%d" % s)
def test_gates_fwd_bf16(ops, measured, shape, af, with_masks):
    B, T, H = shape
    L, ld = ops._lib.lib(), H + LD_EXTRA
    gs = T * B * ld + HIST_PAD
    gen = torch.Generator().manual_seed(161 + B + af)
    gi, a, hp = torch.randn(3, B, T, H, generator=gen), torch.randn(3, B, H, generator=gen), torch.randn(B, H, generator=gen)
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    gi_d, a_d, hp_d, m_d = _d(gi), _d(a), _d(hp), _d(masks)
    bars = Bars()
    for t in _steps(T):
        with_next = t + 1 < T
        out, saved, hist = _sentinel(T, B, H), _sentinel(4, T, B, H), _sentinel(3, gs, dtype=BF)
        ops._launch("gru_gates_fwd_bf16", shape, L.vqa_gru_gates_fwd_bf16, _ptr(gi_d), _ptr(a_d), _ptr(hp_d), _ptr(m_d), _ptr(out[t]),
                    _ptr(hist, (t + 1) * B * ld) if with_next else None, gs, ld, _ptr(saved[0, t]), _ptr(saved[1, t]), _ptr(saved[2, t]),
                    _ptr(saved[3, t]), B, T, H, t, af)
        torch.cuda.synchronize()
        got = {"h_new": out[t].clone(), "r": saved[0, t].clone(), "i": saved[1, t].clone(), "n": saved[2, t].clone(), "a_n": saved[3, t].clone()}
        ref64, ref32 = _both(gates_fwd_ref, (gi[:, :, t], a, hp, af))
        for k in got:
            bars.check("fwd %s t=%d" % (k, t), got[k], ref64[k], ref32[k])
        out[t].fill_(SENT)
        saved[:, t].fill_(SENT)
        assert _untouched(out) and _untouched(saved), "an fp32 output went to another slot than t = %d" % t
        if with_next:
            slot = hist[:, (t + 1) * B * ld:(t + 2) * B * ld].view(3, B, ld)
            want = (got["h_new"][None] * m_d if m_d is not None else got["h_new"][None].expand(3, B, H)).to(BF)    # one rounding of the fp32 product
            assert _same_bits(slot[:, :, :H], want), "hm is not bf(h' * m_g) of the kernel's own h'"
            slot[:, :, :H] = SENT
        assert _untouched(hist), "a masked copy went into a pad column or another slot (t = %d)" % t
    bars.report(measured, "gates fwd bf16")


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("shape", GATE_SHAPES, ids=lambda s: "B%dT%dH%d" % s)
def test_gates_bwd_bf16(ops, measured, shape, af, with_masks):
    B, T, H = shape
    L, ld = ops._lib.lib(), H + LD_EXTRA
    gs = T * B * ld + HIST_PAD
    gen = torch.Generator().manual_seed(171 + B + af)
    rn = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    r, i, an, hp, d_out, carry, dhm = torch.sigmoid(rn(B, H)), torch.sigmoid(rn(B, H)), rn(B, H), rn(B, H), rn(B, H), rn(B, H), rn(3, B, H)
    n = torch.relu(rn(B, H)) if af == 1 else torch.tanh(rn(B, H))
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    ins = [_d(x) for x in (d_out, carry, dhm, masks, r, i, n, an, hp)]
    ref64, ref32 = _both(gates_bwd_ref, (d_out, carry, dhm, masks, r, i, n, an, hp, af))
    bars = Bars()
    for t in _steps(T):
        gz, d_gi, co = _sentinel(3, gs, dtype=BF), _sentinel(3, B, T, H), _sentinel(B, H)
        ops._launch("gru_gates_bwd_bf16", shape, L.vqa_gru_gates_bwd_bf16, *[_ptr(x) for x in ins], _ptr(gz, t * B * ld), gs, ld, _ptr(d_gi),
                    _ptr(co), B, T, H, t, af)
        torch.cuda.synchronize()
        got_gi = d_gi[:, :, t].clone()
        bars.check("bwd d_gi t=%d" % t, got_gi, ref64["d_gi"], ref32["d_gi"])
        bars.check("bwd carry_out t=%d" % t, co, ref64["carry_out"], ref32["carry_out"])
        slot = gz[:, t * B * ld:(t + 1) * B * ld].view(3, B, ld)
        assert _same_bits(slot[:2, :, :H], got_gi[:2].to(BF)), "gz[0:2] is not bf(d_gi[0:2])"
        dan, want = slot[2, :, :H].float().cpu().double(), ref64["dan"]
        bad = (dan - want).abs() > EPS_BF16 * want.abs() + RTOL_F32 * float(want.abs().max())
        assert not bool(bad.any()), "gz[2]: %d elements outside one bf16 rounding of dan" % int(bad.sum())
        slot[:, :, :H] = SENT
        d_gi[:, :, t].fill_(SENT)
        assert _untouched(gz), "gz went into a pad column or another slot (t = %d)" % t
        assert _untouched(d_gi), "d_gi went to another step than t = %d" % t
    bars.report(measured, "gates bwd bf16")


# ---- 5. refusals (no GPU needed: every check precedes the launch) -------------------------------------------------------------------
def test_bf16_encoder_kernels_refuse_what_they_cannot_run():
    from vqa_playground_pytorch_amd import _lib
    L = _lib.lib()
    p, odd = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x10004)
    L.vqa_launch_log_reset()

    def fwd(B=2, T=3, H=8, t=1, af=1, gi=p, h_new=p, hm=p, ld=64):
        return L.vqa_gru_gates_fwd_bf16(gi, p, p, None, h_new, hm, T * B * 64, ld, p, p, p, p, B, T, H, t, af, None)

    def bwd(B=2, T=3, H=8, t=1, af=3, r_s=p, gz=p, ld=64):
        return L.vqa_gru_gates_bwd_bf16(None, None, None, None, r_s, p, p, p, p, gz, T * B * 64, ld, p, p, B, T, H, t, af, None)

    for call in (fwd, bwd):
        assert call(H=12) == E_UNSUPPORTED and b"H % 8" in L.vqa_last_error()
        assert call(H=4) == E_UNSUPPORTED
        assert call(af=2) == E_BADARG and call(t=3) == E_BADARG and call(t=-1) == E_BADARG
        assert call(B=0) == E_BADARG and call(T=0) == E_BADARG and call(H=0) == E_BADARG
        assert call(H=72, ld=64) == E_BADARG and call(ld=68) == E_UNSUPPORTED
    assert fwd(gi=None) == E_BADARG and fwd(h_new=None) == E_BADARG and fwd(hm=odd) == E_UNSUPPORTED
    assert bwd(r_s=None) == E_BADARG and bwd(gz=None) == E_BADARG and bwd(gz=odd) == E_UNSUPPORTED

    ok = L.vqa_gru_gemm_bf16_supported
    assert ok(1, 8, 8, 64, 64, 8) == 1 and ok(512, 2400, 2400, 2432, 2432, 2400) == 1
    assert ok(0, 8, 8, 64, 64, 8) == 0 and ok(5, 12, 8, 64, 64, 12) == 0 and ok(5, 8, 12, 64, 64, 8) == 0      # M >= 1, N % 8, K % 8
    assert ok(5, 72, 72, 72, 128, 72) == 0 and ok(5, 72, 72, 128, 72, 72) == 0 and ok(5, 72, 72, 128, 128, 72) == 1     # rows padded to 64
    assert ok(5, 72, 72, 132, 128, 72) == 0 and ok(5, 72, 72, 128, 128, 71) == 0                                      # lda % 8, ldc >= N

    def gemm(a=p, w=p, c=p, G=3, M=5, N=72, K=72, a_gs=5 * 128):
        return L.vqa_gru_gemm_bf16(a, a_gs, 128, w, 72 * 128, 128, c, M * N, N, G, M, N, K, None)

    assert gemm(a=None) == E_BADARG and gemm(w=None) == E_BADARG and gemm(c=None) == E_BADARG
    assert gemm(G=0) == E_BADARG and gemm(M=0) == E_BADARG
    assert gemm(N=76) == E_UNSUPPORTED and gemm(K=76) == E_UNSUPPORTED and b"multiple of 64" in L.vqa_last_error()
    assert gemm(a=odd) == E_UNSUPPORTED and gemm(a_gs=5 * 128 + 4) == E_UNSUPPORTED
    assert L.vqa_launch_log((ctypes.c_ulonglong * 16)(), 16) == 0, "a refused call launched a kernel"


@gpu
def test_gru_sequence_bf16_names_the_width_limit(ops):
    gi, w = torch.zeros(3, 2, 3, 12, device=dev()), torch.zeros(3, 12, 12, device=dev())
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.gru_sequence(gi, w, None, "tanh", compute_dtype=BF)
    ops.gru_sequence(gi, w, None, "tanh")                      # the fp32 path takes it as before
    with pytest.raises(ValueError, match="compute_dtype must be"):
        ops.gru_sequence(gi, w, None, "tanh", compute_dtype="fp16")


# ---- the sequence --------------------------------------------------------------------------------------------------------------------
def bf(x):
    return x.to(torch.float32).to(BF).to(torch.float64)


def emulate_sequence(gi, w, masks, af, d_out):
    """The contract in float64, forward and backward written out (no autograd): gi [3,B,T,H], w [3,H,H], masks [3,B,H] or None,
    d_out [T,B,H] -> out [T,B,H], d_gi, d_w, min |pre-activation of n|."""
    _, B, T, H = gi.shape
    m = masks if masks is not None else torch.ones(3, B, H, dtype=torch.float64)
    wb = bf(w)
    h = torch.zeros(B, H, dtype=torch.float64)
    hs, hms, rs, is_, ns, ans, pres = [], [], [], [], [], [], []
    for t in range(T):
        hm = bf(h[None] * m) if t else torch.zeros(3, B, H, dtype=torch.float64)
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
        gzb = bf(torch.stack([dzr, dzi, dn * r]))
        d_w += torch.einsum("gbn,gbk->gnk", gzb, hms[t])
        dhm = torch.einsum("gbn,gnk->gbk", gzb, wb)
        carry = dh * i
    return out, d_gi, d_w, float(torch.stack(pres).abs().min())


@functools.lru_cache(maxsize=None)
def sequence_case(shape, af, with_masks):
    B, T, H = shape
    gen = torch.Generator().manual_seed(7 * B + T + H + (af == "relu"))
    gi = torch.randn(3, B, T, H, generator=gen)
    if af == "relu":       # no relu decision on a knife edge
        sign = torch.where(torch.rand(B, T, H, generator=gen) < 0.5, -1.0, 1.0)
        gi[2] = sign * (0.5 + torch.randn(B, T, H, generator=gen).abs())
        w = 0.1 * torch.randn(3, H, H, generator=gen) / H ** 0.5
    else:
        w = torch.randn(3, H, H, generator=gen) / H ** 0.5
    masks = (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75 if with_masks else None
    d_out = torch.randn(T, B, H, generator=gen)
    ref = emulate_sequence(gi.double(), w.double(), masks.double() if masks is not None else None, af, d_out.double())
    return gi, w, masks, d_out, ref


def run_sequence(ops, gi, w, masks, d_out, af, compute_dtype):
    gi_d, w_d = _d(gi).requires_grad_(), _d(w).requires_grad_()
    out = ops.gru_sequence(gi_d, w_d, _d(masks), af, compute_dtype=compute_dtype)
    out.backward(_d(d_out))
    torch.cuda.synchronize()
    return out.detach(), gi_d.grad, w_d.grad


SEQ_SHAPES = [(5, 4, 72), (33, 6, 520), (70, 3, 2400)]


@gpu
@pytest.mark.parametrize("with_masks", [True, False], ids=["masks", "nomasks"])
@pytest.mark.parametrize("af", ["tanh", "relu"])
@pytest.mark.parametrize("shape", SEQ_SHAPES, ids=lambda s: "B%dT%dH%d" % s)
def test_gru_sequence_bf16_against_the_float64_emulation(ops, monkeypatch, measured, shape, af, with_masks):
    B, T, H = shape
    gi, w, masks, d_out, (out64, dgi64, dw64, min_pre) = sequence_case(shape, af, with_masks)
    if af == "relu":
        assert min_pre >= 0.05, min_pre
    bmms, bmm = [], torch.bmm
    with monkeypatch.context() as m:
        launches = spy_launches(m, ops)
        m.setattr(torch, "bmm", lambda *a, **k: (bmms.append(1), bmm(*a, **k))[1])
        got = run_sequence(ops, gi, w, masks, d_out, af, BF)
    seen = [name for name, _ in launches]
    assert seen.count("gru_gemm_bf16") == 2 * (T - 1), seen
    assert seen.count("gru_gates_fwd_bf16") == T and seen.count("gru_gates_bwd_bf16") == T and seen.count("gemm_bf16_tn") == 3, seen
    assert not bmms and not {"gemm_nt_split_batched", "gemm_tn_split", "grouped_gemm", "grouped_gemm_split", "gru_gates_fwd", "gru_gates_bwd"} & set(seen), seen
    tag = "B%dT%dH%d %s %s" % (B, T, H, af, "masks" if with_masks else "nomasks")
    for name, g, r in zip(("out", "d_gi", "d_w"), got, (out64, dgi64, dw64)):
        assert bool(torch.isfinite(g).all()), name
        err = float((g.cpu().double() - r).abs().max()) / float(r.abs().max())
        measured("%s %s err / scale" % (tag, name), err, RTOL_MID)
        assert err <= RTOL_MID, (name, err)
    again = run_sequence(ops, gi, w, masks, d_out, af, BF)
    for name, g, h in zip(("out", "d_gi", "d_w"), got, again):
        assert _same_bits(g, h), "%s differs between two runs from the same inputs" % name


@gpu
@pytest.mark.parametrize("shape", [(33, 6, 520), (70, 3, 2400)], ids=lambda s: "B%dT%dH%d" % s)
def test_gru_sequence_default_is_the_fp32_function_bit_for_bit(ops, shape):
    gi, w, masks, d_out, (out64, _, _, _) = sequence_case(shape, "tanh", True)
    gi_d, w_d = _d(gi).requires_grad_(), _d(w).requires_grad_()
    want = ops.GruSequence.apply(gi_d, w_d, _d(masks), "tanh")
    want.backward(_d(d_out))
    want = (want.detach(), gi_d.grad, w_d.grad)
    for dtype in (None, torch.float32):
        got = run_sequence(ops, gi, w, masks, d_out, "tanh", dtype)
        assert all(_same_bits(g, r) for g, r in zip(got, want)), dtype
    mixed = run_sequence(ops, gi, w, masks, d_out, "tanh", "bf16")
    assert not torch.equal(mixed[0], want[0]), "the bf16 mode returned the fp32 result"


# ---- the model -----------------------------------------------------------------------------------------------------------------------
VOCAB = ["PAD", "UNK"] + ["w%d" % i for i in range(38)]
ANSWERS, MB, MT = 20, 8, 5


def _model(encoder_dtype):
    from vqa_playground_pytorch_amd import cor2
    torch.manual_seed(17)
    return cor2.Model(VOCAB, ANSWERS, seq2vec="skipthoughts", encoder_dtype=encoder_dtype).to(dev())


def _batch():
    gen = torch.Generator().manual_seed(19)
    v = torch.randn(MB, 36, 2048, generator=gen).abs()
    # left-aligned token ids, 0 = PAD; no word appears twice in the batch: the embedding's weight gradient (the input side, fp32
    # and outside of this mode) is an index_add_ whose atomic adds to one row arrive in any order, and the run-to-run check below
    # is about the recurrent path
    q = (1 + torch.randperm(len(VOCAB) - 1, generator=gen))[:MB * MT - 1]
    q = torch.cat([q, q.new_zeros(1)]).view(MB, MT)
    q[1, 3:] = 0
    q[4, 1:] = 0
    assert len(set(q[q > 0].tolist())) == int((q > 0).sum())
    a = torch.softmax(2.0 * torch.randn(MB, ANSWERS, generator=gen), dim=1)
    return {"v": v.to(dev()), "q_idxes": q.to(dev())}, a.to(dev())


@gpu
def test_cor2_eval_logits_with_the_bf16_encoder(measured):
    sample, _ = _batch()
    f32, b16 = _model(None).eval(), _model(BF).eval()
    assert b16.seq2vec.compute_dtype == BF and f32.seq2vec.compute_dtype == torch.float32
    for (k, x), (_, y) in zip(f32.state_dict().items(), b16.state_dict().items()):
        assert torch.equal(x, y), k
    with torch.no_grad():
        want, got = f32(sample), b16(sample)
    err = float((got - want).abs().max() / want.abs().max())
    measured("CoR2 eval logits, bf16 encoder vs fp32 encoder", err, RTOL_MID)
    assert bool(torch.isfinite(got).all()) and err <= RTOL_MID and not torch.equal(got, want), err


@gpu
def test_cor2_trains_and_evaluates_under_graph_replay_with_the_bf16_encoder(lib_option):
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    # MB = 8 is below the batch from which the attention-pool backward takes its one-launch form (VQA_K3_FUSED_MIN_B: 64 for fp32
    # regions); the three-launch form below it adds its partial sums with float atomics in arrival order, so two runs of this step
    # differed in the last bits of the loss now and then (tests/test_gpu_models.py::test_step_is_bitwise_reproducible_...).  The
    # run-to-run check below is about the recurrent path: take the fixed-order form, as tests/test_gpu_kernels.py does.
    lib_option("VQA_K3_FUSED_MIN_B", 1)
    sample, a = _batch()
    losses = []
    for _ in range(2):
        model = _model(BF).train()
        torch.manual_seed(23)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
        for _ in range(5):
            loss, norm = tr.step(sample, a)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(loss)) and bool(torch.isfinite(norm))
        assert tr._graph is not None, "the step was not captured"
        assert all(c.get("memset", 0) == 0 for c in tr.graph_nodes.values()), tr.graph_nodes
        losses.append(int(loss.detach().view(torch.int32).item()))
    assert losses[0] == losses[1], "two runs from the same seeds disagree: %s" % losses
    ev = Evaluator(model, graph=True)
    out = ev.step(dict(sample, a=a))
    torch.cuda.synchronize()
    assert out["pred"].shape == (MB,) and bool(((out["pred"] >= 0) & (out["pred"] < ANSWERS)).all())
