"""GPU parity tests of the mixed-precision (bf16 storage / bf16 MFMA / fp32 accumulate) side -- BASELINE configs[4]
"CoR2 bf16, 100x2048 dense regions" -- against the float64 numpy oracle (oracle/kernels_np.py).

Every bf16 kernel is fed inputs that are exactly representable in bf16, so the oracle sees the same numbers and the
only differences are (i) fp32 accumulation order and (ii) the rounding of bf16 OUTPUTS / saved bf16 intermediates.
Tolerances are therefore stated in units of the bf16 epsilon 2^-8:
  - fp32 outputs computed from bf16 inputs            : RTOL_F32 = 2e-4 of the output scale
  - bf16 outputs (one rounding)                       : elementwise |err| <= 2^-8 |ref| + RTOL_F32 * scale
  - results that pass through a bf16 intermediate     : RTOL_MID = 2e-2 of the output scale (h1 / g*h2 are rounded to
    (K4 backward)                                       bf16 before the second contraction)
Run on the GPU box with:  python -m pytest tests -m gpu
"""
import os

import numpy as np
import pytest
import torch

from kernel_harness import EPS_BF16, dev
from oracle import kernels_np as K
from oracle import seeded

pytestmark = pytest.mark.gpu

RTOL_F32 = 2e-4
RTOL_MID = 2e-2


def bf_round(a):
    """numpy fp32 -> nearest bf16 value (as fp32)."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def gbf(a, requires_grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev()).to(torch.bfloat16)
    return t.requires_grad_() if requires_grad else t


def g32(a, requires_grad=False):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev())
    return t.requires_grad_() if requires_grad else t


def npy(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def close_f32(name, got, want, rtol=RTOL_F32):
    got, want = npy(got) if isinstance(got, torch.Tensor) else np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name + ": non-finite output"
    scale = max(np.abs(want).max(), 1e-20)
    err = np.abs(got - want).max() / scale
    assert err <= rtol, "%s: rel err %.3e > %.1e" % (name, err, rtol)


def close_bf16(name, got, want, extra=RTOL_F32):
    """bf16 output: one rounding of the exact value (plus fp32 accumulation noise)."""
    assert got.dtype == torch.bfloat16, (name, got.dtype)
    got, want = npy(got), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert np.isfinite(got).all(), name + ": non-finite output"
    scale = max(np.abs(want).max(), 1e-20)
    bad = np.abs(got - want) > EPS_BF16 * np.abs(want) + extra * scale
    assert not bad.any(), "%s: %d of %d elements outside one bf16 rounding (worst %.3e of scale)" % (
        name, int(bad.sum()), bad.size, (np.abs(got - want).max() / scale))


@pytest.fixture(scope="module")
def ops():
    from vqa_playground_pytorch_amd import ops as o
    return o


# ----------------------------------------------------------------------------------------------- K1 / K3 in bf16
@pytest.mark.parametrize("B,N,D,G,glimpse", [(3, 5, 12, 1, 0), (2, 36, 2048, 4, 0), (2, 100, 2048, 4, 0), (2, 37, 1024, 2, 1)])
@pytest.mark.parametrize("mode", [0, 1])
def test_pairwise_relation_bf16(ops, B, N, D, G, glimpse, mode):
    v = bf_round(seeded.seeded_array((B, N, D), 201))
    q1 = 1 / (1 + np.exp(-seeded.seeded_array((B, D), 202)))
    q2 = 1 / (1 + np.exp(-seeded.seeded_array((B, D), 203)))
    al = np.abs(seeded.seeded_array((B, N, G), 204)) + 0.05
    gout = bf_round(seeded.seeded_array((B, N, D), 205))
    q1, q2, al = (np.asarray(a, np.float32) for a in (q1, q2, al))
    vt, q1t, q2t, alt = gbf(v, True), g32(q1, True), g32(q2, True), g32(al, True)
    out = ops.pairwise_relation_reduce(vt, q1t, q2t, alt, glimpse=glimpse, mode=mode)
    close_bf16("v2", out, K.pairwise_relation_reduce_fwd(v, q1, q2, al[:, :, glimpse]))
    out.backward(gbf(gout))
    da, dq1, dq2, dv = K.pairwise_relation_reduce_bwd(v, q1, q2, al[:, :, glimpse], gout)
    da_full = np.zeros_like(al, dtype=np.float64)
    da_full[:, :, glimpse] = da
    close_f32("d_alpha", alt.grad, da_full)
    close_f32("d_q1", q1t.grad, dq1)
    close_f32("d_q2", q2t.grad, dq2)
    close_bf16("d_v", vt.grad, dv)


@pytest.mark.parametrize("B,N,D,G", [(2, 36, 2048, 4), (2, 100, 2048, 4), (3, 7, 260, 3), (1, 1, 8, 1)])
def test_softmax_attention_pool_bf16(ops, B, N, D, G):
    logits = seeded.seeded_array((B, N, G), 211).astype(np.float32)
    v = bf_round(seeded.seeded_array((B, N, D), 212))
    dpool = seeded.seeded_array((B, G, D), 213).astype(np.float32)
    dal = seeded.seeded_array((B, N, G), 214).astype(np.float32)
    lt, vt = g32(logits, True), gbf(v, True)
    alpha, pooled = ops.softmax_attention_pool(lt, vt)
    a_ref, p_ref = K.softmax_attention_pool_fwd(logits, v)
    close_f32("alpha", alpha, a_ref)
    close_f32("pooled", pooled, p_ref)
    (alpha * g32(dal)).sum().add((pooled * g32(dpool)).sum()).backward()
    dl_ref, dv_ref = K.softmax_attention_pool_bwd(a_ref, v, dpool, dal)
    close_f32("d_logits", lt.grad, dl_ref)
    close_bf16("d_v", vt.grad, dv_ref)


# ----------------------------------------------------------------------------------------------- bf16 GEMM engine
@pytest.mark.parametrize("M,N,K", [(64, 64, 64), (300, 320, 320), (128, 512, 1024), (1000, 64, 128), (257, 192, 64),
                                   (12800, 512, 320)])
@pytest.mark.parametrize("act", [None, "relu"])
def test_gemm_bf16_nt(ops, M, N, K, act):
    a = bf_round(seeded.seeded_array((M, K), 221))
    b = bf_round(seeded.seeded_array((N, K), 222) / np.sqrt(K))   # deliberately asymmetric operands
    bias = seeded.seeded_array((N,), 223).astype(np.float32)
    c = ops.gemm_bf16_nt(gbf(a), gbf(b), g32(bias), act)
    ref = a.astype(np.float64) @ b.astype(np.float64).T + bias
    if act == "relu":
        ref = np.maximum(ref, 0)
    close_bf16("c", c, ref)


@pytest.mark.parametrize("Kd,N1,N2", [(64, 64, 64), (1000, 1024, 320), (50, 128, 64), (3600, 320, 2048), (12800, 1024, 320),
                                      (777, 8, 72)])
def test_gemm_bf16_tn(ops, Kd, N1, N2):
    a = bf_round(seeded.seeded_array((Kd, N1), 231))
    b = bf_round(seeded.seeded_array((Kd, N2), 232))
    c = ops.gemm_bf16_tn(gbf(a), gbf(b))
    ref = a.astype(np.float64).T @ b.astype(np.float64)
    close_f32("c", c, ref)
    c2 = ops.gemm_bf16_tn(gbf(a), gbf(b))
    assert torch.equal(c, c2), "split-K reduction must be bitwise reproducible"


@pytest.mark.parametrize("M,Kd,N,act", [(200, 2048, 310, "relu"), (77, 320, 510, None), (3600, 2048, 310, "relu")])
def test_linear_bf16(ops, M, Kd, N, act):
    """LinearBf16 (= the compress_v / compress_v2 projections in bf16): forward and backward against the oracle, with the
    relu gate taken from the kernel's own output on both sides."""
    Kp = ops.pad_to(Kd)
    x = bf_round(seeded.seeded_array((M, Kd), 261))
    w = bf_round(seeded.seeded_array((N, Kd), 262) / np.sqrt(Kd))
    b = (0.1 * seeded.seeded_array((N,), 263)).astype(np.float32)
    gy = bf_round(seeded.seeded_array((M, N), 264))
    xp = np.zeros((M, Kp), np.float32)
    xp[:, :Kd] = x
    xt, wt, bt = gbf(xp, True), g32(w, True), g32(b, True)
    y = ops.linear_bf16(xt, wt, bt, act)
    Np = ops.pad_to(N)
    assert y.shape == (M, Np) and y.dtype == torch.bfloat16
    close_bf16("y", y[:, :N], K.linear_act_fwd(x, w, b, act))
    assert Np == N or float(y[:, N:].detach().float().abs().max()) == 0.0
    gp = np.zeros((M, Np), np.float32)
    gp[:, :N] = gy
    y.backward(gbf(gp))
    dx, dw, db = K.linear_act_bwd(x, w, npy(y[:, :N]), gy, act)
    close_bf16("d_x", xt.grad[:, :Kd], dx)
    close_f32("d_w", wt.grad, dw)
    close_f32("d_b", bt.grad, db)


@pytest.mark.parametrize("M,Kd,N", [(200, 2048, 310), (3600, 2048, 310), (12800, 2048, 310)])
def test_linear_bf16_with_in_kernel_dropout(ops, M, Kd, N):
    """compress_v in the mixed-precision training step: the p = 0.5 input dropout (config/CoR2.py:72-75) is applied while
    the GEMM kernels stage x -- forward (NT, A operand) and weight gradient (TN, B operand) regenerate the same counter-hash
    mask, which vqa_linear_dropout_mask exports for the oracle.  The gradients land in master-shaped tensors (cropped)."""
    x = bf_round(seeded.seeded_array((M, Kd), 271))
    w = bf_round(seeded.seeded_array((N, Kd), 272) / np.sqrt(Kd))
    b = (0.1 * seeded.seeded_array((N,), 273)).astype(np.float32)
    gy = bf_round(seeded.seeded_array((M, N), 274))
    seed = 4242
    xt, wt, bt = gbf(x), g32(w, True), g32(b, True)
    y = ops.linear_bf16(xt, wt, bt, "relu", 0.5, seed)
    mask = npy(ops.linear_dropout_mask(M, Kd, 0.5, seed, dev()))
    assert set(np.unique(mask).tolist()) == {0.0, 2.0} and abs(mask.mean() - 1.0) < 0.02
    xd = x.astype(np.float64) * mask
    Np = ops.pad_to(N)
    close_bf16("y", y[:, :N], K.linear_act_fwd(xd, w, b, "relu"))
    assert float(y[:, N:].detach().float().abs().max()) == 0.0
    gp = np.zeros((M, Np), np.float32)
    gp[:, :N] = gy
    y.backward(gbf(gp))
    _, dw, db = K.linear_act_bwd(xd, w, npy(y[:, :N]), gy, "relu")
    assert wt.grad.shape == (N, Kd) and wt.grad.is_contiguous()
    close_f32("d_w", wt.grad, dw)
    close_f32("d_b", bt.grad, db)


def test_gemm_bf16_nt_gate_and_tn_groups(ops):
    """The relu gate in the NT store (zero where gate <= 0, incl. -0 and negative values) and the grouped / cropped output of
    the TN reduction (R padded ranks -> R master-shaped gradients)."""
    M, N, Kd = 300, 320, 128
    a = bf_round(seeded.seeded_array((M, Kd), 281))
    b = bf_round(seeded.seeded_array((N, Kd), 282) / np.sqrt(Kd))
    gate = bf_round(seeded.seeded_array((M, N), 283))
    gate[::7, ::3] = 0.0
    gate[1::7, 1::3] = -0.0
    c = ops.gemm_bf16_nt(gbf(a), gbf(b), gate=gbf(gate))
    ref = (a.astype(np.float64) @ b.astype(np.float64).T) * (gate > 0)
    close_bf16("gated c", c, ref)
    assert float(npy(c)[gate <= 0].__abs__().max()) == 0.0
    Kr, R, Hp, H, Lp, L = 500, 2, 256, 250, 128, 70
    ga = bf_round(seeded.seeded_array((Kr, R * Hp), 284))
    xb = bf_round(seeded.seeded_array((Kr, Lp), 285))
    outs = [torch.full((H, L), 9.0, device=dev()) for _ in range(R)]
    ops.gemm_bf16_tn(gbf(ga), gbf(xb), outs=outs, out_rows=H, out_cols=L)
    full = ga.astype(np.float64).T @ xb.astype(np.float64)
    for r in range(R):
        close_f32("group %d" % r, outs[r], full[r * Hp:r * Hp + H, :L])


def test_shadow_plan_packs_like_the_single_kernels(ops):
    """ops.ShadowPlan (one vqa_pack_many launch per step) fills the same bf16 / padded-fp32 shadows as the per-weight
    pack_bf16 launches it replaces: padded, transposed-with-offset, and fp32 bias rows."""
    w = [g32(seeded.seeded_array((10, 7), 291 + r)) for r in range(2)]
    bias = [g32(seeded.seeded_array((10,), 295 + r)) for r in range(2)]
    plan = ops.ShadowPlan()
    wp = torch.zeros(2, 16, 64, device=dev(), dtype=torch.bfloat16)
    wt = torch.zeros(64, 2 * 16, device=dev(), dtype=torch.bfloat16)
    bp = torch.zeros(2, 16, device=dev())
    for r in range(2):
        plan.add(w[r], wp, 64, 1, offset=r * 16 * 64)
        plan.add(w[r], wt, 1, 2 * 16, offset=r * 16)
        plan.add(bias[r], bp, 16, 1, offset=r * 16)
    plan.pack()
    want_p, want_t = torch.zeros_like(wp), torch.zeros_like(wt)
    for r in range(2):
        ops.pack_bf16(w[r], want_p, 0, 64, 1, zero_fill=False, offset=r * 16 * 64)
        ops.pack_bf16(w[r], want_t, 0, 1, 2 * 16, zero_fill=False, offset=r * 16)
    assert torch.equal(wp, want_p) and torch.equal(wt, want_t)
    assert torch.equal(bp[:, :10], torch.stack(bias)) and float(bp[:, 10:].abs().max()) == 0.0
    w[0].mul_(2.0)                   # the masters moved on (an optimizer step): the next pack sees it
    plan.pack()
    assert torch.equal(wp[0, :10, :7].float(), w[0].to(torch.bfloat16).float())


def test_pack_bf16(ops):
    w = seeded.seeded_array((3, 10, 7), 241).astype(np.float32)
    dst = torch.full((3, 16, 64), 7.0, device=dev(), dtype=torch.bfloat16)
    ops.pack_bf16(g32(w), dst, 16 * 64, 64, 1)
    want = np.zeros((3, 16, 64), np.float32)
    want[:, :10, :7] = bf_round(w)
    assert np.array_equal(npy(dst), want.astype(np.float64))
    # transposed with the batch axis concatenated: dst[c, b*16 + r] = w[b, r, c]
    dst_t = torch.full((8, 48), 7.0, device=dev(), dtype=torch.bfloat16)
    ops.pack_bf16(g32(w), dst_t, 16, 1, 48)
    want_t = np.zeros((8, 48), np.float32)
    for b in range(3):
        want_t[:7, b * 16:b * 16 + 10] = bf_round(w[b]).T
    assert np.array_equal(npy(dst_t), want_t.astype(np.float64))


# ----------------------------------------------------------------------------------------------- K4 in bf16
@pytest.mark.parametrize("B,N,L,H,R", [(2, 5, 20, 30, 2), (3, 36, 310, 510, 2), (2, 100, 310, 510, 2), (4, 1, 130, 510, 3),
                                       (130, 1, 64, 256, 1), (520, 3, 64, 510, 2),   # the last: the large-batch prep form
                                       (128, 100, 310, 510, 2), (17, 37, 128, 256, 2)])
@pytest.mark.parametrize("form", ["fold", "rgemm"])
def test_lowrank_bilinear_fusion_bf16(ops, B, N, L, H, R, form, monkeypatch):
    """both forms of the bf16 K4: R GEMMs (csrc/bf16_path.hip, the default: ops.K4_BF16_FORM = "rgemm") and rank-folded
    (csrc/bilinear_fold_bf16.hip, VQA_K4_BF16_FORM=fold, taken where R = 2 and N <= 128) -- against the float64 closed forms on
    bf16-rounded operands"""
    monkeypatch.setattr(ops, "K4_BF16_FORM", form)
    Lp = ops.pad_to(L)
    x = bf_round(seeded.seeded_array((B, N, L), 251))
    w1 = bf_round(seeded.seeded_array((R, H, L), 252) / np.sqrt(L))
    b1 = (0.1 * seeded.seeded_array((R, H), 253)).astype(np.float32)
    h2 = seeded.seeded_array((B, R, H), 254).astype(np.float32)
    gout = bf_round(seeded.seeded_array((B, N, H), 255))
    xp = np.zeros((B, N, Lp), np.float32)
    xp[..., :L] = x
    xt, h2t = gbf(xp, True), g32(h2, True)
    ws = [g32(w1[r], True) for r in range(R)]
    bs = [g32(b1[r], True) for r in range(R)]
    out = ops.lowrank_bilinear_fusion(xt, h2t, ws, bs)
    Hp = ops.pad_to(H, 256)
    assert out.shape == (B, N, Hp) and out.dtype == torch.bfloat16
    ref, _ = K.lowrank_bilinear_fusion_fwd(x, w1, b1, h2)
    # (fold: the per-sample weight sum_r h2_r W1_r is itself rounded to bf16 before the product -- L rounding errors of 2^-9
    #  relative, averaging out to ~1e-4..1e-3 of the output's scale; the R-GEMM form rounds the output only)
    close_bf16("out", out[..., :H], ref, extra=2e-3 if form == "fold" else RTOL_F32)
    assert Hp == H or float(out[..., H:].detach().float().abs().max()) == 0.0, "pad columns must be exactly zero"
    gp = np.zeros((B, N, Hp), np.float32)
    gp[..., :H] = gout
    out.backward(gbf(gp))
    dx, dw1, db1, dh2 = K.lowrank_bilinear_fusion_bwd(x, w1, b1, h2, gout)
    close_f32("d_x", xt.grad[..., :L], dx, RTOL_MID)
    assert Lp == L or float(xt.grad[..., L:].float().abs().max()) == 0.0
    close_f32("d_h2", h2t.grad, dh2, RTOL_MID)
    for r in range(R):
        close_f32("d_w1[%d]" % r, ws[r].grad, dw1[r], RTOL_MID)
        close_f32("d_b1[%d]" % r, bs[r].grad, db1[r], RTOL_MID)


@pytest.mark.parametrize("form", ["fold", "rgemm"])
def test_lowrank_bilinear_fusion_bf16_gated_and_prepacked(ops, form, monkeypatch):
    """K4 bf16 with the shadows handed over by a ShadowPlan and the relu gate of the layer in front applied in the store of
    the data gradient: same outputs / weight gradients, d_x = (x > 0) * d_x."""
    monkeypatch.setattr(ops, "K4_BF16_FORM", form)
    B, N, L, H, R = 3, 36, 310, 510, 2
    Lp, Hp = ops.pad_to(L), ops.pad_to(H, 256)
    x = np.maximum(bf_round(seeded.seeded_array((B, N, L), 351)), 0)        # a relu output: about half zeros
    w1 = bf_round(seeded.seeded_array((R, H, L), 352) / np.sqrt(L))
    b1 = (0.1 * seeded.seeded_array((R, H), 353)).astype(np.float32)
    h2 = seeded.seeded_array((B, R, H), 354).astype(np.float32)
    gout = bf_round(seeded.seeded_array((B, N, H), 355))
    xp = np.zeros((B, N, Lp), np.float32)
    xp[..., :L] = x
    ws = [g32(w1[r], True) for r in range(R)]
    bs = [g32(b1[r], True) for r in range(R)]
    plan = ops.ShadowPlan()
    w1p = torch.zeros(R, Hp, Lp, device=dev(), dtype=torch.bfloat16)
    b1p = torch.zeros(R, Hp, device=dev())
    w1t = torch.zeros(Lp, R * Hp, device=dev(), dtype=torch.bfloat16)
    for r in range(R):
        plan.add(ws[r].detach(), w1p, Lp, 1, offset=r * Hp * Lp)
        plan.add(bs[r].detach(), b1p, Hp, 1, offset=r * Hp)
        plan.add(ws[r].detach(), w1t, 1, R * Hp, offset=r * Hp)
    plan.pack()
    xt, h2t = gbf(xp, True), g32(h2, True)
    out = ops.lowrank_bilinear_fusion(xt, h2t, ws, bs, gate_dx=True, packed=(w1p, b1p, w1t))
    ref, _ = K.lowrank_bilinear_fusion_fwd(x, w1, b1, h2)
    close_bf16("out", out[..., :H], ref, extra=2e-3 if form == "fold" else RTOL_F32)
    gp = np.zeros((B, N, Hp), np.float32)
    gp[..., :H] = gout
    out.backward(gbf(gp))
    dx, dw1, db1, dh2 = K.lowrank_bilinear_fusion_bwd(x, w1, b1, h2, gout)
    close_f32("d_x", xt.grad[..., :L], dx * (x > 0), RTOL_MID)
    assert float(npy(xt.grad[..., :L])[x <= 0].__abs__().max()) == 0.0
    close_f32("d_h2", h2t.grad, dh2, RTOL_MID)
    for r in range(R):
        assert ws[r].grad.shape == (H, L)
        close_f32("d_w1[%d]" % r, ws[r].grad, dw1[r], RTOL_MID)
        close_f32("d_b1[%d]" % r, bs[r].grad, db1[r], RTOL_MID)


def test_lowrank_bilinear_fusion_bf16_rejects_unpadded(ops):
    from vqa_playground_pytorch_amd._lib import VqaLibraryError
    x = torch.zeros(2, 3, 310, device=dev(), dtype=torch.bfloat16)
    h2 = torch.zeros(2, 1, 510, device=dev())
    w = torch.zeros(510, 310, device=dev())
    b = torch.zeros(510, device=dev())
    with pytest.raises((ValueError, VqaLibraryError)):
        ops.lowrank_bilinear_fusion(x, h2, [w], [b])


# ----------------------------------------------------------------------------------------------- CoR2 head in bf16
RTOL_MODEL = 1e-2   # bf16-compute logits / attention maps against the fp32 oracle, relative to the tensor's own scale:
#                     the region side passes through ~6 bf16 roundings (2^-8 each) between v and the pooled features
#                     (measured: 1.5e-3 on the logits)
GRAD_RELF = 0.15    # parameter gradients, relative Frobenius error.  Not a rounding-sized number: a bf16 rounding flips
GRAD_COS = 0.99     # the relu gate of the few units whose pre-activation sits within 2^-8 of zero, and a gradient that
#                     is a sum over ~M/2 active units with random signs moves by ~sqrt(2 * flipped fraction) -- 3..8 %
#                     measured, at varying parameters from run to run -- while staying aligned (cosine >= 0.99).  The
#                     kernels' own backward parity (same gates on both sides) is pinned at 2e-2 / 2e-4 above.


def _build_cor2(nans, **kw):
    from vqa_playground_pytorch_amd import CoR2Model
    return seeded.load_state(CoR2Model(["PAD", "UNK"], nans, **kw), 0).eval().to(dev())


@pytest.mark.parametrize("B,N", [(2, 100), (3, 36)])
@pytest.mark.parametrize("gemm", ["engine", "library"])
def test_cor2_bf16_against_fp32_oracle(B, N, gemm):
    """BASELINE configs[4] (bf16 compute, fp32 accumulate, fp32 master weights, N=100 dense regions): the reference
    hard-codes fp32 and 36 regions, so the fp32 CPU oracle is the checker, at a tolerance stated for bf16."""
    from oracle import reference_faithful as RF
    from vqa_playground_pytorch_amd import layers
    nans = 500
    old = layers.MyConv1d.bf16_gemm
    layers.MyConv1d.bf16_gemm = gemm
    try:
        model = _build_cor2(nans, compute_dtype=torch.bfloat16)
        oracle = seeded.load_state(RF.CoR2Oracle(nans), 0).eval()
        v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=78)
        got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
        want = oracle({"v": torch.from_numpy(v), "q": torch.from_numpy(q)})
        assert got.dtype == torch.float32 and got.shape == (B, nans)
        close_f32("logits", got, want.detach().numpy(), RTOL_MODEL)
        ad = model.alpha_dict
        close_f32("alpha1", torch.cat(ad["alpha1"], 2), torch.cat(oracle.alpha_dict["alpha1"], 2).detach().numpy(), RTOL_MODEL)
        close_f32("alpha2", torch.cat(ad["alpha2"], 2), torch.cat(oracle.alpha_dict["alpha2"], 2).detach().numpy(), RTOL_MODEL)
        RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
        RF.kld_sum_loss(want, torch.from_numpy(a)).backward()
        for (n, p), (_, po) in zip(model.named_parameters(), oracle.named_parameters()):
            assert p.grad.dtype == torch.float32 and p.grad.shape == p.shape, n
            ref = po.grad.numpy().astype(np.float64)
            if np.sqrt((ref ** 2).sum()) < 1e-6:     # mathematically-zero gradients (biases in front of the softmax)
                continue
            got_g = npy(p.grad)
            err = np.sqrt(((got_g - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum())
            cos = (got_g * ref).sum() / np.sqrt((got_g ** 2).sum() * (ref ** 2).sum())
            assert err <= GRAD_RELF and cos >= GRAD_COS, "%s: relative Frobenius error %.3e, cosine %.5f" % (n, err, cos)
    finally:
        layers.MyConv1d.bf16_gemm = old


RTOL_AWARE = 4e-2     # against the bf16-AWARE oracle (oracle/mixed_precision.py: the same tensors rounded to bf16 at the same
#                       points, forward and backward): logits / attention maps on their scale, and the relative Frobenius
#                       error of every parameter gradient once the rows hit by a flipped gate are set aside (below)
RTOL_AWARE_MAX = 1e-1  # largest element of that error on the tensor's own scale
RTOL_AWARE_ALL = 1e-1  # relative Frobenius error of the WHOLE gradient tensor, flipped gates included (one flipped unit of a
#                       155-unit glimpse layer alone: 4.8e-2)
# What is left between the two sides is fp32-vs-float64 accumulation straddling a bf16 rounding boundary or a relu gate -- and
# bf16 rounding AMPLIFIES it: an fp32-sized difference (1e-7) in the question-side factors flips the rounding of a few fusion
# outputs by one bf16 step (4e-3), which moves the attention maps and t = q1 * pooled by ~1e-5, which flips the rounding of
# ~0.25 % of the relation tensor's elements, which decides ~1e-4 of compress_v2's relu gates the other way.  So WHICH gates
# differ -- and with them 1-2 % of a weight gradient -- depends on the fp32 summation order of the [B,.] layers, i.e. on the
# kernel build and the head form.  Measured over this round's builds (the grouped GEMM's contraction order and split counts
# changed several times; same inputs, same comparison, B = 128, N = 100): worst tensor compress_v2.weight or a 155-unit
# glimpse layer, Frobenius 0.8e-2 / 1.2e-2 / 1.9e-2 / 2.3e-2 / 2.6e-2 (in the last build every parameter behind the relation step
# sits at 1.8-2.6e-2: the flipped compress_v2 gates reach them all), max-abs 6.7e-2 ... 4.1e-1 when one sample's whole
# contribution to a glimpse unit flips.  The bar leaves that spread 1.5 x of room.  A flipped gate moves ONE row (output unit) of a weight gradient: the element-wise bars
# are applied with the rows holding the largest 1 % of the squared error set aside, the whole tensor is bounded separately.


def _gradient_error(g, ref):
    """-> (max-abs on the tensor's scale and relative Frobenius error without the worst 1 % of the rows, whole-tensor
    relative Frobenius error).  Rows = the first axis (output units; a bias: one element per unit)."""
    err = g - ref
    rows = (err.reshape(err.shape[0], -1) ** 2).sum(1)
    norm = np.sqrt((ref ** 2).sum())
    kept = err[np.argsort(rows)[:-max(1, (len(rows) + 99) // 100)]]
    return np.abs(kept).max() / np.abs(ref).max(), np.sqrt((kept ** 2).sum()) / norm, np.sqrt(rows.sum()) / norm


@pytest.mark.parametrize("B,N,k4_form", [(128, 100, "rgemm"), (16, 36, "rgemm"), (128, 100, "fold")])
def test_cor2_bf16_at_size_against_bf16_aware_oracle(B, N, k4_form, monkeypatch):
    """BASELINE configs[4] at the size it is benchmarked at -- one rank's share of batch 1024: B = 128 samples of 100 x 2048
    regions, bf16 compute -- eval mode: logits, attention maps and EVERY parameter gradient against the bf16-aware
    restatement at RTOL_AWARE (relative Frobenius; RTOL_AWARE_MAX bounds the largest single element).  The comparison with
    the plain fp32 oracle (test_cor2_bf16_against_fp32_oracle) needs cosine / 15 % Frobenius bars for the same tensors:
    there every relu gate a bf16 rounding flips counts as error."""
    from oracle import mixed_precision as MP
    from oracle import reference_faithful as RF
    from vqa_playground_pytorch_amd import ops as ops_mod
    # k4_form: the product's K4 in its default R-GEMM form, and rank-folded (VQA_K4_BF16_FORM=fold; the restatement rounds the
    # per-sample folded weight where that form does)
    monkeypatch.setattr(ops_mod, "K4_BF16_FORM", k4_form)
    nans = 2000
    model = _build_cor2(nans, compute_dtype=torch.bfloat16)
    aware = seeded.load_state(MP.CoR2MixedOracle(nans, k4_form=k4_form), 0).eval().double()
    v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=1024)
    got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    assert got.dtype == torch.float32 and got.shape == (B, nans)
    RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    want = []
    for lo in range(0, B, 32):                 # float64 on the CPU, 32 samples at a time; the loss is a sum over samples
        w = aware({"v": torch.from_numpy(v[lo:lo + 32]).double(), "q": torch.from_numpy(q[lo:lo + 32]).double()})
        RF.kld_sum_loss(w, torch.from_numpy(a[lo:lo + 32]).double()).backward()
        want.append(w.detach())
        if lo == 0:
            alpha2 = torch.cat(aware.alpha_dict["alpha2"], 2).detach().numpy()
    want = torch.cat(want).numpy()
    close_f32("logits", got, want, RTOL_AWARE)
    k = min(B, 32)
    close_f32("alpha2", torch.cat(model.alpha_dict["alpha2"], 2)[:k], alpha2[:k], RTOL_AWARE)
    worst = (0.0, 0.0, "")
    params = dict(model.named_parameters())
    zero_grads = {"%s.list_linear1.%d.linear.bias" % (f, r) for f in ("fusion_vq1", "fusion_vq2") for r in range(2)} | \
        {"att1.conv_att.conv.bias", "att2.conv_att.conv.bias"}
    for (n, p), (_, po) in zip(model.named_parameters(), aware.named_parameters()):
        ref = po.grad.numpy().astype(np.float64)
        g = npy(p.grad)
        assert np.isfinite(g).all(), n
        scale = np.abs(ref).max()
        if n in zero_grads:
            # Mathematically zero: a bias in front of the softmax over regions shifts every region's logit alike.  In fp32
            # both sides hold ~1e-9; with bf16-rounded gradients of the fusion output the cancellation is only as exact as
            # the roundings, so each side holds its own rounding noise -- small against the gradient of the weight next to
            # it, and not comparable element by element.
            w_scale = np.abs(npy(params[n.replace(".bias", ".weight")].grad)).max()
            assert np.abs(g).max() <= 5e-2 * w_scale and scale <= 5e-2 * w_scale, (n, np.abs(g).max(), scale, w_scale)
            continue
        e_max, e_fro, e_all = _gradient_error(g, ref)
        if os.environ.get("VQA_TEST_VERBOSE"):
            print("  %-45s max-abs %.2e  Frobenius %.2e  whole %.2e" % (n, e_max, e_fro, e_all))
        assert e_max <= RTOL_AWARE_MAX and e_fro <= RTOL_AWARE and e_all <= RTOL_AWARE_ALL, \
            "%s: max-abs %.3e of scale, Frobenius %.3e (whole tensor %.3e)" % (n, e_max, e_fro, e_all)
        if e_max > worst[0]:
            worst = (e_max, e_fro, n)
    print("[cor2 bf16 B=%d N=%d] logits rel err %.2e; worst gradient: %s max-abs %.2e, Frobenius %.2e"
          % (B, N, np.abs(npy(got) - want).max() / np.abs(want).max(), worst[2], worst[0], worst[1]))


RTOL_FORCED = 1e-2       # with the product's relu gates handed to the oracle: relative Frobenius error of EVERY parameter
RTOL_FORCED_MAX = 2e-2   # gradient, whole tensor, nothing set aside / its largest element on the tensor's scale
#                          (measured on the MI355X at B = 128, N = 100: 3.1e-3 / 3.6e-3 at the worst tensor, logits 1.3e-4)
FLIP_FRACTION = 5e-4     # units per site where the oracle's own gate differs from the product's (measured: <= 6.3e-5: 123 of
FLIP_EDGE = 5e-3         # 3 968 000 compress_v2 units), and how far from zero the oracle's pre-activation may be at such a
#                          unit, in rms of the layer's pre-activations (measured: <= 4.8e-4)


@pytest.mark.parametrize("B,N", [(128, 100), (16, 36)])
def test_cor2_bf16_at_size_with_the_products_gates(B, N):
    """The same comparison with the ONE chaotic ingredient taken out.  What separates the two sides beyond rounding is the
    relu gate of units whose pre-activation sits within a bf16 rounding of zero: which way such a unit falls
    depends on the fp32 summation order of kernels upstream, and each flipped unit moves a whole row of a gradient.  Here the
    product's own decisions at the four sites a bf16 rounding reaches -- compress_v, compress_v2 (bf16 outputs) and the two
    glimpse projections (fed by attention maps that moved with them) -- are recorded in the forward and handed to the
    bf16-aware oracle (oracle/mixed_precision.py: forced_gates), which reports where its own gates differ.  Asserted:
      * the two sides differ at <= FLIP_FRACTION of a site's units, and only at knife-edge units (the oracle's |pre-activation|
        <= FLIP_EDGE of the layer's rms) -- a wrong gate in the product (a mis-cropped pad row, a wrong tile) would show here;
      * with the gates equal, logits and EVERY parameter gradient agree as whole tensors at RTOL_FORCED (relative Frobenius)
        and RTOL_FORCED_MAX (largest element), NO rows set aside."""
    from oracle import mixed_precision as MP
    from oracle import reference_faithful as RF
    nans = 2000
    model = _build_cor2(nans, compute_dtype=torch.bfloat16)
    aware = seeded.load_state(MP.CoR2MixedOracle(nans), 0).eval().double()
    v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=1024)
    gates = {}
    hooks = [getattr(model, site).register_forward_hook(
        lambda mod, args, out, site=site: gates.__setitem__(site, (out[..., :mod.out_channels] > 0).cpu()))
        for site in ("compress_v", "compress_v2")]
    for site in ("att1", "att2"):      # the glimpse projections run inside attend(): wrap it
        att = getattr(model, site)
        inner = att.attend

        def attend(*args, _inner=inner, _site=site, **kw):
            res = _inner(*args, **kw)
            gates[_site + ".glimpses"] = (res[0] > 0).cpu()
            return res
        att.attend = attend
    try:
        got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
    finally:
        for h in hooks:
            h.remove()
        for site in ("att1", "att2"):
            del getattr(model, site).attend
    assert set(gates) == {"compress_v", "compress_v2", "att1.glimpses", "att2.glimpses"}
    RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    want, flips = [], {}
    for lo in range(0, B, 32):                 # float64 on the CPU, 32 samples at a time; the loss is a sum over samples
        w = aware({"v": torch.from_numpy(v[lo:lo + 32]).double(), "q": torch.from_numpy(q[lo:lo + 32]).double(),
                   "forced_gates": {k: g[lo:lo + 32] for k, g in gates.items()}})
        RF.kld_sum_loss(w, torch.from_numpy(a[lo:lo + 32]).double()).backward()
        want.append(w.detach())
        for site, (n, units, edge) in aware.gate_flips.items():
            f = flips.get(site, (0, 0, 0.0))
            flips[site] = (f[0] + n, f[1] + units, max(f[2], edge))
    for site, (n, units, edge) in flips.items():
        print("  gates %-14s differ at %d of %d units (%.1e), largest |pre| / rms there %.1e" % (site, n, units, n / units, edge))
        assert n <= FLIP_FRACTION * units and edge <= FLIP_EDGE, (site, n, units, edge)
    want = torch.cat(want).numpy()
    close_f32("logits", got, want, RTOL_FORCED)
    zero_grads = {"%s.list_linear1.%d.linear.bias" % (f, r) for f in ("fusion_vq1", "fusion_vq2") for r in range(2)} | \
        {"att1.conv_att.conv.bias", "att2.conv_att.conv.bias"}
    worst = (0.0, 0.0, "")
    for (n, p), (_, po) in zip(model.named_parameters(), aware.named_parameters()):
        if n in zero_grads:       # (mathematically zero: held to their weight's scale by the test above)
            continue
        ref, g = po.grad.numpy().astype(np.float64), npy(p.grad).astype(np.float64)
        e_fro = np.sqrt(((g - ref) ** 2).sum()) / np.sqrt((ref ** 2).sum())
        e_max = np.abs(g - ref).max() / np.abs(ref).max()
        if os.environ.get("VQA_TEST_VERBOSE"):
            print("  %-45s max-abs %.2e  Frobenius %.2e" % (n, e_max, e_fro))
        assert e_fro <= RTOL_FORCED and e_max <= RTOL_FORCED_MAX, "%s: Frobenius %.3e, max-abs %.3e of scale" % (n, e_fro, e_max)
        if e_fro > worst[1]:
            worst = (e_max, e_fro, n)
    print("[cor2 bf16 B=%d N=%d, gates forced] logits rel err %.2e; worst gradient: %s Frobenius %.2e, max-abs %.2e"
          % (B, N, np.abs(npy(got) - want).max() / np.abs(want).max(), worst[2], worst[1], worst[0]))


def _compare_gradients(model, aware, tag, dropout=False, rtol_fro=None, rtol_max=None):
    """Every parameter gradient of `model` against `aware`'s at RTOL_AWARE (relative Frobenius) / RTOL_AWARE_MAX (largest
    element on the tensor's scale); the mathematically-zero bias gradients on their weight's scale.  -> worst (max, fro, name)
    Zero by construction: the bias of the logits convolution (a per-glimpse shift of every region's logit, which the softmax
    over regions cancels) and -- only without dropout between the fusion and that convolution -- the fusion's own biases."""
    rtol_fro = RTOL_AWARE if rtol_fro is None else rtol_fro
    rtol_max = RTOL_AWARE_MAX if rtol_max is None else rtol_max
    worst = (0.0, 0.0, "")
    params = dict(model.named_parameters())
    zero_grads = {"att1.conv_att.conv.bias", "att2.conv_att.conv.bias"}
    if not dropout:
        zero_grads |= {"%s.list_linear1.%d.linear.bias" % (f, r) for f in ("fusion_vq1", "fusion_vq2") for r in range(2)}
    for (n, p), (_, po) in zip(model.named_parameters(), aware.named_parameters()):
        ref = po.grad.numpy().astype(np.float64)
        g = npy(p.grad)
        assert np.isfinite(g).all(), n
        scale = np.abs(ref).max()
        if n in zero_grads:
            w_scale = np.abs(npy(params[n.replace(".bias", ".weight")].grad)).max()
            assert np.abs(g).max() <= 5e-2 * w_scale and scale <= 5e-2 * w_scale, (tag, n, np.abs(g).max(), scale, w_scale)
            continue
        e_max, e_fro, e_all = _gradient_error(g, ref)
        assert e_max <= rtol_max and e_fro <= rtol_fro and e_all <= RTOL_AWARE_ALL, \
            "%s %s: max-abs %.3e of scale, Frobenius %.3e (whole tensor %.3e)" % (tag, n, e_max, e_fro, e_all)
        if e_max > worst[0]:
            worst = (e_max, e_fro, n)
    return worst


@pytest.mark.parametrize("B,N", [(128, 100)])
def test_cor2_bf16_training_step_with_shared_masks_at_size(B, N):
    """configs[4] as it is benchmarked -- B = 128 x 100 regions, bf16 compute, TRAINING mode, dropout 0.5 at all nineteen
    Drop* layers -- against the bf16-aware restatement fed the SAME masks.  Every mask of the HIP path is a pure function of
    (seed, element index): the test records the seeds the forward draws (nine call sites), rebuilds each mask with
    vqa_linear_dropout_mask, switches the restatement's own F.dropout off and multiplies each layer's input by the mask of its
    site (the 1x1-convolution sites through sample["site_masks"], the linear layers by forward pre-hooks).  Covers what the
    eval-mode test at this size cannot: dropout inside the bf16 NT / TN GEMMs (compress_v), the dropped relation tensor
    written for compress_v2, the pooled glimpses masked inside K3 and inside the relation map, backward regenerating the masks."""
    from oracle import mixed_precision as MP
    from oracle import reference_faithful as RF
    from vqa_playground_pytorch_amd import head, ops
    if head.MODE == "legacy":
        pytest.skip("the question-side masks are reported by the grouped head's spy (default / VQA_HEAD=grouped)")
    nans = 2000
    model = _build_cor2(nans, compute_dtype=torch.bfloat16).train()
    v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=2048)
    seeds, rec, orig = [], [], {}
    for name in ("next_dropout_seed", "linear_bf16", "attention_logits", "softmax_attention_pool_drop", "relation_apply"):
        orig[name] = getattr(ops, name)

    def next_seed():
        seeds.append(orig["next_dropout_seed"]())
        return seeds[-1]

    def site(kind, rows, cols, p_drop, seed, shape):
        if p_drop:
            rec.append((kind, ops.linear_dropout_mask(rows, cols, p_drop, seed, dev()).view(shape)))

    def spy_linear_bf16(x, w, bias=None, act=None, p_drop=0.0, seed=0, **kw):
        site("linear_bf16", x.numel() // x.shape[-1], x.shape[-1], p_drop, seed, tuple(x.shape))
        return orig["linear_bf16"](x, w, bias, act, p_drop, seed, **kw)

    def spy_attention_logits(x, w, bias, p_drop=0.0, seed=0):
        K = w.shape[-1]                          # the mask is indexed over the layer's own width, not x's padded one
        site("attention_logits", x.numel() // x.shape[-1], K, p_drop, seed, tuple(x.shape[:-1]) + (K,))
        return orig["attention_logits"](x, w, bias, p_drop, seed)

    def spy_pool_drop(logits, inputs, p_drop, seed, *rest):
        site("pool_drop", inputs.shape[0] * logits.shape[2], inputs.shape[2], p_drop, seed, (inputs.shape[0], logits.shape[2], inputs.shape[2]))
        return orig["softmax_attention_pool_drop"](logits, inputs, p_drop, seed, *rest)

    def spy_relation_apply(x, t, c2, p_drop=0.0, seed=0):
        site("relation_apply", x.numel() // x.shape[-1], x.shape[-1], p_drop, seed, tuple(x.shape))
        return orig["relation_apply"](x, t, c2, p_drop, seed)

    spies = {"next_dropout_seed": next_seed, "linear_bf16": spy_linear_bf16, "attention_logits": spy_attention_logits,
             "softmax_attention_pool_drop": spy_pool_drop, "relation_apply": spy_relation_apply}
    for name, f in spies.items():
        setattr(ops, name, f)
    head._mask_spy = lambda s_, rows, cols, p_, seed: rec.append(("head:" + s_, ops.linear_dropout_mask(rows, cols, p_, seed, dev())))
    try:
        torch.manual_seed(7)
        got = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())})
        RF.kld_sum_loss(got, torch.from_numpy(a).to(dev())).backward()
    finally:
        head._mask_spy = None
        for name, f in orig.items():
            setattr(ops, name, f)
    kinds = [k for k, _ in rec]
    assert kinds == ["head:question_in", "head:question_out", "linear_bf16", "attention_logits", "pool_drop", "relation_apply",
                     "attention_logits", "relation_apply", "head:fusion_out"], kinds
    assert len(set(seeds)) == len(seeds) == len(rec)
    m = [t.cpu() for _, t in rec]
    for t in m:     # keep rate 1/2 within four standard deviations of the mask's size
        assert set(torch.unique(t).tolist()) == {0.0, 2.0} and abs(float(t.mean()) - 1.0) < 4.0 / t.numel() ** 0.5
    m[0], m[1] = m[0].view(4, B, 2400), m[1].view(2, B, 310)
    assert m[2].shape == (B, N, 2048) and m[3].shape == (B, N, 510) and m[4].shape == (B, 4, 2048) and m[5].shape == (B, N, 2048) \
        and m[6].shape == (B, N, 510) and m[7].shape == (B, 4, 2048) and m[8].shape == (B, 510)
    lin = {"compress_q": m[0][0], "linear_q": m[0][1], "compress_q_1": m[0][2], "compress_q_2": m[0][3],
           "expand_q_1": m[1][0], "expand_q_2": m[1][1], "linear_classif": m[8]}
    for g in range(4):
        lin["att1.list_linear_v_fusion.%d" % g] = m[4][:, g]
        lin["att2.list_linear_v_fusion.%d" % g] = m[7][:, g]
    conv = {"compress_v": m[2], "att1.conv_att": m[3], "compress_v2": m[5], "att2.conv_att": m[6]}

    aware = seeded.load_state(MP.CoR2MixedOracle(nans), 0).train().double()
    rng = [0, 0]
    sites = 0
    for name, mod in aware.named_modules():
        if isinstance(mod, RF.DropLinear) and mod.p:
            assert mod.p == 0.5 and name in lin, name
            mod.p = None                                  # (its own F.dropout off: the hook masks the site's input)
            mod.register_forward_pre_hook(lambda _m, args, name=name: (args[0] * lin[name][rng[0]:rng[1]].double(),))
            sites += 1
    assert sites == len(lin) == 15
    want = []
    for lo in range(0, B, 32):                 # float64 on the CPU, 32 samples at a time; the loss is a sum over samples
        rng[0], rng[1] = lo, lo + 32
        w = aware({"v": torch.from_numpy(v[lo:lo + 32]).double(), "q": torch.from_numpy(q[lo:lo + 32]).double(),
                   "site_masks": {k: t[lo:lo + 32].double() for k, t in conv.items()}})
        RF.kld_sum_loss(w, torch.from_numpy(a[lo:lo + 32]).double()).backward()
        want.append(w.detach())
    want = torch.cat(want).numpy()
    close_f32("logits (training)", got, want, RTOL_AWARE)
    # With dropout a kept activation carries the factor 1/(1-p) = 2, so the one relu gate that fp32 and float64 accumulation
    # decide differently moves its row of a weight gradient twice as far as in eval mode: the max-abs bar is the eval test's
    # doubled, the Frobenius bar 1.5 x (measured with the flipped rows aside: 0.9e-2 ... 1.2e-2).
    worst = _compare_gradients(model, aware, "train", dropout=True, rtol_fro=1.5 * RTOL_AWARE, rtol_max=2 * RTOL_AWARE_MAX)
    print("[cor2 bf16 train B=%d N=%d] logits rel err %.2e; worst gradient: %s max-abs %.2e, Frobenius %.2e"
          % (B, N, np.abs(npy(got) - want).max() / np.abs(want).max(), worst[2], worst[0], worst[1]))


def test_cor2_bf16_train_steps():
    """Three optimiser steps in bf16 compute (train mode, dropout on): finite, and the eval loss on the training batch
    goes down -- the fp32 master weights really receive the bf16-path gradients."""
    from oracle import reference_faithful as RF
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    torch.manual_seed(3)
    model = _build_cor2(300, compute_dtype=torch.bfloat16)
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(8, regions=100, answers=300, seed=31))
    batch = {"v": v.to(torch.bfloat16), "q_idxes": q}
    with torch.no_grad():
        before = RF.kld_sum_loss(model(batch), a).item()
    tr = DataParallelTrainer(model.train(), lr=1e-3, clip=0.25)
    for _ in range(3):
        loss, norm = tr.step(batch, a)
        assert torch.isfinite(loss) and torch.isfinite(norm)
    with torch.no_grad():
        after = RF.kld_sum_loss(model.eval()(batch), a).item()
    assert after < before, (before, after)


@pytest.mark.parametrize("B,N", [(8, 100), (40, 36)])
def test_cor2_bf16_pairwise_relation_trains(B, N):
    """bf16 compute with the pairwise relation kernel (relation_mode=0) in TRAIN mode: compress_v2 then reads a tensor
    that needs a gradient (through q_gate_1 / q_gate_2 / alpha1), so its input dropout cannot be the in-kernel mask of
    ops.LinearBf16 (no data gradient there) -- the layer drops beforehand.  Regression of round 3 (the backward raised).
    Every parameter receives a finite gradient, and in eval mode the step agrees with relation_mode=1's (same function)."""
    from oracle import reference_faithful as RF
    torch.manual_seed(11)
    v, q, a = (torch.from_numpy(x).to(dev()) for x in seeded.seeded_inputs(B, regions=N, answers=300, seed=17))
    batch = {"v": v.to(torch.bfloat16), "q_idxes": q}
    grads = {}
    for mode in (0, 1):
        model = _build_cor2(300, compute_dtype=torch.bfloat16, relation_mode=mode)
        model.train()
        RF.kld_sum_loss(model(batch), a).backward()
        for n, p in model.named_parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all(), (mode, n)
            assert float(p.grad.abs().max()) > 0 or "conv_att.conv.bias" in n, (mode, n)
        model.zero_grad(set_to_none=True)
        model.eval()
        logits = model(batch)
        RF.kld_sum_loss(logits, a).backward()
        grads[mode] = (npy(logits), {n: npy(p.grad) for n, p in model.named_parameters()})
    np.testing.assert_allclose(grads[0][0], grads[1][0], rtol=0, atol=RTOL_MODEL * np.abs(grads[1][0]).max())
    for n, g1 in grads[1][1].items():
        g0 = grads[0][1][n]
        # mathematically zero in eval mode (a per-glimpse constant in front of the softmax over regions): rounding noise on
        # both sides
        zero = n.endswith("conv_att.conv.bias") or (n.startswith(("fusion_vq1.list_linear1", "fusion_vq2.list_linear1"))
                                                    and n.endswith(".bias"))
        if zero or np.sqrt((g1 ** 2).sum()) < 1e-6:
            continue
        err = np.sqrt(((g0 - g1) ** 2).sum()) / np.sqrt((g1 ** 2).sum())
        assert err <= GRAD_RELF, "%s: relation_mode 0 vs 1 relative Frobenius error %.3e" % (n, err)
