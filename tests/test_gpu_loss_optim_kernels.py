"""Kernel-level checks of the BCE / CE loss kernels (csrc/loss.hip) and the SGD / RMSprop passes
(csrc/optimizer_sgd_rms.hip) against torch's own classes in float64 on the CPU, at the sizes where the kernels change path:
the 256-thread boundaries and the 4096-column register limit of a row, the 256-row stride of the one-workgroup total, the
float4 / scalar-tail / block boundaries of the flat optimizer pass.

Bars: 1e-5 relative on a loss and 1e-5 of the float64 gradient's maximum on d_logits (the project's restatement bar,
SURVEY 8c); 2e-6 absolute on a parameter after five optimizer steps (the bar test_fused_adam_matches_torch_adam holds Adam to)
and 1e-6 of its maximum on a state buffer."""
import numpy as np
import pytest
import torch

from kernel_harness import dev
from vqa_playground_pytorch_amd import metrics, ops

pytestmark = pytest.mark.gpu

BAR = 1e-5


# ---- the inputs and their float64 references, made once per shape -------------------------------------------------------------
_cases = {}


def loss_case(B, C):
    """logits uniform in [-15, 15]; BCE targets ~1 % non-zero in [0, 1] with an all-zero row (B > 1) and a row holding a 1.0;
    CE labels that include 0 and C - 1; the float64 loss and gradient of torch's criteria for both."""
    if (B, C) not in _cases:
        g = torch.Generator().manual_seed(1000 * B + C)
        z = (torch.rand(B, C, generator=g) * 30 - 15).float()
        a = (torch.rand(B, C, generator=g) * (torch.rand(B, C, generator=g) < 0.01)).float()
        a[0] = 0.0
        a[B - 1, C // 2] = 1.0
        labels = torch.randint(0, C, (B,), generator=g)
        labels[0] = 0
        labels[B - 1] = C - 1
        ref = {}
        zd = z.double().requires_grad_()
        torch.nn.BCELoss()(torch.sigmoid(zd), a.double()).backward()
        ref["bce"] = (torch.nn.BCELoss()(torch.sigmoid(z.double()), a.double()).item(), zd.grad.clone())
        zd = z.double().requires_grad_()
        torch.nn.CrossEntropyLoss()(zd, labels).backward()
        ref["ce"] = (torch.nn.CrossEntropyLoss()(z.double(), labels).item(), zd.grad.clone())
        _cases[(B, C)] = (z, a, labels, ref)
    return _cases[(B, C)]


@pytest.mark.parametrize("C", [1, 5, 255, 256, 257, 3000, 4096])
@pytest.mark.parametrize("B", [1, 3, 257])
def test_bce_and_ce_match_torch_in_float64(B, C, measured):
    z, a, labels, ref = loss_case(B, C)
    zg = z.to(dev())
    for kind, got in (("bce", ops.bce_mean_loss_and_grad(zg, a.to(dev()))), ("ce", ops.ce_mean_loss_and_grad(zg, labels.to(dev())))):
        loss, d = got[0].item(), got[1].cpu().double()
        want, want_d = ref[kind]
        assert np.isfinite(loss) and torch.isfinite(d).all()
        e_loss = abs(loss - want) / abs(want) if want != 0.0 else abs(loss)
        e_grad = (d - want_d).abs().max().item() / want_d.abs().max().item() if want_d.abs().max() > 0 else d.abs().max().item()
        measured("%s loss rel B=%d C=%d" % (kind, B, C), e_loss, BAR)
        measured("%s grad/max B=%d C=%d" % (kind, B, C), e_grad, BAR)
        assert e_loss <= BAR, (kind, loss, want)
        assert e_grad <= BAR, kind


def test_scale_is_the_callers():
    """The data-parallel scale: a rank holding B of 2 * B rows passes 1 / (2 * B * C) resp. 1 / (2 * B) and gets half the values."""
    z, a, labels, ref = loss_case(3, 257)
    zg = z.to(dev())
    for kind, target, scale in (("bce", a, 1.0 / (2 * 3 * 257)), ("ce", labels, 1.0 / (2 * 3))):
        fn = getattr(ops, kind + "_mean_loss_and_grad")
        loss, d = fn(zg, target.to(dev()), scale)
        want, want_d = ref[kind]
        assert abs(loss.item() - want / 2) <= BAR * abs(want / 2)
        assert (d.cpu().double() - want_d / 2).abs().max().item() <= BAR * (want_d / 2).abs().max().item()


def test_saturated_logits_stay_finite():
    """z = +-100: torch's float64 result saturates there (the clamp at -100) and is not a target; the loss and the gradient are
    finite and no gradient exceeds the scale."""
    B, C = 5, 1000
    g = torch.Generator().manual_seed(3)
    z = torch.where(torch.rand(B, C, generator=g) < 0.5, -100.0, 100.0).float()
    a = torch.rand(B, C, generator=g).float()
    a[0] = 0.0
    a[1] = 1.0
    labels = torch.randint(0, C, (B,), generator=g)
    for got, scale in ((ops.bce_mean_loss_and_grad(z.to(dev()), a.to(dev())), 1.0 / (B * C)),
                       (ops.ce_mean_loss_and_grad(z.to(dev()), labels.to(dev())), 1.0 / B)):
        loss, d = got[0].item(), got[1].cpu()
        assert np.isfinite(loss) and loss >= 0.0
        assert torch.isfinite(d).all() and d.abs().max().item() <= np.float32(scale)


def hits_case(B, C, seed):
    """logits with ties (a few distinct values), rows of NaNs, a row that is all NaN; targets with tied maxima."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randint(-3, 4, (B, C), generator=g).float()                  # heavy ties
    z[B // 2:] += torch.randn(B - B // 2, C, generator=g)                  # ... and rows without
    a = (torch.rand(B, C, generator=g) * (torch.rand(B, C, generator=g) < 0.05)).float()
    a[0] = 0.0                                                             # all tied: the target is column 0
    if B > 2:
        a[1, :] = 0.0
        a[1, C // 3] = a[1, C - 1] = 0.7                                   # tied maxima: the first one
        z[2, ::3] = float("nan")                                           # NaNs rank first
    if B > 3:
        z[3] = float("nan")
    labels = torch.randint(0, C, (B,), generator=g)
    labels[0] = 0
    labels[B - 1] = C - 1
    return z, a, labels


@pytest.mark.parametrize("B,C,k", [(1, 1, 1), (3, 5, 5), (9, 257, 5), (257, 300, 16), (7, 4096, 16)])
def test_hits_follow_the_documented_order_and_leave_the_loss_alone(B, C, k):
    z, a, labels = hits_case(B, C, 7 * B + C)
    zg = z.to(dev())
    for kind, target in (("bce", a), ("ce", labels)):
        plain = getattr(ops, kind + "_mean_loss_and_grad")(zg, target.to(dev()))
        loss, d, hits = getattr(ops, kind + "_mean_loss_and_grad_hits")(zg, target.to(dev()), k)
        # the restatement of loss.hip's order on the CPU (tests/test_metrics.py pins it to torch.topk)
        assert hits.dtype == torch.int32 and hits.cpu().tolist() == metrics.topk_hits(z, target, k).tolist(), kind
        # torch.topk itself, on the rows where it has no choice to make: no NaN and the target's logit tied with no other
        t = target if kind == "ce" else a.max(1).indices
        zt = z.gather(1, t[:, None])
        clear = ~torch.isnan(z).any(1) & ((z == zt).sum(1) == 1)
        if clear.any():
            pred = z[clear].topk(k, 1, True, True).indices
            want = [(pred[:, :j + 1] == t[clear][:, None]).any(1).sum().item() for j in range(k)]
            sub = getattr(ops, kind + "_mean_loss_and_grad_hits")(z[clear].to(dev()), target[clear].to(dev()), k)[2]
            assert sub.cpu().tolist() == want, kind
        # bitwise the loss and gradient of the entry point without hits
        assert torch.equal(loss.view(torch.int32), plain[0].view(torch.int32)), kind
        assert torch.equal(d.view(torch.int32), plain[1].view(torch.int32)), kind


def test_wrappers_refuse_bad_inputs():
    z = torch.zeros(4, 10, device=dev())
    a = torch.zeros(4, 10, device=dev())
    lab = torch.zeros(4, dtype=torch.int64, device=dev())
    with pytest.raises(ValueError):
        ops.bce_mean_loss_and_grad(z, a[:, :9])
    with pytest.raises(ValueError):
        ops.bce_mean_loss_and_grad(z, a.double())
    with pytest.raises(ValueError):
        ops.ce_mean_loss_and_grad(z, lab.int())
    with pytest.raises(ValueError):
        ops.ce_mean_loss_and_grad(z, lab[:3])
    with pytest.raises(ValueError):
        ops.ce_mean_loss_and_grad(z, lab + 10)                 # a label outside [0, C): caught on the host
    with pytest.raises(ValueError):
        ops.ce_mean_loss_and_grad(z, lab - 1)
    with pytest.raises(ValueError):
        ops.ce_mean_loss_and_grad_hits(z, lab, 11)             # k over C
    with pytest.raises(ValueError):
        ops.bce_mean_loss_and_grad(z, a, scale=0.0)
    p = torch.zeros(8, device=dev())
    with pytest.raises(ValueError):
        ops.sgd_step(p, p.clone(), torch.zeros(7, device=dev()), None, 0.1)
    with pytest.raises(ValueError):
        ops.rmsprop_step(p, p.clone().double(), p.clone(), None, 0.1)


# ---- SGD and RMSprop ----------------------------------------------------------------------------------------------------------
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 4099, 2 ** 20 + 3]
LR = 1e-3


@pytest.mark.parametrize("clip", [0.25, None])
@pytest.mark.parametrize("optim", ["sgd", "rms"])
@pytest.mark.parametrize("n", SIZES)
def test_sgd_and_rmsprop_match_torch_in_float64(n, optim, clip, measured):
    g0 = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g0)
    grad = torch.randn(n, generator=g0)
    p, state = p0.to(dev()), torch.zeros(n, device=dev())
    nc = torch.zeros(2, device=dev())
    ws = torch.empty(1024, device=dev(), dtype=torch.float64)
    ref_p = p0.double().requires_grad_()
    opt = torch.optim.SGD([ref_p], lr=LR, momentum=0.9) if optim == "sgd" else torch.optim.RMSprop([ref_p], lr=LR)
    for step in range(1, 6):
        gi = grad * step
        gd = gi.to(dev())
        ops.grad_norm_clip_coef(gd, clip if clip else 0.0, nc, ws)
        if optim == "sgd":
            ops.sgd_step(p, gd, state, nc, LR, 0.9)
        else:
            ops.rmsprop_step(p, gd, state, nc, LR, 0.99, 1e-8)
        ref_p.grad = gi.double()
        if clip:
            torch.nn.utils.clip_grad_norm_([ref_p], clip)
        opt.step()
    want_state = opt.state[ref_p]["momentum_buffer" if optim == "sgd" else "square_avg"]
    e_p = (p.cpu().double() - ref_p.detach()).abs().max().item()
    e_s = (state.cpu().double() - want_state).abs().max().item() / want_state.abs().max().item()
    measured("%s p abs n=%d clip=%s" % (optim, n, clip), e_p, 2e-6)
    measured("%s state/max n=%d clip=%s" % (optim, n, clip), e_s, 1e-6)
    assert e_p <= 2e-6
    assert e_s <= 1e-6


@pytest.mark.parametrize("optim", ["sgd", "rms"])
@pytest.mark.parametrize("n", [5, 1025, 2 ** 20 + 3])
def test_lr_from_device_memory_is_the_same_step(n, optim):
    g0 = torch.Generator().manual_seed(n + 1)
    p0, grad, s0 = torch.randn(n, generator=g0), torch.randn(n, generator=g0), torch.rand(n, generator=g0)
    nc = torch.tensor([3.0, 0.37], device=dev())                # (norm, coef): the coefficient is read from word 1
    scalars = torch.tensor([LR, 123.0], device=dev())           # word 0 is the learning rate; word 1 is not read
    out = []
    for dyn in (False, True):
        p, s, gd = p0.to(dev()), s0.to(dev()), grad.to(dev())
        if optim == "sgd":
            ops.sgd_step_dyn(p, gd, s, nc, scalars, 0.9) if dyn else ops.sgd_step(p, gd, s, nc, LR, 0.9)
        else:
            ops.rmsprop_step_dyn(p, gd, s, nc, scalars, 0.99, 1e-8) if dyn else ops.rmsprop_step(p, gd, s, nc, LR, 0.99, 1e-8)
        out.append((p, s))
        assert not torch.equal(p, p0.to(dev()))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32))
    assert torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))
