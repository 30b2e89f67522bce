"""The driver's grid of criteria (KLD / BCE / CE), optimizers (adam / sgd / rms) and the scheduler switch, without a GPU:
the new C-ABI entry points exist and reject bad arguments, DataParallelTrainer.from_config applies the defaulting rules of
the reference driver (train.py:402-447, :519-548), and the CPU trainer reproduces a hand-written loop of torch's own criteria
and optimizers in the reference's order (train.py:63-86), through its checkpoints too."""
import copy
import importlib
import types

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from vqa_playground_pytorch_amd import _lib, metrics
from vqa_playground_pytorch_amd.trainer import DataParallelTrainer

NEW_SYMBOLS = ("vqa_mean_loss_workspace_bytes", "vqa_mean_loss_hits_workspace_bytes", "vqa_bce_mean_loss", "vqa_bce_mean_loss_hits",
               "vqa_ce_mean_loss", "vqa_ce_mean_loss_hits", "vqa_sgd_step", "vqa_sgd_step_dyn", "vqa_rmsprop_step",
               "vqa_rmsprop_step_dyn")
GAMMA = 0.5 ** (1 / 50000)


def test_new_symbols_are_bound_and_the_abi_version_stays():
    handle = _lib.lib()
    assert handle.vqa_version() == 14 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(handle, name), name
    assert handle.vqa_mean_loss_workspace_bytes(512) >= 512 * 4 and handle.vqa_mean_loss_workspace_bytes(0) == 0
    assert handle.vqa_mean_loss_hits_workspace_bytes(512, 5) >= 512 * 8


def test_loss_entry_points_reject_bad_arguments_without_a_gpu():
    h = _lib.lib()
    p, big = 16, 1 << 20     # never dereferenced: the checks come first
    for fn in (h.vqa_bce_mean_loss, h.vqa_ce_mean_loss):
        assert fn(p, p, p, p, 0.5, p, big, 4, 4097, None) == -2                          # C over 4096
        assert b"4097" in h.vqa_last_error()
        assert fn(p, p, p, p, 0.5, p, big, 0, 300, None) == -1                           # B = 0
        assert fn(None, p, p, p, 0.5, p, big, 4, 300, None) == -1                        # null logits
        assert fn(p, None, p, p, 0.5, p, big, 4, 300, None) == -1                        # null target / labels
        assert fn(p, p, None, p, 0.5, p, big, 4, 300, None) == -1                        # null loss
        assert fn(p, p, p, p, 0.5, None, big, 4, 300, None) == -1                        # null workspace
        assert fn(p, p, p, p, 0.5, p, 4 * 4 - 1, 4, 300, None) == -1                     # workspace too small
        assert fn(p, p, p, p, 0.0, p, big, 4, 300, None) == -1                           # scale not positive
        assert fn(p, p, p, p, 0.5, 18, big, 4, 300, None) == -2                          # misaligned workspace
    assert h.vqa_ce_mean_loss(p, 20, p, p, 0.5, p, big, 4, 300, None) == -2              # misaligned int64 labels
    for fn in (h.vqa_bce_mean_loss_hits, h.vqa_ce_mean_loss_hits):
        assert fn(p, p, p, p, p, 5, 0.5, p, big, 4, 4097, None) == -2
        assert fn(p, p, p, p, p, 5, 0.5, p, big, 0, 300, None) == -1
        assert fn(p, p, p, p, None, 5, 0.5, p, big, 4, 300, None) == -1                  # null hits
        assert fn(p, p, p, p, p, 17, 0.5, p, big, 4, 300, None) == -1                    # kmax over 16
        assert fn(p, p, p, p, p, 6, 0.5, p, big, 4, 5, None) == -1                       # kmax over C
        assert fn(p, p, p, p, p, 5, 0.5, p, 4 * 8 - 1, 4, 300, None) == -1               # workspace too small (floats + ranks)


def test_optimizer_entry_points_reject_bad_arguments_without_a_gpu():
    h = _lib.lib()
    p = 16
    calls = ((h.vqa_sgd_step, (0.1, 0.9)), (h.vqa_sgd_step_dyn, (p, 0.9)), (h.vqa_rmsprop_step, (0.1, 0.99, 1e-8)),
             (h.vqa_rmsprop_step_dyn, (p, 0.99, 1e-8)))
    for fn, tail in calls:
        assert fn(p, p, p, 0, p, *tail, None) == -1                                      # n = 0
        for hole in range(3):                                                            # null p / g / state
            args = [p, p, p]
            args[hole] = None
            assert fn(*args, 8, p, *tail, None) == -1
        for hole in range(3):                                                            # a buffer off the float4 grid
            args = [p, p, p]
            args[hole] = 20
            assert fn(*args, 8, p, *tail, None) == -2
            assert b"16-byte" in h.vqa_last_error()
    assert h.vqa_sgd_step_dyn(p, p, p, 8, p, None, 0.9, None) == -1                      # the _dyn forms need their step scalars
    assert h.vqa_rmsprop_step_dyn(p, p, p, 8, p, None, 0.99, 1e-8, None) == -1


# ---- from_config: the defaulting table ------------------------------------------------------------------------------------
class Tiny(nn.Module):       # the model of tests/test_trainer_gloo.py
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(12, 16)
        self.b = nn.Linear(16, 9)

    def forward(self, sample):
        return self.b(torch.tanh(self.a(sample["x"])))


def _cfg(**kw):
    return types.SimpleNamespace(lr=3e-3, **kw)


def _grid(tr):
    return tr.loss_kind, tr.optim_kind, tr.lr_scheduler, tr.clip


@pytest.mark.parametrize("given,expected", [
    ({}, ("KLD", "adam", True, None)),                                                   # everything missing
    ({"clip_grad": True}, ("KLD", "adam", True, 0.25)),
    ({"clip_grad": False, "optim": "sgd"}, ("KLD", "sgd", True, None)),
    ({"optim": "rms", "lr_scheduler": False}, ("KLD", "rms", False, None)),
    ({"optim": "adam", "lr_scheduler": 0}, ("KLD", "adam", False, None)),
    ({"samplingans": False, "loss_metric": "BCE"}, ("BCE", "adam", True, None)),
    ({"samplingans": False, "loss_metric": "KLD"}, ("KLD", "adam", True, None)),
    ({"samplingans": False}, ("KLD", "adam", True, None)),                                # loss_metric missing -> KLD
    ({"samplingans": True}, ("CE", "adam", True, None)),                                  # loss_metric missing -> CE
    ({"samplingans": True, "loss_metric": "KLD"}, ("CE", "adam", True, None)),            # samplingans wins
    ({"samplingans": True, "loss_metric": "BCE", "optim": "rms", "clip_grad": True}, ("CE", "rms", True, 0.25)),
])
def test_from_config_applies_the_drivers_defaults(given, expected):
    tr = DataParallelTrainer.from_config(Tiny(), _cfg(**given))
    assert _grid(tr) == expected
    assert tr.base_lr == tr.lr == 3e-3


def test_from_config_refuses_what_the_driver_refuses():
    with pytest.raises(ValueError, match="sgd has been deprecated. Please use optim"):
        DataParallelTrainer.from_config(Tiny(), _cfg(sgd=True))
    with pytest.raises(ValueError, match="sgd has been deprecated. Please use optim"):
        DataParallelTrainer.from_config(Tiny(), _cfg(sgd=False, optim="sgd"))
    with pytest.raises(ValueError, match="Optim is set adagrad"):
        DataParallelTrainer.from_config(Tiny(), _cfg(optim="adagrad"))
    with pytest.raises(ValueError, match="<train.py> loss"):
        DataParallelTrainer.from_config(Tiny(), _cfg(samplingans=False, loss_metric="MSE"))
    with pytest.raises(ValueError, match="<train.py> loss"):
        DataParallelTrainer.from_config(Tiny(), _cfg(samplingans=False, loss_metric="CE"))   # CE is reached by samplingans only
    with pytest.raises(AttributeError, match="lr must be set manually"):
        DataParallelTrainer.from_config(Tiny(), types.SimpleNamespace(optim="adam"))
    with pytest.raises(ValueError, match="Optim is set lamb"):
        DataParallelTrainer(Tiny(), optim="lamb")
    with pytest.raises(ValueError, match="<train.py> loss"):
        DataParallelTrainer(Tiny(), loss="MSE")
    # keywords override the config
    tr = DataParallelTrainer.from_config(Tiny(), _cfg(optim="sgd"), optim="rms", topk=(1, 5))
    assert tr.optim_kind == "rms" and tr.topk == (1, 5)


@pytest.mark.parametrize("name", ["CoR2", "ODA"])
def test_shipped_configs_select_the_default_cell(name):
    cf = importlib.import_module("config." + name)
    tr = DataParallelTrainer.from_config(Tiny(), cf)
    assert _grid(tr) == ("KLD", "adam", True, 0.25) and tr.base_lr == cf.lr


# ---- CPU trainer == a hand-written loop of torch's classes ---------------------------------------------------------------
def make_data(loss, steps=4, batch=8):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(steps):
        x = torch.randn(batch, 12, generator=g)
        if loss == "CE":
            a = torch.randint(0, 9, (batch,), generator=g)
        elif loss == "BCE":
            a = torch.rand(batch, 9, generator=g) * (torch.rand(batch, 9, generator=g) < 0.3)
        else:
            a = torch.softmax(torch.randn(batch, 9, generator=g), 1)
        out.append((x, a))
    return out


def criterion_of(loss):
    if loss == "CE":
        return nn.CrossEntropyLoss()
    if loss == "BCE":
        bce = nn.BCELoss()
        return lambda z, a: bce(torch.sigmoid(z), a)
    kld = nn.KLDivLoss(reduction="sum")
    return lambda z, a: kld(F.log_softmax(z, dim=1), a)


def optimizer_of(optim, params, lr):
    if optim == "sgd":
        return torch.optim.SGD(params, lr=lr, momentum=0.9)
    if optim == "rms":
        return torch.optim.RMSprop(params, lr=lr)
    return torch.optim.Adam(params, lr=lr)


def reference_loop(model, loss, optim, data, lr=1e-2, clip=0.25, scheduler=True):
    """train.py:63-86: output, loss, scheduler.step(), zero_grad, backward, clip, optimizer.step()."""
    crit = criterion_of(loss)
    opt = optimizer_of(optim, model.parameters(), lr)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, GAMMA) if scheduler else None
    out = []
    for x, a in data:
        value = crit(model({"x": x}), a)
        if sched:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")       # (scheduler before optimizer: the reference's order)
                sched.step()
        opt.zero_grad()
        value.backward()
        norm = nn.utils.clip_grad_norm_(model.parameters(), clip) if clip else None
        opt.step()
        out.append((value.item(), None if norm is None else norm.item()))
    return out, opt


@pytest.mark.parametrize("optim", ["adam", "sgd", "rms"])
@pytest.mark.parametrize("loss", ["KLD", "BCE", "CE"])
def test_cpu_trainer_equals_a_loop_of_torchs_classes(loss, optim):
    torch.manual_seed(0)
    model = Tiny()
    ref_model = copy.deepcopy(model)
    data = make_data(loss)
    tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, loss=loss, optim=optim)
    got = [tuple(t.item() for t in tr.step({"x": x}, a)) for x, a in data]
    ref, opt = reference_loop(ref_model, loss, optim, data)
    for (l, n), (rl, rn) in zip(got, ref):
        assert l == pytest.approx(rl, rel=1e-6) and n == pytest.approx(rn, rel=1e-5)
    assert tr.lr == pytest.approx(opt.param_groups[0]["lr"], rel=1e-12) == pytest.approx(1e-2 * GAMMA ** 4, rel=1e-12)
    for p, rp in zip(model.parameters(), ref_model.parameters()):
        torch.testing.assert_close(p, rp, rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize("optim", ["sgd", "rms"])
def test_without_scheduler_and_clip_the_lr_holds(optim):
    torch.manual_seed(0)
    model = Tiny()
    ref_model = copy.deepcopy(model)
    data = make_data("BCE")
    tr = DataParallelTrainer(model, lr=1e-2, clip=None, loss="BCE", optim=optim, lr_scheduler=False)
    for x, a in data:
        loss, norm = tr.step({"x": x}, a)
        assert norm is None and tr.lr == 1e-2
    assert tr.iteration == 4                                   # the iteration counter still advances
    reference_loop(ref_model, "BCE", optim, data, clip=None, scheduler=False)
    for p, rp in zip(model.parameters(), ref_model.parameters()):
        torch.testing.assert_close(p, rp, rtol=1e-5, atol=1e-7)


def test_topk_with_labels_equals_torch_topk():
    torch.manual_seed(0)
    model = Tiny()
    tr = DataParallelTrainer(model, lr=1e-2, loss="CE", optim="sgd", topk=(1, 5))
    for x, a in make_data("CE", steps=2, batch=32):
        tr.step({"x": x}, a)
        z = tr.last_logits
        pred = z.topk(5, 1, True, True).indices
        correct = pred.eq(a[:, None])
        want = [100.0 * correct[:, :k].any(1).sum().item() / 32 for k in (1, 5)]
        assert list(tr.accuracy()) == want
    # the CPU hit count takes integer classes as they are, and refuses what is neither a class list nor a [B,C] target
    z = torch.tensor([[0.0, 2.0, 1.0], [3.0, 3.0, 0.0], [float("nan"), 1.0, 5.0]])
    assert metrics.topk_hits(z, torch.tensor([1, 1, 2]), 2).tolist() == [1, 3]
    assert metrics.topk_hits(z, torch.tensor([1, 1, 2], dtype=torch.int32), 2).tolist() == [1, 3]
    with pytest.raises(ValueError):
        metrics.topk_hits(z, torch.tensor([1.0, 1.0, 2.0]), 2)


# ---- checkpoints ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optim,cls", [("sgd", torch.optim.SGD), ("rms", torch.optim.RMSprop)])
def test_optimizer_state_travels_to_torch_and_back(optim, cls):
    torch.manual_seed(0)
    model = Tiny()
    data = make_data("BCE", steps=4)
    tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, loss="BCE", optim=optim)
    for x, a in data[:3]:
        tr.step({"x": x}, a)
    sd = tr.optimizer_state_dict()
    state_key = "momentum_buffer" if optim == "sgd" else "square_avg"
    assert set(sd["state"]) == {0, 1, 2, 3} and state_key in sd["state"][0]
    group = sd["param_groups"][0]
    if optim == "sgd":
        assert (group["momentum"], group["dampening"], group["nesterov"]) == (0.9, 0, False)
    else:
        assert (group["alpha"], group["eps"], group["centered"]) == (0.99, 1e-8, False)
        step = sd["state"][0]["step"]
        assert torch.is_tensor(step) and step.dtype == torch.float32 and step.dim() == 0 and float(step) == 3.0

    # into a fresh torch optimizer over a copy of the model ...
    torch_model = copy.deepcopy(model)
    opt = cls(torch_model.parameters(), lr=1e-2, **({"momentum": 0.9} if optim == "sgd" else {}))
    opt.load_state_dict(copy.deepcopy(sd))
    # ... and from torch back into a fresh trainer
    back_model = copy.deepcopy(model)
    back = DataParallelTrainer(back_model, lr=1e-2, clip=0.25, loss="BCE", optim=optim)
    back.load_optimizer_state_dict(copy.deepcopy(opt.state_dict()))

    # a fourth step is equal on both sides.  The checkpoint does not carry the scheduler (the reference re-creates it), so
    # both sides take it at the lr of a scheduler that starts over: lr0 * gamma
    x, a = data[3]
    lr4 = 1e-2 * GAMMA
    for g in opt.param_groups:
        g["lr"] = lr4
    opt.zero_grad()
    criterion_of("BCE")(torch_model({"x": x}), a).backward()
    nn.utils.clip_grad_norm_(torch_model.parameters(), 0.25)
    opt.step()
    back.step({"x": x}, a)
    assert back.lr == pytest.approx(lr4, rel=1e-12)
    for p, rp in zip(back_model.parameters(), torch_model.parameters()):
        torch.testing.assert_close(p, rp, rtol=1e-6, atol=1e-8)


def test_a_state_dict_of_another_optimizer_is_refused():
    model = Tiny()
    dicts = {}
    for optim in ("adam", "sgd", "rms"):
        tr = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, optim=optim)
        x, a = make_data("KLD", steps=1)[0]
        tr.step({"x": x}, a)
        dicts[optim] = tr.optimizer_state_dict()
    for optim in ("adam", "sgd", "rms"):
        tr = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, optim=optim)
        for other, sd in dicts.items():
            if other == optim:
                tr.load_optimizer_state_dict(copy.deepcopy(sd))
            else:
                with pytest.raises(ValueError, match="belongs to optim"):
                    tr.load_optimizer_state_dict(copy.deepcopy(sd))


def test_reset_optimizer_recreates_the_chosen_optimizer():
    model = Tiny()
    for optim, cls in (("sgd", torch.optim.SGD), ("rms", torch.optim.RMSprop), ("adam", torch.optim.Adam)):
        tr = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, optim=optim)
        x, a = make_data("KLD", steps=1)[0]
        tr.step({"x": x}, a)
        tr.reset_optimizer(5e-3)
        assert type(tr.optimizer) is cls and not tr.optimizer.state_dict()["state"]
        assert tr.lr == 5e-3 and tr.iteration == 0
