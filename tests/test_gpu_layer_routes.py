"""MyConv1d on the GPU: the route MyConv1d._route names is the op that runs.

tests/test_layer_routes.py writes the routing table out and checks it on the CPU with a stand-in tensor; this file builds, for
every form, the smallest layer and input that reach it, spies on the four ops of ops.py a route can name (calling through),
and asserts which one ran, with which activation / dropout rate / pregated flag -- and that output and gradients are finite
and of the expected shape and dtype.  What the kernels compute is pinned elsewhere (tests/test_gpu_k5_kernels.py,
tests/test_gpu_bf16_kernels.py, tests/test_gpu_region_kernels.py): K = 2 is the smallest K the K5 tests launch, 64 the smallest
padded width of the bf16 ones."""
import pytest
import torch

from kernel_harness import BF, F32, dev, ops  # noqa: F401  (ops: the fixture)
from vqa_playground_pytorch_amd.layers import MyConv1d

pytestmark = pytest.mark.gpu

FWD, PRE, ACT = "forward", "predropped", "pre_activation"
OP_OF = {"logits": "attention_logits", "k5": "linear_act", "bf16_engine": "linear_bf16", "bf16_library": "linear", "library": "linear"}
# (id, (cin, cout, af), layer attributes, x shape, x dtype, x needs grad, call, form, (act, rate in the kernel, pregated), seed
# draws, torch dropout in front, output dtype).  32 x 32 = 1024 rows: K5's threshold; 31 x 33 = 1023.
CASES = [
    ("logits-f32", (16, 2, "softmax"), {}, (2, 3, 16), F32, True, ACT, "logits", (None, 0.5, None), 1, False, F32),
    ("logits-bf16", (16, 2, "softmax"), {}, (2, 3, 16), BF, True, ACT, "logits", (None, 0.5, None), 1, False, F32),
    ("k5-rows1024", (2, 32, "relu"), {}, (32, 32, 2), F32, True, FWD, "k5", ("relu", 0.5, False), 1, False, F32),
    ("library-rows1023", (2, 32, "relu"), {}, (31, 33, 2), F32, True, FWD, "library", ("relu", None, None), 0, True, F32),
    ("bf16-engine", (64, 64, "relu"), {}, (2, 3, 64), BF, False, FWD, "bf16_engine", ("relu", 0.5, False), 1, False, BF),
    ("bf16-engine-grad", (64, 64, "relu"), {}, (2, 3, 64), BF, True, FWD, "bf16_engine", ("relu", 0.0, False), 0, True, BF),
    ("bf16-library", (64, 64, "relu"), {"bf16_gemm": "library"}, (2, 3, 64), BF, True, FWD, "bf16_library", (None, None, None), 0, True, BF),
    ("predropped-f32", (2, 32, "relu"), {"grad_pregated": True}, (32, 32, 2), F32, True, PRE, "k5", ("relu", 0.0, True), 0, False, F32),
    ("predropped-bf16", (64, 64, "relu"), {"grad_pregated": True}, (2, 3, 64), BF, True, PRE, "bf16_engine", ("relu", 0.0, True), 0, False, BF),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_the_named_route_is_the_op_that_runs(ops, monkeypatch, case):
    _, (cin, cout, af), attrs, shape, dtype, needs_grad, call, form, (act, rate, pregated), draws, dropped, out_dtype = case
    torch.manual_seed(3)
    layer = MyConv1d(cin, cout, 1, 1, p=0.5, af=af, dim=1).to(dev()).train()
    layer.fused, layer.bf16_gemm = True, "engine"      # (the knobs' defaults, whatever the environment says)
    for name, value in attrs.items():
        setattr(layer, name, value)
    x = torch.randn(shape, device=dev()).to(dtype).requires_grad_(needs_grad)

    calls, dropouts = [], []
    for name in sorted(set(OP_OF.values())):
        def spy(*args, _name=name, _real=getattr(ops, name), **kwargs):
            calls.append((_name, args, kwargs))
            return _real(*args, **kwargs)
        monkeypatch.setattr(ops, name, spy)
    real_dropout = torch.nn.functional.dropout

    def dropout_spy(t, p=0.5, training=True, inplace=False):
        dropouts.append((p, training))
        return real_dropout(t, p, training, inplace)
    monkeypatch.setattr(torch.nn.functional, "dropout", dropout_spy)

    route = layer._route(x, predropped=call == PRE, pre_activation=call == ACT)
    assert route.form == form
    before = ops.host_seed_draws
    y = layer.pre_activation(x) if call == ACT else layer(x, predropped=call == PRE)
    assert ops.host_seed_draws - before == draws
    assert dropouts == ([(0.5, True)] if dropped else [])
    assert [c[0] for c in calls] == [OP_OF[form]], [c[0] for c in calls]
    _, args, kwargs = calls[0]
    w, b = layer.conv.weight, layer.conv.bias
    if form == "logits":
        assert len(args) == 5 and not kwargs and args[0] is x and args[3] == rate and args[4] != 0
        assert args[1].data_ptr() == w.data_ptr() and args[1].shape == (cout, cin) and args[2] is b
    elif form in ("k5", "bf16_engine"):
        assert len(args) == 6 and args[2] is b and args[1].data_ptr() == w.data_ptr() and args[1].shape == (cout, cin)
        assert (args[0] is x) == (not dropped)
        assert args[3] == act and args[4] == rate and (args[5] != 0) == (draws == 1)
        assert kwargs == ({"pregated": pregated} if form == "k5" else {"pregated": pregated, "packed": None})
    elif form == "bf16_library":
        assert len(args) == 3 and not kwargs.get("act") and args[1].dtype == BF and args[1].shape == (cout, cin) and args[2].dtype == BF
    else:
        assert len(args) == 3 and kwargs == {"act": act} and args[1].data_ptr() == w.data_ptr() and args[2] is b
        assert args[0] is not x                     # the dropped copy

    assert y.shape == shape[:2] + (cout,) and y.dtype == out_dtype and bool(torch.isfinite(y.float()).all())
    if af == "relu":
        assert bool((y >= 0).all())
    y.float().sum().backward()
    torch.cuda.synchronize()
    for name, g, like in (("x", x.grad, x), ("weight", w.grad, w), ("bias", b.grad, b)):
        if like is x and not needs_grad:
            assert g is None
            continue
        assert g is not None and g.shape == like.shape and g.dtype == like.dtype and bool(torch.isfinite(g.float()).all()), name
    assert bool((w.grad != 0).any())
