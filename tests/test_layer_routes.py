"""The host-side routing of the region layers, the parts that need no GPU.

MyConv1d._route names the form that serves a call -- which op, which activation inside it, which dropout rate as a torch pass
in front and which inside the kernel, which torch activation behind -- from the layer's settings and five plain attributes of
the input.  ROUTES below is that decision written out by hand, one row per line of the routing rules and one per side of every
threshold; a stand-in object plays the (GPU) tensor, so nothing is launched.  tests/test_gpu_layer_routes.py holds the other
half: that the op a route names is the op that runs.

Below the table: the front that cor2.Model and oda.Model share (layers.RegionQuestionModel) -- the seq2vec slot's refusals, the
'v_len' refusals, and the state_dict names and order of both models."""
import pytest
import torch

from kernel_harness import forbid_launches
from vqa_playground_pytorch_amd import CoR2Model, ODAModel, layers, ops
from vqa_playground_pytorch_amd.layers import MyConv1d

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64


class FakeTensor:
    """what MyConv1d._route may read of its input, and nothing else"""

    def __init__(self, shape, dtype=F32, cuda=True, grad=False):
        self.shape, self.dtype, self.is_cuda, self.requires_grad = torch.Size(shape), dtype, cuda, grad

    def dim(self):
        return len(self.shape)


def X(*shape, dtype=F32, cuda=True, grad=False):
    return FakeTensor(shape, dtype, cuda, grad)


def L(cin, cout, af="relu", p=0.5, train=True, fused=True, gemm="engine"):
    return dict(cin=cin, cout=cout, af=af, p=p, train=train, fused=fused, gemm=gemm)


FWD, PRE, ACT = "forward", "predropped", "pre_activation"
# (id, layer, input, call, (form, act, drop, p, post)).  drop: the rate of the torch dropout pass in front of the op; p: the rate
# handed to the op's own in-kernel mask.  32 x 32 = 1024 rows, 31 x 33 = 1023.
ROUTES = [
    # ---- forward(x, predropped=True): bf16 form at rate 0, else K5 at rate 0, else the fp32 library GEMM; never the logits kernel
    ("pre-bf16-engine", L(64, 64), X(2, 3, 64, dtype=BF16), PRE, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("pre-bf16-engine-grad", L(64, 64), X(2, 3, 64, dtype=BF16, grad=True), PRE, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("pre-bf16-out32", L(64, 32), X(2, 3, 64, dtype=BF16), PRE, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("pre-bf16-out31", L(64, 31), X(2, 3, 64, dtype=BF16), PRE, ("bf16_library", None, 0.0, 0.0, "relu")),
    ("pre-bf16-library", L(64, 64, gemm="library"), X(2, 3, 64, dtype=BF16), PRE, ("bf16_library", None, 0.0, 0.0, "relu")),
    ("pre-bf16-tanh", L(64, 64, af="tanh"), X(2, 3, 64, dtype=BF16), PRE, ("bf16_library", None, 0.0, 0.0, "tanh")),
    ("pre-bf16-logits-shape", L(16, 2, af="softmax"), X(2, 3, 16, dtype=BF16), PRE, ("bf16_library", None, 0.0, 0.0, "softmax")),
    ("pre-k5", L(16, 32), X(32, 32, 16), PRE, ("k5", "relu", 0.0, 0.0, None)),
    ("pre-k5-grad", L(16, 32), X(32, 32, 16, grad=True), PRE, ("k5", "relu", 0.0, 0.0, None)),
    ("pre-k5-af-none", L(16, 32, af=None), X(32, 32, 16), PRE, ("k5", None, 0.0, 0.0, None)),
    ("pre-k5-rows1023", L(16, 32), X(31, 33, 16), PRE, ("library", "relu", 0.0, 0.0, None)),
    ("pre-k5-out31", L(16, 31), X(32, 32, 16), PRE, ("library", "relu", 0.0, 0.0, None)),
    ("pre-k5-fused-off", L(16, 32, fused=False), X(32, 32, 16), PRE, ("library", "relu", 0.0, 0.0, None)),
    ("pre-k5-tanh", L(16, 32, af="tanh"), X(32, 32, 16), PRE, ("library", None, 0.0, 0.0, "tanh")),
    ("pre-k5-f64", L(16, 32), X(32, 32, 16, dtype=F64), PRE, ("library", "relu", 0.0, 0.0, None)),
    ("pre-cpu", L(16, 32), X(32, 32, 16, cuda=False), PRE, ("library", None, 0.0, 0.0, "relu")),
    ("pre-logits-shape", L(16, 2, af="softmax"), X(2, 3, 16), PRE, ("library", None, 0.0, 0.0, "softmax")),
    ("pre-logits-shape-relu", L(16, 2), X(2, 3, 16), PRE, ("library", "relu", 0.0, 0.0, None)),
    # ---- forward(x).  1: bf16 input with af None / relu -> the bf16 form at p_now.  Engine: the mask is in-kernel only at 0.5 on
    # an input without gradient, any other rate is a torch pass in front
    ("fwd-bf16-p0.5", L(64, 64), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", "relu", 0.0, 0.5, None)),
    ("fwd-bf16-p0.5-grad", L(64, 64), X(2, 3, 64, dtype=BF16, grad=True), FWD, ("bf16_engine", "relu", 0.5, 0.0, None)),
    ("fwd-bf16-p0.3", L(64, 64, p=0.3), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", "relu", 0.3, 0.0, None)),
    ("fwd-bf16-p0.3-grad", L(64, 64, p=0.3), X(2, 3, 64, dtype=BF16, grad=True), FWD, ("bf16_engine", "relu", 0.3, 0.0, None)),
    ("fwd-bf16-p0", L(64, 64, p=0), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("fwd-bf16-p0-grad", L(64, 64, p=None), X(2, 3, 64, dtype=BF16, grad=True), FWD, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("fwd-bf16-eval", L(64, 64, train=False), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("fwd-bf16-eval-grad", L(64, 64, train=False), X(2, 3, 64, dtype=BF16, grad=True), FWD, ("bf16_engine", "relu", 0.0, 0.0, None)),
    ("fwd-bf16-af-none", L(64, 64, af=None), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", None, 0.0, 0.5, None)),
    ("fwd-bf16-out32", L(64, 32), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", "relu", 0.0, 0.5, None)),
    ("fwd-bf16-out31", L(64, 31), X(2, 3, 64, dtype=BF16), FWD, ("bf16_library", None, 0.5, 0.0, "relu")),
    ("fwd-bf16-library", L(64, 64, gemm="library"), X(2, 3, 64, dtype=BF16), FWD, ("bf16_library", None, 0.5, 0.0, "relu")),
    ("fwd-bf16-library-p0.3", L(64, 64, p=0.3, gemm="library"), X(2, 3, 64, dtype=BF16), FWD, ("bf16_library", None, 0.3, 0.0, "relu")),
    ("fwd-bf16-library-eval", L(64, 64, train=False, gemm="library"), X(2, 3, 64, dtype=BF16), FWD, ("bf16_library", None, 0.0, 0.0, "relu")),
    ("fwd-bf16-cpu", L(64, 64), X(2, 3, 64, dtype=BF16, cuda=False), FWD, ("bf16_engine", "relu", 0.0, 0.5, None)),
    # (af None / relu on bf16 comes before the logits kernel, whatever the shape)
    ("fwd-bf16-relu-logits-shape", L(16, 2), X(2, 3, 16, dtype=BF16), FWD, ("bf16_library", None, 0.5, 0.0, "relu")),
    # 2: K5 at p_now
    ("fwd-k5", L(16, 32), X(32, 32, 16), FWD, ("k5", "relu", 0.0, 0.5, None)),
    ("fwd-k5-grad", L(16, 32), X(32, 32, 16, grad=True), FWD, ("k5", "relu", 0.0, 0.5, None)),
    ("fwd-k5-p0.3", L(16, 32, p=0.3), X(32, 32, 16), FWD, ("k5", "relu", 0.0, 0.3, None)),
    ("fwd-k5-eval", L(16, 32, train=False), X(32, 32, 16), FWD, ("k5", "relu", 0.0, 0.0, None)),
    ("fwd-k5-p-none", L(16, 32, p=None), X(32, 32, 16), FWD, ("k5", "relu", 0.0, 0.0, None)),
    ("fwd-k5-af-none", L(16, 32, af=None), X(32, 32, 16), FWD, ("k5", None, 0.0, 0.5, None)),
    ("fwd-k5-af-empty", L(16, 32, af=""), X(32, 32, 16), FWD, ("library", None, 0.5, 0.0, "")),
    # 3: relu, fp32, cuda and no logits shape -> torch dropout, then the library GEMM with the relu in its epilogue
    ("fwd-rows1023", L(16, 32), X(31, 33, 16), FWD, ("library", "relu", 0.5, 0.0, None)),
    ("fwd-rows1023-eval", L(16, 32, train=False), X(31, 33, 16), FWD, ("library", "relu", 0.0, 0.0, None)),
    ("fwd-out31", L(16, 31), X(32, 32, 16), FWD, ("library", "relu", 0.5, 0.0, None)),
    ("fwd-fused-off", L(16, 32, fused=False), X(32, 32, 16), FWD, ("library", "relu", 0.5, 0.0, None)),
    ("fwd-relu-out9", L(16, 9), X(2, 3, 16), FWD, ("library", "relu", 0.5, 0.0, None)),
    # 4: everything else is the activation over pre_activation's route
    ("fwd-relu-out8-logits", L(16, 8), X(2, 3, 16), FWD, ("logits", None, 0.0, 0.5, "relu")),
    ("fwd-softmax-logits", L(16, 2, af="softmax"), X(2, 3, 16), FWD, ("logits", None, 0.0, 0.5, "softmax")),
    ("fwd-softmax-logits-eval", L(16, 2, af="softmax", train=False), X(2, 3, 16), FWD, ("logits", None, 0.0, 0.0, "softmax")),
    ("fwd-softmax-logits-bf16", L(16, 2, af="softmax"), X(2, 3, 16, dtype=BF16), FWD, ("logits", None, 0.0, 0.5, "softmax")),
    ("fwd-softmax-bf16-narrow", L(14, 2, af="softmax"), X(2, 3, 14, dtype=BF16), FWD, ("bf16_library", None, 0.5, 0.0, "softmax")),
    ("fwd-tanh-bf16-wide", L(64, 64, af="tanh"), X(2, 3, 64, dtype=BF16), FWD, ("bf16_engine", None, 0.0, 0.5, "tanh")),
    ("fwd-tanh-bf16-wide-grad", L(64, 64, af="tanh"), X(2, 3, 64, dtype=BF16, grad=True), FWD, ("bf16_engine", None, 0.5, 0.0, "tanh")),
    ("fwd-tanh-bf16-library", L(64, 64, af="tanh", gemm="library"), X(2, 3, 64, dtype=BF16), FWD, ("bf16_library", None, 0.5, 0.0, "tanh")),
    ("fwd-tanh", L(16, 32, af="tanh"), X(32, 32, 16), FWD, ("library", None, 0.5, 0.0, "tanh")),
    ("fwd-relu-cpu", L(16, 32), X(32, 32, 16, cuda=False), FWD, ("library", None, 0.5, 0.0, "relu")),
    ("fwd-relu-cpu-eval", L(16, 32, train=False), X(32, 32, 16, cuda=False), FWD, ("library", None, 0.0, 0.0, "relu")),
    ("fwd-relu-f64", L(16, 32), X(32, 32, 16, dtype=F64), FWD, ("library", None, 0.5, 0.0, "relu")),
    # ---- pre_activation(x): the logits kernel (K3a) at p_now wherever it takes the shape, else the bf16 form without
    # activation, else torch dropout and the library GEMM.  Never K5.
    ("act-logits", L(16, 2, af="softmax"), X(2, 3, 16), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-grad", L(16, 2, af="softmax"), X(2, 3, 16, grad=True), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-p0.3", L(16, 2, af="softmax", p=0.3), X(2, 3, 16), ACT, ("logits", None, 0.0, 0.3, None)),
    ("act-logits-eval", L(16, 2, af="softmax", train=False), X(2, 3, 16), ACT, ("logits", None, 0.0, 0.0, None)),
    ("act-logits-bf16", L(16, 2, af="softmax"), X(2, 3, 16, dtype=BF16), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-bf16-relu", L(16, 2), X(2, 3, 16, dtype=BF16), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-out8", L(16, 8, af="softmax"), X(2, 3, 16), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-out9", L(16, 9, af="softmax"), X(2, 3, 16), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-logits-in512", L(512, 4, af="softmax"), X(2, 3, 512), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-in514", L(514, 4, af="softmax"), X(2, 3, 514), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-logits-in-odd", L(15, 4, af="softmax"), X(2, 3, 16), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-logits-last-even", L(16, 4, af="softmax"), X(2, 3, 18), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-last-odd", L(16, 4, af="softmax"), X(2, 3, 17), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-logits-bf16-last-mod4", L(14, 4, af="softmax"), X(2, 3, 16, dtype=BF16), ACT, ("logits", None, 0.0, 0.5, None)),
    ("act-logits-bf16-last-mod2", L(14, 4, af="softmax"), X(2, 3, 14, dtype=BF16), ACT, ("bf16_library", None, 0.5, 0.0, None)),
    ("act-logits-cpu", L(16, 2, af="softmax"), X(2, 3, 16, cuda=False), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-logits-cpu-eval", L(16, 2, af="softmax", train=False), X(2, 3, 16, cuda=False), ACT, ("library", None, 0.0, 0.0, None)),
    ("act-bf16-engine", L(64, 64), X(2, 3, 64, dtype=BF16), ACT, ("bf16_engine", None, 0.0, 0.5, None)),
    ("act-bf16-engine-grad", L(64, 64), X(2, 3, 64, dtype=BF16, grad=True), ACT, ("bf16_engine", None, 0.5, 0.0, None)),
    ("act-bf16-engine-p0.3", L(64, 64, p=0.3), X(2, 3, 64, dtype=BF16), ACT, ("bf16_engine", None, 0.3, 0.0, None)),
    ("act-bf16-engine-eval", L(64, 64, train=False), X(2, 3, 64, dtype=BF16), ACT, ("bf16_engine", None, 0.0, 0.0, None)),
    ("act-bf16-out31", L(64, 31), X(2, 3, 64, dtype=BF16), ACT, ("bf16_library", None, 0.5, 0.0, None)),
    ("act-bf16-library", L(64, 64, gemm="library"), X(2, 3, 64, dtype=BF16), ACT, ("bf16_library", None, 0.5, 0.0, None)),
    ("act-no-k5", L(16, 32), X(32, 32, 16), ACT, ("library", None, 0.5, 0.0, None)),
    ("act-no-k5-eval", L(16, 32, train=False), X(32, 32, 16), ACT, ("library", None, 0.0, 0.0, None)),
]


def _layer(cin, cout, af, p, train, fused, gemm):
    layer = MyConv1d(cin, cout, 1, 1, p=p, af=af, dim=1)
    layer.fused, layer.bf16_gemm = fused, gemm      # (class attributes with environment defaults: assigned like the models do)
    return layer.train(train)


def _ask(layer, x, call):
    return layer._route(x, predropped=call == PRE, pre_activation=call == ACT)


@pytest.mark.parametrize("case", ROUTES, ids=lambda c: c[0])
def test_route_table(case):
    _, spec, x, call, want = case
    layer = _layer(**spec)
    draws, state = ops.host_seed_draws, torch.get_rng_state()
    got = _ask(layer, x, call)
    assert tuple(got) == want, (got, want)
    assert isinstance(got.drop, float) and isinstance(got.p, float)
    assert ops.host_seed_draws == draws and torch.equal(torch.get_rng_state(), state), "asking for a route drew a seed"


def test_route_table_reaches_every_form_from_every_call():
    ids = [c[0] for c in ROUTES]
    assert len(set(ids)) == len(ids)
    reached = {(c[3], c[4][0]) for c in ROUTES}
    assert reached == {(PRE, "bf16_engine"), (PRE, "bf16_library"), (PRE, "k5"), (PRE, "library"),
                       (FWD, "bf16_engine"), (FWD, "bf16_library"), (FWD, "k5"), (FWD, "library"), (FWD, "logits"),
                       (ACT, "bf16_engine"), (ACT, "bf16_library"), (ACT, "library"), (ACT, "logits")}


def test_a_real_cpu_tensor_takes_the_route_the_table_names():
    """the stand-in and a tensor answer alike, and running the route draws from torch's generator only where it says `drop`"""
    layer = _layer(**L(16, 32))
    x = torch.randn(2, 3, 16)
    assert tuple(layer._route(x)) == ("library", None, 0.5, 0.0, "relu")
    assert tuple(layer._route(x, predropped=True)) == ("library", None, 0.0, 0.0, "relu")
    state, draws = torch.get_rng_state(), ops.host_seed_draws
    y = layer(x, predropped=True)
    assert y.shape == (2, 3, 32) and bool((y >= 0).all()) and torch.equal(torch.get_rng_state(), state)
    assert torch.equal(layer.eval()(x), y) and torch.equal(torch.get_rng_state(), state)
    layer.train()(x)
    assert not torch.equal(torch.get_rng_state(), state) and ops.host_seed_draws == draws


@pytest.mark.parametrize("call", [FWD, PRE, ACT])
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_rank_is_checked_once_in_front_of_the_route(call, dtype, monkeypatch):
    layer = _layer(**L(16, 32))
    monkeypatch.setattr(layer, "_route", lambda *a, **k: pytest.fail("the route was asked for a tensor of the wrong rank"))
    for shape in ((6, 16), (2, 3, 1, 16)):
        x = torch.zeros(shape, dtype=dtype)
        with pytest.raises(ValueError) as err:
            layer.pre_activation(x) if call == ACT else layer(x, predropped=call == PRE)
        assert str(err.value) == "[error] putils.Conv1d(16, 32, 1, 1): input_dim (%d) should equal to 3" % len(shape)


def test_last_dimension_error_keeps_its_text():
    want = "[error] putils.Linear(7, 5): last dimension of input(6) should equal to in_features(7)"
    assert str(layers._last_dim_error(7, 5, 6)) == want
    x = torch.zeros(2, 6)
    for call in (lambda: layers.Linear(7, 5)(x), lambda: layers.MyLinear(7, 5)(x),
                 lambda: layers.MutanFusion(7, 3, 5, 2)(torch.zeros(2, 4, 6), torch.zeros(2, 3)),
                 lambda: layers.MutanFusion(3, 7, 5, 2)(torch.zeros(2, 4, 3), x)):
        with pytest.raises(ValueError) as err:
            call()
        assert str(err.value) == want


def test_rate_and_seed_helpers_draw_only_at_a_nonzero_rate():
    m = layers.MyLinear(4, 4, p=0.5)
    assert layers._rate(m) == 0.5 and layers._rate(m.eval()) == 0.0
    assert layers._rate(layers.MyLinear(4, 4, p=None)) == 0.0 and layers._rate(layers.MyLinear(4, 4, p=0)) == 0.0
    assert layers._rate(layers.Linear(4, 4)) == 0.0                     # a module without a rate of its own
    draws, state = ops.host_seed_draws, torch.get_rng_state()
    assert layers._seed(0.0) == 0 and layers._seed(0) == 0
    assert ops.host_seed_draws == draws and torch.equal(torch.get_rng_state(), state)
    torch.manual_seed(11)
    first = layers._seed(0.5)
    assert ops.host_seed_draws == draws + 1
    torch.manual_seed(11)
    assert layers._seed(0.3) == first                                     # torch.manual_seed governs it
    torch.set_rng_state(state)


# (layer, input, fused relation + projection node?)  compress_v2 is MyConv1d(2048, 310): 29 x 36 = 1044 rows, 28 x 36 = 1008
RELATION_NODE = [
    ("cor2", L(2048, 310), X(29, 36, 2048), True), ("rows1008", L(2048, 310), X(28, 36, 2048), False),
    ("fused-off", L(2048, 310, fused=False), X(29, 36, 2048), False), ("af-none", L(2048, 310, af=None), X(29, 36, 2048), False),
    ("bf16", L(2048, 310), X(29, 36, 2048, dtype=BF16), False), ("cpu", L(2048, 310), X(29, 36, 2048, cuda=False), False),
    ("v-needs-grad", L(2048, 310), X(29, 36, 2048, grad=True), False), ("regions35", L(2048, 310), X(30, 35, 2048), False),
    ("out30", L(2048, 30), X(29, 36, 2048), False), ("out32", L(2048, 32), X(29, 36, 2048), True),
]


@pytest.mark.parametrize("case", RELATION_NODE, ids=lambda c: c[0])
def test_relation_projection_node_shares_k5s_clause(case):
    _, spec, v, want = case
    assert bool(_layer(**spec).relation_projection_ok(v)) is want


# ====================================================================================================== the models' shared front
def _wb(*names):
    return [n + s for n in names for s in (".weight", ".bias")]


def _mutan(name, R):
    return _wb(*["%s.list_linear%d.%d.linear" % (name, side, r) for side in (1, 2) for r in range(R)])


def _att(name):
    return _wb(name + ".conv_att.conv", *["%s.list_linear_v_fusion.%d.linear" % (name, g) for g in range(4)])


COR2_KEYS = (_wb("compress_v.conv", "compress_v2.conv", "compress_q.linear") + _mutan("fusion_vq1", 2) + _att("att1")
             + _mutan("fusion_vq2", 2) + _att("att2") + _wb("linear_q.linear") + _mutan("fusion_final", 2)
             + _wb("linear_classif.linear", "compress_q_1.linear", "expand_q_1.linear", "compress_q_2.linear", "expand_q_2.linear"))
ODA_KEYS = (_wb("compress_v.conv", "compress_q.linear") + _att("att") + _wb("linear_q.linear") + _mutan("fusion_final", 5)
            + _wb("linear_classif.linear"))
MODELS = [(CoR2Model, {}), (ODAModel, {"region_counts": True})]


def test_state_dict_names_and_order_are_the_parents():
    assert len(COR2_KEYS) == 62 and COR2_KEYS[4] == "compress_q.linear.weight" and COR2_KEYS[-1] == "expand_q_2.linear.bias"
    assert len(ODA_KEYS) == 38 and ODA_KEYS[14] == "linear_q.linear.weight" and ODA_KEYS[25] == "fusion_final.list_linear1.4.linear.bias"
    cor2, oda = CoR2Model(num_ans=20), ODAModel(num_ans=20)
    assert list(cor2.state_dict().keys()) == COR2_KEYS
    assert list(oda.state_dict().keys()) == ODA_KEYS
    for model in (cor2, oda):       # the shared base adds nothing that a checkpoint would see
        assert isinstance(model, layers.RegionQuestionModel) and list(model.buffers()) == []
        assert [n for n, _ in model.named_parameters()] == list(model.state_dict().keys())


@pytest.mark.parametrize("cls,kw", MODELS, ids=["cor2", "oda"])
def test_seq2vec_slot(cls, kw):
    for slot in (None, "vector"):
        assert isinstance(cls(num_ans=20, seq2vec=slot, **kw).seq2vec, layers.QuestionVectorInput)
    own = torch.nn.Identity()
    assert cls(num_ans=20, seq2vec=own, **kw).seq2vec is own
    text = "%s configures the SkipThoughts encoder that seq2vec='skipthoughts' builds; it cannot be given with seq2vec=%s"
    for key in ("encoder_dtype", "encoder_input_dtype"):
        for slot, shown in ((None, "None"), ("vector", "'vector'"), (own, "'Identity'")):
            with pytest.raises(ValueError) as err:
                cls(num_ans=20, seq2vec=slot, **{key: "bf16"}, **kw)
            assert str(err.value) == text % (key, shown)
    with pytest.raises(ValueError) as err:      # both given: the first one is named
        cls(num_ans=20, encoder_dtype="bf16", encoder_input_dtype="bf16", **kw)
    assert str(err.value) == text % ("encoder_dtype", "None")
    with pytest.raises(ValueError) as err:
        cls(num_ans=20).seq2vec(torch.zeros(2, 7))
    assert str(err.value) == ("seq2vec slot holds no encoder: pass the 2400-d question vector as sample['q_idxes'] "
                              "(or construct the Model with seq2vec=<your encoder>)")


def _sample(B=3, regions=36, **more):
    return dict({"v": torch.zeros(B, regions, 2048), "q_idxes": torch.zeros(B, 2400)}, **more)


@pytest.mark.parametrize("cls,kw", MODELS, ids=["cor2", "oda"])
def test_v_len_refusals(cls, kw, monkeypatch):
    """wrong rank, wrong length, not a tensor, not integers, out of range -- each a ValueError before any layer runs"""
    forbid_launches(monkeypatch, ops)
    model = cls(["PAD", "UNK"], 20, **kw).eval()
    monkeypatch.setattr(model.compress_v, "forward", lambda *a, **k: pytest.fail("a layer ran"))
    i32 = torch.int32
    for bad, text in ((torch.ones(3, 1, dtype=i32), "v_len must be [B] = [3], got (3, 1)"),
                      (torch.tensor(36, dtype=i32), "v_len must be [B] = [3], got ()"),
                      (torch.ones(2, dtype=i32), "v_len must be [B] = [3], got (2,)"),
                      (torch.ones(4, dtype=torch.int64), "v_len must be [B] = [3], got (4,)"),
                      ([36, 36, 36], "v_len must be [B] = [3], got <class 'list'>"),
                      (36, "v_len must be [B] = [3], got <class 'int'>"),
                      (torch.tensor([36.0, 1.0, 2.0]), "v_len must be an int32 or int64 tensor [B] of region counts"),
                      (torch.tensor([36, 0, 1], dtype=i32), "v_len holds 0..36: every region count must lie in 1..36"),
                      (torch.tensor([1, 37, 1]), "v_len holds 1..37: every region count must lie in 1..36"),
                      (torch.tensor([-3, 2, 1]), "v_len holds -3..2: every region count must lie in 1..36")):
        with pytest.raises(ValueError) as err:
            model(_sample(v_len=bad))
        assert str(err.value) == text
    v, v_len = model._region_input(_sample(B=2, regions=5, v_len=torch.tensor([5, 1])))
    assert v.shape == (2, 5, 2048) and v_len.dtype == i32 and v_len.tolist() == [5, 1]
    v, v_len = model._region_input({"v": torch.zeros(2, 5 * 2048)})
    assert v.shape == (2, 5, 2048) and v_len is None


def test_oda_without_region_counts_refuses_the_key_and_reads_none():
    model = ODAModel(["PAD", "UNK"], 20).eval()
    with pytest.raises(ValueError) as err:
        model(_sample(v_len=torch.full((3,), 36, dtype=torch.int32)))
    assert str(err.value) == ("ODA.Model takes no per-sample region counts: drop 'v_len' from the sample, or build the model "
                              "with region_counts=True (CoR2Model masks with it)")
    with pytest.raises(ValueError, match="region_counts=True"):     # refused for being there, whatever it holds
        model(_sample(v_len="thirty-six"))
    with pytest.raises(ValueError) as err:
        ODAModel(["PAD", "UNK"], 20, regions=10).eval()(_sample(regions=36))
    assert str(err.value) == "ODA.Model was built for 10 regions, input has 36"


def test_cut_aliases_and_forward_with_cut_are_shared():
    assert CoR2Model.forward_with_cut is ODAModel.forward_with_cut is layers.RegionQuestionModel.forward_with_cut
    a, b = torch.ones(2, requires_grad=True) * 2, torch.ones(2)
    cut = []
    ins = layers.RegionQuestionModel._cut_aliases(cut, [a, b])
    assert cut[0][0] is a and cut[0][1] is b and len(cut[0]) == 2 and cut[1] is ins
    assert [t.requires_grad for t in ins] == [True, False] and all(t.grad_fn is None for t in ins)
    assert ins[0].data_ptr() == a.data_ptr() and ins[1].data_ptr() == b.data_ptr()
