"""Host-side mirror of the reference's layer library for the CoR2 / ODA hot path.

Same class names, constructor arguments, parameter names/shapes and error
behaviour as the reference, so its checkpoints load and its call sites read the same:

  Linear, MutanFusion, bmul, bmatmul   <- putils/__init__.py:16-33, :205-241, :98-104, :89-95
  MyConv1d, MyLinear, MyATT            <- config/CoR2.py:56-157 (identical copies in config/ODA.py:73-174)

What differs is underneath: the python per-sample loops are gone; MutanFusion's region side, the
attention softmax+pooling, the region projections (MyConv1d: K5, dropout + GEMM + bias + relu in one
kernel) and (in the models) the pairwise relation / object-difference tensors run in hand-written
HIP kernels through libvqa_mi355x.so (ops.py); the [B,.]-sized MyLinear layers run as grouped
phases (head.py, K6) -- except, under VQA_HEAD=auto, CoR2's glimpse projections and ODA's [B,.]
layers, which are one batched library GEMM each with HIP epilogues (my_linears below).
On GPU tensors every layer takes the HIP path and raises if the library is missing; the plain torch
expressions in this file (bmul, bmatmul, _activation, the non-CUDA branches) exist for CPU tensors
only -- shape checks and the state_dict tests -- and are never part of a measured step.
"""
import collections
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import head, ops


def bmul(inputs1, inputs2):
    """putils/__init__.py:98-104: out[b] = inputs1[b] * inputs2[b] (inputs2 broadcasts over the
    middle axes of inputs1) -- one fused broadcast multiply instead of B launches + stack."""
    b = inputs1.size(0)
    shape = [b] + [1] * (inputs1.dim() - inputs2.dim()) + list(inputs2.shape[1:])
    return inputs1 * inputs2.reshape(shape)


def bmatmul(inputs1, inputs2):
    """putils/__init__.py:89-95: out[b] = inputs1[b] @ inputs2[b]."""
    return torch.matmul(inputs1, inputs2)


def _activation(x, af, dim):
    if not af:
        return x
    if af == "softmax":
        return F.softmax(x, dim=dim)
    if af == "sigmoid":
        return torch.sigmoid(x)
    if af == "tanh":
        return torch.tanh(x)
    return getattr(F, af)(x)


# How MyConv1d serves one call (MyConv1d._route): form = the op ("logits": K3a ops.attention_logits, "k5": ops.linear_act,
# "bf16_engine": ops.linear_bf16, "bf16_library" / "library": ops.linear on packed bf16 / the fp32 operands), act = the
# activation inside that op, drop = the rate of a torch dropout pass in front of it, p = the rate of the mask inside the
# kernel, post = the torch activation applied to its result.
_Route = collections.namedtuple("_Route", "form act drop p post")


def _rate(module):
    """The module's input dropout rate in its current mode: its ``p`` while training, 0.0 in eval or without dropout."""
    p = getattr(module, "p", None)
    return float(p) if (p and module.training) else 0.0


def _seed(p):
    """A dropout seed for a kernel that masks at rate p, drawn from torch's CPU generator (so torch.manual_seed governs the
    mask) -- only when there is a mask to draw: at rate 0 nothing is consumed."""
    return ops.next_dropout_seed() if p else 0


def _last_dim_error(in_features, out_features, got):
    return ValueError("[error] putils.Linear(%s, %s): last dimension of input(%s) should equal to in_features(%s)"
                      % (in_features, out_features, got, in_features))


def _same_config(mods, keys):
    first = mods[0]
    return all(all(getattr(m, k) == getattr(first, k) for k in keys) for m in mods)


def my_linears(mods, x, group_first=False, predropped=False):
    """[m(x_g) for m in mods] for G same-shaped MyLinear / Linear modules as ONE batched GEMM: x is [B,K] (every module
    reads the same input, each with its own dropout draw, as when the reference calls them one after the other) or
    [B,G,K] (module g reads x[:, g, :]).  Returns [B,G,A], or [G,B,A] when group_first (each result contiguous).
    The modules keep their own parameters (state_dict names unchanged); weights are stacked per call.
    predropped: the producer of x ([B,G,K]) has already applied the modules' input dropout."""
    first = mods[0]
    lins = [m.linear for m in mods]
    p = getattr(first, "p", None)
    af = getattr(first, "af", None)
    if predropped and x.dim() != 3:
        raise ValueError("my_linears: predropped needs one input per module ([B,G,K])")
    ok = x.is_cuda and _same_config(mods, ("in_features", "out_features")) and \
        all(getattr(m, "p", None) == p and getattr(m, "af", None) == af for m in mods) and \
        all((l.bias is None) == (lins[0].bias is None) for l in lins)
    G = len(mods)
    if not ok:
        outs = [m(x if x.dim() == 2 else x[:, g, :]) for g, m in enumerate(mods)]
        return torch.stack(outs, 0 if group_first else 1)
    if x.size(-1) != first.in_features:
        raise _last_dim_error(first.in_features, first.out_features, x.size(-1))
    rate = _rate(first)
    if x.dim() == 2 and not group_first and not rate and af in (None, "") and x.dtype == torch.float32:
        # G layers on ONE input without dropout or activation (Mutan's rank factors, putils/__init__.py:232-238): a
        # plain GEMM against the [G*A, K] stack -- the sum over the groups in the data gradient happens inside the GEMM
        # (no expand / reduce pair around a batched one), the bias gradient is one column sum
        w = ops.stack_params([l.weight for l in lins])
        if w.is_contiguous():
            b = None
            if lins[0].bias is not None:       # (through ops.linear: its bias gradient is the replay-safe column sum)
                b = ops.stack_params([l.bias for l in lins]).reshape(G * first.out_features)
            y = ops.linear(x, w.view(G * first.out_features, first.in_features), b)
            return y.view(x.size(0), G, first.out_features)
    drop = bool(rate) and not predropped
    if x.dim() == 2 and drop and x.dtype == torch.float32:
        x = ops.dropout(x, p, groups=G).transpose(0, 1)              # G independent draws over the one input: [B,G,K] view
        drop = False
    elif x.dim() == 2:
        x = x.unsqueeze(1).expand(x.size(0), G, x.size(1))          # stride-0 group axis: no copy
    if drop:
        # one draw over [B,G,K]: G independent masks (hash mask on the GPU fp32 path; torch's generator otherwise)
        if x.dtype != torch.float32:
            x = F.dropout(x, p=p, training=True)
        elif x.dim() == 3 and not x.is_contiguous() and x.transpose(0, 1).is_contiguous():
            x = ops.dropout(x.transpose(0, 1), p).transpose(0, 1)    # a [G,B,K] tensor seen as [B,G,K]: mask it as stored
        else:
            x = ops.dropout(x, p)
    w = ops.stack_params([l.weight for l in lins])                   # [G,A,K]: a view of the flat parameter buffer
    b = ops.stack_params([l.bias for l in lins]) if lins[0].bias is not None else None   # when the trainer laid it out
    if af in (None, "", "relu", "sigmoid"):
        return ops.batched_linear(x, w, b, group_first, af or None)      # bias + activation in the GEMM's epilogue kernel
    return _activation(ops.batched_linear(x, w, b, group_first), af, None)


def linear_stack_groups(mods):
    """[[weights...], [biases...]] of same-shaped Linear / MyLinear modules that ``my_linears`` runs as one batched GEMM:
    the trainer places each list at equal spacing in its flat parameter buffer so that stacking them is a view."""
    lins = [m.linear for m in mods]
    groups = [[l.weight for l in lins]]
    if lins[0].bias is not None:
        groups.append([l.bias for l in lins])
    return groups


class Linear(nn.Module):
    """putils/__init__.py:16-33."""

    def __init__(self, in_features, out_features, bias=True, seed=None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        if seed:
            torch.manual_seed(seed)
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, x):
        if x.size()[-1] != self.in_features:
            raise _last_dim_error(self.in_features, self.out_features, x.size(-1))
        return ops.linear(x, self.linear.weight, self.linear.bias)


class MyLinear(nn.Module):
    """config/CoR2.py:94-122: af(linear(dropout_p(x)))."""

    def __init__(self, in_features, out_features, seed=None, p=None, af=None, dim=None):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.p = p
        self.af = af
        self.dim = dim
        if seed:
            torch.manual_seed(seed)
        self.linear = nn.Linear(in_features, out_features, bias=True)

    def forward(self, x):
        if x.size()[-1] != self.in_features:
            raise _last_dim_error(self.in_features, self.out_features, x.size(-1))
        p = _rate(self)
        if p:
            x = ops.dropout(x, p) if (x.is_cuda and x.dtype == torch.float32) else F.dropout(x, p=p, training=True)
        return _activation(ops.linear(x, self.linear.weight, self.linear.bias), self.af, self.dim)


class MyConv1d(nn.Module):
    """config/CoR2.py:56-91 with kernel_size 1 (the only use): af(conv1d(dropout_p(x)^T)^T) on
    [B,N,Cin].  The parameter keeps nn.Conv1d's (Cout,Cin,1) shape under the name ``conv``; the
    contraction itself is a row-major GEMM on the [B*N,Cin] view (no transposes)."""

    def __init__(self, in_channels, out_channels, kernel_size=1, stride=1, padding=0, seed=None, p=None, af=None,
                 dim=None):
        super().__init__()
        if kernel_size != 1 or stride != 1 or padding != 0:
            raise ValueError("MyConv1d: only kernel_size=1, stride=1, padding=0 is on the CoR2/ODA path")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = kernel_size
        self.stride = stride
        self.p = p
        self.af = af
        self.dim = dim
        if seed:
            torch.manual_seed(seed)
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size, stride, padding=padding, dilation=1, groups=1,
                              bias=True)

    # bf16 path: "engine" = the hand-written bf16 MFMA GEMMs (ops.LinearBf16), "library" = hipBLASLt through F.linear
    bf16_gemm = os.environ.get("VQA_BF16_GEMM", "engine")
    # K5 (fused dropout+GEMM+bias+relu on the hand-written fp32 MFMA engines) vs the library GEMM + a separate dropout
    # pass: set per process with VQA_FUSED_LINEAR=0/1.  Default: fused -- since the register-tile engine
    # (csrc/gemm_f32_rt.hpp) the forward beats the library GEMM at these shapes and no dropout pass over
    # [B,36,2048] exists any more (see profiles/README.md)
    fused = os.environ.get("VQA_FUSED_LINEAR", "1") == "1"
    # Set by a model whose ONLY consumer of this layer's relu output hands the gradient back already multiplied by
    # relu'(output) (MutanFusion(..., relu_input=True)): the fused backward then skips its own gate.
    grad_pregated = False

    def _check_rank(self, x):
        if x.dim() != 3:
            raise ValueError("[error] putils.Conv1d(%s, %s, %s, %s): input_dim (%s) should equal to 3"
                             % (self.in_channels, self.out_channels, self.kernel_size, self.stride, x.dim()))

    def _k5_ok(self, x):
        return self.fused and self.af in (None, "relu") and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32 \
            and self.out_channels >= 32 and x.shape[0] * x.shape[1] >= 1024

    def relation_projection_ok(self, v):
        """Can ops.relation_projection (the pairwise-relation step and this projection as ONE autograd node) stand in for
        ops.relation_apply followed by this layer on v [B,N,D]?  Wherever K5 would serve the layer and the node's kernels
        take the shape."""
        return self.af == "relu" and self._k5_ok(v) and ops.relation_projection_supported(v, self.conv.weight.squeeze(-1))

    def _bf16_route(self, x, af, p):
        """Mixed-precision forms (x bf16, last dim possibly zero-padded past in_channels): bf16 operands, fp32
        accumulate, fp32 master weights.  Wide layers return the output padded to a multiple of 64 (pad = 0) so the
        next bf16 GEMM needs no tail; narrow ones (the G attention logits) come back as fp32."""
        if self.out_channels >= 32 and self.bf16_gemm == "engine" and af in (None, "", "relu"):
            if p and (p != 0.5 or x.requires_grad):
                # the in-kernel mask exists at p = 0.5 and has no data gradient (compress_v reads the model input); an x
                # that needs one (compress_v2 behind the pairwise relation, relation_mode=0) is dropped beforehand
                return _Route("bf16_engine", af, p, 0.0, None)
            return _Route("bf16_engine", af, 0.0, p, None)
        return _Route("bf16_library", None, p, 0.0, af)

    def _route(self, x, predropped=False, pre_activation=False):
        """Which form serves this call, at which dropout rate -> _Route.  Reads the layer's settings and x.is_cuda / dtype /
        dim() / shape / requires_grad only: nothing is launched and no seed is drawn.  x is 3-D (_check_rank).
        predropped: the producer of x has applied this layer's input dropout; pre_activation: the caller wants the
        convolution's output without the layer's activation (MyATT applies its softmax inside K3)."""
        af = None if pre_activation else self.af
        p = 0.0 if predropped else _rate(self)
        bf16 = x.dtype == torch.bfloat16
        if bf16 and not pre_activation and (predropped or af in (None, "relu")):
            return self._bf16_route(x, af, p)
        if not pre_activation and self._k5_ok(x):
            # large region-side projection (compress_v / compress_v2): dropout + GEMM + bias + relu in ONE kernel
            # on the fp32 MFMA tile engine (K5); the dropout mask is a counter hash keyed by a seed drawn from
            # torch's CPU generator, so torch.manual_seed governs it and no mask tensor exists
            return _Route("k5", af, 0.0, p, None)
        if not predropped and ops.attention_logits_supported(x, self.in_channels, self.out_channels):
            # the G attention logits of MyATT: dropout + 1x1 conv in one HIP kernel (K3a), fp32 out for either storage
            return _Route("logits", None, 0.0, p, af)
        if bf16:
            return self._bf16_route(x, None, p)._replace(post=af)
        if af == "relu" and x.is_cuda and (predropped or x.dtype == torch.float32):
            return _Route("library", "relu", p, 0.0, None)      # the relu rides in the library GEMM's epilogue (ops.LinearFn)
        return _Route("library", None, p, 0.0, af)

    def _run(self, x, route, packed=None):
        form, act, drop, p, post = route
        w, b = self.conv.weight.squeeze(-1), self.conv.bias
        if drop:
            x = F.dropout(x, p=drop, training=True)
        if form == "logits":
            y = ops.attention_logits(x, w, b, p, _seed(p))
        elif form == "k5":
            y = ops.linear_act(x, w, b, act, p, _seed(p), pregated=self.grad_pregated)
        elif form == "bf16_engine":
            y = ops.linear_bf16(x, w, b, act, p, _seed(p), pregated=self.grad_pregated, packed=packed)
        elif form == "bf16_library":
            wide = self.out_channels >= 32
            n_p = ops.pad_to(self.out_channels) if wide else self.out_channels
            wp = ops.PackedWeightBf16.apply(w, n_p, x.size(-1))
            bp = F.pad(b, (0, n_p - self.out_channels)).to(torch.bfloat16)
            y = ops.linear(x, wp, bp)
            y = y if wide else y.float()
        else:
            y = ops.linear(x, w, b, act=act)
        return _activation(y, post, self.dim)

    def pre_activation(self, x):
        self._check_rank(x)
        return self._run(x, self._route(x, pre_activation=True))

    def forward(self, x, predropped=False, packed=None):
        """predropped=True: the producer of x has already applied this layer's input dropout (ops.relation_apply).
        packed (bf16 inputs): this layer's shadows from the model's ops.ShadowPlan (else they are packed here)."""
        self._check_rank(x)
        return self._run(x, self._route(x, predropped), packed)


class MutanFusion(nn.Module):
    """putils/__init__.py:205-241: sum_r Linear1_r(x1) * Linear2_r(x2) (x2 [B,in2] broadcasts over the
    region axis of x1 [B,N,in1]).  Region side + product + rank sum = HIP kernel K4 (fp32 MFMA)."""

    def __init__(self, input_dim1, input_dim2, hidden_dim, R, seed=None):
        super().__init__()
        self.input_dim1 = input_dim1
        self.input_dim2 = input_dim2
        self.hidden_dim = hidden_dim
        self.R = R
        self.list_linear1 = nn.ModuleList([Linear(input_dim1, hidden_dim) for _ in range(R)])
        self.list_linear2 = nn.ModuleList([Linear(input_dim2, hidden_dim) for _ in range(R)])

    def stack_groups(self):
        return linear_stack_groups(list(self.list_linear2)) + linear_stack_groups(list(self.list_linear1))

    def forward(self, inputs1, inputs2, relu_input=False, packed=None, h2=None):
        """relu_input: inputs1 is the relu output of the layer in front and the gradient returned for it may come back
        multiplied by (inputs1 > 0) already (that layer's backward then skips the gate: MyConv1d.grad_pregated).
        packed (bf16 inputs1): the region-side shadows from the model's ops.ShadowPlan.
        h2 [B,R,H]: the question-side rank factors Linear2_r(inputs2) when a grouped phase of the model has computed them
        already (head.GatesAndRankFactors); inputs2 is then not read."""
        # (bf16 region tensors carry the feature dim zero-padded to a multiple of 64: see ops.pad_to)
        want = ops.pad_to(self.input_dim1) if inputs1.dtype == torch.bfloat16 else self.input_dim1
        if inputs1.size(-1) != want:
            raise _last_dim_error(self.input_dim1, self.hidden_dim, inputs1.size(-1))
        if h2 is None:
            if inputs2.dim() != 2 or inputs2.size(0) != inputs1.size(0):
                raise ValueError("MutanFusion: inputs2 must be [B, input_dim2] with the batch of inputs1")
            # question side: R small [B,in2]x[in2,H] GEMMs (Linear's own check raises ValueError on a bad last dim)
            if inputs2.size(-1) != self.input_dim2:
                raise _last_dim_error(self.input_dim2, self.hidden_dim, inputs2.size(-1))
            h2 = my_linears(list(self.list_linear2), inputs2)                          # [B,R,H], one batched GEMM
        if inputs1.dim() == 2 and inputs1.is_cuda:
            # vector-vector fusion (fusion_final: B rows, not B*N): a few hundred MFLOP, far too little for the K4 tile
            # kernels (16-64 workgroups, each walking the whole K = 1240 twice: 85 us forward).  Both sides run as
            # library GEMMs and the rank sum is one fused multiply-reduce kernel (ops.rank_product).
            h1 = my_linears(list(self.list_linear1), inputs1)                          # [B,R,H]
            return ops.rank_product(h1, h2)
        weights = [lin.linear.weight for lin in self.list_linear1]
        biases = [lin.linear.bias for lin in self.list_linear1]
        return ops.lowrank_bilinear_fusion(inputs1, h2, weights, biases, gate_dx=relu_input, packed=packed)


class MyATT(nn.Module):
    """config/CoR2.py:125-157: alpha = softmax over regions of conv_att(fuse); pooled = alpha^T @ inputs;
    one MyLinear per glimpse; concat.  Returns (x_v [B,att_dim], tuple of G tensors [B,N,1]) like the
    reference.  Softmax + pooling = HIP kernel K3."""

    def __init__(self, fuse_dim, glimpses, inputs_dim, att_dim, seed=None, af="tanh"):
        super().__init__()
        assert att_dim % glimpses == 0
        self.glimpses = glimpses
        self.inputs_dim = inputs_dim
        self.att_dim = att_dim
        self.conv_att = MyConv1d(fuse_dim, glimpses, 1, 1, seed=seed, p=0.5, af="softmax", dim=1)
        self.list_linear_v_fusion = nn.ModuleList(
            [MyLinear(inputs_dim, int(att_dim / glimpses), p=0.5, af=af) for _ in range(glimpses)])
        self.af = af

    def stack_groups(self):
        return linear_stack_groups(list(self.list_linear_v_fusion))

    def glimpse_dropout(self):
        """Input dropout rate of the per-glimpse MyLinear list in the current mode (0.0 in eval)."""
        return _rate(self.list_linear_v_fusion[0])

    def _fused_dropout_ok(self):
        """The G glimpse layers share one dropout rate (else each draws its own mask at its own rate: the batched form and
        the fused store do not apply)."""
        mods = list(self.list_linear_v_fusion)
        return os.environ.get("VQA_FUSE_POOL_DROPOUT", "1") == "1" and all(getattr(m, "p", None) == mods[0].p for m in mods)

    def glimpse_projection(self, pooled, predropped=False, grouped=False):
        """cat_g MyLinear_g(pooled[:, g, :]) (config/CoR2.py:143-147).  The G layers have one shape, so they run as ONE
        batched GEMM over the [B,G,D] tensor (one dropout draw over all of it, one bias add, one activation) instead of
        G x {slice, dropout, GEMM, activation} and, backward, G slice gradients that autograd zero-fills and adds.
        grouped: the caller runs the grouped head; under VQA_HEAD=grouped the projections are a phase of it
        (head.GlimpseProjections) -- ONLY when the consumer of the result is the head's fusion phase, which hands the
        gradient back gated by the relu (gating it again, as the batched form does, changes nothing)."""
        if grouped and head.glimpses_grouped():
            mods = list(self.list_linear_v_fusion)
            pd = self.glimpse_dropout()
            if pd and not predropped:
                pooled = ops.dropout(pooled, pd)
            return head.GlimpseProjections.apply(pooled.contiguous(), *[m.linear.weight for m in mods],
                                                 *[m.linear.bias for m in mods])
        y = my_linears(list(self.list_linear_v_fusion), pooled, predropped=predropped)   # [B,G,A]
        return y.reshape(y.size(0), -1)

    def grouped_ok(self, inputs):
        """Can the glimpse projections run as a grouped phase?  (relu layers of one shape, fp32 GPU tensors)"""
        mods = list(self.list_linear_v_fusion)
        return inputs.is_cuda and self.af == "relu" and self.inputs_dim % 2 == 0 and \
            all(getattr(m, "af", None) == "relu" and m.out_features == mods[0].out_features and m.p == mods[0].p for m in mods)

    def attend(self, inputs, logits, pooled_map=None, return_pooled=False, grouped=False, lens=None):
        """logits [B,N,G] (pre-softmax) -> (x_v, list_att, alpha [B,N,G][, pooled[:, 0] [B,D]]).  pooled_map (optional):
        ``pooled_map(pooled, p) -> tensor`` transforms the pooled features before the glimpse projections AND applies
        their input dropout at rate p (so the two share one pass).  lens (optional): int32 [B] on the inputs' device, the
        number of real regions of every sample -- the rows beyond get alpha = 0 exactly and are never read.  (Nothing that carries an autograd graph is kept on
        the module: a tensor stashed across steps would pin the previous step's graph.)"""
        first = None
        pd = self.glimpse_dropout()
        counts = {} if lens is None else {"lens": lens}       # (without counts: today's calls, argument for argument)
        if pooled_map is None and inputs.is_cuda and (pd > 0 or return_pooled) and self._fused_dropout_ok():
            # the glimpse projections' input dropout rides in the pooling kernel's store (one pass fewer each way), and
            # glimpse 0 comes back undropped as its own tensor for the caller (CoR2's relation step)
            res = ops.softmax_attention_pool_drop(logits, inputs, pd, _seed(pd), return_pooled, **counts)
            alpha, pooled = res[0], res[1]
            if return_pooled:
                first = res[2]
            x_v = self.glimpse_projection(pooled, predropped=True, grouped=grouped)
        else:
            alpha, pooled = ops.softmax_attention_pool(logits, inputs, **counts)           # [B,N,G], [B,G,D]
            if return_pooled:       # glimpse 0 for the caller (CoR2's relation step), the whole tensor for the projections
                pooled, first = ops.with_first_group(pooled)
            if pooled_map is None:
                x_v = self.glimpse_projection(pooled, grouped=grouped)
            else:
                x_v = self.glimpse_projection(pooled_map(pooled, pd), predropped=True, grouped=grouped)
        out = (x_v, torch.split(alpha, 1, dim=2), alpha)
        return out + (first,) if return_pooled else out

    def forward(self, inputs, fuse, lens=None):
        x_v, list_att, _ = self.attend(inputs, self.conv_att.pre_activation(fuse), lens=lens)
        return x_v, list_att


class SideOutputs(dict):
    """The ``alpha_dict`` side output of a model (read by visu.py:198-207 after a forward) with entries that may be computed
    on first access: a value stored as a zero-argument callable is replaced by its result when it is read.  Only a
    TRAINING forward stores such an entry (``alpha_dict['feature']``: a training step never reads it, so the kernel that
    would materialise it does not run in the step; read after a graph-replayed step it reflects the latest replay); an
    eval forward -- the visualisation path -- stores plain tensors like the reference.  Every way of getting the values
    out (indexing, get, items, values, iteration-based copies, dict(), ``**``, copy, pickling) resolves them first."""

    def _resolve(self, key):
        value = dict.__getitem__(self, key)
        if callable(value) and not isinstance(value, torch.Tensor):
            value = value()
            dict.__setitem__(self, key, value)
        return value

    def _resolve_all(self):
        for k in list(dict.keys(self)):
            self._resolve(k)

    def __getitem__(self, key):
        return self._resolve(key)

    def get(self, key, default=None):
        return self._resolve(key) if key in self else default

    def items(self):
        self._resolve_all()
        return dict.items(self)

    def values(self):
        self._resolve_all()
        return dict.values(self)

    def keys(self):          # dict(d) / {**d} walk keys() and then index: resolve up front so C-level fast paths see tensors
        self._resolve_all()
        return dict.keys(self)

    def __iter__(self):
        self._resolve_all()
        return dict.__iter__(self)

    def copy(self):
        self._resolve_all()
        return SideOutputs(dict.copy(self))

    def __reduce__(self):
        self._resolve_all()
        return (SideOutputs, (dict(dict.items(self)),))


class QuestionVectorInput(nn.Module):
    """Stand-in for the question encoder slot ``seq2vec`` (putils.SkipThoughts, putils/__init__.py:878-985,
    is upstream of the hot path and needs weight files that are not available offline): the sample's
    'q_idxes' entry already holds the 2400-d question vector and is passed through."""

    def __init__(self, dim=2400):
        super().__init__()
        self.dim = dim

    def forward(self, q):
        if not torch.is_floating_point(q) or q.size(-1) != self.dim:
            raise ValueError("seq2vec slot holds no encoder: pass the %d-d question vector as sample['q_idxes'] "
                             "(or construct the Model with seq2vec=<your encoder>)" % self.dim)
        return q


def question_feature(seq2vec, q):
    """What ``Model.forward`` feeds the head: ``seq2vec(q_idxes)`` for int64 token ids [B,T] as the reference does
    (config/CoR2.py:205, fed by datasets.py:928-969), and -- north_star's "(region-feature, question-embedding)"
    interface -- a floating [B,2400] tensor taken as the question vector itself, whatever the slot holds."""
    if torch.is_floating_point(q) and q.dim() == 2 and q.size(-1) == 2400:
        return q
    return seq2vec(q)


class RegionQuestionModel(nn.Module):
    """What cor2.Model and oda.Model share around their own reasoning steps: the question-encoder slot, the region input,
    the cut between an early and a late part of backward, and the grouped head's last two phases.  Holds no parameter or
    buffer of its own."""

    compute_dtype = torch.float32       # storage type of the region-side tensors (cor2.Model sets its own)

    def _set_seq2vec(self, seq2vec, vocab_words, encoder_dtype, encoder_input_dtype, encoder_length_aware=None):
        """The ``seq2vec`` slot: "skipthoughts" (the reference's encoder, config/CoR2.py:166, randomly initialised here),
        "vector" / None (sample['q_idxes'] holds the 2400-d question vector) or the caller's own module."""
        if seq2vec == "skipthoughts":
            from .encoder import SkipThoughts, encoder_dtype_from, encoder_input_dtype_from, encoder_length_aware_from
            seq2vec = SkipThoughts(vocab_list=vocab_words, gru="BayesianGRU", return_last=True, af="relu",
                                   compute_dtype=encoder_dtype_from(encoder_dtype),
                                   input_dtype=encoder_input_dtype_from(encoder_input_dtype),
                                   length_aware=encoder_length_aware_from(encoder_length_aware))
        elif encoder_dtype is not None or encoder_input_dtype is not None or encoder_length_aware is not None:
            given = seq2vec if seq2vec is None or isinstance(seq2vec, str) else type(seq2vec).__name__
            raise ValueError("%s configures the SkipThoughts encoder that seq2vec='skipthoughts' builds; "
                             "it cannot be given with seq2vec=%r"
                             % ("encoder_dtype" if encoder_dtype is not None else
                                "encoder_input_dtype" if encoder_input_dtype is not None else "encoder_length_aware", given))
        if seq2vec == "vector":
            seq2vec = None
        self.seq2vec = seq2vec if seq2vec is not None else QuestionVectorInput(2400)

    def _region_input(self, sample, counts=True):
        """-> (v [B,N,2048], v_len).  v_len: sample['v_len'] (optional, read when `counts`) -- the number of real regions of
        every sample, the rest of its N rows being (finite) padding -- as the int32 device tensor the masked kernels read
        (ops.region_counts), else None.  bf16 regions on their way into an fp32 model are the feed's transport format
        (feed.store_batches(region_dtype=torch.bfloat16): half the host -> device bytes), widened exactly by one HIP pass.
        A packed batch carries 'v_packed' [B*N, 2048] (fp32 or bf16: the capacity-sized buffer whose first sum(v_len) rows are the
        samples' real rows back to back) and the then mandatory 'v_len' instead of 'v': ops.unpack_regions rebuilds the padded
        tensor, exact zeros on the padding, in one pass -- bf16 rows into an fp32 model widened by that same pass, fp32 rows into
        a bf16 model unpacked as fp32 and cast where a padded fp32 'v' is.
        A resident-store batch carries 'v_idx' int [B], the image of each sample, and no region rows at all: ops.gather_regions
        reads them out of the store attached with use_region_store, and v_len comes from the store when it has counts."""
        if "v_idx" in sample:
            return self._resident_region_input(sample, counts)
        if "v_packed" in sample:
            return self._packed_region_input(sample, counts)
        v = sample["v"]
        b = v.size(0)
        v = v.contiguous().view(b, -1, 2048)
        v_len = sample.get("v_len") if counts else None
        if v_len is not None:
            if not isinstance(v_len, torch.Tensor) or v_len.dim() != 1 or v_len.size(0) != b:
                raise ValueError("v_len must be [B] = [%d], got %s"
                                 % (b, tuple(v_len.shape) if isinstance(v_len, torch.Tensor) else type(v_len)))
            v_len = ops.region_counts(v_len, v.size(1), v.device)
        if v.is_cuda and v.dtype == torch.bfloat16 and self.compute_dtype == torch.float32:
            v = ops.widen_bf16(v)
        return v, v_len

    region_store = None                 # the attached feed.DeviceFeatureStore (use_region_store): a plain attribute

    def use_region_store(self, dstore):
        """Attach (or, with None, detach) a device-resident region store (feed.DeviceFeatureStore): batches may then carry 'v_idx'
        instead of 'v' / 'v_packed' / 'v_len'.  The store is a plain attribute -- no module, buffer or parameter: state_dict(),
        parameters() and .to() do not see it.  A batch without 'v_idx' runs exactly as without a store.  -> self."""
        if dstore is not None:
            N, D = dstore.sample_shape
            regions = getattr(self, "regions", None)
            if D != 2048 or (regions is not None and N != regions):
                raise ValueError("region store of %d x %d rows per image does not fit this model (%s regions of 2048)"
                                 % (N, D, regions if regions is not None else "any number of"))
        object.__setattr__(self, "region_store", dstore)
        return self

    def _resident_region_input(self, sample, counts):
        """'v_idx' -> (v, v_len) out of the attached store.  bf16 rows into an fp32 model are widened in the gather, bf16 rows
        into a bf16 model copied, fp32 rows gathered as fp32 (and cast by the model where a padded fp32 'v' is)."""
        clash = [k for k in ("v", "v_packed", "v_len") if k in sample]
        if clash:
            raise ValueError("a batch names its images ('v_idx') or carries their rows and counts (%s), not both"
                             % ", ".join(repr(k) for k in clash))
        store = self.region_store
        if store is None:
            raise ValueError("'v_idx' needs a resident region store: attach one with model.use_region_store(DeviceFeatureStore(...))")
        if store.counts is not None and not counts:
            raise ValueError("this model reads no per-sample region counts and so takes no resident store that has them")
        widen = store.rows.dtype == torch.bfloat16 and self.compute_dtype == torch.float32
        return ops.gather_regions(store, sample["v_idx"], torch.float32 if widen else store.rows.dtype, want_len=counts)

    def _packed_region_input(self, sample, counts):
        if "v" in sample:
            raise ValueError("a batch carries its regions padded ('v') or packed ('v_packed'), not both")
        if not counts:
            raise ValueError("this model reads no per-sample region counts and so takes no packed batch ('v_packed')")
        vp, v_len = sample["v_packed"], sample.get("v_len")
        if v_len is None:
            raise ValueError("'v_packed' needs 'v_len': the region counts are what delimits the samples' rows")
        if not isinstance(v_len, torch.Tensor) or v_len.dim() != 1 or v_len.size(0) < 1:
            raise ValueError("v_len must be [B], got %s" % (tuple(v_len.shape) if isinstance(v_len, torch.Tensor) else type(v_len),))
        b = v_len.size(0)
        if not isinstance(vp, torch.Tensor) or vp.dim() != 2 or vp.size(1) != 2048 or vp.size(0) < b or vp.size(0) % b:
            raise ValueError("v_packed must be [B*N, 2048] with B = %d, got %s"
                             % (b, tuple(vp.shape) if isinstance(vp, torch.Tensor) else type(vp)))
        v_len = ops.region_counts(v_len, vp.size(0) // b, vp.device)
        widen = vp.dtype == torch.bfloat16 and self.compute_dtype == torch.float32
        return ops.unpack_regions(vp, v_len, b, torch.float32 if widen else vp.dtype), v_len

    def forward_with_cut(self, sample):
        """-> (logits, outs, ins): ``outs`` are the results of the early part of the model that the late part
        (``late_parameters``) reads, ``ins`` the detached aliases it actually consumed.  d loss / d ins fed as grad_outputs
        of ``outs`` completes the backward."""
        cut = []
        logits = self(sample, cut)
        return logits, cut[0], cut[1]

    @staticmethod
    def _cut_aliases(cut, outs):
        """The late part runs on detached aliases of `outs`, so a backward pass from the loss ends at the aliases (some of
        the originals may be ancestors of others and would otherwise drag the early layers into it); a second pass then
        carries the aliases' gradients from the originals to the inputs (trainer.DataParallelTrainer, overlap=True)."""
        ins = [t.detach().requires_grad_(t.requires_grad) for t in outs]
        cut.extend([outs, ins])
        return ins

    def _grouped_tail(self, h2_final, *inputs):
        """The grouped head's last two phases: fusion_final (its first input is cat(inputs), never materialised) with the
        rank product and the classifier's input dropout in its epilogue, then the classifier -- one seed for both."""
        p_c = _rate(self.linear_classif)
        seed = _seed(p_c)
        lins = list(self.fusion_final.list_linear1)
        x = head.VectorFusion.apply(h2_final, p_c, seed, len(inputs), *inputs, *[l.linear.weight for l in lins],
                                    *[l.linear.bias for l in lins])
        return head.Classifier.apply(x, self.linear_classif.linear.weight, self.linear_classif.linear.bias, p_c, seed)
