"""Train step of the reference (train.py:41-107, :286-299, :535-548) for one process per GPU.

The reference wraps the model in single-process ``nn.DataParallel`` (train.py:517): per step it scatters
the batch, re-broadcasts every parameter, gathers logits and reduce-adds all gradients to GPU 0.  Here
every rank owns a replica and a contiguous batch shard; the only data-path collective is ONE
sum-all-reduce (RCCL over xGMI; ``gloo`` in the CPU tests) of a flat fp32 gradient buffer per step:

  * parameter ``.grad`` tensors are views into the flat buffer, so autograd accumulates in place and no
    gather/scatter copy is needed around the collective;
  * SUM, not mean: the reference loss is a sum over the global batch (KLDivLoss(size_average=False),
    train.py:541) and DataParallel adds replica gradients, so clip_grad_norm_(0.25) (train.py:82) sees
    the same global-batch gradient on every rank;
  * step order as train.py:63-86: forward, loss, scheduler.step(), zero_grad, backward, [all-reduce],
    clip, optimizer.step().  lr follows ExponentialLR(gamma = 0.5 ** (1/50000)) stepped every iteration.
"""
import torch
import torch.distributed as dist
import torch.nn.functional as F


def kld_sum_loss(logits, target):
    """train.py:536-544: KLDivLoss(size_average=False)(F.log_softmax(logits), target).  GPU tensors go through the
    fused HIP kernel (ops.KldSumLoss); CPU tensors (the gloo tests of the host logic) through the torch ops."""
    if logits.is_cuda:
        from . import ops
        return ops.kld_sum_loss(logits, target)
    return F.kl_div(F.log_softmax(logits, dim=1), target, reduction="sum")


class SparseTarget:
    """A step's answer target as the feed's (answer id, probability) pairs -- a_idx int32 [B,K], a_val float32 [B,K], the
    format ops.densify defines -- with the few tensor methods the step's graph bookkeeping uses on a dense target: the pair
    is a graph input like the dense ``a`` (compared by shape and address, cloned into a private buffer, copied into it)."""

    __slots__ = ("a_idx", "a_val")

    def __init__(self, a_idx, a_val):
        from . import ops
        ops.check_sparse_target("step", a_idx, a_val)
        self.a_idx, self.a_val = a_idx, a_val

    @property
    def shape(self):
        return ("sparse",) + tuple(self.a_idx.shape)

    def data_ptr(self):
        return (self.a_idx.data_ptr(), self.a_val.data_ptr())

    def clone(self):
        return SparseTarget(self.a_idx.clone(), self.a_val.clone())

    def copy_(self, other, non_blocking=False):
        self.a_idx.copy_(other.a_idx, non_blocking=non_blocking)
        self.a_val.copy_(other.a_val, non_blocking=non_blocking)
        return self


_HIP_NODE_TYPES = {0: "kernel", 1: "memcpy", 2: "memset", 3: "host", 4: "graph", 5: "empty", 6: "wait_event",
                   7: "event_record"}


def graph_node_types(graph):
    """{node type: count} of a captured (keep_graph=True, not yet re-captured) torch.cuda.CUDAGraph, read through
    hipGraphGetNodes / hipGraphNodeGetType.  Returns {} when the runtime library cannot be queried."""
    import ctypes
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        handle = ctypes.c_void_p(graph.raw_cuda_graph())
        count = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(handle, None, ctypes.byref(count)) != 0:
            return {}
        nodes = (ctypes.c_void_p * count.value)()
        if hip.hipGraphGetNodes(handle, nodes, ctypes.byref(count)) != 0:
            return {}
        out = {}
        for node in nodes:
            kind = ctypes.c_int(-1)
            if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
                return {}
            name = _HIP_NODE_TYPES.get(kind.value, "type%d" % kind.value)
            out[name] = out.get(name, 0) + 1
        return out
    except (OSError, AttributeError, RuntimeError):
        return {}


def audit_and_instantiate(graphs, what):
    """Instantiate the captured graphs {name: CUDAGraph} of `what` (named in the errors) -> {name: node counts}.

    Audit before instantiating: a memset node (hipMemsetAsync under capture) is replayed correctly once and then writes
    garbage on ROCm 7.2 (tools/graph_memset_check.py).  The library and the models issue none -- zero fills are kernels,
    the loss and the bias gradients avoid torch's semaphore-based reductions -- and a graph that contains one anyway (a
    user-supplied seq2vec, a new torch op) must not be replayed."""
    nodes = {k: graph_node_types(v) for k, v in graphs.items()}
    if any("kernel" not in c for c in nodes.values()):
        # the audit could not read the graphs (runtime library not queryable): unknown is not "clean" -- stay eager
        raise RuntimeError("cannot audit the captured %s for memset nodes (hipGraphGetNodes unavailable)" % what)
    memsets = sum(c.get("memset", 0) for c in nodes.values())
    if memsets:
        raise RuntimeError("captured %s holds %d memset node(s), which do not replay reliably" % (what, memsets))
    for v in graphs.values():
        v.instantiate()
    torch.cuda.synchronize()
    return nodes


def report_capture_failure(who, error, then):
    """A failed capture is survived (`then` says how); say so once on stderr and let the device drain the attempt."""
    import sys
    print("[vqa %s] hipGraph capture failed (%s: %s); %s" % (
        who, type(error).__name__, str(error).splitlines()[0] if str(error) else "", then), file=sys.stderr)
    torch.cuda.synchronize()


class FlatGradients:
    """One contiguous fp32 buffer holding every parameter's gradient (views installed as p.grad)."""

    def __init__(self, params):
        self.params = [p for p in params if p.requires_grad]
        total = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.buffer = torch.zeros(total, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            n = p.numel()
            p.grad = self.buffer[off:off + n].view_as(p)
            off += n

    def zero(self):
        self.buffer.zero_()

    def all_reduce_sum(self, group=None):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dist.all_reduce(self.buffer, op=dist.ReduceOp.SUM, group=group)

    def clip_(self, max_norm):
        """torch.nn.utils.clip_grad_norm_ semantics (L2, eps 1e-6) on the flat buffer; returns the norm."""
        # accumulate in fp64: one long fp32 sum over ~12M elements is visibly (1e-3) off on some backends
        norm = torch.linalg.vector_norm(self.buffer, dtype=torch.float64).to(torch.float32)
        coef = torch.clamp(max_norm / (norm + 1e-6), max=1.0)
        self.buffer.mul_(coef)
        return norm


def collect_stack_groups(model):
    """Every module's ``stack_groups()`` (lists of same-shaped parameters that are stacked per step)."""
    groups = []
    for m in model.modules():
        fn = getattr(m, "stack_groups", None)
        if callable(fn):
            groups.extend(fn())
    return groups


class FlatState:
    """GPU path: parameters, gradients and both Adam moments each live in ONE flat fp32 buffer (segments aligned
    to 16 bytes, the members of a stack group packed back to back).  ``p.data`` become views of the parameter buffer (state_dict / load_state_dict keep working);
    after backward the per-parameter gradients autograd produced are gathered into the gradient buffer by one
    multi-tensor copy (cheaper than zero + ~70 accumulate-adds), which is then the all-reduce payload and the
    input of the fused clip + Adam kernels (csrc/optimizer.hip)."""

    def __init__(self, params, stack_groups=(), moments=("m", "v")):
        # members of a stack group (same-shaped parameters that layers.my_linears stacks for one batched GEMM) are laid
        # out next to each other, in group order, so that the stack is a strided view of this buffer (ops.StackParams)
        params = [p for p in params if p.requires_grad]
        member = {}
        for group in stack_groups:
            group = [p for p in group if p.requires_grad]
            if len(group) > 1 and not any(id(p) in member for p in group):
                for p in group:
                    member[id(p)] = group
        ordered, placed = [], set()
        for p in params:
            for q in member.get(id(p), [p]):
                if id(q) not in placed:
                    placed.add(id(q))
                    ordered.append(q)
        self.params = ordered
        dev = self.params[0].device
        # segments start 16-byte aligned; the members of a stack group follow each other without padding (8-byte
        # aligned: even sizes), so the stack [G, ...] is a CONTIGUOUS view (ops.StackParams) -- e.g. the G biases of 510
        offs, off = [], 0
        for i, p in enumerate(self.params):
            group = member.get(id(p))
            tight = group is not None and p.numel() % 2 == 0
            inside = tight and i > 0 and member.get(id(self.params[i - 1])) is group
            if not inside:
                off = (off + 3) // 4 * 4
            offs.append(off)
            off += p.numel()
        off = (off + 3) // 4 * 4
        self.total = off
        self.offsets = offs
        self.p = torch.zeros(off, device=dev, dtype=torch.float32)
        self.g = torch.zeros(off, device=dev, dtype=torch.float32)
        # the optimizer's state: Adam keeps both moments, SGD only m (its momentum buffer), RMSprop only v (its square average)
        self.m = torch.zeros(off, device=dev, dtype=torch.float32) if "m" in moments else None
        self.v = torch.zeros(off, device=dev, dtype=torch.float32) if "v" in moments else None
        self.g_views = []
        with torch.no_grad():
            for p, o in zip(self.params, offs):
                view = self.p[o:o + p.numel()].view_as(p)
                view.copy_(p.data)
                p.data = view
                self.g_views.append(self.g[o:o + p.numel()].view_as(p))
        from . import _lib
        self.norm_and_coef = torch.zeros(2, device=dev, dtype=torch.float32)
        self.workspace = torch.empty(_lib.lib().vqa_grad_norm_workspace_bytes() // 8, device=dev, dtype=torch.float64)

    def drop_grads(self):
        for p in self.params:
            p.grad = None

    def store_grads(self, params, grads):
        """Gradients computed by torch.autograd.grad for a subset of the parameters -> their slots of the flat buffer."""
        if not hasattr(self, "_view_of"):
            self._view_of = {id(p): v for p, v in zip(self.params, self.g_views)}
        src, dst = [], []
        for p, g in zip(params, grads):
            view = self._view_of[id(p)]
            if g is None:
                view.zero_()
            elif g.data_ptr() != view.data_ptr() or g.stride() != view.stride():
                src.append(g)
                dst.append(view)
            p.grad = view
        if src:
            torch._foreach_copy_(dst, src)

    def offset_of(self, p):
        return self.offsets[next(i for i, q in enumerate(self.params) if q is p)]

    def gather_grads(self):
        """Whatever backward left in p.grad -> the flat gradient buffer.  Gradients the kernels wrote there themselves
        (ops._grad_like: autograd adopted the slot as .grad) are in place already; only the rest is copied."""
        src, dst = [], []
        for p, view in zip(self.params, self.g_views):
            if p.grad is None:
                view.zero_()
            elif p.grad.data_ptr() != view.data_ptr() or p.grad.stride() != view.stride():
                src.append(p.grad)
                dst.append(view)
        self.last_gathered = len(src)       # (tests: 0 when every gradient was written in place)
        if src:
            torch._foreach_copy_(dst, src)
        for p, view in zip(self.params, self.g_views):
            p.grad = view

    def begin_backward(self):
        """Called right before a backward pass: parameter gradients may be written straight into the flat buffer."""
        from . import ops
        ops.set_grad_slots(self.p, self.g)
        self.drop_grads()

    def end_backward(self):
        from . import ops
        ops.set_grad_slots(self.p, None)


class DataParallelTrainer:
    """Replicated model + flat-gradient sum-all-reduce + the reference's clip/Adam/ExponentialLR."""

    # graph=True: steps launched kernel by kernel before the step is captured (the capture itself runs one more forward +
    # backward on a side stream first, torch's recipe).  Two suffice for the allocator, the kernels' LDS attributes and the
    # recorded GEMM solutions; every further step of a short warm-up is then already a replay at its steady clock.
    EAGER_STEPS_BEFORE_CAPTURE = 2

    def __init__(self, model, lr=1e-4, clip=0.25, gamma=0.5 ** (1 / 50000), broadcast=True, group=None,
                 fused_adam=None, graph=False, adopt_inputs=False, overlap=None, input_slots=1, topk=None,
                 loss="KLD", optim="adam", lr_scheduler=True):
        self.model = model
        # the reference driver's grid (train.py:286-299, :519-548): loss = KLD (sum over the batch) | BCE | CE (means over the
        # GLOBAL batch), optim = adam | sgd (momentum 0.9) | rms, lr_scheduler = the per-iteration ExponentialLR on or off.
        # The defaults are the step this trainer always ran: the same launches, the same graph nodes, the same bits.
        if optim not in self.OPTIMS:
            raise ValueError('Optim is set %s' % optim)
        if loss not in self.LOSSES:
            raise ValueError("<train.py> loss")
        self.loss_kind, self.optim_kind, self.lr_scheduler = loss, optim, bool(lr_scheduler)
        self.momentum, self.alpha = 0.9, 0.99               # train.py:288; torch.optim.RMSprop's default
        # topk=(1, 5): the loss of every step also counts the target's top-k hits (the reference's accuracy(), train.py:22-38,
        # :70-72) from the same pass over the logits (ops.kld_sum_loss_and_grad_hits); last_hits / last_logits / accuracy()
        # expose them.  None (the default) issues exactly the launches and captures exactly the graph nodes it did before.
        self.topk = tuple(int(k) for k in topk) if topk else None
        if self.topk and not all(1 <= k <= 16 for k in self.topk):
            raise ValueError("topk=%s: every k must lie in [1, 16] (and not exceed the number of answers)" % (topk,))
        self.kmax = max(self.topk) if self.topk else 0
        self._front_out = (None, None, 0)    # (hits, logits, local batch) of the last step's loss launch
        self._labels = None                  # CE from a sparse target: the labels the last step's loss launch drew
        self.group = group
        self.clip = clip
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        # the gradient all-reduce runs whenever there is more than one rank; VQA_FORCE_ALLREDUCE=1 also issues it in a
        # process group of ONE rank (an identity), which is how a single-GPU box exercises the real RCCL path -- init, the
        # collective between / beside the replayed hipGraphs, the async work handle (tests/test_gpu_nccl1.py)
        import os as _os
        self.reduce = self.world > 1 or (_os.environ.get("VQA_FORCE_ALLREDUCE") == "1" and dist.is_available()
                                         and dist.is_initialized())
        if broadcast and self.world > 1:
            # identical initial weights on every rank, once (replaces DataParallel's per-step broadcast)
            for t in list(model.parameters()) + list(model.buffers()):
                dist.broadcast(t.data, src=0, group=group)
        self.gamma = gamma
        self.iteration = 0          # scheduler.last_epoch: restarts with every (re-)created scheduler, also on resume
        self.adam_steps = 0         # Adam's per-parameter `step`: travels with the optimizer state
        self.base_lr = lr
        self._lr = lr
        self.betas, self.eps = (0.9, 0.999), 1e-8           # torch.optim.Adam defaults (train.py:290)
        first = next(p for p in model.parameters() if p.requires_grad)
        self.hip = first.is_cuda                              # GPU: fused HIP tail; CPU (gloo tests): torch ops
        if self.hip:
            # the [B,*]-sized layers stay on library GEMMs: look their shapes up in the shipped solution table (tuned_gemms.py)
            from . import tuned_gemms
            tuned_gemms.enable()
        # graph=True: after a few eager steps the step is captured into two hipGraphs (forward+loss+backward+gather,
        # and clip+Adam) with the all-reduce launched eagerly between them; replays cost ~3 host launches instead of
        # ~600.  Falls back to eager if a forward draws a host-side dropout seed (fused K2/K5 masks).
        self.want_graph = bool(graph)
        # The replayed graphs read their batch from fixed buffers.  By default those are private copies and every batch is
        # copied into them (one device-to-device pass over the batch per step).  adopt_inputs=True makes the tensors of
        # the batch the step was captured on the graph's input buffers: no copy when the caller hands over the same
        # tensors every step (resident synthetic data), but later batches OVERWRITE those tensors -- never combine it
        # with a feeder that recycles its own buffers (feed.DevicePrefetcher).
        self.adopt_inputs = bool(adopt_inputs)
        # input_slots > 1 (with adopt_inputs): the feeder hands over batches in a RING of that many resident buffers (a DMA
        # target per slot).  The forward + backward graph is then captured once PER SLOT, reading that slot's tensors in
        # place -- the first step that sees a new slot runs kernel by kernel and captures it -- so no step pays a
        # device-to-device copy of its batch into a private input buffer; clip + Adam (which read no inputs) stay one graph.
        # The graphs share one memory pool: they never run concurrently.  A batch in none of the slots is copied into slot 0.
        self.input_slots = max(1, int(input_slots)) if self.adopt_inputs else 1
        self._slots = []
        self._graph = None
        self.graph_nodes = {}
        self._eager_steps = 0
        # overlap (GPU path, models that offer late_parameters() / forward_with_cut(): CoR2, ODA): backward runs in two halves;
        # the gradients of the second reasoning step -- complete after the first half -- are all-reduced while the second
        # half runs.  OPT-IN (overlap=True or VQA_DP_OVERLAP=1): what it costs a single GPU is the split of the backward
        # graph (0.03 ms at B = 512), what it could hide is ~60 % of the all-reduce payload behind ~40 % of the backward --
        # but its gain over xGMI has never been measured (no multi-GPU node in this build's reach) and the register-tile
        # kernels run one or two workgroups per CU, so a concurrent RCCL kernel can also slow the backward it hides behind.
        # Until a scaling run says otherwise the default is the single all-reduce between backward and clip.
        # tests/test_gpu_dp2.py runs both on two ranks sharing one GPU.  "force" also splits at world size 1.
        requested = overlap
        if overlap is None:
            import os
            requested = overlap = os.environ.get("VQA_DP_OVERLAP", "0") == "1"
        self.overlap = False
        if self.hip:
            params = list(model.parameters())
            can_split = bool(overlap) and hasattr(model, "late_parameters") and hasattr(model, "forward_with_cut") and \
                (self.world > 1 or overlap == "force")
            if can_split:
                late_ids = {id(p) for p in model.late_parameters()}
                params = [p for p in params if id(p) in late_ids] + [p for p in params if id(p) not in late_ids]
            self.flat = FlatState(params, collect_stack_groups(model), self.OPTIMS[optim])
            if can_split:
                late = [p for p in self.flat.params if id(p) in late_ids]
                early = [p for p in self.flat.params if id(p) not in late_ids]
                if late and early:
                    split = min(self.flat.offset_of(p) for p in early)
                    if all(self.flat.offset_of(p) + p.numel() <= split for p in late):
                        self.overlap, self._late, self._early, self._split = True, late, early, split
            # the backward phases of a step (_run_phases), each with the gradient bucket it completes: the whole backward
            # and the whole buffer, or the two halves with the late bucket (a prefix of the buffer) and the rest
            g = self.flat.g
            self._phases = (("front_a", g[:self._split]), ("front_b", g[self._split:])) if self.overlap else (("front", g),)
            # say once which reduction schedule is in effect -- also when the split was asked for and could not be had
            # (the model offers no cut, or a stack group mixes late and early parameters so the late bucket is not a prefix)
            if self.overlap:
                self.overlap_note = "two-half backward, late bucket %d of %d floats reduced under the second half" % (
                    self._split, self.flat.total)
            elif requested:
                if not (hasattr(model, "late_parameters") and hasattr(model, "forward_with_cut")):
                    why = "model has no late_parameters()/forward_with_cut()"
                elif not can_split:
                    why = "world size 1"
                else:
                    why = "late parameters are not a prefix of the flat buffer"
                self.overlap_note = "single all-reduce after backward (overlap requested but unavailable: %s)" % why
            else:
                self.overlap_note = "single all-reduce after backward"
            if (self.world > 1 or requested) and (not dist.is_initialized() or dist.get_rank(group) == 0):
                import sys
                print("[vqa trainer] gradient reduction: %s (world %d)" % (self.overlap_note, self.world), file=sys.stderr)
            # the per-step device words the replayed graphs read -- Adam's two step scalars (fp32) and the dropout seed of the
            # fused kernels (int64; every replay reads the current value) -- are ONE 16-byte block, refreshed by ONE
            # host-to-device copy per step (a pinned-memory copy is a blit kernel of ~8 us that the step waits for)
            self._step_block = torch.zeros(16, device=first.device, dtype=torch.uint8)
            self.step_scalars = self._step_block[:8].view(torch.float32)
            self.seed_word = self._step_block[8:].view(torch.int64)
            # pinned staging: a ring, so a slot is not rewritten while an earlier (asynchronous) copy from it may still be
            # pending on the stream
            self._ring = 8
            self._ring_events = [None] * self._ring       # recorded behind a slot's copy; waited for before it is rewritten
            self._step_block_host = torch.zeros(self._ring, 16, dtype=torch.uint8).pin_memory()
            self._step_scalars_host = self._step_block_host[:, :8].view(torch.float32)      # [ring, 2]
            self._seed_host = self._step_block_host[:, 8:].view(torch.int64)                # [ring, 1]
            self.grads = None
            self.optimizer = None
        else:
            self.grads = FlatGradients(model.parameters())
            self.optimizer = self._torch_optimizer(self.grads.params, lr)

    # optim -> the flat state buffers it keeps (FlatState)
    OPTIMS = {"adam": ("m", "v"), "sgd": ("m",), "rms": ("v",)}
    LOSSES = ("KLD", "BCE", "CE")

    def _torch_optimizer(self, params, lr):
        """train.py:286-292 (the CPU path's optimizer; on the GPU path the template of optimizer_state_dict's param group)."""
        if self.optim_kind == "sgd":
            return torch.optim.SGD(params, lr=lr, momentum=self.momentum)
        if self.optim_kind == "rms":
            return torch.optim.RMSprop(params, lr=lr, alpha=self.alpha, eps=self.eps)
        return torch.optim.Adam(params, lr=lr)

    @classmethod
    def from_config(cls, model, cf, **kw):
        """The trainer the reference driver would build from the config module ``cf``, by the defaulting rules of
        train.py:402-447 and :519-548: ``cf.sgd`` is refused, ``optim`` defaults to adam and ``lr_scheduler`` to on,
        ``samplingans`` means CE whatever ``loss_metric`` says, otherwise ``loss_metric`` (default KLD) must be BCE or KLD,
        ``clip_grad`` switches the 0.25 clip, ``lr = cf.lr``.  Keywords override what the config gives."""
        if hasattr(cf, "sgd"):
            raise ValueError('sgd has been deprecated. Please use optim')
        if not hasattr(cf, "lr"):
            raise AttributeError('lr must be set manually.')
        sampling = bool(getattr(cf, "samplingans", False))
        metric = str(cf.loss_metric) if hasattr(cf, "loss_metric") else ("CE" if sampling else "KLD")
        if sampling:
            loss = "CE"
        elif metric in ("BCE", "KLD"):
            loss = metric
        else:
            raise ValueError("<train.py> loss")
        args = dict(lr=cf.lr, clip=0.25 if getattr(cf, "clip_grad", False) else None, loss=loss,
                    optim=str(cf.optim) if hasattr(cf, "optim") else "adam",
                    lr_scheduler=bool(cf.lr_scheduler) if hasattr(cf, "lr_scheduler") else True)
        args.update(kw)
        return cls(model, **args)

    @staticmethod
    def _model_keys(sample):
        """The entries of a sample dict the models read (config/CoR2.py:203-205): feeder batches also carry the target
        'a' and 'q_id', which must not be cloned / re-copied into the graph's input buffers every step."""
        v = "v_packed" if "v_packed" in sample else "v"              # packed region batches (feed.store_batches(packed=True))
        v = "v_idx" if "v_idx" in sample else v                      # resident store: the images' indices (store_batches(resident=))
        keys = {v, "q_idxes"} if "q_idxes" in sample else {v, "q"}
        return keys | {"v_len"} if "v_len" in sample else keys       # per-sample region counts (cor2.Model.forward)

    def shard(self, tensor):
        """This rank's contiguous slice of a global-batch tensor (rank r gets [r*B/P, (r+1)*B/P)).  Per tensor, so not for the
        'v_packed' of a packed batch, whose samples are not equally long: feed.shard(batch, rank, world) shards those."""
        if self.world == 1:
            return tensor
        rank = dist.get_rank(self.group)
        per = tensor.size(0) // self.world
        return tensor[rank * per:(rank + 1) * per]

    def step(self, sample, target):
        """One training step on this rank's shard; returns (local loss tensor, global grad norm tensor).
        Replayed steps return the graph's OWN output tensors: the same two tensors every step, overwritten by the next
        replay -- read them (``.item()`` / ``.clone()``) before the next step if you keep a history; eager steps return
        fresh tensors.
        target: the dense soft answers [B,C] (KLD / BCE) or int64 labels [B] (CE) -- or the sparse pair of the feed,
        ``{"a_idx": int32 [B,K], "a_val": float32 [B,K]}`` (a whole batch dict will do: the two keys are picked out of it), from
        which KLD and BCE are computed directly and CE draws its label per row and step (``last_labels``)."""
        if isinstance(target, dict):
            target = SparseTarget(target["a_idx"], target["a_val"])
        v = sample.get("v_packed", sample.get("v"))     # (None for a resident-store batch: 'v_idx', whose counts the store holds)
        if self.hip and sample.get("v_len") is not None and v is not None and v.is_cuda:
            # per-sample region counts: validated (a host tensor) and brought to the int32 device form once, so that the graph
            # path can keep them in a static input buffer like 'v' and 'q_idxes'.  N of a packed batch is its capacity's:
            # 'v_packed' holds N rows for every entry of 'v_len'
            from . import ops
            b = sample["v_len"].size(0) if "v_packed" in sample else v.size(0)
            sample = dict(sample, v_len=ops.region_counts(sample["v_len"], v.numel() // (max(b, 1) * 2048), v.device))
        if self.hip and self.want_graph:
            return self._graph_step(sample, target)
        return self.step_eager(sample, target)

    # ---- top-k hits of the step (topk=...) --------------------------------------------------------------------------
    @property
    def last_hits(self):
        """int32 [kmax] of THIS rank's shard of the last step: hits[j] = rows whose target ranks <= j among the logits (None
        without topk).  After a replay it is the replayed graph's own output tensor (one per input slot), overwritten by that
        slot's next replay -- like the loss step() returns."""
        return self._front_out[0]

    @property
    def last_logits(self):
        """The logits [B,C] of the last step on this rank (with topk; None otherwise), under the same lifetime rule."""
        return self._front_out[1]

    @property
    def last_labels(self):
        """int64 [B]: the labels the last CE step drew from its sparse target on THIS rank (-1: a row without a positive pair;
        None for every other step), under last_hits' lifetime rule: each input slot's graph owns its tensor."""
        return self._labels

    def accuracy(self):
        """(Acc@k for k in topk), in percent, of the last step over the GLOBAL batch (CE from a sparse target: against the
        labels that step drew, as the reference's accuracy(output, a) sees its sampled a).  Synchronises with the device (the
        counts are read back), and with more than one rank it all-reduces the hit counts and the batch size -- a
        collective: every rank must call it.  step() itself never does either."""
        if not self.topk:
            raise RuntimeError("accuracy() needs a trainer created with topk=(...)")
        from . import metrics
        hits, _, batch = self._front_out
        if hits is None:
            raise RuntimeError("accuracy() before the first step")
        counts = torch.cat([hits.to(torch.int64), torch.tensor([batch], dtype=torch.int64, device=hits.device)])
        if self.world > 1:
            dist.all_reduce(counts, op=dist.ReduceOp.SUM, group=self.group)
        counts = counts.cpu()
        return tuple(metrics.accuracy(counts[:-1], int(counts[-1]), self.topk))

    def _loss_scale(self, logits):
        """BCE and CE are MEANS over the global batch in the reference (under DataParallel the criterion sees the gathered
        outputs), while the gradient all-reduce is a SUM: every rank scales by its local batch x the world size, and the
        loss it returns is its share of the global loss.  (Fixed at capture for a replayed step; a batch of another size
        runs through step_eager.)"""
        B, C = logits.shape
        return 1.0 / (B * self.world * (C if self.loss_kind == "BCE" else 1))

    def _loss_and_grad(self, logits, target):
        """(loss, dL/dlogits) of the fused loss kernel -- with topk, its variant that also counts the hits."""
        from . import ops
        if isinstance(target, SparseTarget):
            # the pairs as they are: KLD / BCE over the live pairs, CE with its label drawn on the device from the step's seed
            # (ranks that share a seed draw independently: the counter starts at rank * B_local)
            rank = dist.get_rank(self.group) if self.world > 1 else 0
            out = ops.sparse_loss_and_grad(self.loss_kind, logits, target.a_idx, target.a_val,
                                           None if self.loss_kind == "KLD" else self._loss_scale(logits),
                                           self.kmax if self.topk else None, None, rank * logits.size(0))
            self._labels = out[3] if self.loss_kind == "CE" else None
            if out[2] is not None:
                self._front_out = (out[2], logits.detach(), logits.size(0))
            return out[0], out[1]
        self._labels = None
        # CE: labels outside [0, C) are refused on the host -- except inside a capture, which reads nothing back (the
        # kernel clamps the index, so a replayed step stays in bounds whatever the labels are)
        if self.loss_kind == "CE" and not torch.cuda.is_current_stream_capturing():
            ops.check_ce_labels(logits, target)
        loss, d_logits, hits = ops._loss_and_grad(self.loss_kind, logits, target,
                                                  None if self.loss_kind == "KLD" else self._loss_scale(logits),
                                                  self.kmax if self.topk else None)
        if hits is not None:
            self._front_out = (hits, logits.detach(), logits.size(0))
        return loss, d_logits

    def _advance_lr(self):
        """scheduler.step() precedes optimizer.step() in the reference (train.py:75-86): step t uses lr0*gamma^t."""
        self.iteration += 1
        self.adam_steps += 1
        if self.lr_scheduler:          # (scheduler = None, train.py:295-298: lr stays cf.lr; the iteration still counts)
            self._lr = self.base_lr * self.gamma ** self.iteration
        return self._lr

    def _cpu_loss(self, logits, target):
        """torch's own criteria (train.py:519-548), BCE / CE as this rank's share of the mean over the global batch."""
        if self.loss_kind == "BCE":
            loss = F.binary_cross_entropy(torch.sigmoid(logits), target)
        elif self.loss_kind == "CE":
            loss = F.cross_entropy(logits, target)
        else:
            return kld_sum_loss(logits, target)
        return loss / self.world if self.world > 1 else loss

    def _cpu_sparse_loss(self, logits, target):
        """The CPU step on a sparse target -> (loss, the target the hits are counted against): KLD / BCE on the dense row it
        stands for (ops.densify), CE on labels drawn with torch.multinomial from torch's generator (-1, which adds nothing to
        loss or gradient, for a row without a positive pair)."""
        from . import ops
        C = logits.size(1)
        if self.loss_kind != "CE":
            dense = ops.densify(target.a_idx, target.a_val, C)
            return self._cpu_loss(logits, dense), dense
        w = torch.where(ops.live_pairs(target.a_idx, C), target.a_val, torch.zeros_like(target.a_val))
        drawable = w.sum(1) > 0
        pick = torch.multinomial(torch.where(drawable[:, None], w, torch.ones_like(w)), 1)[:, 0]
        labels = torch.where(drawable, target.a_idx.gather(1, pick[:, None])[:, 0].to(torch.int64), torch.full_like(pick, -1))
        self._labels = labels
        if bool(drawable.all()):
            return self._cpu_loss(logits, labels), labels
        loss = F.cross_entropy(logits, labels, ignore_index=-1, reduction="sum") / (logits.size(0) * self.world)
        return loss, labels

    def _optimizer_launch(self, lr=None):
        """The optimizer pass of the GPU tail on the clipped gradients: lr given -> a launch argument (eager steps), None ->
        read from the step block on the device (replayed steps)."""
        from . import ops
        f = self.flat
        if self.optim_kind == "sgd":
            if lr is None:
                ops.sgd_step_dyn(f.p, f.g, f.m, f.norm_and_coef, self.step_scalars, self.momentum)
            else:
                ops.sgd_step(f.p, f.g, f.m, f.norm_and_coef, lr, self.momentum)
        elif self.optim_kind == "rms":
            if lr is None:
                ops.rmsprop_step_dyn(f.p, f.g, f.v, f.norm_and_coef, self.step_scalars, self.alpha, self.eps)
            else:
                ops.rmsprop_step(f.p, f.g, f.v, f.norm_and_coef, lr, self.alpha, self.eps)
        elif lr is None:
            ops.adam_step_dyn(f.p, f.g, f.m, f.v, f.norm_and_coef, self.step_scalars, self.betas[0], self.betas[1], self.eps)
        else:
            ops.adam_step(f.p, f.g, f.m, f.v, f.norm_and_coef, lr, self.betas[0], self.betas[1], self.eps, self.adam_steps)

    def step_eager(self, sample, target):
        """The same step launched kernel by kernel (no graph replay)."""
        if self.hip:
            from . import ops
            f = self.flat
            loss = self._run_phases(sample, target, device_seed=False)
            lr = self._advance_lr()
            ops.grad_norm_clip_coef(f.g, self.clip if self.clip else 0.0, f.norm_and_coef, f.workspace)
            self._optimizer_launch(lr)
            return loss, f.norm_and_coef[0]
        logits = self.model(sample)
        self._labels = None
        if isinstance(target, SparseTarget):
            loss, target = self._cpu_sparse_loss(logits, target)
        else:
            loss = self._cpu_loss(logits, target)
        if self.topk:
            from . import metrics
            if self._labels is not None:       # a row without a label ranks C: never a hit
                rank = metrics.target_rank(logits.detach(), target.clamp(min=0))
                hits = metrics._hits_from_rank(torch.where(target < 0, logits.size(1), rank), self.kmax)
            else:
                hits = metrics.topk_hits(logits, target, self.kmax)
            self._front_out = (hits, logits.detach(), logits.size(0))
        for gp in self.optimizer.param_groups:
            gp["lr"] = self._advance_lr()
        self.grads.zero()
        loss.backward()
        self.grads.all_reduce_sum(self.group)
        norm = self.grads.clip_(self.clip) if self.clip else None
        self.optimizer.step()
        return loss.detach(), norm

    # ---- the GPU step: backward phases, each followed by the all-reduce of its gradient bucket -----------------------
    def _run_phases(self, sample=None, target=None, device_seed=True, slot=None):
        """The phases of self._phases in order, launched kernel by kernel or, given a captured input slot, replayed from
        slot[name].  After each phase but the last its bucket's sum-all-reduce is launched asynchronously (it runs under
        the next phase); the last bucket is reduced synchronously, then the pending reductions are waited for.  Nothing
        is reduced on a single rank.  -> the loss of a launched step (None for a replay)."""
        loss, pending = None, []
        for i, (name, bucket) in enumerate(self._phases):
            last = i == len(self._phases) - 1
            if slot is not None:
                slot[name].replay()
            else:
                out = self._phase(i, sample, target, device_seed)
                if i == 0:
                    loss = out
            if self.reduce:
                work = dist.all_reduce(bucket, op=dist.ReduceOp.SUM, group=self.group, async_op=not last)
                if not last:
                    pending.append(work)
        for work in pending:
            work.wait()
        return loss

    def _phase(self, i, sample, target, device_seed=True):
        """Launch phase i kernel by kernel: the first one runs the forward and the loss and returns the loss, a second one
        resumes the backward where the first stopped."""
        launch = getattr(self, "_" + self._phases[i][0])
        return launch(sample, target, device_seed) if i == 0 else launch()

    def _front(self, sample, target, device_seed=True):
        """forward + loss + backward + gradient gather: the one-phase step (graph 1)."""
        from . import ops
        f = self.flat
        if device_seed:
            ops.set_device_seed(self.seed_word)
            ops.begin_step_salts()
        try:
            logits = self.model(sample)
            loss, d_logits = self._loss_and_grad(logits, target)     # (loss and its gradient from one kernel)
        finally:
            if device_seed:
                ops.set_device_seed(None)
        f.begin_backward()
        try:
            torch.autograd.backward(logits, d_logits)
        finally:
            f.end_backward()
        f.gather_grads()
        return loss

    def _tail(self):
        """clip + the optimizer pass with the per-step scalars read from device memory (graph 2)."""
        from . import ops
        f = self.flat
        ops.grad_norm_clip_coef(f.g, self.clip if self.clip else 0.0, f.norm_and_coef, f.workspace)
        self._optimizer_launch()

    def _set_step_scalars(self):
        lr = self._advance_lr()
        slot = self.adam_steps % self._ring
        # A replayed step costs the host a few launches per ~3 ms of GPU work, so a loop that never synchronises runs far
        # ahead: without this wait the slot of step t could be rewritten with step t + ring's values before the GPU has
        # executed the copy of step t (wrong lr / bias correction, the same dropout seed twice).
        pending = self._ring_events[slot]
        if pending is not None:
            pending.synchronize()
        if self.optim_kind == "adam":
            self._step_scalars_host[slot, 0] = lr / (1.0 - self.betas[0] ** self.adam_steps)
            self._step_scalars_host[slot, 1] = 1.0 / (1.0 - self.betas[1] ** self.adam_steps) ** 0.5
        else:
            self._step_scalars_host[slot, 0] = lr         # SGD / RMSprop read the learning rate alone (word 0)
        self._seed_host[slot, 0] = int(torch.randint(0, 2 ** 62, (1,), device="cpu").item())   # torch.manual_seed governs it
        self._step_block.copy_(self._step_block_host[slot], non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        self._ring_events[slot] = done

    # ---- hipGraph replay of the step ---------------------------------------------------------------------------
    def _device_seeded_step(self, sample, target):
        """A step launched kernel by kernel with the launches, device-side seed and step scalars of a replay -> the loss."""
        self._set_step_scalars()
        loss = self._run_phases(sample, target)
        self._tail()
        return loss

    def _graph_step(self, sample, target):
        from . import ops
        f = self.flat
        g = self._graph
        if g is None:
            seeds_before = ops.host_seed_draws
            loss = self._device_seeded_step(sample, target)
            self._eager_steps += 1
            if ops.host_seed_draws != seeds_before:
                self.want_graph = False       # host-seeded dropout mask in the forward: replay would freeze it
            elif self._eager_steps >= self.EAGER_STEPS_BEFORE_CAPTURE:   # warmed up (allocator, LDS attributes, GEMM table): capture
                self._capture(sample, target)
            return loss, f.norm_and_coef[0]
        if self.model.training != g["training"] or target.shape != g["target"].shape or any(
                k not in sample or sample[k].shape != t.shape or sample[k].dtype != t.dtype for k, t in g["sample"].items()) or \
                ("v_len" in sample) != ("v_len" in g["sample"]):
            # a batch of another shape (the last one of an epoch), a batch with region counts after a capture without them (the
            # graph holds the unmasked kernels) or the other way round, a packed batch ('v_packed') or a resident-store batch
            # ('v_idx') after a capture on padded ones or the other way round (one of the captured keys is missing), or the model
            # switched between train() and eval() since the capture (dropout is baked into the graph): this step is launched
            # kernel by kernel; the captured graphs stay valid for the regular steps that follow
            return self.step_eager(sample, target)
        slot = self._slot_of(sample, target)
        if slot is None and len(self._slots) < self.input_slots:
            # a slot of the feeder's ring the step has not been captured on yet: this step runs kernel by kernel (the same
            # launches, device-side seed and step scalars as a replay), then the front is captured on the slot's tensors
            loss = self._device_seeded_step(sample, target)
            self._capture(sample, target)
            return loss, f.norm_and_coef[0]
        if slot is None:
            slot = g
            for k, t in g["sample"].items():
                if sample[k].data_ptr() != t.data_ptr():
                    t.copy_(sample[k], non_blocking=True)
            if target.data_ptr() != g["target"].data_ptr():
                g["target"].copy_(target, non_blocking=True)
        self._set_step_scalars()
        self._front_out, self._labels = slot["out"], slot["labels"]
        self._run_phases(slot=slot)
        g["tail"].replay()
        return slot["loss"], f.norm_and_coef[0]

    def _slot_of(self, sample, target):
        """The captured input slot whose tensors ARE this batch's (same addresses), or None."""
        for slot in self._slots:
            if target.data_ptr() == slot["target"].data_ptr() and all(
                    sample[k].data_ptr() == t.data_ptr() for k, t in slot["sample"].items()):
                return slot
        return None

    def _capture(self, sample, target):
        """Capture the step on this batch: the first time its phases and the tail, in a new memory pool, afterwards the
        phases once more on the tensors of a new input slot (the graphs share the pool: they never run concurrently).
        Any failure keeps training: kernel by kernel after a failed first capture, on the slots captured so far after a
        failed slot capture (further batches of that slot are copied into slot 0)."""
        first = self._graph is None
        try:
            pool = torch.cuda.graph_pool_handle() if first else self._graph["pool"]
            slot = self._capture_front(sample, target, pool)
            if first:
                tail = torch.cuda.CUDAGraph(keep_graph=True)
                with torch.cuda.graph(tail, pool=pool, capture_error_mode=slot["mode"]):
                    self._tail()
                self.graph_nodes.update(audit_and_instantiate({"tail": tail}, "step"))
                self._graph = dict(slot, tail=tail, pool=pool, training=self.model.training)
            self._slots.append(slot)
        except Exception as e:                # noqa: BLE001 -- any capture failure: keep training
            if first:
                self.want_graph = False
                then = "continuing with eager launches"
            else:
                self.input_slots = len(self._slots)
                then = "batches of input slot %d will be copied into slot 0" % len(self._slots)
            report_capture_failure("trainer", e, then)

    def _capture_front(self, sample, target, pool):
        """Capture the phases, one graph each, reading `sample` / `target` -- the caller's tensors with adopt_inputs,
        private copies otherwise.  -> the slot record."""
        static_sample = {k: (v if self.adopt_inputs else v.clone()) for k, v in sample.items()
                         if isinstance(v, torch.Tensor) and k in self._model_keys(sample)}
        if not self.adopt_inputs:
            target = target.clone()
        eager_out, eager_labels = self._front_out, self._labels     # the step that ran just before the capture stays "the last step"
        # torch's capture recipe: one forward+backward on a side stream first, so the parameters' AccumulateGrad
        # nodes belong to a capturable stream (nodes created on the default stream would run there and abort the
        # capture).  It only refills the gradient buffer; no parameter is updated.
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for i in range(len(self._phases)):
                self._phase(i, static_sample, target)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        mode = "global"
        if self.reduce:
            # the collective library's watchdog thread polls events of outstanding work; let every rank drain its
            # work list first and capture in thread-local mode so another thread's query cannot invalidate the capture
            import time
            dist.barrier(group=self.group)
            torch.cuda.synchronize()
            time.sleep(1.0)
            mode = "thread_local"
        graphs, outs = {name: torch.cuda.CUDAGraph(keep_graph=True) for name, _ in self._phases}, []
        for i, graph in enumerate(graphs.values()):
            with torch.cuda.graph(graph, pool=pool, capture_error_mode=mode):
                outs.append(self._phase(i, static_sample, target))
        captured_out, self._front_out = self._front_out, eager_out
        captured_labels, self._labels = self._labels, eager_labels
        self.graph_nodes.update(audit_and_instantiate(graphs, "step"))
        return dict(graphs, loss=outs[0], out=captured_out, labels=captured_labels, sample=static_sample, target=target, mode=mode)

    # ---- backward in two halves, the first all-reduce under the second (overlap=True) ---------------------------------
    def _front_a(self, sample, target, device_seed=True):
        """forward + loss + backward from the loss down to the cut + gather of the late parameters' gradients."""
        from . import ops
        if device_seed:
            ops.set_device_seed(self.seed_word)
            ops.begin_step_salts()
        try:
            logits, outs, ins = self.model.forward_with_cut(sample)
            loss, d_logits = self._loss_and_grad(logits, target)
        finally:
            if device_seed:
                ops.set_device_seed(None)
        live = [(o, i) for o, i in zip(outs, ins) if i.requires_grad]
        ops.set_grad_slots(self.flat.p, self.flat.g)
        try:
            grads = torch.autograd.grad(logits, self._late + [i for _, i in live], grad_outputs=d_logits, allow_unused=True)
        finally:
            ops.set_grad_slots(self.flat.p, None)
        self.flat.store_grads(self._late, grads[:len(self._late)])
        pairs = [(o, g) for (o, _), g in zip(live, grads[len(self._late):]) if g is not None]
        self._cut = ([o for o, _ in pairs], [g for _, g in pairs])
        return loss

    def _front_b(self):
        """backward from the cut to the inputs + gather of the early parameters' gradients."""
        tensors, grads_in = self._cut
        self._cut = None
        from . import ops
        ops.set_grad_slots(self.flat.p, self.flat.g)
        try:
            grads = torch.autograd.grad(tensors, self._early, grad_outputs=grads_in, allow_unused=True)
        finally:
            ops.set_grad_slots(self.flat.p, None)
        self.flat.store_grads(self._early, grads)

    @property
    def lr(self):
        return self._lr

    # ---- optimizer (re-)creation and the reference's checkpoint files -----------------------------------------------
    def _optimizer_params(self):
        # train.py:288-292: filter(lambda p: p.requires_grad, model.parameters()) -- the order of the saved state
        return [p for p in self.model.parameters() if p.requires_grad]

    def reset_optimizer(self, lr=None):
        """``optimizer, scheduler = learning_scheduler(cf)`` (train.py:286-299): fresh Adam moments and step count, the
        learning rate back at ``cf.lr`` and a scheduler that starts over."""
        if lr is not None:
            self.base_lr = lr
        self.iteration = 0
        self.adam_steps = 0
        self._lr = self.base_lr
        if self.hip:
            # fills are kernels and the moment buffers keep their addresses: a captured step stays valid
            for t in (self.flat.m, self.flat.v):
                if t is not None:
                    t.zero_()
        else:
            self.optimizer = self._torch_optimizer(self.grads.params, self.base_lr)

    def begin_epoch(self, epoch, cf):
        """The optimizer re-creation rule at the top of the reference's epoch loop (train.py:718-721): at
        ``cf.restart_epoch``, and before every epoch below ``cf.keeping_epoch``.  Returns True if it was re-created."""
        lr = getattr(cf, "lr", None)
        if hasattr(cf, "restart_epoch") and epoch == cf.restart_epoch:
            self.reset_optimizer(lr)
            return True
        if getattr(cf, "keeping_epoch", None) is not None and epoch < cf.keeping_epoch:
            self.reset_optimizer(lr)
            return True
        return False

    def optimizer_state_dict(self):
        """``optimizer.state_dict()`` of the reference's torch.optim.Adam (train.py:290, saved at :729): per-parameter
        ``step`` / ``exp_avg`` / ``exp_avg_sq`` keyed by the index of the parameter in the filtered
        ``model.parameters()`` order, one param group.  Loadable by ``torch.optim.Adam.load_state_dict``."""
        if not self.hip:
            return self.optimizer.state_dict()
        f = self.flat
        where = {id(p): (o, p) for p, o in zip(f.params, f.offsets)}
        params = self._optimizer_params()
        state = {}
        if self.optim_kind != "adam":
            # torch.optim.SGD: {momentum_buffer}; torch.optim.RMSprop: {step (a float32 scalar tensor), square_avg}; the param
            # group is the one this torch version writes for that optimizer (keys and defaults taken from a throw-away instance)
            if self.adam_steps > 0:
                for i, p in enumerate(params):
                    o, _ = where[id(p)]
                    n = p.numel()
                    if self.optim_kind == "sgd":
                        state[i] = {"momentum_buffer": f.m[o:o + n].view_as(p).clone()}
                    else:
                        state[i] = {"step": torch.tensor(float(self.adam_steps), dtype=torch.float32),
                                    "square_avg": f.v[o:o + n].view_as(p).clone()}
            group = dict(self._torch_optimizer([torch.zeros(1)], self.base_lr).state_dict()["param_groups"][0])
            group.update(lr=self._lr, initial_lr=self.base_lr, params=list(range(len(params))))
            return {"state": state, "param_groups": [group]}
        if self.adam_steps > 0:
            for i, p in enumerate(params):
                o, _ = where[id(p)]
                n = p.numel()
                state[i] = {"step": self.adam_steps,
                            "exp_avg": f.m[o:o + n].view_as(p).clone(),
                            "exp_avg_sq": f.v[o:o + n].view_as(p).clone()}
        group = {"lr": self._lr, "betas": self.betas, "eps": self.eps, "weight_decay": 0, "amsgrad": False,
                 "initial_lr": self.base_lr, "params": list(range(len(params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd):
        """``optimizer.load_state_dict`` (train.py:283).  As in the reference, the scheduler is not part of the
        checkpoint: it was created just before the load (train.py:519,:575) and starts over from ``cf.lr``, while
        Adam's moments and step count continue."""
        kind = self._state_dict_kind(sd)
        if kind != self.optim_kind:
            raise ValueError("loaded state dict belongs to optim = '%s', this trainer runs '%s'" % (kind, self.optim_kind))
        if not self.hip:
            self.optimizer.load_state_dict(sd)
            return
        f = self.flat
        where = {id(p): o for p, o in zip(f.params, f.offsets)}
        params = self._optimizer_params()
        group = sd["param_groups"][0]
        if len(sd["param_groups"]) != 1 or len(group["params"]) != len(params):
            raise ValueError("loaded state dict has a different number of parameter groups / parameters")
        if kind != "adam":
            self._load_flat_state(sd, group, params, where)
            return
        self.betas = tuple(group.get("betas", self.betas))
        self.eps = group.get("eps", self.eps)
        steps = set()
        with torch.no_grad():
            f.m.zero_()
            f.v.zero_()
            for key, p in zip(group["params"], params):
                st = sd["state"].get(key)
                if st is None:
                    continue
                if tuple(st["exp_avg"].shape) != tuple(p.shape):
                    raise ValueError("optimizer state of parameter %d has shape %s, expected %s"
                                     % (key, tuple(st["exp_avg"].shape), tuple(p.shape)))
                o, n = where[id(p)], p.numel()
                f.m[o:o + n].view_as(p).copy_(st["exp_avg"])
                f.v[o:o + n].view_as(p).copy_(st["exp_avg_sq"])
                steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter Adam step counts differ (%s): one fused step count is kept" % sorted(steps))
        self.adam_steps = steps.pop() if steps else 0
        self.iteration = 0
        self._lr = self.base_lr

    @staticmethod
    def _state_dict_kind(sd):
        """Which of the reference's optimizers wrote this state dict, from the keys only that optimizer's param group has."""
        group = sd["param_groups"][0]
        return "adam" if "betas" in group else "rms" if "alpha" in group else "sgd" if "nesterov" in group else "?"

    def _load_flat_state(self, sd, group, params, where):
        """load_optimizer_state_dict for SGD (momentum_buffer -> FlatState.m) and RMSprop (square_avg -> FlatState.v)."""
        f = self.flat
        key_name, buf = ("momentum_buffer", f.m) if self.optim_kind == "sgd" else ("square_avg", f.v)
        if self.optim_kind == "sgd":
            self.momentum = group.get("momentum", self.momentum)
        else:
            self.alpha, self.eps = group.get("alpha", self.alpha), group.get("eps", self.eps)
        steps, loaded = set(), 0
        with torch.no_grad():
            buf.zero_()
            for key, p in zip(group["params"], params):
                st = sd["state"].get(key)
                if st is None or st.get(key_name) is None:     # (SGD keeps momentum_buffer None before its first step)
                    continue
                if tuple(st[key_name].shape) != tuple(p.shape):
                    raise ValueError("optimizer state of parameter %d has shape %s, expected %s"
                                     % (key, tuple(st[key_name].shape), tuple(p.shape)))
                o, n = where[id(p)], p.numel()
                buf[o:o + n].view_as(p).copy_(st[key_name])
                loaded += 1
                if "step" in st:
                    steps.add(int(st["step"]))
        if len(steps) > 1:
            raise ValueError("per-parameter step counts differ (%s): one fused step count is kept" % sorted(steps))
        # SGD's state carries no step count: any positive one says "the buffers are live" (optimizer_state_dict writes them)
        self.adam_steps = steps.pop() if steps else (1 if loaded else 0)
        self.iteration = 0
        self._lr = self.base_lr

    def save_checkpoint(self, info, log_dir):
        """train.py:250-267: ``log_dir/epoch_<n>/ckpt_{info,model,optim}.pth.tar`` holding ``info``, the model's
        ``state_dict()`` (the reference's ``model.module.state_dict()`` names) and the optimizer state.
        Replicas are identical, so only rank 0 writes."""
        import os
        if self.world > 1 and dist.get_rank(self.group) != 0:
            return None
        path = os.path.join(log_dir, "epoch_%d" % info["epoch"])
        os.makedirs(path, exist_ok=True)
        logger = info.get("exp_logger")
        if logger is not None and hasattr(logger, "to_json"):
            logger.to_json(os.path.join(path, "logger.json"))
        torch.save(info, os.path.join(path, "ckpt_info.pth.tar"))
        torch.save({k: v.detach().cpu().clone() for k, v in self.model.state_dict().items()},
                   os.path.join(path, "ckpt_model.pth.tar"))
        optim = self.optimizer_state_dict()
        for st in optim["state"].values():
            for k, v in st.items():
                if torch.is_tensor(v):
                    st[k] = v.cpu()
        torch.save(optim, os.path.join(path, "ckpt_optim.pth.tar"))
        return path

    def load_checkpoint(self, path_ckpt):
        """train.py:270-284; returns ``info['exp_logger']`` like the reference (None if the file holds none)."""
        import os
        info = torch.load(os.path.join(path_ckpt, "ckpt_info.pth.tar"), weights_only=False)
        model_state = torch.load(os.path.join(path_ckpt, "ckpt_model.pth.tar"), map_location="cpu")
        self.model.load_state_dict(model_state)      # copies into the flat parameter buffer's views
        self.load_optimizer_state_dict(torch.load(os.path.join(path_ckpt, "ckpt_optim.pth.tar"), map_location="cpu"))
        return info.get("exp_logger") if isinstance(info, dict) else None
