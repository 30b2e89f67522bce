"""Kernel-level parity of the grouped head's three entry points (K6: vqa_grouped_gemm, vqa_grouped_gemm_split,
vqa_grouped_epilogue; csrc/grouped_gemm.hip, csrc/grouped_gemm_split.hip) with job / problem tables built BY HAND, so the
tests choose S, ksplit, strides, offsets and the path (slab or direct output) themselves:

  A  every epilogue kind on slabs the test wrote, against an fp32 restatement in the kernel's order (bitwise where the
     arithmetic is adds and one multiply) or float64; 8-byte against 4-byte accesses; 24 mixed jobs in one launch; the
     row-index arithmetic next to its 2^24 limit
  B  the direct-output path of both engines against slab + epilogue (bitwise) and against float64
  C  zero-padded operand extents (Ka, Kb, Ma, Nb) with NaN behind the valid extent
  D  head.Phase takes the path it says (Phase.DIRECT)
  E  refusals

Every buffer a kernel writes is allocated two floats and one row larger than the window it may write, pre-filled with a
sentinel, and must still hold the sentinel outside the window afterwards.  (`out` of RANK_PRODUCT and out / out2 of
RANK_PRODUCT_BWD are dense by the ABI -- row stride N resp. R*N -- so their spare room is the row and the floats behind.)"""
import ctypes
import math

import numpy as np
import pytest
import torch

from kernel_harness import E_BADARG, E_UNSUPPORTED, SENT, dev

pytestmark = pytest.mark.gpu
RTOL = 2e-4            # fp32 products against float64, on the output's scale (tests/test_gpu_head.py)
U = 2.0 ** -24         # fp32 unit roundoff
SUM, LINEAR, RANK_PRODUCT, GRAD, RANK_PRODUCT_BWD = 0, 1, 2, 3, 4
NT, NN, TN, NN_A4, TN_A4 = 0, 1, 2, 3, 4


def mods():
    from vqa_playground_pytorch_amd import _lib, head, ops
    return _lib, head, ops


class Win:
    """A [M, N] window of row stride ld at element offset off of a flat sentinel-filled buffer that ends one row and two
    floats behind the window."""

    def __init__(self, M, N, ld=None, off=0, data=None, fill=SENT):
        self.M, self.N, self.ld, self.off = int(M), int(N), int(N if ld is None else ld), int(off)
        assert self.ld >= self.N
        self.fill = fill
        self.buf = torch.full((self.off + (self.M + 1) * self.ld + 2,), fill, device=dev(), dtype=torch.float32)
        if data is not None:
            self.view().copy_(torch.as_tensor(np.ascontiguousarray(data, dtype=np.float32)).view(self.M, self.N))

    def view(self):
        return self.buf.as_strided((self.M, self.N), (self.ld, 1), self.off)

    def ptr(self):
        return self.buf.data_ptr() + 4 * self.off

    def get(self):
        return self.view().cpu().numpy()

    def assert_outside_untouched(self, name):
        b = self.buf.clone()
        b.as_strided((self.M, self.N), (self.ld, 1), self.off).fill_(self.fill)
        assert bool((b == self.fill).all()), "%s: a store outside its [%d,%d] window (ld %d, offset %d)" % (
            name, self.M, self.N, self.ld, self.off)

    def assert_untouched(self, name):
        assert bool((self.buf == self.fill).all()), "%s was written" % name


def launch(name, fn, arr, n):
    """One C-ABI call through ops._launch -> [(grid in work-items, kernel), ...] of the device launches it made."""
    _lib, _, ops = mods()
    L = _lib.lib()
    L.vqa_launch_log_reset()
    ops._launch(name, ("test", n), fn, arr, n)
    buf = (ctypes.c_ulonglong * 16)()
    k = L.vqa_launch_log(buf, 16)
    return [(int(buf[i]), (L.vqa_launch_log_kernel(i) or b"").decode()) for i in range(min(k, 16))]


def refused(name, fn, arr, n, code):
    """The call returns `code` and launches nothing."""
    _lib, _, ops = mods()
    L = _lib.lib()
    L.vqa_launch_log_reset()
    with pytest.raises(_lib.VqaLibraryError, match=r"failed \(%d\)" % code):
        ops._launch(name, ("refused", n), fn, arr, n)
    assert L.vqa_launch_log((ctypes.c_ulonglong * 16)(), 16) == 0, "%s: a refused call launched a kernel" % name
    torch.cuda.synchronize()


def keep_factors(p, seed, drop_base, drop_ld, M, W):
    """[M, W] fp32 keep / (1-p) factors of elements drop_base + m*drop_ld + n: the exported mask of a dense [rows, drop_ld]
    tensor (the header's definition of `keep`).  The exporter takes even widths only; a mask element is a function of the
    seed and its FLAT index alone, so for an odd drop_ld the same flat range is exported as a two-column tensor."""
    if not p:
        return np.ones((M, W), np.float32)
    _, _, ops = mods()
    rows = (drop_base + M * drop_ld) // drop_ld + 1
    shape = (rows, drop_ld) if drop_ld % 2 == 0 else ((rows * drop_ld + 1) // 2, 2)
    flat = ops.linear_dropout_mask(shape[0], shape[1], p, seed, dev()).flatten().cpu().numpy()
    p8 = int(p * 256 + 0.5)
    scale = np.float32(256.0) / np.float32(256.0 - p8)      # (make_drop, csrc/common.hpp)
    assert set(np.unique(flat).tolist()) <= {0.0, float(scale)}
    idx = drop_base + np.arange(M)[:, None] * drop_ld + np.arange(W)[None, :]
    return flat[idx]


class SigmoidBar:
    """The sigmoid bars are not fixed numbers: they rest on the device's expf.  Over the inputs of one test this collects
    torch's own fp32 error against float64 and the kernel's; the kernel is held to four times torch's."""

    def __init__(self):
        self.torch_err, self.kernel_err = 0.0, 0.0

    def add(self, torch_err, kernel_err):
        self.torch_err, self.kernel_err = max(self.torch_err, float(torch_err)), max(self.kernel_err, float(kernel_err))

    def finish(self, measured, name):
        if self.torch_err == 0.0 and self.kernel_err == 0.0:
            return
        measured(name + " torch fp32", self.torch_err)
        measured(name + " kernel", self.kernel_err, 4 * self.torch_err, "(4 x torch's %.3e)" % self.torch_err)
        assert self.kernel_err <= 4 * self.torch_err, "%s: %.3e against 4 x %.3e" % (name, self.kernel_err, self.torch_err)


def sigmoid_errors(z32, keep, got):
    """LINEAR act 2: (torch's fp32 sigmoid(z) * keep, the kernel's output) against float64, absolute."""
    zt, kt = torch.from_numpy(z32).to(dev()), torch.from_numpy(keep).to(dev())
    ref = keep.astype(np.float64) / (1.0 + np.exp(-z32.astype(np.float64)))
    t = (torch.sigmoid(zt) * kt).cpu().numpy().astype(np.float64)
    return np.abs(t - ref).max(), np.abs(got.astype(np.float64) - ref).max()


def sigmoid_gate_errors(s32, y, keep, got):
    """GRAD gate 2: (torch's fp32 s * (y * (1 - y)) * keep, the kernel's output) against float64, relative to |s|."""
    st, yt, kt = (torch.from_numpy(a).to(dev()) for a in (s32, y, keep))
    s64, y64 = s32.astype(np.float64), y.astype(np.float64)
    ref = s64 * (y64 * (1.0 - y64)) * keep
    t = (st * (yt * (1.0 - yt)) * kt).cpu().numpy().astype(np.float64)
    unit = np.abs(s64)
    assert (unit > 0).all()
    return (np.abs(t - ref) / unit).max(), (np.abs(got.astype(np.float64) - ref) / unit).max()


# ================================================================================================ A: the epilogue kernel
class EpiCase:
    """One epilogue job on slabs the test wrote.  W is the width a row's threads cover: N for SUM / LINEAR / GRAD /
    RANK_PRODUCT_BWD, H = N / R for RANK_PRODUCT.  The data depend on (kind, M, W, S, R, act, gate, tag) only -- never on
    strides, offsets or paddings -- so two cases that differ in layout alone hold the same window contents."""

    def __init__(self, kind, M, W, S=2, R=1, act=0, bias=False, gate=0, gate_scale=1.0, p=0.0, seed=0x123456789ABC,
                 dev_seed=False, stride_pad=0, slab_off=0, ldo_pad=2, out_off=2, out2_off=2, ld_aux_pad=2, aux_off=2,
                 aux2_off=2, drop_ld_pad=2, drop_base=6, tag=0):
        self.kind, self.M, self.W, self.S, self.R = kind, M, W, S, R
        self.act, self.gate, self.gate_scale, self.p, self.seed, self.dev_seed = act, gate, float(gate_scale), float(p), seed, dev_seed
        N = self.N = R * W if kind == RANK_PRODUCT else W
        rng = np.random.RandomState([kind, M, W, S, R, act, gate, tag])
        self.slab_np = rng.standard_normal((S, M, N)).astype(np.float32)
        self.bias_np = (rng.standard_normal(N).astype(np.float32) if bias and kind in (LINEAR, RANK_PRODUCT) else None)
        self.stride = M * N + stride_pad
        self.slab = torch.full((slab_off + (S - 1) * self.stride + (M + 1) * N + 2,), SENT, device=dev())
        for s in range(S):
            lo = slab_off + s * self.stride
            self.slab[lo:lo + M * N] = torch.from_numpy(self.slab_np[s].reshape(-1))
        self.slab_ptr = self.slab.data_ptr() + 4 * slab_off
        self.bias = Win(1, N, data=self.bias_np) if self.bias_np is not None else None
        self.aux = self.aux2 = self.out2 = None
        self.aux_np = self.aux2_np = None
        self.ldo = (R * N if kind == RANK_PRODUCT_BWD else W) + ldo_pad
        wide = R * N if kind == RANK_PRODUCT_BWD else N          # width of aux / aux2
        self.ld_aux = wide + ld_aux_pad
        if kind == RANK_PRODUCT or kind == RANK_PRODUCT_BWD or (kind == GRAD and gate):
            a = rng.standard_normal((M, wide)).astype(np.float32)
            if kind == GRAD and gate == 1:
                a[rng.random_sample(a.shape) < 0.1] = 0.0        # y == 0: gated off
            if kind == GRAD and gate == 2:
                a = rng.uniform(0.02, 0.98, a.shape).astype(np.float32)
            self.aux_np, self.aux = a, Win(M, wide, self.ld_aux, aux_off, a)
        if kind == RANK_PRODUCT_BWD:
            self.aux2_np = rng.standard_normal((M, wide)).astype(np.float32)
            self.aux2 = Win(M, wide, self.ld_aux, aux2_off, self.aux2_np)
        if kind == RANK_PRODUCT:
            self.out, self.out2 = Win(M, N, N, out_off), Win(M, W, self.ldo, out2_off)
        elif kind == RANK_PRODUCT_BWD:
            self.out, self.out2 = Win(M, R * N, R * N, out_off), Win(M, R * N, R * N, out2_off)
        else:
            self.out = Win(M, N, self.ldo, out_off)
        self.drop_ld, self.drop_base = W + drop_ld_pad, drop_base
        self.word = None
        if dev_seed:
            self.salt = 77
            self.word = torch.tensor([seed - self.salt], device=dev(), dtype=torch.int64)

    def __repr__(self):
        return "kind %d [%d,%d] S=%d R=%d act=%d gate=%d p=%g stride=%d ldo=%d ld_aux=%d drop=%d+%d" % (
            self.kind, self.M, self.N, self.S, self.R, self.act, self.gate, self.p, self.stride, self.ldo, self.ld_aux,
            self.drop_base, self.drop_ld)

    def job(self):
        _, h, ops = mods()
        sv, sp = ops._seed_args((self.word, self.salt) if self.dev_seed else self.seed) if self.p else (0, None)
        opt = lambda w: w.ptr() if w is not None else None  # noqa: E731
        return h.EpilogueJob(slab=self.slab_ptr, bias=opt(self.bias), aux=opt(self.aux), aux2=opt(self.aux2), out=self.out.ptr(),
                             out2=opt(self.out2), seed_ptr=sp.value if sp is not None else None, seed=sv, slab_stride=self.stride,
                             S=self.S, M=self.M, N=self.N, kind=self.kind, ldo=self.ldo, ld_aux=self.ld_aux, act=self.act,
                             gate=self.gate, R=self.R, seg=0, seg_ld=0, drop_base=self.drop_base, drop_ld=self.drop_ld,
                             p_drop=self.p, gate_scale=self.gate_scale)

    def v2(self):
        """The launcher's rule for 8-byte accesses, restated (the tests check it through the launch's grid size)."""
        j = self.job()
        even = lambda *v: all(int(x) % 2 == 0 for x in v)  # noqa: E731
        al8 = lambda p: p is None or p % 8 == 0  # noqa: E731
        return (even(self.W, j.N, j.ldo, j.ld_aux, j.slab_stride, j.drop_ld, j.drop_base) and al8(j.slab) and al8(j.out) and
                al8(j.out2) and al8(j.aux) and al8(j.aux2) and (self.kind != RANK_PRODUCT_BWD or even(j.R * j.N)))

    def threads(self):
        return self.M * (self.W // (2 if self.v2() else 1))

    def run(self):
        _lib, h, _ = mods()
        arr = (h.EpilogueJob * 1)(self.job())
        log = launch("grouped_epilogue", _lib.lib().vqa_grouped_epilogue, arr, 1)
        assert len(log) == 1 and log[0][0] == (self.threads() + 255) // 256 * 256, (repr(self), log, self.v2())
        return self

    def outputs(self):
        o = {"out": self.out.get()}
        if self.out2 is not None:
            o["out2"] = self.out2.get()
        return o

    def fsum(self):
        a = self.slab_np[0].copy()
        for s in range(1, self.S):
            a = a + self.slab_np[s]                                  # fp32, slab 0 + slab 1 + ...
        return a

    def check(self, sig=None):
        """Sentinels, then the job's own reference.  -> worst error / bar of the bounded (not bitwise) kinds."""
        name = repr(self)
        self.out.assert_outside_untouched(name + " out")
        if self.out2 is not None:
            self.out2.assert_outside_untouched(name + " out2")
        assert bool((self.slab[-(self.N + 2):] == SENT).all())
        got = self.outputs()
        assert all(np.isfinite(v).all() for v in got.values()), name
        M, W, R, N = self.M, self.W, self.R, self.N
        s = self.fsum()
        keep = keep_factors(self.p, self.seed, self.drop_base, self.drop_ld, M, W)
        b = self.bias_np if self.bias_np is not None else np.zeros(N, np.float32)
        k = self.kind
        if k == SUM:
            assert np.array_equal(got["out"], s), name
        elif k == LINEAR:
            z = s + b[None, :]
            if self.act == 2:
                sig.add(*sigmoid_errors(z, keep, got["out"]))
            else:
                want = (np.maximum(z, np.float32(0)) if self.act == 1 else z) * keep
                assert np.array_equal(got["out"], want), name
        elif k == GRAD:
            if self.gate == 2:
                sig.add(*sigmoid_gate_errors(s, self.aux_np, keep, got["out"]))
            else:
                z = s if self.gate == 0 else np.where(self.aux_np > 0, s * np.float32(self.gate_scale), np.float32(0))
                assert np.array_equal(got["out"], z * keep), name
        elif k == RANK_PRODUCT:
            h1 = s + b[None, :]
            assert np.array_equal(got["out"], h1), name + ": stored h1"
            h64, a64 = h1.astype(np.float64).reshape(M, R, W), self.aux_np.astype(np.float64).reshape(M, R, W)
            ref, scale = keep * (h64 * a64).sum(1), keep * (np.abs(h64) * np.abs(a64)).sum(1)
            err = np.abs(got["out2"] - ref)
            bar = (R + 2) * U * scale
            assert (err <= bar).all(), "%s: out2 off by %.3e of sum |h1||aux| (bar %.3e)" % (
                name, (err / np.maximum(scale, 1e-300)).max(), (R + 2) * U)
            return float((err / np.maximum(bar, 1e-300)).max())
        else:
            g64 = (keep.astype(np.float64) * s.astype(np.float64))[:, None, :]
            worst = 0.0
            for key, a in (("out", self.aux_np), ("out2", self.aux2_np)):
                ref = g64 * a.astype(np.float64).reshape(M, R, W)
                err = np.abs(got[key].reshape(M, R, W) - ref)
                assert (err <= 3 * U * np.abs(ref)).all(), "%s: %s off by %.3e relative (bar %.3e)" % (
                    name, key, (err / np.maximum(np.abs(ref), 1e-300)).max(), 3 * U)
                worst = max(worst, float((err / np.maximum(3 * U * np.abs(ref), 1e-300)).max()))
            return worst
        return 0.0


KINDS = {"sum": dict(kind=SUM)}
for _a in (0, 1, 2):
    for _b in (False, True):
        KINDS["linear_act%d%s" % (_a, "_bias" if _b else "")] = dict(kind=LINEAR, act=_a, bias=_b)
for _r in (1, 2, 5):
    KINDS["rank_product_R%d" % _r] = dict(kind=RANK_PRODUCT, R=_r, bias=_r != 2)
    KINDS["rank_product_bwd_R%d" % _r] = dict(kind=RANK_PRODUCT_BWD, R=_r)
KINDS.update(grad_gate0=dict(kind=GRAD), grad_relu_scale1=dict(kind=GRAD, gate=1, gate_scale=1.0),
             grad_relu_scale2=dict(kind=GRAD, gate=1, gate_scale=2.0), grad_sigmoid=dict(kind=GRAD, gate=2))
SHAPES = [(1, 2), (1, 1), (5, 155), (512, 310), (130, 2000), (1, 310)]     # (1, 310): a bias gradient


@pytest.mark.parametrize("cfg", list(KINDS))
def test_epilogue_kind_against_reference(cfg, measured):
    """One kind at every shape x S in {1, 2, 7} x p_drop in {0, 0.5, 0.25}, slab_stride = M*N / + 6 / + 7 (a Latin square
    over S and p), the seed as a host value and as device word + salt (same result, bit for bit).  SUM, LINEAR act 0 / 1 and
    GRAD gate 0 / 1 bitwise against the fp32 restatement (slab 0 + slab 1 + ..., + bias, relu, * gate_scale, * keep: adds and
    single multiplies, nothing a compiler may contract); RANK_PRODUCT within (R + 2) 2^-24 of sum_r |h1||aux| (R fmas and the
    keep multiply; h1 bitwise); RANK_PRODUCT_BWD within 3 * 2^-24 relative (two multiplies); the sigmoid forms within four
    times torch's own fp32 error on the same inputs."""
    sig, worst = SigmoidBar(), 0.0
    for si, (M, W) in enumerate(SHAPES):
        for Si, S in enumerate((1, 2, 7)):
            for pi, p in enumerate((0.0, 0.5, 0.25)):
                pad = (0, 6, 7)[(si + Si + pi) % 3]
                dev_seed = bool((si + Si + pi) & 1)
                case = EpiCase(M=M, W=W, S=S, p=p, stride_pad=pad, dev_seed=dev_seed, seed=0x123456789ABC + 1000 * si + Si,
                               **KINDS[cfg]).run()
                worst = max(worst, case.check(sig))
                if p:
                    other = EpiCase(M=M, W=W, S=S, p=p, stride_pad=pad, dev_seed=not dev_seed, seed=case.seed, **KINDS[cfg]).run()
                    a, b = case.outputs(), other.outputs()
                    for key in a:
                        assert np.array_equal(a[key], b[key]), "%r: device word + salt != host seed (%s)" % (case, key)
    sig.finish(measured, "sigmoid " + cfg)
    if KINDS[cfg]["kind"] in (RANK_PRODUCT, RANK_PRODUCT_BWD):
        measured(cfg + " worst error / bar", worst, 1.0)


PARITY = [("odd N", dict(W=61), False), ("odd ldo", dict(ldo_pad=3), True), ("odd ld_aux", dict(ld_aux_pad=3), True),
          ("odd drop_ld", dict(drop_ld_pad=3), False), ("odd drop_base", dict(drop_base=7), False),
          ("odd slab_stride", dict(stride_pad=1), True), ("slab at an odd offset", dict(slab_off=1), True),
          ("out at an odd offset", dict(out_off=3), True), ("out2 at an odd offset", dict(out2_off=3), True),
          ("aux at an odd offset", dict(aux_off=3), True), ("aux2 at an odd offset", dict(aux2_off=3), True)]


@pytest.mark.parametrize("cfg", list(KINDS))
def test_epilogue_access_width(cfg, measured):
    """One even base case per kind ([9, 62] columns, S = 2, p = 0.5: 8-byte accesses, drop_pair), then ONE parity changed at a
    time so that the job drops to 4-byte accesses and drop_one (seen in the launch's grid size: 9 * 62 threads instead of
    9 * 31).  Each varied case against its own reference; where only the layout moved, against the even case bit for bit --
    the two widths do the same arithmetic in the same order, the sigmoid forms included.  Every pointer stays 4-byte aligned
    and inside its allocation."""
    sig = SigmoidBar()
    kw = dict(M=9, W=62, S=2, p=0.5, **KINDS[cfg])
    base = EpiCase(**kw).run()
    assert base.v2() and base.threads() == 9 * 31
    base.check(sig)
    want = base.outputs()
    used = {"out2": base.out2 is not None, "aux ": base.aux is not None, "aux2": base.aux2 is not None}
    for name, change, same_data in PARITY:
        if not used.get(name[:4], True):
            continue
        case = EpiCase(**{**kw, **change}).run()
        assert not case.v2() and case.threads() == 9 * case.W, name
        case.check(sig)
        if same_data:
            got = case.outputs()
            for key in want:
                assert np.array_equal(got[key], want[key]), "%s, %s: 4-byte accesses differ from 8-byte accesses" % (name, key)
    if KINDS[cfg]["kind"] == RANK_PRODUCT_BWD:     # R*N odd with an odd R; even with an even R (N odd either way)
        case = EpiCase(**{**kw, "W": 61}).run()
        assert (case.R * case.N) % 2 == case.R % 2 and not case.v2()
    sig.finish(measured, "sigmoid " + cfg)


def test_epilogue_full_launch_of_mixed_jobs(measured):
    """VQA_GROUPED_MAX jobs in one launch, kinds and access widths mixed, job boundaries inside a wavefront, a thread count
    that is no multiple of 256: every job gives what it gives when launched alone, bit for bit (and the lone launch is
    held to its reference)."""
    _lib, h, _ = mods()
    cfgs = list(KINDS)
    dims = [(3, 10), (5, 31), (7, 22), (2, 62), (9, 155), (4, 6), (11, 14), (1, 310)]
    sig = SigmoidBar()

    def make(i):
        M, W = dims[i % len(dims)]
        return EpiCase(M=M, W=W, S=1 + i % 3, p=(0.0, 0.5, 0.25)[i % 3], out_off=2 + (i % 5 == 0), drop_base=6 + (i % 7 == 0),
                       dev_seed=bool(i & 1), tag=i, **KINDS[cfgs[i % len(cfgs)]])

    alone = [make(i).run() for i in range(24)]
    for c in alone:
        c.check(sig)
    group = [make(i) for i in range(24)]
    assert len({c.kind for c in group}) == 5 and {c.v2() for c in group} == {False, True}
    first = np.cumsum([0] + [c.threads() for c in group])
    assert first[-1] % 256 != 0 and all(f % 64 != 0 for f in first[1:-1]), first
    arr = (h.EpilogueJob * 24)(*[c.job() for c in group])
    log = launch("grouped_epilogue", _lib.lib().vqa_grouped_epilogue, arr, 24)
    assert len(log) == 1 and log[0][0] == (int(first[-1]) + 255) // 256 * 256, (log, first[-1])
    for i, (a, g) in enumerate(zip(alone, group)):
        g.out.assert_outside_untouched("job %d out" % i)
        if g.out2 is not None:
            g.out2.assert_outside_untouched("job %d out2" % i)
        wa, wg = a.outputs(), g.outputs()
        for key in wa:
            assert np.array_equal(wa[key], wg[key]), "job %d (%r), %s: differs from the same job launched alone" % (i, g, key)
    sig.finish(measured, "sigmoid mixed jobs")


def _copy_job(h, M, N, slab, out):
    return h.EpilogueJob(slab=slab.ptr(), out=out.ptr(), slab_stride=M * N, S=1, M=M, N=N, kind=SUM, ldo=out.ld, ld_aux=0,
                         R=1, drop_base=0, drop_ld=0, p_drop=0.0, gate_scale=1.0)


def test_epilogue_row_index_next_to_its_limit():
    """A thread finds its row as (int)((e + 0.5) * (1 / threads_per_row)) with a +-1 correction, valid while
    M * threads_per_row < 2^24 (a float holds e exactly).  Two SUM jobs, S = 1, in one launch: N = 1 with M = 2^24 - 1 (the
    product rounds to the neighbouring row for every odd e above 2^23) and N = 3 with the largest M below the limit.  The
    output equals the input row for row; nothing outside it is written.  One job AT the limit is refused."""
    _lib, h, _ = mods()
    shapes = [((1 << 24) - 1, 1), (((1 << 24) - 1) // 3, 3)]
    assert 3 * shapes[1][0] < (1 << 24) <= 3 * (shapes[1][0] + 1)
    slabs, outs = [], []
    for M, N in shapes:
        s = Win(M, N, N, 2)
        s.view().copy_(torch.randn(M, N, device=dev()))
        slabs.append(s)
        outs.append(Win(M, N, N + 2, 2))
    arr = (h.EpilogueJob * 2)(*[_copy_job(h, M, N, s, o) for (M, N), s, o in zip(shapes, slabs, outs)])
    launch("grouped_epilogue", _lib.lib().vqa_grouped_epilogue, arr, 2)
    torch.cuda.synchronize()
    for (M, N), s, o in zip(shapes, slabs, outs):
        wrong = (o.view() != s.view()).any(1)
        assert not bool(wrong.any()), "[%d,%d]: %d rows differ, the first at %d" % (M, N, int(wrong.sum()), int(wrong.nonzero()[0]))
        o.assert_outside_untouched("[%d,%d] copy" % (M, N))
    del slabs, outs
    M = 1 << 24
    s, o = Win(M, 1, 1, 2, fill=1.0), Win(M, 1, 3, 2)
    refused("grouped_epilogue", _lib.lib().vqa_grouped_epilogue, (h.EpilogueJob * 1)(_copy_job(h, M, 1, s, o)), 1, E_UNSUPPORTED)
    o.assert_untouched("the output of a job over the limit")


# ================================================================================================ B, C: the GEMM kernels
ENGINES = ["mfma64", "mfma128", "split"]


@pytest.fixture(params=ENGINES)
def engine(request, lib_option):
    """(name, launcher, contraction step): vqa_grouped_gemm at both tile heights (VQA_GROUPED_BM), vqa_grouped_gemm_split."""
    _lib, _, _ = mods()
    L = _lib.lib()
    if request.param == "split":
        return "split", "grouped_gemm_split", L.vqa_grouped_gemm_split, 32
    lib_option("VQA_GROUPED_BM", "128" if request.param == "mfma128" else "64")
    return request.param, "grouped_gemm", L.vqa_grouped_gemm, 16


def gemm_expected_items(name, probs):
    """Work items of a launch: tiles x contraction parts (seen in the grid: says which tile height / width ran)."""
    _lib, _, _ = mods()
    items = 0
    for p in probs:
        parts = math.ceil(p.K / p.ksplit)
        if name == "split":
            bn = _lib.lib().vqa_grouped_gemm_split_tile_cols(p.N)
            items += math.ceil(p.M / 128) * math.ceil(p.N / bn) * parts
        else:
            items += math.ceil(p.M / (128 if name == "mfma128" else 64)) * math.ceil(p.N / 64) * parts
    return items * (512 if name == "split" else 256)


def launch_gemm(engine, probs):
    _, h, _ = mods()
    name, call, fn, _ = engine
    arr = (h.GemmProblem * len(probs))(*probs)
    log = launch(call, fn, arr, len(probs))
    assert len(log) == 1 and log[0][0] == gemm_expected_items(name, probs), (name, log)


def operand_shapes(form, M, N, K):
    """(rows, cols) of A and B as they lie in memory"""
    a = (K, M) if form in (TN, TN_A4) else (M, K)
    b = (N, K) if form == NT else (K, N)
    return a, b


def product64(form, a, b):
    a, b = a.double(), b.double()
    if form in (TN, TN_A4):
        a = a.t()
    return a @ (b.t() if form == NT else b)


DIRECT_CASES = {
    # form: (shapes (M, N, K), epilogue variants (act, gate, p_drop))
    "NT": (NT, [(1, 155, 16), (77, 310, 310), (130, 62, 2400), (512, 2000, 48), (512, 155, 620), (130, 310, 1240)],
           [(a, 0, p) for a in (0, 1, 2) for p in (0.0, 0.5)]),
    "NN": (NN, [(1, 310, 16), (77, 62, 310), (130, 2000, 154), (512, 310, 2400), (512, 62, 620)],
           [(0, g, p) for g in (0, 1, 2) for p in (0.0, 0.5)]),
    "TN": (TN, [(130, 310, 512), (512, 62, 77), (130, 2000, 130), (2, 62, 16)], [(0, 0, 0.0)]),
    "TN_A4": (TN_A4, [(77, 310, 130), (1, 62, 16), (155, 310, 512), (512, 2000, 77)], [(0, 0, 0.0)]),
    "NN_A4": (NN_A4, [(77, 310, 154), (130, 62, 155), (1, 2000, 16), (512, 310, 2399)], [(0, 0, 0.0), (0, 1, 0.5), (0, 2, 0.5)]),
}


@pytest.mark.parametrize("form_name", list(DIRECT_CASES))
def test_direct_output_against_slab_path_and_float64(engine, form_name, measured):
    """The same product twice with the contraction in one part: finished inside the GEMM kernel (out set: bias, activation,
    the gate of the layer in front, dropout, colsum_out), and into a slab followed by the matching epilogue job.  The two are
    equal bit for bit for act 0 / 1, gate 0 / 1 and the column sums -- the accumulators are the same and what follows is the
    same adds and single multiplies in the same order -- and within the measured sigmoid bar for act 2 / gate 2; both within
    RTOL of the float64 layer (relu decided by the float64 pre-activation, kept 1e-4 away from 0 by redrawing weights).
    ldo > N at a non-zero out_off (even, and odd: the split engine's scalar stores on an even width), ld_gate != N,
    drop_base != 0 with drop_ld != N; the A4 forms read A at an odd element offset with an odd row stride."""
    _lib, h, ops = mods()
    name, _, _, step = engine
    form, shapes, variants = DIRECT_CASES[form_name]
    sig, worst, count = SigmoidBar(), {"direct": 0.0, "slab": 0.0}, 0
    for ci, (M, N, K) in enumerate(shapes):
        rng = np.random.RandomState([form, M, N, K])
        (ar, ac), (br, bc) = operand_shapes(form, M, N, K)
        a_np = rng.standard_normal((ar, ac)).astype(np.float32)
        scale = 1.0 / math.sqrt(K)
        b_np = (rng.standard_normal((br, bc)) * scale).astype(np.float32)
        bias_np = rng.standard_normal(N).astype(np.float32) if form == NT else None
        if form == NT:      # keep the pre-activations away from 0: redraw the weight rows of the columns that come close
            for _ in range(50):
                z = a_np.astype(np.float64) @ b_np.astype(np.float64).T + bias_np
                close_cols = (np.abs(z) < 1e-4).any(0)
                if not close_cols.any():
                    break
                b_np[close_cols] = (rng.standard_normal((int(close_cols.sum()), K)) * scale).astype(np.float32)
            assert not close_cols.any()
        a4 = form in (NN_A4, TN_A4)
        assert (a4 or ac % 2 == 0) and bc % 2 == 0
        A = Win(ar, ac, ac + 3 - ac % 2, 1, a_np) if a4 else Win(ar, ac, ac + 2, 0, a_np)     # A4: odd offset, odd row stride
        B = Win(br, bc, bc + 2, 0, b_np)
        bias = Win(1, N, data=bias_np) if bias_np is not None else None
        y_np = rng.standard_normal((M, N)).astype(np.float32)
        y_np[rng.random_sample(y_np.shape) < 0.1] = 0.0
        ksplit = (K + step - 1) // step * step
        for vi, (act, gate, p) in enumerate(variants):
            out_off = 6 + ((ci + vi) % 3 == 2)
            ldo, ld_gate, drop_ld, drop_base, seed = N + 2 + (ci + vi) % 2, N + 3, N + 5, 11, 987654321 + ci
            gy_np = rng.uniform(0.02, 0.98, (M, N)).astype(np.float32) if gate == 2 else y_np
            gate_y = Win(M, N, ld_gate, 3, gy_np) if gate else None
            gate_scale = 2.0 if gate == 1 else 1.0
            colsum = form in (TN, TN_A4)
            common = dict(A=A.ptr(), B=B.ptr(), lda=A.ld, ldb=B.ld, M=M, N=N, K=K, form=form, ksplit=ksplit, slab_base=0)
            # direct
            out_d = Win(M, N, ldo, out_off)
            cs_d = Win(1, M, M + 2, 2) if colsum else None
            launch_gemm(engine, [h.GemmProblem(out=out_d.ptr(), colsum_out=cs_d.ptr() if colsum else None,
                                               bias=bias.ptr() if bias else None, gate_y=gate_y.ptr() if gate else None,
                                               seed=seed, ldo=ldo, ld_gate=ld_gate, act=act, gate=gate, drop_base=drop_base,
                                               drop_ld=drop_ld, p_drop=p, gate_scale=gate_scale, **common)])
            # slab + epilogue
            slab = Win(M, N, N, 0)
            cs_slab = Win(1, M, M, 0) if colsum else None
            launch_gemm(engine, [h.GemmProblem(slab=slab.ptr(), slab_stride=M * N, colsum=cs_slab.ptr() if colsum else None, **common)])
            slab.assert_outside_untouched("slab")
            out_s = Win(M, N, ldo, out_off)
            jobs = [h.EpilogueJob(slab=slab.ptr(), bias=bias.ptr() if bias else None, aux=gate_y.ptr() if gate else None,
                                  out=out_s.ptr(), seed=seed, slab_stride=M * N, S=1, M=M, N=N,
                                  kind=LINEAR if form == NT else (GRAD if form in (NN, NN_A4) else SUM), ldo=ldo, ld_aux=ld_gate,
                                  act=act, gate=gate, R=1, drop_base=drop_base, drop_ld=drop_ld, p_drop=p, gate_scale=gate_scale)]
            cs_s = Win(1, M, M + 2, 2) if colsum else None
            if colsum:
                cs_slab.assert_outside_untouched("colsum slab")
                jobs.append(h.EpilogueJob(slab=cs_slab.ptr(), out=cs_s.ptr(), slab_stride=M, S=1, M=1, N=M, kind=SUM, ldo=M + 2,
                                          R=1, gate_scale=1.0))
            launch("grouped_epilogue", _lib.lib().vqa_grouped_epilogue, (h.EpilogueJob * len(jobs))(*jobs), len(jobs))
            what = "%s %s [%d,%d,%d] act %d gate %d p %g out_off %d ldo %d" % (name, form_name, M, N, K, act, gate, p, out_off, ldo)
            for w, nm in ((out_d, "direct out"), (out_s, "epilogue out"), (cs_d, "colsum_out"), (cs_s, "epilogue colsum")):
                if w is not None:
                    w.assert_outside_untouched(what + " " + nm)
            d, s = out_d.get(), out_s.get()
            assert np.isfinite(d).all() and np.isfinite(s).all(), what
            keep = keep_factors(p, seed, drop_base, drop_ld, M, N)
            if act == 2 or gate == 2:
                acc = slab.get()
                if act == 2:
                    t_err, _ = sigmoid_errors(acc + bias_np[None, :], keep, s)
                    gap = np.abs(d.astype(np.float64) - s).max()
                else:
                    t_err, _ = sigmoid_gate_errors(acc, gy_np, keep, s)
                    gap = (np.abs(d.astype(np.float64) - s) / np.abs(acc)).max()
                sig.add(t_err, gap)
            else:
                assert np.array_equal(d, s), "%s: direct != slab + epilogue at %d elements" % (what, int((d != s).sum()))
            if colsum:
                assert np.array_equal(cs_d.get(), cs_s.get()), what + ": colsum_out != the slab path's column sums"
            # float64
            z = product64(form, A.view(), B.view())
            if bias_np is not None:
                z = z + torch.from_numpy(bias_np).to(dev()).double()
            if act == 1:
                z = torch.relu(z)
            elif act == 2:
                z = torch.sigmoid(z)
            if gate:
                y64 = torch.from_numpy(gy_np).to(dev()).double()
                z = torch.where(y64 > 0, z * gate_scale, torch.zeros_like(z)) if gate == 1 else z * y64 * (1 - y64)
            want = (z * torch.from_numpy(keep).to(dev()).double()).cpu().numpy()
            for key, got in (("direct", d), ("slab", s)):
                err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-20)
                worst[key] = max(worst[key], err)
                assert err <= RTOL, "%s, %s path: %.3e of the output's scale" % (what, key, err)
            if colsum:
                want_cs = A.view().double().sum(0).cpu().numpy()
                err = np.abs(cs_d.get()[0] - want_cs).max() / max(np.abs(want_cs).max(), 1e-20)
                assert err <= RTOL, "%s: column sums %.3e" % (what, err)
            count += 1
    for key, v in worst.items():
        measured("%s %s %s vs float64" % (name, form_name, key), v, RTOL, "(%d cases)" % count)
    sig.finish(measured, "sigmoid %s %s direct - slab" % (name, form_name))


def _padded(rows, cols, valid_rows, valid_cols, ld, off, rng, scale, junk):
    """A [rows, cols] operand whose memory behind the valid extent holds `junk` (ordinary device memory inside the tensor: a
    wrong read shows in the output, never as a fault) -> (Win, its float64 value with the padding as zeros)."""
    a = (rng.standard_normal((rows, cols)) * scale).astype(np.float32)
    held = a.copy()
    held[valid_rows:, :] = junk
    held[:, valid_cols:] = junk
    w = Win(rows, cols, ld, off, held, fill=junk)
    a[valid_rows:, :] = 0.0
    a[:, valid_cols:] = 0.0
    return w, torch.from_numpy(a).to(dev()).double()


EXTENTS = [dict(K=150, Ka=70, Kb=64, M=77, Ma=50, N=75, Nb=40), dict(K=150, Ka=2, Kb=2, M=77, Ma=2, N=75, Nb=2),
           dict(K=70, Ka=64, Kb=70, M=200, Ma=130, N=330, Nb=322)]
EXTENTS_A4 = [dict(K=150, Ka=71, Kb=64, M=77, Ma=51, N=75, Nb=40)]     # forms 3 / 4: no condition on A, odd extents included


@pytest.mark.parametrize("form_name", ["NT", "NN", "TN", "NN_A4", "TN_A4"])
def test_zero_padded_operand_extents(engine, form_name, measured):
    """Ka, Kb, Ma, Nb: the problem's K (M, N) is larger than the operand's valid extent, the memory behind it is allocated
    and NaN, the reference is float64 with the operand zero-padded.  Each case a second time with 1000.0 behind the valid
    extent: the split engine recomputes a non-finite accumulator from the original operands WITH their extents, so there a
    NaN that a staging load lets in is repaired and only a finite wrong value shows.  Valid extents even and 2, padded extents no multiple
    of a tile or step; split (ksplit = 48 / 32: the parts behind min(Ka, Kb) must be all zeros) and in one part; the TN forms'
    column sums over the padded A.  Every slab finite, sum of the slabs within RTOL, nothing outside the slabs written."""
    _, h, _ = mods()
    name, _, _, step = engine
    form = DIRECT_CASES[form_name][0]
    a4, tn = form in (NN_A4, TN_A4), form in (TN, TN_A4)
    worst = 0.0
    for ei, (e, junk) in enumerate((e, junk) for e in EXTENTS + (EXTENTS_A4 if a4 else []) for junk in (float("nan"), 1000.0)):
        M, N, K = e["M"], e["N"], e["K"]
        rng = np.random.RandomState([form, ei, 7])
        (ar, ac), (br, bc) = operand_shapes(form, M, N, K)
        Ka, Kb, Ma, Nb = e["Ka"], e["Kb"], (e["Ma"] if tn else M), (e["Nb"] if form != NT else N)
        a_valid = (Ka, Ma) if tn else (M, Ka)
        b_valid = (N, Kb) if form == NT else (Kb, Nb)
        A, a64 = _padded(ar, ac, a_valid[0], a_valid[1], ac + (3 if a4 else 2) - (0 if a4 else ac % 2), 1 if a4 else 0, rng, 1.0, junk)
        B, b64 = _padded(br, bc, b_valid[0], b_valid[1], bc + 2 - bc % 2, 0, rng, 1.0 / math.sqrt(min(Ka, Kb)), junk)
        want = product64(form, a64, b64).cpu().numpy()
        want_cs = a64.sum(0).cpu().numpy() if tn else None
        for ksplit in (48 if step == 16 else 32, (K + step - 1) // step * step):
            S = math.ceil(K / ksplit)
            stride = M * N + 6
            slab = torch.full((S * stride + N + 2,), SENT, device=dev())
            cs = torch.full((S * M + M + 2,), SENT, device=dev()) if tn else None
            p = h.GemmProblem(A=A.ptr(), B=B.ptr(), slab=slab.data_ptr(), colsum=cs.data_ptr() if tn else None, slab_stride=stride,
                              lda=A.ld, ldb=B.ld, M=M, N=N, K=K, form=form, ksplit=ksplit, slab_base=0, Ka=Ka, Kb=Kb,
                              Ma=Ma if tn else 0, Nb=Nb if form != NT else 0)
            launch_gemm(engine, [p])
            what = "%s %s %r behind it %r, ksplit %d" % (name, form_name, e, junk, ksplit)
            parts = slab[:S * stride].view(S, stride)
            assert bool((parts[:, M * N:] == SENT).all()) and bool((slab[S * stride:] == SENT).all()), what + ": a store outside the slabs"
            got = parts[:, :M * N].reshape(S, M, N)
            assert bool(torch.isfinite(got).all()), "%s: %d non-finite outputs (a read behind a valid extent)" % (
                what, int((~torch.isfinite(got)).sum()))
            for s in range(S):
                if s * ksplit >= min(Ka, Kb):
                    assert bool((got[s] == 0).all()), "%s: part %d lies in the padding and is not zero" % (what, s)
            total = got.double().sum(0).cpu().numpy()
            err = np.abs(total - want).max() / max(np.abs(want).max(), 1e-20)
            worst = max(worst, err)
            assert err <= RTOL, "%s: %.3e of the output's scale" % (what, err)
            assert not total[Ma:].any() and not total[:, Nb:].any(), what + ": outputs of padded rows / columns are not zero"
            if tn:
                assert bool((cs[S * M:] == SENT).all()), what + ": a store outside the column sums"
                sums = cs[:S * M].view(S, M)
                assert bool(torch.isfinite(sums).all()), what + ": non-finite column sums"
                got_cs = sums.double().sum(0).cpu().numpy()
                err = np.abs(got_cs - want_cs).max() / max(np.abs(want_cs).max(), 1e-20)
                assert err <= RTOL and not got_cs[Ma:].any(), "%s: column sums %.3e" % (what, err)
    measured("%s %s padded extents vs float64" % (name, form_name), worst, RTOL)


# ================================================================================================ D: Phase
class LaunchSpy:
    """Wraps ops._launch: the grouped launches a phase makes, with the `out` pointers of its GEMM tables."""

    def __init__(self, monkeypatch):
        _, h, ops = mods()
        self.calls = []
        real = ops._launch

        def spy(name, shape, fn, *args):
            if name.startswith("grouped_gemm"):
                self.calls.append((name, [args[0][i].out for i in range(args[1])]))
            elif name == "grouped_epilogue":
                self.calls.append((name, args[1]))
            return real(name, shape, fn, *args)

        monkeypatch.setattr(ops, "_launch", spy)

    def names(self):
        return [c[0] for c in self.calls]


@pytest.mark.parametrize("eng", ["mfma", "split"])
@pytest.mark.parametrize("act", ["", "relu", "sigmoid"])
def test_phase_direct_on_and_off(eng, act, monkeypatch, measured):
    """A phase whose products are one contraction part each (a forward layer with bias, activation and dropout; a weight
    gradient with its bias gradient): with Phase.DIRECT it launches the GEMMs alone, every table entry carrying an `out`;
    without, GEMMs into slabs plus one epilogue launch.  Same tensors either way: bitwise for none / relu and the gradients,
    within the measured sigmoid bar for sigmoid."""
    _, h, _ = mods()
    B, N, K = 64, 62, 64
    rng = np.random.RandomState(31)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev())  # noqa: E731
    x, w, b, dy = t(B, K), t(N, K) / 8, t(N), t(B, N)
    monkeypatch.setattr(h.Phase, "ENGINE", eng)
    spy = LaunchSpy(monkeypatch)

    def run(direct):
        monkeypatch.setattr(h.Phase, "DIRECT", direct)
        del spy.calls[:]
        y, dw, db = Win(B, N, N + 2, 2), Win(N, K, K, 0), Win(1, N, N, 0)
        ph = h.Phase(dev(), "test")
        t1 = ph.target(B, N)
        ph.gemm(t1, h.NT, x, K, w, K, K)
        ph.job(h.EPI_LINEAR, t1, y.buf, y.ld, out_off=y.off, bias=b, act=h.ACT[act], p_drop=0.5, seed=99, drop_base=0, drop_ld=N)
        t2 = ph.target(N, K)
        ph.gemm(t2, h.TN, dy, N, x, K, B, colsum=True)
        ph.job(h.EPI_SUM, t2, dw.buf, K)
        ph.job(h.EPI_SUM, t2, db.buf, N, colsum=True)
        ph.run()
        torch.cuda.synchronize()
        for wn in (y, dw, db):
            wn.assert_outside_untouched("phase output")
        return (y.get(), dw.get(), db.get()), list(spy.calls)

    on, calls_on = run(True)
    off, calls_off = run(False)
    assert [c[0] for c in calls_on] == ["grouped_gemm_split" if eng == "split" else "grouped_gemm"], calls_on
    assert all(calls_on[0][1]), "a one-part product did not go direct"
    assert [c[0] for c in calls_off] == [calls_on[0][0], "grouped_epilogue"] and not any(calls_off[0][1]) and calls_off[1][1] == 3
    assert np.array_equal(on[1], off[1]) and np.array_equal(on[2], off[2])
    if act == "sigmoid":
        z = (x.double() @ w.double().t() + b.double()).float().cpu().numpy()
        keep = keep_factors(0.5, 99, 0, N, B, N)
        t_err, _ = sigmoid_errors(z, keep, off[0])
        gap = np.abs(on[0].astype(np.float64) - off[0]).max()
        measured("phase sigmoid direct - slab (%s)" % eng, gap, 4 * t_err, "(4 x torch's %.3e)" % t_err)
        assert gap <= 4 * t_err
    else:
        assert np.array_equal(on[0], off[0])
    want = x.double() @ w.double().t() + b.double()
    want = {"": want, "relu": torch.relu(want), "sigmoid": torch.sigmoid(want)}[act].cpu().numpy() * keep_factors(0.5, 99, 0, N, B, N)
    assert np.abs(on[0] - want).max() <= RTOL * np.abs(want).max()


@pytest.mark.parametrize("eng", ["mfma", "split"])
def test_phase_shared_or_split_target_never_goes_direct(eng, monkeypatch):
    """With Phase.DIRECT on: a target two problems add into (one part each) and a target whose one product is cut into
    several parts keep their slabs and their epilogue job."""
    _, h, _ = mods()
    B = 64
    rng = np.random.RandomState(32)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev())  # noqa: E731
    x1, x2, wf, x3, w3 = t(B, 64), t(B, 32), t(62, 96) / 10, t(B, 2400), t(62, 2400) / 49
    monkeypatch.setattr(h.Phase, "ENGINE", eng)
    monkeypatch.setattr(h.Phase, "DIRECT", True)
    spy = LaunchSpy(monkeypatch)
    y1, y2 = Win(B, 62, 64, 2), Win(B, 62, 64, 2)
    ph = h.Phase(dev(), "test")
    t1 = ph.target(B, 62)
    ph.gemm(t1, h.NT, x1, 64, wf, 96, 64)
    ph.gemm(t1, h.NT, x2, 32, wf, 96, 32, b_off=64)
    ph.job(h.EPI_SUM, t1, y1.buf, y1.ld, out_off=y1.off)
    t2 = ph.target(B, 62)
    ph.gemm(t2, h.NT, x3, 2400, w3, 2400, 2400)
    ph.job(h.EPI_SUM, t2, y2.buf, y2.ld, out_off=y2.off)
    ph.run()
    torch.cuda.synchronize()
    assert spy.names() == ["grouped_gemm_split" if eng == "split" else "grouped_gemm", "grouped_epilogue"], spy.calls
    assert len(spy.calls[0][1]) == 3 and not any(spy.calls[0][1]) and spy.calls[1][1] == 2
    for y, want in ((y1, torch.cat([x1, x2], 1).double() @ wf.double().t()), (y2, x3.double() @ w3.double().t())):
        y.assert_outside_untouched("phase output")
        want = want.cpu().numpy()
        assert np.abs(y.get() - want).max() <= RTOL * np.abs(want).max()


# ================================================================================================ E: refusals
def test_epilogue_refusals():
    """Each of these returns an error, launches nothing and leaves the outputs untouched (real, validly sized buffers
    throughout: a check that wrongly passed would launch something harmless)."""
    _lib, h, _ = mods()
    fn = _lib.lib().vqa_grouped_epilogue
    M, N = 6, 12
    slab, aux, out, out2 = Win(2 * M, N, N, 0, fill=1.0), Win(M, N, N, 0, fill=0.5), Win(M, N, N + 2, 2), Win(M, N, N + 2, 2)

    def job(**kw):
        f = dict(slab=slab.ptr(), out=out.ptr(), slab_stride=M * N, S=2, M=M, N=N, kind=SUM, ldo=N + 2, ld_aux=N, R=1,
                 drop_base=0, drop_ld=N, p_drop=0.0, gate_scale=1.0)
        f.update(kw)
        return h.EpilogueJob(**f)

    good = job()
    cases = [("n = 0", [good], 0, E_BADARG), ("n = 25", [good] * 25, 25, E_BADARG), ("S = 0", [job(S=0)], 1, E_BADARG),
             ("kind = 5", [job(kind=5)], 1, E_BADARG), ("p_drop = 1", [job(kind=LINEAR, p_drop=1.0)], 1, E_BADARG),
             ("R does not divide N", [job(kind=RANK_PRODUCT, R=5, aux=aux.ptr(), out2=out2.ptr())], 1, E_BADARG),
             ("a gate without aux", [job(kind=GRAD, gate=1)], 1, E_BADARG),
             ("a good job behind a bad one", [job(kind=5), good], 2, E_BADARG)]
    for name, jobs, n, code in cases:
        refused("grouped_epilogue", fn, (h.EpilogueJob * len(jobs))(*jobs), n, code)
        out.assert_untouched(name + ": out")
        out2.assert_untouched(name + ": out2")
    launch("grouped_epilogue", fn, (h.EpilogueJob * 1)(good), 1)          # (the base job itself is accepted)
    assert bool((out.view() == 2.0).all())


def test_gemm_refusals(engine):
    _, h, _ = mods()
    name, call, fn, step = engine
    M, N, K = 8, 12, 2 * step
    A, B, Bodd = Win(max(M, K), max(M, K), fill=1.0), Win(max(N, K), max(N, K), fill=1.0), Win(N, K, K + 1, fill=1.0)
    slab, cs, out, cs_out = Win(2 * M, N), Win(2, max(M, N)), Win(M, N, N + 2, 2), Win(1, max(M, N), off=2)

    def prob(**kw):
        f = dict(A=A.ptr(), B=B.ptr(), slab=slab.ptr(), slab_stride=M * N, lda=A.ld, ldb=B.ld, M=M, N=N, K=K, form=NT, ksplit=step,
                 slab_base=0, gate_scale=1.0)
        f.update(kw)
        return h.GemmProblem(**f)

    good = prob()
    direct = dict(slab=None, out=out.ptr(), ldo=N + 2)
    cases = [("n = 0", [good], 0, E_BADARG), ("n = 17", [good] * 17, 17, E_BADARG),
             ("a direct output with ksplit < K", [prob(**direct)], 1, E_BADARG),
             ("a direct gate without gate_y", [prob(ksplit=K, gate=1, **direct)], 1, E_BADARG),
             ("a direct output with p_drop = 1", [prob(ksplit=K, p_drop=1.0, **direct)], 1, E_BADARG),
             ("colsum_out without out", [prob(form=TN, colsum_out=cs_out.ptr())], 1, E_BADARG),
             ("column sums on an NT problem", [prob(colsum=cs.ptr())], 1, E_BADARG),
             ("direct column sums on an NT problem", [prob(ksplit=K, colsum_out=cs_out.ptr(), **direct)], 1, E_BADARG),
             ("odd ldb", [prob(B=Bodd.ptr(), ldb=Bodd.ld)], 1, E_UNSUPPORTED),
             ("ksplit no multiple of the step", [prob(ksplit=step + step // 2)], 1, E_BADARG)]
    if name == "split":
        cases.append(("ksplit % 32 != 0", [prob(ksplit=48)], 1, E_BADARG))
    for what, probs, n, code in cases:
        refused(call, fn, (h.GemmProblem * len(probs))(*probs), n, code)
        for w, nm in ((slab, "slab"), (cs, "colsum"), (out, "out"), (cs_out, "colsum_out")):
            w.assert_untouched("%s (%s): %s" % (what, name, nm))
    launch_gemm(engine, [good])                                             # (the base problem itself is accepted)
    got = slab.view()[:M].cpu().numpy()
    assert np.array_equal(got, np.full((M, N), float(step), np.float32))
