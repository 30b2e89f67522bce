"""What the kernel-level GPU tests (tests/test_gpu_*_kernels.py and their siblings) share, said once: sentinel-filled output
windows and NaN-padded input windows, the launch-log reader and the C-ABI call wrapper, the exact-integer comparison, the "four
times the float32 error plus one ulp" bars, the parser of a source file's VQA_LAUNCH( sites and the two patches of ops._launch (a
recording spy, a guard that forbids launches).  The C-ABI call wrapper checks its arguments against the signature bound from the
header; the header's constants come from _lib.DEFINES.  A plain module that the test modules import from by name (`from
kernel_harness import _bits, _win, ...`) and that needs no GPU to import; tests/test_kernel_harness.py shows on the CPU that each
guard here fails when it should.

pytest rewrites assertions in test modules only, so every assert in this file carries its own message."""
import ctypes
import re

import pytest
import torch

from vqa_playground_pytorch_amd._lib import DEFINES, PARAMS

SENT = -12345.0         # fills every output buffer; what is still SENT afterwards was not written
PAD = 8                 # elements of sentinel (outputs) or NaN (inputs) in front of and behind every window: 32 bytes fp32, 16 bytes bf16
E_BADARG, E_UNSUPPORTED = DEFINES["VQA_E_BADARG"], DEFINES["VQA_E_UNSUPPORTED"]
EPS32 = float(torch.finfo(torch.float32).eps)
EPS_BF16 = 2.0 ** -8
F32, F64, BF = torch.float32, torch.float64, torch.bfloat16
NAN, INF = float("nan"), float("inf")


# ---- device and library ------------------------------------------------------------------------------------------------------
def dev():
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def ops():
    from vqa_playground_pytorch_amd import _lib, ops as o
    _lib.lib()
    return o


# ---- bits and windows --------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _ptr(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + t.element_size() * int(off)) if t is not None else None


def _ptrs(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _sentinel(*shape, dtype=F32):
    return torch.full(shape, SENT, device=dev(), dtype=dtype)


def _untouched(t):
    return bool((_bits(t) == _bits(torch.full((1,), SENT, device=t.device, dtype=t.dtype))).all())


def _take(buf, window, what):
    """-> a copy of buf[window]; asserts that nothing else of the sentinel-filled `buf` changed"""
    got = buf[window].clone()
    buf[window] = SENT
    assert _untouched(buf), "%s: a store outside the output window" % what
    return got


def _out(n, dtype=F32):
    """a sentinel-filled buffer with an n-element output window PAD elements in"""
    buf = _sentinel(n + 2 * PAD, dtype=dtype)
    assert buf.data_ptr() % 16 == 0, "the allocator handed out a buffer that is not 16-byte aligned"
    return buf


def _win(buf, shape, what):
    """-> a copy of the window of _out(prod(shape)); asserts that nothing else of `buf` changed"""
    n = 1
    for s in shape:
        n *= s
    return _take(buf, slice(PAD, PAD + n), what).view(*shape)


def _in_host(t, ld=None):
    """the buffer of _in on the CPU"""
    cols = t.shape[-1]
    rows = t.reshape(-1, cols).to(F32)
    assert torch.allclose(rows.to(F64), t.reshape(-1, cols).to(F64), rtol=0.0, atol=0.0, equal_nan=True), "the operand is not exact in fp32"
    ld = cols if ld is None else ld
    buf = torch.full((rows.shape[0] * ld + 2 * PAD,), NAN, dtype=F32)
    buf[PAD:PAD + rows.shape[0] * ld].view(rows.shape[0], ld)[:, :cols] = rows
    return buf


def _in(t, ld=None):
    """CPU tensor (fp32, or wider with values that fp32 holds exactly; a NaN stays one) -> an fp32 GPU buffer that holds it PAD
    elements in, NaN on both sides; with ld: its rows (last dimension) at stride ld, NaN in the gap.  A read outside the window
    that is USED poisons an output"""
    return _in_host(t, ld).to(dev())


# ---- the launch log ----------------------------------------------------------------------------------------------------------
def _logged(L, call):
    """run `call` -> [(kernel expression without blanks, grid in work-items)] of the launches it made"""
    cap = DEFINES["VQA_LAUNCH_LOG_CAP"]
    L.vqa_launch_log_reset()
    call()
    buf = (ctypes.c_ulonglong * cap)()
    n = L.vqa_launch_log(buf, cap)
    return [((L.vqa_launch_log_kernel(i) or b"").decode().replace(" ", ""), int(buf[i])) for i in range(min(n, cap))]


_POINTERS = (ctypes.c_void_p, ctypes.c_char_p)
_FLOATS = (ctypes.c_float, ctypes.c_double)
_BYREF = type(ctypes.byref(ctypes.c_int()))


def check_args(fn, args):
    """`args` (all of them, the stream included) against fn.argtypes, before the library is entered.  ctypes itself takes extra
    arguments of a cdecl function in silence and a bare int as a c_void_p -- a size that slipped into a pointer slot would be launched
    as an address.  Here the count is exact; a pointer slot takes None, a c_void_p, a ctypes array, a pointer or a byref; an integer
    slot a Python int; a float slot an int or a float; a bool is no number."""
    name, slots = fn.__name__, fn.argtypes
    params = PARAMS.get(name, ())
    assert len(args) == len(slots), "%s takes %d arguments (%s), got %d" % (name, len(slots), ", ".join(params), len(args))
    for i, (slot, a) in enumerate(zip(slots, args)):
        number = isinstance(a, (int, float)) and not isinstance(a, bool)
        if slot in _POINTERS:
            takes, ok = "a pointer", a is None or isinstance(a, (ctypes.c_void_p, ctypes.Array, ctypes._Pointer, _BYREF))
        elif slot in _FLOATS:
            takes, ok = "a number", number
        else:
            takes, ok = "an integer", number and isinstance(a, int)
        got = "%s %r" % (type(a).__name__, a) if number or isinstance(a, bool) else type(a).__name__
        assert ok, "argument %d (`%s`) of %s takes %s, got %s" % (i + 1, params[i] if i < len(params) else "?", name, takes, got)


def _call(ops, fn, *args):
    """one C-ABI call on torch's current stream -> (return code, launch log), synchronised; the arguments are checked against
    the bound signature first (check_args)"""
    L = ops._lib.lib()
    args += (ops._stream(),)
    check_args(fn, args)
    rc = []
    log = _logged(L, lambda: rc.append(fn(*args)))
    torch.cuda.synchronize()
    return rc[0], log


# ---- ops._launch, watched or forbidden ---------------------------------------------------------------------------------------
def spy_launches(monkeypatch, ops):
    """-> the list that receives (name, shape) of every ops._launch from now on, each forwarded unchanged.  It ends with the
    test, or with the `monkeypatch.context()` it was given"""
    seen, inner = [], ops._launch

    def spy(name, shape, *args, **kwargs):
        seen.append((name, shape))
        return inner(name, shape, *args, **kwargs)

    monkeypatch.setattr(ops, "_launch", spy)
    return seen


def forbid_launches(monkeypatch, ops):
    monkeypatch.setattr(ops, "_launch", lambda *a, **k: pytest.fail("a kernel was launched"))


def _names(log):
    return [k for k, _ in log]


def set_knobs(lib_option, knobs):
    for k, v in knobs:
        lib_option(k, v)


def spell(site, *values, params):
    """the log's spelling of a launch site: its macro parameters (the names in `params`) replaced, in order, by `values`"""
    vals = list(values)
    out = re.sub(r"\b(%s)(?=[,>])" % "|".join(params), lambda m: str(vals.pop(0)), site)
    assert not vals, "%s has fewer macro parameters than the %d values %r" % (site, len(values), values)
    return out


def launch_sites(path):
    """the first argument of every VQA_LAUNCH( of a source file, blanks removed"""
    text = open(path).read()
    found = []
    for m in re.finditer(r"\bVQA_LAUNCH\(", text):
        depth, i = 0, m.end()
        while depth or text[i] != ",":
            depth += {"(": 1, ")": -1}.get(text[i], 0)
            i += 1
        found.append(re.sub(r"\s+", "", text[m.end():i]))
    return found


# ---- exactness ---------------------------------------------------------------------------------------------------------------
def _ceil(a, b):
    return -(-a // b)


def _amax(t):
    return int(t.abs().max())


def _below_2_24(*bounds):
    for b in bounds:
        assert int(b) < 2 ** 24, "a sum of this case can leave the exact range of fp32: bound %d" % int(b)


def _d(t, dt):
    """CPU integer tensor -> dt on the GPU, exactly"""
    out = t.to(F32).to(dt)
    assert torch.equal(out.to(F64), t.to(F64)), "the operand is not exact in %s" % dt
    return out.to(dev()).contiguous()


def _dbf(t):
    return _d(t, BF)


def _canon(t):
    """the kernel's result on the CPU as fp32 with -0.0 folded into 0.0 (the integer reference has one zero)"""
    return t.detach().float().cpu() + 0.0


def assert_exact(name, got, ref):
    """got (fp32 or bf16 tensor) against the integer reference (int64, or float64 holding integers): fp32 bit for bit (-0.0 folded
    into 0.0: an integer has one zero), bf16 == ref.float().to(bf16) bit for bit"""
    assert tuple(got.shape) == tuple(ref.shape), "%s: got %s %s, the reference is %s" % (name, got.dtype, tuple(got.shape), tuple(ref.shape))
    integers = ref.dtype == torch.int64 or (ref.dtype == F64 and bool((ref == ref.round()).all()))
    assert integers, "%s: the reference (%s) does not hold integers" % (name, ref.dtype)
    _below_2_24(_amax(ref))
    want = ref.float() + 0.0          # (a float64 reference can hold -0.0, a gated product for one: the same zero)
    if got.dtype == BF:
        want = want.to(BF).float()
    else:
        assert got.dtype == F32, "%s: a result of dtype %s" % (name, got.dtype)
    have = _canon(got)
    if not torch.equal(_bits(have), _bits(want)):
        bad = (_bits(have) != _bits(want)).nonzero()
        first = tuple(int(i) for i in bad[0])
        raise AssertionError("%s: %d of %d elements differ from the integer reference; first at %s: got %r, want %r"
                             % (name, len(bad), want.numel(), first, float(have[first]), float(want[first])))


# ---- bars --------------------------------------------------------------------------------------------------------------------
def _error_and_bar(what, got, ref64, ref32):
    """-> (err, e32, bar), all over the reference's largest magnitude: the kernel's largest error against float64 (a bf16 result:
    what of it exceeds one rounding, 2^-8 |ref|, elementwise), the error of the same formulas in float32 with torch on the CPU,
    and the bar, four times that plus one float32 ulp.  A non-finite result: err = inf.  A reference that is all zero has no
    scale and gets no allowance: err is the largest |got| and the bar is 0"""
    assert got.shape == ref64.shape, "%s: got %s, the reference is %s" % (what, tuple(got.shape), tuple(ref64.shape))
    assert got.dtype in (F32, BF), "%s: a result of dtype %s" % (what, got.dtype)
    mag = float(ref64.abs().max())
    if mag == 0.0:
        assert not bool(ref32.any()), "%s: the float64 reference is zero and the float32 one is not" % what
        return float(got.double().abs().max()), 0.0, 0.0
    e32 = float((ref32.double() - ref64).abs().max()) / mag
    diff = (got.double() - ref64).abs()
    if got.dtype == BF:
        diff = (diff - EPS_BF16 * ref64.abs()).clamp_min(0.0)
    err = float(diff.max()) / mag if bool(torch.isfinite(got.float()).all()) else INF
    return err, e32, 4.0 * e32 + EPS32


class Bars:
    """The collecting form, one per case: check() keeps every figure and reports it through `measured` as ("<case> <name>", err,
    bar); close() fails if one missed its bar (`fallback`: the bar the project already states for that output, where the first
    one is missed).  The figures are those of _error_and_bar."""

    def __init__(self, measured, case):
        self.measured, self.case, self.rows = measured, case, []

    def check(self, name, got, ref64, ref32, fallback=None):
        err, _, bar = _error_and_bar("%s %s" % (self.case, name), got.detach().cpu(), ref64, ref32)
        self.rows.append((err, bar, name, fallback))
        self.report(name, err, bar)

    def report(self, name, err, bar):
        self.measured("%s %s" % (self.case, name), err, bar)

    def close(self):
        missed = [r for r in self.rows if not (r[0] <= r[1] or (r[3] is not None and r[0] <= r[3]))]
        assert not missed, "%s: %r" % (self.case, [(n, "%.3e > %.3e" % (e, b)) for e, b, n, _ in missed])


class WorstBar:
    """The immediate form, one per test: check() (fp32 results) and check_bf16() print the figures of _error_and_bar and fail at
    once where one misses its bar or is not finite; report() hands the worst of them, by err / bar, to `measured`.  An all-zero
    reference demands zeros and is not reported."""

    def __init__(self):
        self.worst = (-1.0, 0.0, 0.0, "")

    def _check(self, name, got, ref64, ref32, dtype):
        assert got.dtype == dtype, "%s: a result of dtype %s" % (name, got.dtype)
        err, e32, bar = _error_and_bar(name, got.detach().cpu(), ref64, ref32)
        if bar == 0.0:
            assert err == 0.0, "%s: the reference is zero, the result reaches %.3e" % (name, err)
            return
        print("[%s] kernel %.3e  float32 torch %.3e  bar %.3e" % (name, err, e32, bar))
        if err / bar > self.worst[0]:
            self.worst = (err / bar, err, bar, name)
        assert err <= bar, "%s: error %.3e over the bar %.3e (float32 torch: %.3e)" % (name, err, bar, e32)

    def check(self, name, got, ref64, ref32):
        self._check(name, got, ref64, ref32, F32)

    def check_bf16(self, name, got, ref64, ref32):
        """reported: the largest |err| - 2^-8 |ref| over the magnitude, against the fp32 bar"""
        self._check(name, got, ref64, ref32, BF)

    def report(self, measured, tag):
        measured("%s err / max|ref|" % tag, self.worst[1], self.worst[2], self.worst[3])
