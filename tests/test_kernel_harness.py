"""tests/kernel_harness.py on the CPU: every guard the kernel tests lean on fails when it should.  Buffers are built with torch.full
where the harness would allocate on the GPU; the Bars cases use dyadic numbers, so every comparison below is exact."""
import ctypes

import pytest
import torch

from kernel_harness import (BF, EPS32, F32, F64, INF, NAN, PAD, SENT, Bars, WorstBar, _in_host, _same_bits, _take, _untouched, _win,
                            assert_exact, check_args, forbid_launches, launch_sites, spell, spy_launches)
from vqa_playground_pytorch_amd import _lib

fails = pytest.raises(AssertionError)


# ---- the window guard --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF], ids=["f32", "bf16"])
def test_a_store_outside_the_window_is_caught(dtype):
    n = 6
    for at, value in ((PAD - 1, 1.0), (PAD + n, 1.0), (0, NAN), (PAD + n + PAD - 1, NAN)):
        buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype)
        buf[at] = value
        with pytest.raises(AssertionError, match="case 7: a store outside the output window"):
            _win(buf, (2, 3), "case 7")
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype)
    buf[PAD:PAD + n] = torch.arange(6.0).to(dtype)
    got = _win(buf, (2, 3), "inside")
    assert got.dtype == dtype and torch.equal(got, torch.arange(6.0).to(dtype).view(2, 3))
    assert _untouched(buf), "_win hands the window back as it found the buffer: all sentinel"
    buf[3] = 2.0
    assert not _untouched(buf)
    with fails:
        _take(buf, slice(4, 5), "next to it")
    assert float(_take(buf, slice(3, 4), "it")) == 2.0


def test_same_bits_is_by_bits_dtype_and_shape():
    one = torch.ones(2)
    assert _same_bits(one, one.clone()) and _same_bits(torch.tensor([NAN]), torch.tensor([NAN]))
    assert not _same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))
    assert not _same_bits(one, one.view(1, 2)) and not _same_bits(one, one.to(BF)) and _same_bits(one.to(BF), one.to(BF))


# ---- the exact comparison ----------------------------------------------------------------------------------------------------
def test_assert_exact():
    ref = torch.tensor([[0, 3, -5], [7, 0, 257]])
    got = ref.float()
    got[0, 0] = -0.0
    assert_exact("an integer has one zero", got, ref)
    assert_exact("float64 integers", got, ref.double())
    assert_exact("a float64 -0.0 is the same zero", got, torch.where(ref == 0, torch.tensor(-0.0, dtype=F64), ref.double()))
    off = got.clone()
    off[1, 2] = torch.nextafter(off[1, 2], torch.tensor(INF))
    with pytest.raises(AssertionError, match=r"one ulp: 1 of 6 elements differ .* first at \(1, 2\): got 257.00003\d*, want 257.0"):
        assert_exact("one ulp", off, ref)
    with pytest.raises(AssertionError, match="a float64 result: a result of dtype torch.float64"):
        assert_exact("a float64 result", got.double(), ref)
    with pytest.raises(AssertionError, match="does not hold integers"):
        assert_exact("halves", got, ref.double() + 0.5)
    with fails:
        assert_exact("another shape", got.view(3, 2), ref)
    big = torch.tensor([2 ** 24])
    assert_exact("the last exact sum", (big - 1).float(), big - 1)
    with pytest.raises(AssertionError, match="can leave the exact range of fp32: bound 16777216"):
        assert_exact("2^24", big.float(), big)
    assert_exact("bf16: 257 rounds to 256", torch.tensor([[0, 3, -5], [7, 0, 256]]).to(BF), ref)
    with fails:
        assert_exact("bf16 is not compared as fp32", torch.tensor([[0, 3, -5], [7, 0, 258]]).to(BF), ref)
    with fails:
        assert_exact("fp32 is not rounded", torch.tensor([[0.0, 3, -5], [7, 0, 256]]), ref)


# ---- the bars ----------------------------------------------------------------------------------------------------------------
E = 2.0 ** -20
REF64 = torch.tensor([1.0, 0.5, -0.25], dtype=F64)                    # largest magnitude 1: every figure is an absolute one
REF32 = (REF64 + torch.tensor([0.0, E, 0.0], dtype=F64)).float()      # the float32 formulas are 2^-20 off
BAR = 4.0 * E + EPS32                                                 # 2^-18 + 2^-23


def _got(err):
    return (REF64 + torch.tensor([err, 0.0, 0.0], dtype=F64)).float()


def test_collecting_bars_hold_four_times_the_float32_error_plus_one_ulp():
    rows = []
    bars = Bars(lambda *a: rows.append(a), "case")
    bars.check("below", _got(BAR - EPS32), REF64, REF32)
    bars.check("at", _got(BAR), REF64, REF32)
    bars.close()
    assert rows == [("case below", BAR - EPS32, BAR), ("case at", BAR, BAR)]
    bars.check("above", _got(BAR + EPS32), REF64, REF32)
    with pytest.raises(AssertionError, match=r"case: \[\('above', '4.053e-06 > 3.934e-06'\)\]"):
        bars.close()
    assert rows[2:] == [("case above", BAR + EPS32, BAR)]


def test_collecting_bars_fallback_non_finite_and_shape():
    for fallback, ok in ((2.0 * BAR, True), (BAR, False), (None, False)):
        bars = Bars(lambda *a: None, "fallback %r" % fallback)
        bars.check("d_w", _got(BAR + EPS32), REF64, REF32, fallback)
        if ok:
            bars.close()
        else:
            with fails:
                bars.close()
    rows = []
    bars = Bars(lambda *a: rows.append(a), "case")
    bars.check("nan", _got(NAN), REF64, REF32, 1.0)
    assert rows == [("case nan", INF, BAR)]
    with fails:
        bars.close()
    with pytest.raises(AssertionError, match="case shape"):
        bars.check("shape", _got(0.0).view(1, 3), REF64, REF32)
    with pytest.raises(AssertionError, match="torch.float64"):
        bars.check("dtype", _got(0.0).double(), REF64, REF32)


def test_collecting_bars_zero_reference_demands_zeros():
    zero64, rows = torch.zeros(3, dtype=F64), []
    bars = Bars(lambda *a: rows.append(a), "zero")
    bars.check("exact", torch.tensor([0.0, -0.0, 0.0]), zero64, torch.zeros(3))
    bars.close()
    tiny = 2.0 ** -149
    bars.check("tiny", torch.tensor([0.0, tiny, 0.0]), zero64, torch.zeros(3))
    assert rows == [("zero exact", 0.0, 0.0), ("zero tiny", tiny, 0.0)]
    with fails:
        bars.close()
    with pytest.raises(AssertionError, match="the float32 one is not"):
        bars.check("ref32", torch.zeros(3), zero64, torch.tensor([0.0, tiny, 0.0]))


def test_collecting_bars_bf16_allowance_is_one_rounding():
    """a bf16 result gets 2^-8 |ref| elementwise: 1 for 1 + 2^-8 (a tie of the rounding) is inside, 1 for 1 + 2^-8 + 2^-12 is not,
    and what is reported is the excess over the magnitude (2, the other element)"""
    got, rows = torch.tensor([1.0, 2.0]).to(BF), []
    bars = Bars(lambda *a: rows.append(a), "bf16")
    inside = torch.tensor([1.0 + 2.0 ** -8, 2.0], dtype=F64)
    bars.check("inside", got, inside, inside.float())
    bars.close()
    outside = torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -12, 2.0], dtype=F64)
    bars.check("outside", got, outside, outside.float())
    assert rows == [("bf16 inside", 0.0, EPS32), ("bf16 outside", (2.0 ** -12 - 2.0 ** -16 - 2.0 ** -20) / 2.0, EPS32)]
    with fails:
        bars.close()
    bars = Bars(lambda *a: None, "fp32 gets none")
    bars.check("inside", got.float(), inside, inside.float())
    with fails:
        bars.close()


def test_immediate_bars_fail_in_check_and_report_the_worst():
    rows, bars = [], WorstBar()
    bars.check("half", _got(BAR / 2.0), REF64, REF32)
    bars.check("at", _got(BAR), REF64, REF32)
    bars.check("quarter", _got(BAR / 4.0), REF64, REF32)
    bars.check("zero", torch.zeros(3), torch.zeros(3, dtype=F64), torch.zeros(3))
    bars.report(lambda *a: rows.append(a), "gates")
    assert rows == [("gates err / max|ref|", BAR, BAR, "at")]
    for name, got in (("above", _got(BAR + EPS32)), ("nan", _got(NAN)), ("bf16", _got(0.0).to(BF))):
        with pytest.raises(AssertionError, match=name):
            bars.check(name, got, REF64, REF32)
    with pytest.raises(AssertionError, match="the reference is zero"):
        bars.check("zero", torch.tensor([0.0, 1.0, 0.0]), torch.zeros(3, dtype=F64), torch.zeros(3))
    ref = torch.tensor([1.0 + 2.0 ** -8, 2.0], dtype=F64)
    bars.check_bf16("one rounding", torch.tensor([1.0, 2.0]).to(BF), ref, ref.float())
    with pytest.raises(AssertionError, match="two roundings"):
        bars.check_bf16("two roundings", torch.tensor([1.0 - 2.0 ** -8, 2.0]).to(BF), ref, ref.float())
    with pytest.raises(AssertionError, match="torch.float32"):
        bars.check_bf16("fp32", torch.tensor([1.0, 2.0]), ref, ref.float())


# ---- the launch log's spellings ----------------------------------------------------------------------------------------------
def test_launch_sites(tmp_path):
    src = tmp_path / "k.hip"
    src.write_text("""
        VQA_LAUNCH(plain_kernel, dim3(g, 2), 256, 0, stream, a, b);
        if (x) VQA_LAUNCH((k<A_, (T & 4) ? 2 : 1>), grid, block, 0, s, x);
        MY_VQA_LAUNCH(not_a_site, grid);
        VQA_LAUNCH(
            (long_kernel<float,
                         NT>),
            grid, 256, lds_bytes(N, 4), s);
    """)
    assert launch_sites(str(src)) == ["plain_kernel", "(k<A_,(T&4)?2:1>)", "(long_kernel<float,NT>)"]


def test_spell():
    site = "(k<BM_,BN_,7,PF_>)"
    assert spell(site, 64, 128, 2, params=("BM_", "BN_", "PF_")) == "(k<64,128,7,2>)"
    assert spell(site, 64, 2, params=("PF_", "BM_")) == "(k<64,BN_,7,2>)"          # (in the site's order, not the tuple's)
    assert spell("(k<NBM_,BM_X>)", params=("BM_",)) == "(k<NBM_,BM_X>)"
    with pytest.raises(AssertionError, match="fewer macro parameters"):
        spell(site, 64, 128, 2, 9, params=("BM_", "BN_", "PF_"))


# ---- the input window --------------------------------------------------------------------------------------------------------
def test_in_pads_with_nan_and_refuses_what_fp32_cannot_hold():
    t = torch.arange(1.0, 7.0, dtype=F64).view(1, 2, 3)
    flat = _in_host(t)
    assert flat.dtype == F32 and flat.shape == (6 + 2 * PAD,)
    assert torch.equal(flat[PAD:PAD + 6], t.reshape(-1).float()) and bool(flat[:PAD].isnan().all()) and bool(flat[PAD + 6:].isnan().all())
    wide = _in_host(t, 5)
    want = torch.full((10 + 2 * PAD,), NAN)
    want[PAD:PAD + 3], want[PAD + 5:PAD + 8] = t[0, 0].float(), t[0, 1].float()
    assert wide.shape == want.shape and torch.equal(wide.isnan(), want.isnan()) and torch.equal(wide.nan_to_num(), want.nan_to_num())
    t[0, 1, 1] = NAN
    assert bool(_in_host(t)[PAD + 4].isnan())            # (the isolation tests put a NaN into an operand)
    with pytest.raises(AssertionError, match="not exact in fp32"):
        _in_host(torch.tensor([[1.0, 1.0 + 2.0 ** -30]], dtype=F64))
    with pytest.raises(AssertionError, match="not exact in fp32"):
        _in_host(torch.tensor([[2 ** 24 + 1]]))


# ---- the argument check of _call ---------------------------------------------------------------------------------------------
class _Bound:
    """a stand-in for a bound entry point: its name and the header's argument types, never called"""

    def __init__(self, name):
        self.__name__, self.argtypes = name, _lib.SIGNATURES[name][1]


def test_call_checks_its_arguments_against_the_bound_signature():
    fn = _Bound("vqa_softmax_attention_pool_len_fwd")     # (logits, v, lens, alpha, pooled, first, p_drop, seed, seed_ptr, B, N, D, G, stream)
    p, words = ctypes.c_void_p(4096), (ctypes.c_uint64 * 1)()
    good = [p, p, p, p, p, None, 0.5, 7, words, 2, 36, 64, 4, ctypes.c_void_p(0)]
    check_args(fn, good)
    check_args(fn, good[:6] + [0, 2 ** 40, ctypes.byref(words), 2, 36, 64, 4, None])
    check_args(fn, [ctypes.pointer(words)] + good[1:])

    def bad(at, value, message):
        args = list(good)
        args[at] = value
        with pytest.raises(AssertionError, match=message):
            check_args(fn, args)

    bad(2, 36, r"argument 3 \(`lens`\) of vqa_softmax_attention_pool_len_fwd takes a pointer, got int 36")
    bad(0, 0.5, r"argument 1 \(`logits`\) of .* takes a pointer, got float 0.5")
    bad(5, False, r"argument 6 \(`first`\) of .* takes a pointer, got bool False")
    bad(1, torch.zeros(2), r"argument 2 \(`v`\) of .* takes a pointer, got Tensor")
    bad(13, 0, r"argument 14 \(`stream`\) of .* takes a pointer, got int 0")
    bad(9, torch.tensor(2), r"argument 10 \(`B`\) of .* takes an integer, got Tensor")
    bad(10, 36.0, r"argument 11 \(`N`\) of .* takes an integer, got float 36.0")
    bad(11, True, r"argument 12 \(`D`\) of .* takes an integer, got bool True")
    bad(7, p, r"argument 8 \(`seed`\) of .* takes an integer, got c_void_p")
    bad(6, None, r"argument 7 \(`p_drop`\) of .* takes a number, got NoneType")
    bad(6, torch.tensor(0.5), r"argument 7 \(`p_drop`\) of .* takes a number, got Tensor")
    for args in (good[:-1], good + [None], good[:9] + good[10:]):
        with pytest.raises(AssertionError, match=r"vqa_softmax_attention_pool_len_fwd takes 14 arguments \(logits, v, lens, .*, stream\), got %d" % len(args)):
            check_args(fn, args)
    check_args(_Bound("vqa_rmsprop_step"), [p, p, p, 10, None, 0.1, 0.99, 1e-8, None])
    with pytest.raises(AssertionError, match=r"argument 7 \(`alpha`\) of vqa_rmsprop_step takes a number, got c_void_p"):
        check_args(_Bound("vqa_rmsprop_step"), [p, p, p, 10, None, 0.1, p, 1e-8, None])


# ---- ops._launch, watched or forbidden ---------------------------------------------------------------------------------------
class _Ops:
    def __init__(self):
        self.calls = []
        self._launch = lambda name, shape, fn, *args: self.calls.append((name, shape, fn, args)) or 7


def test_spy_launches_records_and_forwards(monkeypatch):
    ops = _Ops()
    with monkeypatch.context() as m:
        seen = spy_launches(m, ops)
        assert ops._launch("a", (1, 2), len, 3, 4) == 7 and ops._launch("b", (), None) == 7
    ops._launch("c", (5,), None)
    assert seen == [("a", (1, 2)), ("b", ())]
    assert ops.calls == [("a", (1, 2), len, (3, 4)), ("b", (), None, ()), ("c", (5,), None, ())]


def test_forbid_launches_fails_the_test_that_launches(monkeypatch):
    ops = _Ops()
    forbid_launches(monkeypatch, ops)
    with pytest.raises(pytest.fail.Exception, match="a kernel was launched"):
        ops._launch("a", (1,), None)
    assert ops.calls == []
