"""Per-sample region counts for ODA: the masked object-difference kernels (csrc/object_difference_masked.hip,
vqa_object_difference_attention_len_{fwd,bwd}) through the C ABI, one dispatch form at a time, and oda.Model(region_counts=True).
The conventions are those of tests/test_gpu_oda_kernels.py (tests/kernel_harness.py, and the unmasked file's own operands, host mask
and calls, which are imported): outputs sit in sentinel-filled buffers that
are compared whole, inputs in NaN-padded windows, the workspace is exactly _len_bwd_workspace_bytes long, NaN-filled, with a fence
behind it, the launch log says which kernel ran, the mask is drawn on the host (host_keep).

  A  small integers (|value| <= 3, with zeros; every partial sum below 2^24, asserted per case) against an int64 reference that is
     CUT per sample: sample b uses vl[b, :n], w.view(G, N, L)[:, :n] and mask[b, :n, :n].  The padded rows of vl and d_logits hold
     NaN: a NaN in any output fails, so does a non-zero in logits / d_vl rows >= n_b or in d_w slots >= max n_b.  Every backward
     case runs twice and must give the same bits.
  B  lens = N, N <= 36, G <= 4, p in {0, 0.5}, default knobs: all five outputs equal the unmasked entry points' bit for bit.
  C  p = 0.25 (factor 4/3), random operands, mixed counts, against float64 per cut sample under the project's bar (four times the
     error of the same formulas in float32 with torch on the CPU plus one float32 ulp); every case reports what it measured.
  D  a NaN in a sample's valid rows stays in that sample; device counts outside 1..N are clamped; refusals launch nothing.
  E  oda.Model(region_counts=True): float64 restatement per cut sample, padding invisible bit for bit in training, full counts
     equal no key bit for bit (the forward and the head's gradients; the gradients behind the attention's backward do NOT, and
     test_full_counts_equal_a_backward_without_the_key is left failing with its figures), no key issues a default model's
     launches, graph trainer and evaluator.

Dispatch form (as the launch log spells it) -> the cases that launch it and assert that it did:

  oda_len_fwd_mfma_kernel<true>, <false>                 A [mfma-*], [groups-*], [ones] (p = 0.5 / p = 0); B; D
  (oda_len_fwd_kernel<G,kLenBit>)                        A [valu-*-p0.5] (N = 37, 128; G = 5; VQA_K2_MFMA=0)
  (oda_len_fwd_kernel<G,kLenByte>)                       A [valu-*-p0.75], [valu-byteknob]; C
  (oda_len_fwd_kernel<G,kLenPlain>)                      A [valu-*-p0]
  (oda_len_bwd_data_bits_split_kernel<G>)                A [groups-B257-p0.5]; B at B = 257
  (oda_len_bwd_data_bits_kernel<G>)                      A [mfma-*-p0.5], [valu-*-p0.5]
  (oda_len_bwd_data_kernel<G,kLenByte>), <G,kLenPlain>   A [*-p0.75], [*-p0]
  oda_len_bwd_weight_mfma_kernel<true>, <false>          A [mfma-*], [groups-*], [ones]
  (oda_len_bwd_weight_kernel<G,kLenBit>), <G,kLenByte>, <G,kLenPlain>    A [valu-*]
  oda_len_reduce_kernel, oda_len_dbias_kernel<G>         the last launches of every backward case"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from kernel_harness import (E_BADARG, E_UNSUPPORTED, F32, NAN, PAD, Bars, _amax, _below_2_24, _call, _ceil, _out, _ptr, _same_bits,
                            _sentinel, _untouched, _win, assert_exact, dev, ops, set_knobs)  # noqa: F401  (ops: the fixture)
from test_gpu_oda_kernels import (BYTE_KNOB, NO_MFMA, amplitude, bounds, case_seed, drop_cfg, host_keep, keep_factor, mfma_groups, nt_of,
                                  operands, run_bwd, run_fwd, seed_args)

pytestmark = pytest.mark.gpu

F_MFMA_T, F_MFMA_F = "oda_len_fwd_mfma_kernel<true>", "oda_len_fwd_mfma_kernel<false>"
F_BIT, F_BYTE, F_PLAIN = ("(oda_len_fwd_kernel<G,kLen%s>)" % m for m in ("Bit", "Byte", "Plain"))
D_SPLIT, D_BITS = "(oda_len_bwd_data_bits_split_kernel<G>)", "(oda_len_bwd_data_bits_kernel<G>)"
D_BYTE, D_PLAIN = "(oda_len_bwd_data_kernel<G,kLenByte>)", "(oda_len_bwd_data_kernel<G,kLenPlain>)"
W_MFMA_T, W_MFMA_F = "oda_len_bwd_weight_mfma_kernel<true>", "oda_len_bwd_weight_mfma_kernel<false>"
W_BIT, W_BYTE, W_PLAIN = ("(oda_len_bwd_weight_kernel<G,kLen%s>)" % m for m in ("Bit", "Byte", "Plain"))
REDUCE, DBIAS = "oda_len_reduce_kernel", "oda_len_dbias_kernel<G>"


# ---- which kernels a call must launch, restated from the dispatch rules -----------------------------------------------------
def forms_of(B, N, L, G, p, knobs):
    """-> (forward, data gradient, weight gradient) forms and whether the one-bit layout draws the mask"""
    knobs = dict(knobs)
    p8 = drop_cfg(p)[0]
    mode = "Plain" if p8 == 0 else ("Bit" if p8 == 128 and "VQA_K2_BYTE_MASK" not in knobs else "Byte")
    mfma = knobs.get("VQA_K2_MFMA") != 0 and G <= 4 and N <= 36 and mode != "Byte"
    fwd = (F_MFMA_T if mode == "Bit" else F_MFMA_F) if mfma else {"Bit": F_BIT, "Byte": F_BYTE, "Plain": F_PLAIN}[mode]
    if mode == "Bit":
        data = D_SPLIT if _ceil(N, 12) <= 4 and B * _ceil(L, 64) >= 512 else D_BITS
    else:
        data = D_BYTE if mode == "Byte" else D_PLAIN
    weight = (W_MFMA_T if mode == "Bit" else W_MFMA_F) if mfma else {"Bit": W_BIT, "Byte": W_BYTE, "Plain": W_PLAIN}[mode]
    return fwd, data, weight, mode == "Bit"


def fwd_log(form, B, N, L):
    if form in (F_MFMA_T, F_MFMA_F):
        nsets = _ceil(L, 16)
        return [(form, B * 64 * (8 if nsets >= 8 else min(nsets, 4)))]
    return [(form, _ceil(N, 12) * B * nt_of(L))]


def bwd_log(data, weight, B, N, L, G):
    first = (data, _ceil(L, 64) * B * 64 * _ceil(N, 12) if data == D_SPLIT else B * nt_of(L))
    if weight in (W_MFMA_T, W_MFMA_F):
        second = (weight, mfma_groups(B)[0] * 128 * min(_ceil(L, 16), 4))
    else:
        second = (weight, _ceil(N, 12) * min(B, 128) * nt_of(L))
    return [first, second, (REDUCE, _ceil(G * N * L, 64) * 256), (DBIAS, 1024)]


# ---- buffers ------------------------------------------------------------------------------------------------------------------
def _buf(t):
    """fp32 CPU tensor (NaN allowed) -> a GPU buffer that holds it PAD elements in, NaN on both sides"""
    flat = t.reshape(-1).to(F32)
    buf = torch.full((flat.numel() + 2 * PAD,), NAN, dtype=F32)
    buf[PAD:PAD + flat.numel()] = flat
    return buf.to(dev())


def _lens_d(lens):
    return torch.tensor([int(x) for x in lens], dtype=torch.int32, device=dev())


def padded_operands(host, lens):
    """the five operand buffers; rows >= n_b of vl and d_logits hold NaN"""
    vl, ql, w, bias, dS = (t.to(F32).clone() for t in host)
    for b, n in enumerate(lens):
        vl[b, n:] = NAN
        dS[b, n:] = NAN
    return [_buf(t) for t in (vl, ql, w, bias, dS)]


def run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word):
    vl, ql, w, bias, _ = dv
    buf = _out(B * N * G)
    sa, sp, keepalive = seed_args(seed, via_word)
    rc, log = _call(ops, ops._lib.lib().vqa_object_difference_attention_len_fwd, _ptr(vl, PAD), _ptr(ql, PAD), _ptr(w, PAD),
                    _ptr(bias, PAD), _ptr(lens_d), _ptr(buf, PAD), p, sa, sp, B, N, L, G)
    return rc, log, buf


def run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word, gate):
    vl, ql, w, _, dS = dv
    Lb = ops._lib.lib()
    nbytes = Lb.vqa_object_difference_attention_len_bwd_workspace_bytes(B, N, L, G)
    assert nbytes == max(min(B, 256), min(B, 128)) * G * N * L * 4
    ws = _sentinel(nbytes // 4 + PAD)
    ws[:nbytes // 4] = NAN
    outs = [_out(B * N * L), _out(B * L), _out(G * N * L), _out(G)]
    sa, sp, keepalive = seed_args(seed, via_word)
    rc, log = _call(ops, Lb.vqa_object_difference_attention_len_bwd, _ptr(vl, PAD), _ptr(ql, PAD), _ptr(w, PAD), _ptr(dS, PAD),
                    _ptr(lens_d), *(_ptr(o, PAD) for o in outs), _ptr(ws), nbytes, p, sa, sp, B, N, L, G, gate)
    if rc != 0:
        return rc, log, None
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    shapes = [(B, N, L), (B, L), (G, N * L), (G,)]
    return rc, log, tuple(_win(o, sh, n) for o, sh, n in zip(outs, shapes, ("d_vl", "d_ql", "d_w", "d_bias")))


# ======================================================================================================================= A
def cut_reference(host, lens, p, seed, bit_layout, gate):
    """int64, sample by sample on its cut -> (logits, d_vl, d_ql, d_w, d_bias); zeros on the padding and in the untrained slots"""
    vl, ql, w, bias, dS = host
    B, N, L = vl.shape
    G = w.shape[0]
    s = keep_factor(p)
    _below_2_24(*bounds(B, N, L, G, s, _amax(vl), _amax(ql), _amax(w), _amax(bias), _amax(dS)))
    logits, d_vl, d_ql = torch.zeros(B, N, G, dtype=torch.int64), torch.zeros(B, N, L, dtype=torch.int64), torch.zeros(B, L, dtype=torch.int64)
    d_w, d_bias = torch.zeros(G, N, L, dtype=torch.int64), torch.zeros(G, dtype=torch.int64)
    w3 = w.view(G, N, L)
    for b, n in enumerate(lens):
        keep = torch.from_numpy(host_keep(p, seed, B, N, L, bit_layout, b, b + 1)[0, :n, :n]).long()       # [n, n, L]
        T = vl[b, :n] * ql[b]
        X = (keep * (T[:, None, :] - T[None, :, :])).reshape(n, n * L)
        wc = w3[:, :n].reshape(G, n * L)
        logits[b, :n] = s * (X @ wc.t()) + bias
        ds = dS[b, :n]
        d_w[:, :n] += s * (ds.t() @ X).view(G, n, L)
        U = keep * (ds @ wc).view(n, n, L)
        dT = U.sum(1) - U.sum(0)
        dv = s * dT * ql[b]
        d_vl[b, :n] = torch.where(vl[b, :n] > 0, dv, torch.zeros_like(dv)) if gate else dv
        d_ql[b] = s * (dT * vl[b, :n]).sum(0)
        d_bias += ds.sum(0)
    return logits, d_vl, d_ql, d_w.view(G, N * L), d_bias


def _cycle(values, B):
    return tuple(values[i % len(values)] for i in range(B))


EDGE = (36, 1, 33, 5, 32, 2, 35, 31, 3, 4)

# (id, B, N, L, G, p, knobs, gates, counts)
CASES = [
    # the 4x4-MFMA forms: N = 36 (regions 32..35 live in the second mask word) and N = 13; L = 1, 70, 310 (last feature set partial)
    ("mfma-N36-L310-G4-p0.5", 3, 36, 310, 4, 0.5, (), (0, 1), (36, 5, 33)),
    ("mfma-N36-L310-G4-p0", 3, 36, 310, 4, 0.0, (), (0, 1), (32, 1, 35)),
    ("mfma-N36-L70-G3-p0.5", 4, 36, 70, 3, 0.5, (), (1,), (31, 2, 36, 4)),
    ("mfma-N36-L70-G3-p0", 4, 36, 70, 3, 0.0, (), (0,), (3, 36, 32, 33)),
    ("mfma-N36-L1-G1-p0.5", 5, 36, 1, 1, 0.5, (), (0,), (3, 36, 33, 32, 1)),
    ("mfma-N36-L1-G1-p0", 5, 36, 1, 1, 0.0, (), (1,), (35, 4, 31, 2, 5)),
    ("mfma-N13-L70-G3-p0.5", 3, 13, 70, 3, 0.5, (), (0, 1), (13, 1, 5)),
    ("mfma-N13-L310-G4-p0", 3, 13, 310, 4, 0.0, (), (0,), (4, 13, 2)),
    ("mfma-N13-L1-G1-p0.5", 3, 13, 1, 1, 0.5, (), (0,), (3, 12, 13)),
    # group arithmetic: one sample; B = 3 above (odd, uneven sample slots); B = 257 at L = 70 (two samples per group, the last
    # group short, and B ceil(L / 64) = 514 >= 512: the split data gradient); every count 1
    ("groups-B1-p0.5", 1, 36, 70, 4, 0.5, (), (0,), (35,)),
    ("groups-B257-p0.5", 257, 36, 70, 4, 0.5, (), (1,), _cycle(EDGE, 257)),
    ("groups-B257-p0", 257, 36, 70, 2, 0.0, (), (0,), _cycle(EDGE[::-1], 257)),
    ("ones", 4, 36, 70, 4, 0.5, (), (0,), (1, 1, 1, 1)),
    # the VALU family: N > 36, G > 4, VQA_K2_MFMA=0, p = 0.75, VQA_K2_BYTE_MASK=1
    ("valu-N37-L100-G8-p0.5", 3, 37, 100, 8, 0.5, (), (0, 1), (37, 12, 33)),
    ("valu-N37-L100-G8-p0", 3, 37, 100, 8, 0.0, (), (0,), (36, 13, 1)),
    ("valu-N37-L100-G8-p0.75", 3, 37, 100, 8, 0.75, (), (1,), (32, 37, 12)),
    ("valu-N128-L33-G2-p0.5", 3, 128, 33, 2, 0.5, (), (0,), (128, 127, 33)),
    ("valu-N128-L33-G2-p0.75", 3, 128, 33, 2, 0.75, (), (0,), (1, 13, 128)),
    ("valu-N128-L33-G2-p0", 3, 128, 33, 2, 0.0, (), (1,), (32, 127, 12)),
    ("valu-N36-G5-p0.5", 3, 36, 70, 5, 0.5, (), (0,), (36, 35, 13)),
    ("valu-N36-G5-p0", 3, 36, 70, 5, 0.0, (), (0,), (12, 36, 1)),
    ("valu-N36-G5-p0.75", 3, 36, 70, 5, 0.75, (), (0,), (33, 32, 35)),
    ("valu-nomfma-p0.5", 3, 36, 310, 4, 0.5, (NO_MFMA,), (0, 1), (36, 12, 33)),
    ("valu-nomfma-p0", 3, 36, 310, 4, 0.0, (NO_MFMA,), (0,), (13, 35, 32)),
    ("valu-byteknob", 3, 36, 70, 4, 0.5, (BYTE_KNOB,), (0,), (35, 1, 32)),
]


@functools.lru_cache(maxsize=2)
def _case_reference(name, gate):
    _, B, N, L, G, p, knobs, _, lens = next(c for c in CASES if c[0] == name)
    seed, _ = case_seed(name)
    s = keep_factor(p)
    host = operands(B, N, L, G, amplitude(B, N, L, G, s, True), bool(gate))
    return host, cut_reference(host, lens, p, seed, forms_of(B, N, L, G, p, knobs)[3], gate)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_small_integers_are_exact(ops, lib_option, case):
    name, B, N, L, G, p, knobs, gates, lens = case
    assert len(lens) == B and all(1 <= n <= N for n in lens)
    set_knobs(lib_option, knobs)
    seed, via_word = case_seed(name)
    f_form, d_form, w_form, _ = forms_of(B, N, L, G, p, knobs)
    lens_d = _lens_d(lens)
    for gate in gates:
        host, ref = _case_reference(name, gate)
        dv = padded_operands(host, lens)
        rc, log, buf = run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word)
        assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
        assert log == fwd_log(f_form, B, N, L), (name, log)
        assert_exact(name + " logits", _win(buf, (B, N, G), name), ref[0])
        runs = []
        for _ in range(2):
            rc, blog, got = run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word, gate)
            assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
            assert blog == bwd_log(d_form, w_form, B, N, L, G), (name, blog)
            runs.append(got)
        for key, got, want, again in zip(("d_vl", "d_ql", "d_w", "d_bias"), runs[0], ref[1:], runs[1]):
            assert_exact("%s gate %d %s" % (name, gate, key), got, want)
            assert _same_bits(got, again), "%s %s: two runs differ" % (name, key)
        if name == "ones":
            # a sample of one region has no differences: logits = bias there, d_bias the sum of row 0, everything else exactly 0
            logits = _win(run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word)[2], (B, N, G), name).cpu()
            assert torch.equal(logits[:, 0], host[3].to(F32).expand(B, G)) and not bool(logits[:, 1:].any())
            assert not any(bool(t.any()) for t in runs[0][:3])
            assert torch.equal(runs[0][3].cpu(), host[4][:, 0].sum(0).to(F32))


# ======================================================================================================================= B
def _random_operands(B, N, L, G, seed):
    gen = torch.Generator().manual_seed(seed)
    vl, ql = torch.randn(B, N, L, generator=gen).clamp_min(0.0), torch.randn(B, L, generator=gen).abs()
    w, bias = torch.randn(G, N * L, generator=gen) / (N * L) ** 0.5, 0.1 * torch.randn(G, generator=gen)
    return vl, ql, w, bias, torch.randn(B, N, G, generator=gen)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("B,N,L,G", [(3, 36, 70, 4), (3, 36, 310, 4), (257, 36, 70, 4), (257, 36, 310, 4), (3, 13, 70, 3)])
def test_full_length_equals_the_unmasked_entry_points(ops, B, N, L, G, p):
    """lens = N under default knobs: the masked kernels are the unmasked default kernels stopped at n_b, so logits and all four
    gradients carry the unmasked entry points' bits (gate on: the model's form)"""
    seed, via_word = case_seed("full-%d-%d-%d-%g" % (B, N, L, p))
    dv = [_buf(t) for t in _random_operands(B, N, L, G, 31 * B + L)]
    lens_d = _lens_d([N] * B)
    rc, _, plain = run_fwd(ops, dv, B, N, L, G, p, seed, via_word)
    assert rc == 0
    rc, log, masked = run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word)
    f_form, d_form, w_form, _ = forms_of(B, N, L, G, p, ())
    assert rc == 0 and log == fwd_log(f_form, B, N, L), (rc, log)
    a, b = _win(plain, (B, N, G), "logits"), _win(masked, (B, N, G), "masked logits")
    assert bool(torch.isfinite(a).all()) and _same_bits(a, b), "logits: %d elements differ" % int((a != b).sum())
    rc, _, want = run_bwd(ops, dv, B, N, L, G, p, seed, via_word, 1)
    assert rc == 0
    rc, blog, got = run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word, 1)
    assert rc == 0 and blog == bwd_log(d_form, w_form, B, N, L, G), (rc, blog)
    for key, x, y in zip(("d_vl", "d_ql", "d_w", "d_bias"), want, got):
        assert bool(torch.isfinite(x).all()) and _same_bits(x, y), "%s: %d elements differ" % (key, int((x != y).sum()))


# ======================================================================================================================= C
def cut_formulas(vl, ql, w, bias, mask, dS, lens):
    """the contract per cut sample in the dtype of the operands (float64: the reference; float32: the bar's yardstick)"""
    B, N, L = vl.shape
    G = w.shape[0]
    logits, d_vl, d_ql = torch.zeros(B, N, G, dtype=vl.dtype), torch.zeros_like(vl), torch.zeros_like(ql)
    d_w, d_bias = torch.zeros(G, N, L, dtype=vl.dtype), torch.zeros(G, dtype=vl.dtype)
    w3 = w.view(G, N, L)
    for b, n in enumerate(lens):
        m = mask[b, :n, :n]
        diff = vl[b, :n, None, :] - vl[b, None, :n, :]
        vq = (diff * ql[b] * m).reshape(n, n * L)
        wc = w3[:, :n].reshape(G, n * L)
        logits[b, :n] = vq @ wc.t() + bias
        d_w[:, :n] += (dS[b, :n].t() @ vq).view(G, n, L)
        dvq = (dS[b, :n] @ wc).view(n, n, L) * m
        dd = dvq * ql[b]
        d_vl[b, :n] = dd.sum(1) - dd.sum(0)
        d_ql[b] = (dvq * diff).sum((0, 1))
        d_bias += dS[b, :n].sum(0)
    return logits, d_vl, d_ql, d_w.view(G, N * L), d_bias


@pytest.mark.parametrize("B,N,L,G,lens", [(3, 36, 310, 4, (36, 20, 7)), (2, 37, 100, 8, (37, 13))])
def test_non_dyadic_rate_against_float64(ops, measured, B, N, L, G, lens):
    """p = 0.25: the byte-layout VALU family with random operands and mixed counts, padding NaN"""
    p, seed = 0.25, (5 << 32) + 1000 * N + G
    host = _random_operands(B, N, L, G, 97 * N + G)
    mask = torch.from_numpy(host_keep(p, seed, B, N, L, False).astype(np.float32) * np.float32(drop_cfg(p)[1]))
    dv = padded_operands(host, lens)
    lens_d = _lens_d(lens)
    rc, log, buf = run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, False)
    assert rc == 0 and log == fwd_log(F_BYTE, B, N, L), (rc, log)
    rc, blog, got = run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, True, 0)
    assert rc == 0 and blog == bwd_log(D_BYTE, W_BYTE, B, N, L, G), (rc, blog)
    ref64 = cut_formulas(*(t.double() for t in host[:4]), mask.double(), host[4].double(), lens)
    ref32 = cut_formulas(*host[:4], mask, host[4], lens)
    bars = Bars(measured, "B%d N%d L%d G%d" % (B, N, L, G))
    for name, have, r64, r32 in zip(("logits", "d_vl", "d_ql", "d_w", "d_bias"), (_win(buf, (B, N, G), "logits"),) + got, ref64, ref32):
        bars.check(name, have, r64, r32)
    bars.close()


# ======================================================================================================================= D
@pytest.mark.parametrize("name,G,p,knobs", [("mfma-p0.5", 2, 0.5, ()), ("mfma-p0", 2, 0.0, ()), ("byte", 2, 0.75, ()),
                                            ("bits", 2, 0.5, (NO_MFMA,)), ("plain", 5, 0.0, ())], ids=lambda x: x if isinstance(x, str) else None)
def test_a_nan_stays_in_its_sample(ops, lib_option, name, G, p, knobs):
    """a NaN in a VALID row of vl of sample 1: logits, d_vl and d_ql of every other sample are bit for bit those of the clean run"""
    B, N, L = 4, 13, 70
    lens = (13, 9, 4, 12)
    set_knobs(lib_option, knobs)
    seed, via_word = case_seed("len-nan-" + name)
    host = operands(B, N, L, G, 3, False)
    f_form, d_form, w_form, _ = forms_of(B, N, L, G, p, knobs)
    lens_d = _lens_d(lens)
    runs = []
    for dirty in (False, True):
        hv = [t.to(F32).clone() for t in host]
        if dirty:
            hv[0][1, 3, 7] = NAN
        dv = padded_operands(hv, lens)
        rc, log, out = run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word)
        assert rc == 0 and log == fwd_log(f_form, B, N, L), (name, rc, log)
        rc, blog, got = run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word, 0)
        assert rc == 0 and blog == bwd_log(d_form, w_form, B, N, L, G), (name, rc, blog)
        runs.append((_win(out, (B, N, G), "logits"), got[0], got[1]))
    others = [0, 2, 3]
    for key, clean, dirt in zip(("logits", "d_vl", "d_ql"), *runs):
        assert bool(torch.isfinite(clean).all()), (name, key)
        assert _same_bits(clean[others], dirt[others]), "%s %s: the NaN of sample 1 reached another sample" % (name, key)
    assert bool(torch.isnan(runs[1][0][1]).any()), "the NaN did not reach its own sample's logits"


@pytest.mark.parametrize("G,p", [(4, 0.5), (5, 0.75)], ids=["mfma", "valu"])
def test_device_counts_outside_1_to_n_are_clamped(ops, G, p):
    """lens = (0, -5, N + 9, 5) on the device computes what (1, 1, N, 5) computes"""
    B, N, L = 4, 13, 70
    seed, via_word = case_seed("clamp-%d" % G)
    s = keep_factor(p)
    host = operands(B, N, L, G, amplitude(B, N, L, G, s, True), False)
    lens = (1, 1, N, 5)
    ref = cut_reference(host, lens, p, seed, forms_of(B, N, L, G, p, ())[3], 0)
    dv = padded_operands(host, lens)
    lens_d = _lens_d((0, -5, N + 9, 5))
    rc, _, buf = run_len_fwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word)
    assert rc == 0
    assert_exact("logits", _win(buf, (B, N, G), "logits"), ref[0])
    rc, _, got = run_len_bwd(ops, dv, lens_d, B, N, L, G, p, seed, via_word, 0)
    assert rc == 0
    for key, have, want in zip(("d_vl", "d_ql", "d_w", "d_bias"), got, ref[1:]):
        assert_exact(key, have, want)


def test_refusals_launch_nothing(ops):
    """the refusals of the unmasked entry points, plus lens = NULL: an error text, no launch, the outputs untouched"""
    Lb = ops._lib.lib()
    n = 1 << 20
    src = torch.zeros(n, device=dev())
    lens = torch.ones(65536, dtype=torch.int32, device=dev())
    outs = [_sentinel(n) for _ in range(5)]
    buf = (ctypes.c_ulonglong * 16)()
    ws_of = Lb.vqa_object_difference_attention_len_bwd_workspace_bytes

    def refused(code, fn, *args):
        Lb.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, args, Lb.vqa_last_error())
        assert Lb.vqa_last_error() and Lb.vqa_launch_log(buf, 16) == 0, "a refused call launched a kernel"

    def fwd(B=2, N=5, L=8, G=2, p=0.5, null=None):
        ptrs = [_ptr(src)] * 4 + [_ptr(lens), _ptr(outs[0])]
        if null is not None:
            ptrs[null] = None
        return (Lb.vqa_object_difference_attention_len_fwd, *ptrs, p, 7, None, B, N, L, G)

    def bwd(B=2, N=5, L=8, G=2, p=0.5, null=None, short=0):
        ptrs = [_ptr(src)] * 4 + [_ptr(lens)] + [_ptr(o) for o in outs]
        if null is not None:
            ptrs[null] = None
        need = ws_of(B, N, L, G)
        assert need <= 4 * n and max(B * N * L, G * N * L, 1) <= n
        return (Lb.vqa_object_difference_attention_len_bwd, *ptrs, (need or 4 * n) - short, p, 7, None, B, N, L, G, 0)

    for i in range(6):
        refused(E_BADARG, *fwd(null=i))
    for i in range(10):
        refused(E_BADARG, *bwd(null=i))
    for kw in (dict(B=0), dict(N=0), dict(L=-1), dict(G=0), dict(p=-0.25), dict(p=1.0)):
        refused(E_BADARG, *fwd(**kw))
        refused(E_BADARG, *bwd(**kw))
    refused(E_BADARG, *bwd(short=1))
    assert ws_of(0, 5, 8, 2) == 0 and ws_of(2, 5, 8, 2) == 2 * 2 * 40 * 4
    for kw in (dict(G=9), dict(B=1, N=129), dict(B=1, L=1025), dict(B=65536, N=1, L=1, G=1)):
        refused(E_UNSUPPORTED, *fwd(**kw))
        refused(E_UNSUPPORTED, *bwd(**kw))
    for p in (0.0, 0.5, 0.75):
        refused(E_UNSUPPORTED, *bwd(B=2, N=40, L=1024, G=8, p=p))
    assert b"LDS" in Lb.vqa_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert _untouched(t)


def test_ops_take_lens_and_refuse_bad_ones(ops):
    """ops.object_difference_attention(lens=): int32 [B] on vl's device or a ValueError before anything launches; with it the
    `_len_` entry points run, without it today's"""
    B, N, L, G = 3, 13, 70, 2
    vl, ql, w, bias, dS = (t.to(dev()) for t in _random_operands(B, N, L, G, 5))
    names = []
    orig = ops._launch

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)

    ops._launch = spy
    try:
        for bad in (torch.ones(B, dtype=torch.int64, device=dev()), torch.ones(B - 1, dtype=torch.int32, device=dev()),
                    torch.ones(B, dtype=torch.int32), torch.ones(B, device=dev()), [1, 2, 3]):
            with pytest.raises(ValueError, match="lens"):
                ops.object_difference_attention(vl, ql, w, bias, 0.0, 0, lens=bad)
        assert names == []
        vl.requires_grad_()
        w.requires_grad_()
        lens = _lens_d((9, 2, 7))
        out = ops.object_difference_attention(vl, ql, w, bias, 0.5, 11, gate_dvl=True, lens=lens)
        out.backward(dS)
        assert names == ["object_difference_attention_len_fwd", "object_difference_attention_len_bwd"]
        assert not bool(out[1, 2:].any()) and not bool(vl.grad[1, 2:].any()) and not bool(w.grad.view(G, N, L)[:, 9:].any())
        assert bool(w.grad.view(G, N, L)[:, 8].any())
        del names[:]
        ops.object_difference_attention(vl, ql, w, bias, 0.5, 11, gate_dvl=True).backward(dS)
        assert names == ["object_difference_attention_fwd", "object_difference_attention_bwd"]
    finally:
        ops._launch = orig


# ======================================================================================================================= E
V_LEN = [36, 20, 2, 7]
RTOL, ATOL = 1e-3, 1e-7       # the bars of the CoR2 region-count test (tests/test_gpu_region_counts.py)


def _model(nans, region_counts=True, train=False):
    from oracle import seeded
    from vqa_playground_pytorch_amd import ODAModel
    model = seeded.load_state(ODAModel(["PAD", "UNK"], nans, region_counts=region_counts), 0)
    return (model.train() if train else model.eval()).to(dev())


def _padded_inputs(B, v_len, nans, seed, fill="noise"):
    """seeded inputs whose rows n >= v_len[b] are overwritten: N(0, 10^2) noise, or zeros"""
    from oracle import seeded
    v, q, a = seeded.seeded_inputs(B, regions=36, answers=nans, seed=seed)
    noise = seeded.seeded_array(v.shape, 4242, scale=10.0)
    for b, n in enumerate(v_len):
        v[b, n:] = noise[b, n:] if fill == "noise" else 0.0
    return v, q, a


def restated_oda(P, v, q, n, N=36):
    """config/ODA.py's forward in eval mode from a dict of float64 parameters, on ONE sample cut to its n regions: v [1,n,2048],
    q [1,2400]; conv_att's weight is cut to the first n region slots -> (logits [1,A], alpha [n,4])"""
    relu = torch.relu

    def lin(x, name):
        return x @ P[name + ".linear.weight"].t() + P[name + ".linear.bias"]

    v_low = relu(v @ P["compress_v.conv.weight"][:, :, 0].t() + P["compress_v.conv.bias"])            # [1,n,310]
    q_low = relu(lin(q, "compress_q"))                                                               # [1,310]
    low = v_low.size(2)
    vq = ((v_low[:, :, None, :] - v_low[:, None, :, :]) * q_low[:, None, None, :]).reshape(1, n, n * low)
    wc = P["att.conv_att.conv.weight"][:, :, 0].view(4, N, low)[:, :n].reshape(4, n * low)
    alpha = torch.softmax(vq @ wc.t() + P["att.conv_att.conv.bias"], dim=1)                          # [1,n,4]
    pooled = alpha.transpose(1, 2) @ v                                                               # [1,4,2048]
    v_final = torch.cat([relu(lin(pooled[:, g], "att.list_linear_v_fusion.%d" % g)) for g in range(4)], 1)
    q_final = relu(lin(q, "linear_q"))
    x = sum(lin(v_final, "fusion_final.list_linear1.%d" % r) * lin(q_final, "fusion_final.list_linear2.%d" % r) for r in range(5))
    return lin(x, "linear_classif"), alpha[0]


def _rel(got, want):
    got, want = got.detach().cpu().numpy().astype(np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all()
    return np.abs(got - want).max() / max(np.abs(want).max(), 1e-20)


def test_model_with_counts_matches_the_float64_restatement_per_cut_sample(measured):
    from oracle import reference_faithful as RF
    nans = 2000
    model = _model(nans)
    v, q, a = _padded_inputs(4, V_LEN, nans, 1)
    logits = model({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev()), "v_len": torch.tensor(V_LEN)})
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    P = {n: p.detach().cpu().double().requires_grad_() for n, p in model.named_parameters()}
    want_logits, want_loss = [], 0.0
    alphas = model.alpha_dict["alphas"].reshape(4, 36, -1)
    for b, n in enumerate(V_LEN):
        lo, alpha = restated_oda(P, torch.from_numpy(v[b:b + 1, :n]).double(), torch.from_numpy(q[b:b + 1]).double(), n)
        ls = RF.kld_sum_loss(lo, torch.from_numpy(a[b:b + 1]).double())
        ls.backward()                                                      # parameter gradients add up over the four samples
        want_loss += float(ls)
        want_logits.append(lo.detach().numpy())
        assert not bool(alphas[b, n:].any()), "alphas not exactly 0 on the padding of sample %d" % b
        assert _rel(alphas[b, :n, 0], alpha[:, 0].detach().numpy()) <= RTOL
    err = _rel(logits, np.concatenate(want_logits))
    worst = max((float(np.abs(p.grad.detach().cpu().numpy().astype(np.float64) - P[n].grad.numpy()).max()
                       / (RTOL * np.abs(P[n].grad.numpy()).max() + ATOL)), n) for n, p in model.named_parameters())
    measured("logits", err, RTOL)
    measured("worst gradient / bar", worst[0], 1.0, worst[1])
    assert err <= RTOL and abs(loss.item() - want_loss) <= RTOL * abs(want_loss)
    assert worst[0] <= 1.0, worst


def _train_step(model, v, q, a, v_len):
    from oracle import reference_faithful as RF
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)                    # (the fused masks' seeds are drawn from torch's CPU generator)
    sample = {"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev())}
    if v_len is not None:
        sample["v_len"] = v_len
    logits = model(sample)
    loss = RF.kld_sum_loss(logits, torch.from_numpy(a).to(dev()))
    loss.backward()
    return (logits.detach().clone(), loss.detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters()},
            model.alpha_dict["alphas"].clone())


def test_padding_is_invisible_to_a_training_step():
    """train mode (dropout on), the same seeds twice, B = 64: padded rows of zeros, then of N(0, 10^2) noise (finite: compress_v
    itself runs over all rows).  Logits, loss, alphas (exactly 0 on the padding) and every parameter gradient are bit-identical"""
    B, nans = 64, 300
    rs = np.random.RandomState(11)
    v_len = rs.randint(1, 37, size=B)
    v_len[3], v_len[B - 2] = 1, 36
    model = _model(nans, train=True)
    lens_d = torch.from_numpy(v_len.astype(np.int32)).to(dev())
    runs = [_train_step(model, *_padded_inputs(B, v_len, nans, 31, fill), lens_d) for fill in ("zeros", "noise")]
    assert torch.equal(runs[0][0], runs[1][0]), "logits"
    assert torch.equal(runs[0][1], runs[1][1]), "loss"
    assert torch.equal(runs[0][3], runs[1][3]), "alphas"
    for b, n in enumerate(v_len):
        assert not bool(runs[1][3].reshape(B, 36, -1)[b, n:].any()), "alphas not exactly 0 on the padding of sample %d" % b
    differ = [n for n in runs[0][2] if not torch.equal(runs[0][2][n], runs[1][2][n])]
    assert not differ, differ
    assert all(bool(torch.isfinite(g).all()) for g in runs[1][2].values())


# the parameters whose gradients pass through the attention's backward (K3): d_logits -> K2's backward -> conv_att, compress_v, compress_q
BEHIND_K3 = ("compress_v.conv.weight", "compress_v.conv.bias", "compress_q.linear.weight", "compress_q.linear.bias",
             "att.conv_att.conv.weight", "att.conv_att.conv.bias")


def _full_and_plain(train, B=8):
    from oracle import seeded
    nans = 300
    model = _model(nans, train=train)
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=77)
    return _train_step(model, v, q, a, None), _train_step(model, v, q, a, torch.full((B,), 36, dtype=torch.int64))


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_full_counts_equal_a_forward_without_the_key(train):
    """v_len = 36 everywhere: logits, loss and alphas of the masked model equal the same model's without the key bit for bit, and so
    does every parameter gradient that does not pass through the attention's own backward"""
    plain, full = _full_and_plain(train)
    assert torch.equal(plain[0], full[0]) and torch.equal(plain[1], full[1]) and torch.equal(plain[3], full[3])
    differ = [n for n in plain[2] if n not in BEHIND_K3 and not torch.equal(plain[2][n], full[2][n])]
    assert not differ, differ


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_full_counts_equal_a_backward_without_the_key(train, measured):
    """v_len = 36 everywhere: EVERY parameter gradient equals the same model's without the key, bit for bit.

    B = 64, the smallest batch at which the run WITHOUT the key has bits of its own to compare with: below it the unmasked
    attention backward (attention_pool.hip, launch_bwd: fp32 takes the one-launch form from 64 samples on) adds its partial dot
    products with float atomics in whatever order the waves arrive, so two runs without the key already differ in the last bit of
    d_logits and of the six gradients behind it (BEHIND_K3) -- at B = 8 they differed from the masked run by 1e-7..1e-6 of scale,
    the rounding of that sum.  From 64 samples on both attention backwards sum in one fixed order, and it is the same order:
    per wave the 16-lane butterfly and the four DPP rows, then the waves' slots in wave order.  The masked K2 returns the unmasked
    K2's bits from the same d_logits (test_full_length_equals_the_unmasked_entry_points above)."""
    plain, full = _full_and_plain(train, B=64)
    for n in BEHIND_K3:
        g0, g1 = plain[2][n], full[2][n]
        measured(n, float((g0 - g1).abs().max()) / max(float(g0.abs().max()), 1e-30))
    differ = [n for n in plain[2] if not torch.equal(plain[2][n], full[2][n])]
    assert not differ, differ


def _launch_names(ops, fn):
    names, orig = [], ops._launch

    def spy(name, shape, *a):
        names.append((name, tuple(shape)))
        return orig(name, shape, *a)

    ops._launch = spy
    try:
        fn()
    finally:
        ops._launch = orig
    return names


def test_a_counts_model_without_the_key_issues_a_default_models_launches(ops):
    from oracle import seeded
    B, nans = 8, 300
    v, q, a = seeded.seeded_inputs(B, answers=nans, seed=3)
    logs = [_launch_names(ops, lambda: _train_step(_model(nans, region_counts=rc, train=True), v, q, a, None)) for rc in (False, True)]
    assert logs[0] == logs[1] and any(n == "object_difference_attention_fwd" for n, _ in logs[0])
    assert not any("_len_" in n for n, _ in logs[1])
    with_key = _launch_names(ops, lambda: _train_step(_model(nans, train=True), v, q, a, torch.full((B,), 36, dtype=torch.int32)))
    assert any(n == "object_difference_attention_len_bwd" for n, _ in with_key)
    with pytest.raises(ValueError, match="v_len"):
        _model(nans, region_counts=False)({"v": torch.from_numpy(v).to(dev()), "q_idxes": torch.from_numpy(q).to(dev()),
                                           "v_len": torch.full((B,), 36, dtype=torch.int32)})


def test_captured_step_reads_the_counts_of_every_batch():
    """DataParallelTrainer(graph=True) on the masked model, eval mode: the two replays after the capture take different counts and
    give the losses and parameters of a second trainer that launches the same steps kernel by kernel (its capture put off),
    bit for bit; a batch without the key after a capture with it is stepped kernel by kernel and the graph keeps serving"""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    B, nans = 8, 300
    rs = np.random.RandomState(5)
    warm = DataParallelTrainer.EAGER_STEPS_BEFORE_CAPTURE
    lens = [rs.randint(1, 37, size=B) for _ in range(warm + 2)]
    out = {}
    for replay in (False, True):
        model = _model(nans)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
        if not replay:
            tr.EAGER_STEPS_BEFORE_CAPTURE = 10 ** 9
        losses = []
        for step, v_len in enumerate(lens):
            v, q, a = (torch.from_numpy(x).to(dev()) for x in _padded_inputs(B, v_len, nans, 40 + step))
            counts = torch.from_numpy(v_len) if step % 2 else torch.from_numpy(v_len.astype(np.int32)).to(dev())
            loss, norm = tr.step({"v": v, "q_idxes": q, "v_len": counts}, a)
            losses.append((loss.detach().clone(), norm.detach().clone()))
        if replay:
            assert tr._graph is not None and "v_len" in tr._graph["sample"], "the step was not captured with its counts"
        else:
            assert tr._graph is None
        out[replay] = (losses, [p.detach().clone() for p in model.parameters()])
        if replay:
            v, q, a = (torch.from_numpy(x).to(dev()) for x in _padded_inputs(B, [36] * B, nans, 90))
            loss, _ = tr.step({"v": v, "q_idxes": q}, a)                      # no key: falls back, kernel by kernel
            assert bool(torch.isfinite(loss)) and tr._graph is not None
            loss, _ = tr.step({"v": v, "q_idxes": q, "v_len": torch.from_numpy(lens[0])}, a)
            assert bool(torch.isfinite(loss))
    for (l0, n0), (l1, n1) in zip(out[False][0], out[True][0]):
        assert torch.equal(l0, l1) and torch.equal(n0, n1), (out[False][0], out[True][0])
    assert all(torch.equal(p0, p1) for p0, p1 in zip(out[False][1], out[True][1]))
    assert len({float(l) for l, _ in out[True][0]}) == len(lens)


def test_evaluator_replays_the_forward_with_the_counts_of_each_batch():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    B, nans = 8, 300
    rs = np.random.RandomState(9)
    batches = []
    for i in range(Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 2):
        v_len = rs.randint(1, 37, size=B)
        v, q, a = _padded_inputs(B, v_len, nans, 60 + i)
        batches.append({"v": torch.from_numpy(v), "q_idxes": torch.from_numpy(q), "a": torch.from_numpy(a), "v_len": torch.from_numpy(v_len)})
    out = {}
    for graph in (False, True):
        ev = Evaluator(_model(nans), graph=graph)
        out[graph] = [{k: t.clone() for k, t in ev.step(b).items() if t is not None} for b in batches]
        if graph:
            assert ev._graph is not None and "v_len" in ev._graph["inputs"], "the forward was not captured with its counts"
    for plain, replayed in zip(out[False], out[True]):
        assert torch.equal(plain["pred"], replayed["pred"]) and torch.equal(plain["top_idx"], replayed["top_idx"])
        assert torch.equal(plain["hits"], replayed["hits"])
    with pytest.raises(ValueError):
        Evaluator(_model(nans), graph=False).step(dict(batches[0], v_len=torch.zeros(B, dtype=torch.int64)))
