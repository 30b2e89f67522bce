"""Every launch form of the object-difference attention kernels (csrc/object_difference.hip: K2), through the C ABI, one dispatch
form at a time.  tests/test_gpu_kernels.py reaches this file through autograd under a loose tolerance and never says which kernel
ran; here every VQA_LAUNCH site is launched, the launch log (kernel expression and grid in work-items, the grid restated from B, N,
L and G) says that it was, and its result is compared whole.

  M  the dropout mask, drawn on the CPU from (p, seed) by host_keep() below -- an independent restatement of mask_word32 /
     drop_key / mask_word / make_drop and of the two counter layouts documented at the top of the .hip file.
     vqa_object_difference_dropout_mask equals it bit for bit in both layouts; every reference below uses the host mask only.
  A  small-integer operands (|vl|, |ql|, |w|, |bias|, |d_logits| <= 3, with zeros; vl >= 0 under gate_dvl = 1; p in {0, 0.5, 0.75}:
     keep factors 2 and 4): every fp32 partial sum is an integer below 2^24 (asserted per case from the operands' magnitudes; the
     amplitude is lowered where 3 would leave that range), so any order of summation gives the same bits.  The reference is int64
     on the CPU, chunked over b.  Outputs sit in sentinel-filled buffers that are compared whole, inputs in NaN-padded ones, the
     workspace is exactly _bwd_workspace_bytes long, pre-filled with NaN, with a sentinel fence behind it.
  B  p = 0.25 (factor 4/3) with random operands against float64 (oracle/kernels_np.py, fed with the host mask), under the project's
     bar (Bars of tests/kernel_harness.py): four times the error of the same formula in float32 with torch on the
     CPU plus one float32 ulp of the tensor's largest magnitude.  Every case reports what it measured.
  C  a NaN stays in its sample (what a dropped NaN becomes INSIDE its sample is not asserted: the bit layout ANDs it to 0, the byte
     layout multiplies it); refusals launch nothing and leave the outputs alone.  The forward accepts N = 40, L = 1024 (case
     [bits-N40-L1024] of section A), the backward refuses it: its data gradient would need 165 504 bytes of LDS.
  D  test_every_launch_site_is_declared (no GPU): every VQA_LAUNCH first argument of the file is the form of some case below.

Not tested, on purpose: the flips to 64-bit counters (oda_bits_mode's fall-back to the byte layout and oda_mfma_ok's size test)
need B N L near 2^30, 4 GB of vl.  VQA_K2_BYTE_MASK is tested as `1` only: the dispatcher asks whether the knob is set, so `0`
selects the byte layout as well.

Dispatch form (as the launch log spells it) -> the test that launches it and asserts that it did:

  oda_mask_kernel                                   test_exported_mask_is_the_host_mask, .._device_seed_word
  (oda_fwd_mfma_kernel<true,true>)                  test_forward_small_integers_are_exact [mfma-pk-*] (L = 1 .. 1024: 1, 2, 3, 4, 8 waves)
  oda_fwd_mfma_kernel<true>                         ... [mfma-nopk-*] (VQA_K2_PK=0)
  oda_fwd_mfma_kernel<false>                        ... [mfma-false-*] (p = 0)
  (oda_fwd_bits_kernel<G>)                          ... [bits-*] (G = 5..8; G <= 4 under VQA_K2_MFMA=0; N = 32 .. 128; L = 1024)
  (oda_fwd_kernel<G,true>)                          ... [byte-*] (p = 0.75, G = 1..8; p = 0.5 under VQA_K2_BYTE_MASK=1)
  (oda_fwd_kernel<G,false>)                         ... [plain-*] (p = 0: N = 37, VQA_K2_MFMA=0 or G >= 5)
  (oda_bwd_data_bits_split_kernel<G>)               test_backward_small_integers_are_exact [split-*], [groups-B513], [G*-p0.5-B512], [dbias-*]
  (oda_bwd_data_bits_kernel<G>)                     ... [nosplit-*], [full-p0.5], [lds-p0.5], [G*-p0.5]
  (oda_bwd_data_kernel<G,true>), <G,false>          ... [G*-p0.75], [G*-p0], [lds-*]
  (oda_bwd_weight_mfma_staged_kernel<true,1>)       ... [full-p0.5], [groups-*]          (the VQA_K2_STAGED macro site, four expansions)
  (oda_bwd_weight_mfma_staged_kernel<false,1>)      ... [full-p0], [groups-B257-p0]
  (oda_bwd_weight_mfma_staged_kernel<true,2>), <false,2>   ... [halves-*] (VQA_K2_WSTAGE=2)
  (oda_bwd_weight_mfma_kernel<true,true>)           ... [unstaged-p0.5] (VQA_K2_WSTAGE=0)
  oda_bwd_weight_mfma_kernel<true>, <false>         ... [nopk-*] (VQA_K2_PK=0), [unstaged-p0]
  (oda_bwd_weight_bits_kernel<G>)                   ... [G*-p0.5], [valu-groups-*], [split-N48], [nosplit-N49], [lds-p0.5], [N128-p0.5]
  (oda_bwd_weight_kernel<G,true>), <G,false>        ... [G*-p0.75], [G*-p0], [valu-groups-*]
  (oda_bwd_fused_kernel<true>), <false>             ... [fused-*] (VQA_K2_FUSED=1), then oda_reduce_kernel and oda_dbias_kernel<G>
  oda_reduce_kernel, oda_dbias_kernel<G>            the last launches of every backward case (G N L % 64 != 0 in most; B N = 8191, 8192,
                                                    8193 in [dbias-*])"""
import ctypes
import functools
import os
import re
import zlib

import numpy as np
import pytest
import torch

from kernel_harness import (E_BADARG, E_UNSUPPORTED, F32, NAN, PAD, Bars, _amax, _below_2_24, _call, _ceil, _in, _out, _ptr, _same_bits,
                            _sentinel, _untouched, _win, assert_exact, dev, launch_sites, ops, set_knobs)  # noqa: F401  (ops: the fixture)

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
SALT = 0x1F00000007     # what a call that passes its seed through the device word adds on the host side

# ---- the launch log's spelling of every dispatch form (blanks removed) -------------------------------------------------------
MASK_K = "oda_mask_kernel"
FWD_MFMA_PK, FWD_MFMA_T, FWD_MFMA_F = "(oda_fwd_mfma_kernel<true,true>)", "oda_fwd_mfma_kernel<true>", "oda_fwd_mfma_kernel<false>"
FWD_BITS, FWD_BYTE, FWD_PLAIN = "(oda_fwd_bits_kernel<G>)", "(oda_fwd_kernel<G,true>)", "(oda_fwd_kernel<G,false>)"
D_SPLIT, D_BITS = "(oda_bwd_data_bits_split_kernel<G>)", "(oda_bwd_data_bits_kernel<G>)"
D_BYTE, D_PLAIN = "(oda_bwd_data_kernel<G,true>)", "(oda_bwd_data_kernel<G,false>)"
STAGED_SITE = "(oda_bwd_weight_mfma_staged_kernel<MASK_,JH_>)"          # the macro's launch site as the source spells it
W_STAGED = {(m, jh): "(oda_bwd_weight_mfma_staged_kernel<%s,%d>)" % ("true" if m else "false", jh) for m in (True, False) for jh in (1, 2)}
W_MFMA_PK, W_MFMA_T, W_MFMA_F = "(oda_bwd_weight_mfma_kernel<true,true>)", "oda_bwd_weight_mfma_kernel<true>", "oda_bwd_weight_mfma_kernel<false>"
W_BITS, W_BYTE, W_PLAIN = "(oda_bwd_weight_bits_kernel<G>)", "(oda_bwd_weight_kernel<G,true>)", "(oda_bwd_weight_kernel<G,false>)"
FUSED_T, FUSED_F = "(oda_bwd_fused_kernel<true>)", "(oda_bwd_fused_kernel<false>)"
REDUCE, DBIAS = "oda_reduce_kernel", "oda_dbias_kernel<G>"
FWD_MFMA_FORMS = (FWD_MFMA_PK, FWD_MFMA_T, FWD_MFMA_F)
W_MFMA_FORMS = tuple(W_STAGED.values()) + (W_MFMA_PK, W_MFMA_T, W_MFMA_F)


# ======================================================================================================================= M: the host mask
def _hash32(x):
    """lowbias32 on a uint64 numpy array of 32-bit values (mask_word32 without its key)"""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def drop_cfg(p):
    """make_drop: (p8, the keep factor in float32)"""
    p8 = min(max(int(np.float32(p) * np.float32(256.0) + np.float32(0.5)), 0), 255)
    return p8, float(np.float32(256.0) / (np.float32(256.0) - np.float32(p8)))


def drop_key(seed):
    s = int(seed) & M64
    return (s & M32) ^ (((s >> 32) * 0x9E3779B9) & M32)


def host_keep(p, seed, B, N, L, bit_layout, b0=0, b1=None):
    """keep(b, i, j, d) of samples b0 .. b1 - 1 as a bool numpy array [b1 - b0, N, N, L].
    one-bit layout: bit i & 31 of the hash word of the 32-bit counter ((b NI + i / 32) N + j) L + d, NI = ceil(N / 32);
    byte layout: byte i & 3 of the word of the 64-bit counter ((b NQ + i / 4) N + j) L + d, NQ = ceil(N / 4), whose high half
    perturbs the key; keep iff byte >= p8"""
    b1 = B if b1 is None else b1
    p8, _ = drop_cfg(p)
    if p8 == 0:
        return np.ones((b1 - b0, N, N, L), dtype=bool)
    u = np.uint64
    key = u(drop_key(seed))
    b = np.arange(b0, b1, dtype=np.uint64)[:, None, None, None]
    j = np.arange(N, dtype=np.uint64)[None, None, :, None]
    d = np.arange(L, dtype=np.uint64)[None, None, None, :]
    i = np.arange(N)
    if bit_layout:
        assert p8 == 128
        NI = _ceil(N, 32)
        assert B * NI * N * L < 2 ** 32
        iw = np.arange(NI, dtype=np.uint64)[None, :, None, None]
        words = _hash32((((b * u(NI) + iw) * u(N) + j) * u(L) + d) ^ key)                 # [b, NI, j, d]
        return ((words[:, i // 32] >> (i % 32).astype(np.uint64)[None, :, None, None]) & u(1)).astype(bool)
    NQ = _ceil(N, 4)
    iq = np.arange(NQ, dtype=np.uint64)[None, :, None, None]
    cnt = ((b * u(NQ) + iq) * u(N) + j) * u(L) + d
    key2 = key ^ (((cnt >> u(32)) * u(0x85EBCA6B)) & u(M32))
    words = _hash32((cnt & u(M32)) ^ key2)                                                 # [b, NQ, j, d]
    return ((words[:, i // 4] >> (u(8) * (i % 4).astype(np.uint64))[None, :, None, None]) & u(255)) >= u(p8)


def bit_layout_of(p, knobs=()):
    """oda_bits_mode at sizes below 2^32 counters: p8 == 128 and VQA_K2_BYTE_MASK not set"""
    return drop_cfg(p)[0] == 128 and "VQA_K2_BYTE_MASK" not in dict(knobs)


def test_host_hash_known_answers():
    """the host restatement against values worked out by hand from the definitions: lowbias32(0) = 0 (every step maps 0 to 0);
    lowbias32 is a bijection (no two of 2^16 consecutive counters share a word); the key folds the seed's high half in"""
    assert int(_hash32(np.array([0], dtype=np.uint64))[0]) == 0
    x = 1
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    assert int(_hash32(np.array([1], dtype=np.uint64))[0]) == x
    assert len(np.unique(_hash32(np.arange(1 << 16, dtype=np.uint64)))) == 1 << 16
    assert drop_key(5) == 5 and drop_key((1 << 32) + 5) == 5 ^ 0x9E3779B9 and drop_key(-1) == drop_key(M64)
    assert drop_cfg(0.5) == (128, 2.0) and drop_cfg(0.75) == (192, 4.0) and drop_cfg(0.0) == (0, 1.0)
    assert drop_cfg(0.25)[0] == 64 and drop_cfg(0.999)[0] == 255 and drop_cfg(0.001)[0] == 0


def test_host_mask_layouts():
    """the two layouts of host_keep against a scalar loop over (b, i, j, d) at a small shape; the keep rate of both is near 1 - p"""
    B, N, L, seed = 2, 37, 5, (7 << 32) + 11
    key = drop_key(seed)

    def word(c):
        return int(_hash32(np.array([(c & M32) ^ key ^ (((c >> 32) * 0x85EBCA6B) & M32)], dtype=np.uint64))[0])

    bits, byte = host_keep(0.5, seed, B, N, L, True), host_keep(0.25, seed, B, N, L, False)
    for b, i, j, d in ((0, 0, 0, 0), (1, 31, 36, 4), (1, 32, 0, 3), (0, 36, 35, 1), (1, 5, 7, 2)):
        assert bool(bits[b, i, j, d]) == bool((word(((b * 2 + i // 32) * N + j) * L + d) >> (i & 31)) & 1)
        assert bool(byte[b, i, j, d]) == (((word(((b * 10 + i // 4) * N + j) * L + d) >> (8 * (i & 3))) & 255) >= 64)
    assert abs(bits.mean() - 0.5) < 0.02 and abs(byte.mean() - 0.75) < 0.02
    assert host_keep(0.0, seed, B, N, L, False).all()
    assert np.array_equal(host_keep(0.5, seed, B, N, L, True, 1, 2), bits[1:2])


def run_mask(ops, p, seed, seed_word, B, N, L):
    buf = _out(B * N * N * L)
    rc, log = _call(ops, ops._lib.lib().vqa_object_difference_dropout_mask, _ptr(buf, PAD), p, seed, _ptr(seed_word), B, N, L)
    assert rc == 0 and log == [(MASK_K, _ceil(N * L, 256) * N * B * 256)], (rc, log)
    return _win(buf, (B, N, N, L), "mask").cpu()


def host_mask_f32(p, seed, B, N, L, bit_layout):
    return torch.from_numpy(host_keep(p, seed, B, N, L, bit_layout).astype(np.float32) * np.float32(drop_cfg(p)[1]))


# (N, L): N on both sides of every word (32) and quad (4) boundary, L no multiple of 64
MASK_SHAPES = [(1, 70), (31, 70), (32, 33), (33, 70), (36, 310), (65, 70), (128, 33)]


@gpu
@pytest.mark.parametrize("N,L", MASK_SHAPES)
def test_exported_mask_is_the_host_mask(ops, lib_option, N, L):
    """one-bit layout (p = 0.5) and byte layout (p = 0.25, 0.75, and 0.5 under VQA_K2_BYTE_MASK=1), B = 2 and 3"""
    for B, p, knob, seed in ((2, 0.5, False, 12345), (3, 0.25, False, (9 << 32) + 1), (2, 0.75, False, 3), (2, 0.5, True, 12345)):
        lib_option("VQA_K2_BYTE_MASK", 1 if knob else None)
        got = run_mask(ops, p, seed, None, B, N, L)
        want = host_mask_f32(p, seed, B, N, L, p == 0.5 and not knob)
        assert _same_bits(got, want), (N, L, B, p, knob, int((got != want).sum()))
    lib_option("VQA_K2_BYTE_MASK", None)
    assert bool((run_mask(ops, 0.0, 1, None, 2, N, L) == 1.0).all())


def seed_word(value):
    """a DEVICE uint64 holding `value`"""
    v = int(value) & M64
    return torch.tensor([v - (1 << 64) if v >> 63 else v], dtype=torch.int64, device=dev())


@gpu
def test_exported_mask_with_a_device_seed_word(ops, lib_option):
    """seed_ptr holding s1 with salt s2 draws the mask of host seed s1 + s2: a carry out of the low 32 bits, and one out of bit 63"""
    B, N, L = 2, 33, 70
    for s1, s2 in ((0x12FFFFFFFF, 1), (0x7FFFFFFF80000001, 0x800000007FFFFFFF), (M64, 2)):
        for p, knob in ((0.5, False), (0.25, False), (0.5, True)):
            lib_option("VQA_K2_BYTE_MASK", 1 if knob else None)
            word = seed_word(s1)
            got = run_mask(ops, p, s2, word, B, N, L)
            want = host_mask_f32(p, (s1 + s2) & M64, B, N, L, p == 0.5 and not knob)
            assert _same_bits(got, want), (hex(s1), hex(s2), p, knob)
            assert _same_bits(got, run_mask(ops, p, (s1 + s2) & M64, None, B, N, L))
            assert not _same_bits(got, run_mask(ops, p, s1, None, B, N, L)), "the salt was ignored"


# ======================================================================================================================= A
def keep_factor(p):
    p8, _ = drop_cfg(p)
    assert 256 % (256 - p8) == 0, "p = %g has no integer keep factor" % p
    return 256 // (256 - p8)


def bounds(B, N, L, G, s, av, aq, aw, ab, ad):
    """the largest sum of absolute values of the terms of an element of (logits, d_w, d_vl, d_ql, d_bias): a kept difference is at
    most 2 av aq, u = sum_g dS w at most G ad aw, dT[n] has 2 N terms u (N over j, N over i)"""
    u = G * ad * aw
    return (N * L * aw * s * 2 * av * aq + ab, B * N * ad * s * 2 * av * aq, 2 * N * u * s * aq, N * 2 * N * u * av * s, B * N * ad)


def amplitude(B, N, L, G, s, backward):
    """3, or the largest amplitude below it that keeps every sum of the case under 2^24"""
    for a in (3, 2, 1):
        bs = bounds(B, N, L, G, s, a, a, a, a, a)
        if max(bs if backward else bs[:1]) < 2 ** 24:
            return a
    raise AssertionError("no amplitude keeps this shape exact")


@functools.lru_cache(maxsize=4)
def operands(B, N, L, G, amp, nonneg):
    """int64 on the CPU: vl [B,N,L] (within [0, amp] if nonneg), ql [B,L], w [G,N L], bias [G], d_logits [B,N,G] within +-amp"""
    gen = torch.Generator().manual_seed(1000003 * B + 10007 * N + 101 * L + 7 * G + amp + 50 * nonneg)
    r = lambda lo, *shape: torch.randint(lo, amp + 1, shape, generator=gen)      # noqa: E731
    return r(0 if nonneg else -amp, B, N, L), r(-amp, B, L), r(-amp, G, N * L), r(-amp, G), r(-amp, B, N, G)


def reference(host, p, seed, bit_layout, gate, backward):
    """int64, chunked over b -> (logits, d_vl, d_ql, d_w, d_bias) (the gradients None without `backward`)"""
    vl, ql, w, bias, dS = host
    B, N, L = vl.shape
    G = w.shape[0]
    s = keep_factor(p)
    bs = bounds(B, N, L, G, s, _amax(vl), _amax(ql), _amax(w), _amax(bias), _amax(dS))
    _below_2_24(*(bs if backward else bs[:1]))
    logits = torch.empty(B, N, G, dtype=torch.int64)
    d_vl, d_ql, d_w = (torch.empty(B, N, L, dtype=torch.int64), torch.empty(B, L, dtype=torch.int64),
                       torch.zeros(G, N * L, dtype=torch.int64)) if backward else (None, None, None)
    chunk = max(1, (1 << 22) // (N * N * L))
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        keep = torch.from_numpy(host_keep(p, seed, B, N, L, bit_layout, b0, b1)).long()
        T = vl[b0:b1] * ql[b0:b1, None, :]
        X = (keep * (T[:, :, None, :] - T[:, None, :, :])).reshape((b1 - b0) * N, N * L)
        logits[b0:b1] = (s * (X @ w.t()) + bias).view(b1 - b0, N, G)
        if backward:
            ds = dS[b0:b1].reshape((b1 - b0) * N, G)
            d_w += s * (ds.t() @ X)
            U = keep * (ds @ w).reshape(b1 - b0, N, N, L)
            dT = U.sum(2) - U.sum(1)
            dv = s * dT * ql[b0:b1, None, :]
            d_vl[b0:b1] = torch.where(vl[b0:b1] > 0, dv, torch.zeros_like(dv)) if gate else dv
            d_ql[b0:b1] = s * (dT * vl[b0:b1]).sum(1)
    return logits, d_vl, d_ql, d_w, (dS.sum((0, 1)) if backward else None)


def case_seed(name):
    """(seed, whether the call hands it over through the device word) -- fixed per case id"""
    c = zlib.crc32(name.encode())
    return ((c & 0xFF) << 32) + c, bool(c & 1)


def seed_args(seed, via_word):
    """-> (seed argument, seed_ptr argument, the tensor to keep alive)"""
    if not via_word:
        return seed, None, None
    word = seed_word(seed - SALT)
    return SALT, _ptr(word), word


def nt_of(L):
    return _ceil(min(L, 1024), 64) * 64


def fwd_grid(form, B, N, L):
    """work-items of the forward launch: MFMA forms one workgroup per sample with 1..4 or 8 waves (one per 16 features up to 4, 8
    from 8 sets on); the VALU forms (ceil(N / 18 or 12), B) workgroups of one lane per feature, at most 1024"""
    if form in FWD_MFMA_FORMS:
        nsets = _ceil(L, 16)
        return B * 64 * (8 if nsets >= 8 else min(nsets, 4))
    return _ceil(N, 18 if form == FWD_BITS else 12) * B * nt_of(L)


def mfma_groups(B):
    """(sample groups, samples per group) of the MFMA weight gradient: at most 256 groups"""
    spg = _ceil(B, min(B, 256))
    return _ceil(B, spg), spg


def bwd_log(data, weight, B, N, L, G):
    tail = [(REDUCE, _ceil(G * N * L, 64) * 256), (DBIAS, 1024)]
    nw = min(_ceil(L, 16), 4)
    if data in (FUSED_T, FUSED_F):
        return [(data, mfma_groups(B)[0] * 128 * nw)] + tail
    first = (data, _ceil(L, 64) * B * 64 * _ceil(N, 12) if data == D_SPLIT else B * nt_of(L))
    if weight in W_MFMA_FORMS:
        second = (weight, mfma_groups(B)[0] * 128 * nw * (2 if weight in (W_STAGED[True, 2], W_STAGED[False, 2]) else 1))
    else:
        second = (weight, _ceil(N, 12) * min(B, 128) * nt_of(L))        # (the VALU forms launch 128 groups from B = 128 on)
    return [first, second] + tail


def run_fwd(ops, dv, B, N, L, G, p, seed, via_word):
    """dv: the NaN-padded operand buffers on the GPU -> (rc, log, logits buffer)"""
    vl, ql, w, bias, _ = dv
    buf = _out(B * N * G)
    sa, sp, keepalive = seed_args(seed, via_word)
    rc, log = _call(ops, ops._lib.lib().vqa_object_difference_attention_fwd, _ptr(vl, PAD), _ptr(ql, PAD), _ptr(w, PAD), _ptr(bias, PAD),
                    _ptr(buf, PAD), p, sa, sp, B, N, L, G)
    return rc, log, buf


def run_bwd(ops, dv, B, N, L, G, p, seed, via_word, gate):
    """-> (rc, log, (d_vl, d_ql, d_w, d_bias)), every output taken whole out of its sentinel-filled buffer; the workspace is exactly as
    long as the library asks for, NaN-filled, and the sentinel behind it must survive"""
    vl, ql, w, _, dS = dv
    Lb = ops._lib.lib()
    nbytes = Lb.vqa_object_difference_attention_bwd_workspace_bytes(B, N, L, G)
    assert nbytes == max(min(B, 256), min(B, 128)) * G * N * L * 4
    ws = _sentinel(nbytes // 4 + PAD)
    ws[:nbytes // 4] = NAN
    outs = [_out(B * N * L), _out(B * L), _out(G * N * L), _out(G)]
    sa, sp, keepalive = seed_args(seed, via_word)
    rc, log = _call(ops, Lb.vqa_object_difference_attention_bwd, _ptr(vl, PAD), _ptr(ql, PAD), _ptr(w, PAD), _ptr(dS, PAD),
                    *(_ptr(o, PAD) for o in outs), _ptr(ws), nbytes, p, sa, sp, B, N, L, G, gate)
    if rc != 0:
        return rc, log, None
    assert _untouched(ws[nbytes // 4:]), "a store behind the workspace"
    shapes = [(B, N, L), (B, L), (G, N * L), (G,)]
    return rc, log, tuple(_win(o, sh, n) for o, sh, n in zip(outs, shapes, ("d_vl", "d_ql", "d_w", "d_bias")))


NO_MFMA, NO_PK, BYTE_KNOB = ("VQA_K2_MFMA", 0), ("VQA_K2_PK", 0), ("VQA_K2_BYTE_MASK", 1)

# (id, form, B, N, L, G, p, knobs)
FWD_CASES = []
# L = 1 .. 1024: 1, 1, 2, 3, 4, 4, 8, 8, 8 waves, the last feature set partial except at 16, 48, 112 and 1024
for _i, (_L, _N, _G) in enumerate(zip((1, 16, 17, 48, 49, 112, 113, 310, 1024), (1, 3, 4, 5, 33, 36, 34, 36, 36), (1, 2, 3, 4, 1, 2, 3, 4, 4))):
    FWD_CASES += [("mfma-false-L%d" % _L, FWD_MFMA_F, 3, _N, _L, _G, 0.0, ()), ("mfma-pk-L%d" % _L, FWD_MFMA_PK, 3, _N, _L, _G, 0.5, ()),
                  ("mfma-nopk-L%d" % _L, FWD_MFMA_T, 3, _N, _L, _G, 0.5, (NO_PK,))]
FWD_CASES += [
    # the one-bit VALU form: i0 = 18 with N = 33 .. 36 straddles two mask words; N = 37 is a third pass; NI = 2, 3 and 4
    ("bits-G5-N32", FWD_BITS, 3, 32, 70, 5, 0.5, ()), ("bits-G6-N33", FWD_BITS, 3, 33, 100, 6, 0.5, ()),
    ("bits-G7-N36", FWD_BITS, 3, 36, 70, 7, 0.5, ()), ("bits-G8-N37-L1024", FWD_BITS, 2, 37, 1024, 8, 0.5, ()),
    ("bits-G5-N64", FWD_BITS, 2, 64, 70, 5, 0.5, ()), ("bits-G6-N65", FWD_BITS, 2, 65, 70, 6, 0.5, ()),
    ("bits-G3-N65", FWD_BITS, 2, 65, 33, 3, 0.5, ()), ("bits-G8-N128", FWD_BITS, 2, 128, 70, 8, 0.5, ()),
    ("bits-N40-L1024", FWD_BITS, 2, 40, 1024, 8, 0.5, ()),
    ("bits-nomfma-G1", FWD_BITS, 3, 13, 70, 1, 0.5, (NO_MFMA,)), ("bits-nomfma-G2", FWD_BITS, 3, 36, 310, 2, 0.5, (NO_MFMA,)),
    ("bits-nomfma-G3", FWD_BITS, 3, 33, 49, 3, 0.5, (NO_MFMA,)), ("bits-nomfma-G4", FWD_BITS, 3, 5, 20, 4, 0.5, (NO_MFMA,)),
]
# the byte layout: p = 0.75 at every G (N no multiple of 12 or of 4 in most), p = 0.5 under the knob
FWD_CASES += [("byte-G%d-N%d" % (_G, _N), FWD_BYTE, 2, _N, _L, _G, 0.75, ())
              for _G, _N, _L in zip(range(1, 9), (1, 5, 13, 33, 37, 36, 65, 128), (70, 20, 70, 100, 100, 310, 33, 70))]
FWD_CASES += [("byte-knob-G2", FWD_BYTE, 3, 13, 70, 2, 0.5, (BYTE_KNOB,)), ("byte-knob-G4", FWD_BYTE, 3, 36, 310, 4, 0.5, (BYTE_KNOB,)),
              ("byte-knob-G6-L1024", FWD_BYTE, 2, 37, 1024, 6, 0.5, (BYTE_KNOB,))]
FWD_CASES += [("plain-G1-N37", FWD_PLAIN, 2, 37, 100, 1, 0.0, ()), ("plain-G2-N37", FWD_PLAIN, 2, 37, 70, 2, 0.0, ()),
              ("plain-G3-nomfma", FWD_PLAIN, 3, 13, 70, 3, 0.0, (NO_MFMA,)), ("plain-G4-nomfma", FWD_PLAIN, 3, 36, 310, 4, 0.0, (NO_MFMA,)),
              ("plain-G5", FWD_PLAIN, 3, 5, 20, 5, 0.0, ()), ("plain-G6", FWD_PLAIN, 2, 33, 49, 6, 0.0, ()),
              ("plain-G7-L1024", FWD_PLAIN, 2, 14, 1024, 7, 0.0, ()), ("plain-G8-N128", FWD_PLAIN, 2, 128, 33, 8, 0.0, ())]


@gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=lambda c: c[0])
def test_forward_small_integers_are_exact(ops, lib_option, case):
    name, form, B, N, L, G, p, knobs = case
    set_knobs(lib_option, knobs)
    seed, via_word = case_seed(name)
    host = operands(B, N, L, G, amplitude(B, N, L, G, keep_factor(p), False), False)
    ref = reference(host, p, seed, bit_layout_of(p, knobs), 0, False)[0]
    rc, log, buf = run_fwd(ops, [_in(t) for t in host], B, N, L, G, p, seed, via_word)
    assert rc == 0, (name, rc, ops._lib.lib().vqa_last_error())
    assert log == [(form, fwd_grid(form, B, N, L))], (name, log)
    assert_exact(name, _win(buf, (B, N, G), name), ref)


W_S1, W_S1F = W_STAGED[True, 1], W_STAGED[False, 1]
FUSED, HALVES, UNSTAGED, NO_SPLIT = ("VQA_K2_FUSED", 1), ("VQA_K2_WSTAGE", 2), ("VQA_K2_WSTAGE", 0), ("VQA_K2_DATA_SPLIT", 0)

# (id, data form (or the fused form), weight form, B, N, L, G, p, knobs, gates)
BWD_CASES = [
    ("full-p0.5", D_BITS, W_S1, 3, 36, 310, 4, 0.5, (), (0, 1)), ("full-p0", D_PLAIN, W_S1F, 3, 36, 310, 4, 0.0, (), (0, 1)),
    ("halves-p0.5", D_BITS, W_STAGED[True, 2], 3, 33, 100, 3, 0.5, (HALVES,), (0, 1)),
    ("halves-p0", D_PLAIN, W_STAGED[False, 2], 3, 33, 100, 3, 0.0, (HALVES,), (1,)),
    ("halves-p0.5-L310", D_BITS, W_STAGED[True, 2], 3, 36, 310, 4, 0.5, (HALVES,), (0,)),
    ("unstaged-p0.5", D_BITS, W_MFMA_PK, 3, 13, 70, 2, 0.5, (UNSTAGED,), (0, 1)),
    ("unstaged-p0", D_PLAIN, W_MFMA_F, 3, 13, 70, 2, 0.0, (UNSTAGED,), (0,)),
    ("nopk-p0.5", D_BITS, W_MFMA_T, 3, 5, 17, 1, 0.5, (NO_PK,), (0, 1)), ("nopk-p0.5-full", D_BITS, W_MFMA_T, 3, 36, 310, 4, 0.5, (NO_PK,), (1,)),
    ("nopk-p0", D_PLAIN, W_MFMA_F, 3, 34, 113, 3, 0.0, (NO_PK,), (0,)),
    # sample groups of the MFMA forms: 1 sample per group up to B = 256, then 2 (129 groups, the last short), 3 at B = 513 (171)
    ("groups-B255", D_BITS, W_S1, 255, 5, 20, 4, 0.5, (), (0,)), ("groups-B256", D_BITS, W_S1, 256, 5, 20, 3, 0.5, (), (1,)),
    ("groups-B257", D_BITS, W_S1, 257, 5, 20, 2, 0.5, (), (0,)), ("groups-B257-p0", D_PLAIN, W_S1F, 257, 5, 20, 4, 0.0, (), (1,)),
    ("groups-B513", D_SPLIT, W_S1, 513, 5, 20, 4, 0.5, (), (0, 1)), ("groups-B513-halves", D_SPLIT, W_STAGED[True, 2], 513, 5, 20, 1, 0.5, (HALVES,), (0,)),
    ("groups-B513-unstaged", D_SPLIT, W_MFMA_PK, 513, 5, 20, 4, 0.5, (UNSTAGED,), (1,)),
    # the split data gradient from B ceil(L / 64) = 512 on, with at most four chunks of 12 regions
    ("split-B512-L64", D_SPLIT, W_S1, 512, 5, 64, 2, 0.5, (), (0, 1)), ("nosplit-B511-L64", D_BITS, W_S1, 511, 5, 64, 2, 0.5, (), (0, 1)),
    ("split-B256-L65", D_SPLIT, W_S1, 256, 5, 65, 3, 0.5, (), (0, 1)), ("nosplit-knob", D_BITS, W_S1, 512, 5, 64, 2, 0.5, (NO_SPLIT,), (0, 1)),
    ("split-N48", D_SPLIT, W_BITS, 512, 48, 20, 2, 0.5, (), (1,)), ("nosplit-N49", D_BITS, W_BITS, 512, 49, 20, 2, 0.5, (), (1,)),
    # sample groups of the VALU forms: 1 sample per group up to B = 128, then 2
    ("valu-groups-B127", D_BITS, W_BITS, 127, 5, 20, 5, 0.5, (), (0,)), ("valu-groups-B128", D_BYTE, W_BYTE, 128, 5, 20, 6, 0.75, (), (1,)),
    ("valu-groups-B129-p0", D_PLAIN, W_PLAIN, 129, 5, 20, 7, 0.0, (), (0,)), ("valu-groups-B129", D_BITS, W_BITS, 129, 5, 20, 8, 0.5, (), (1,)),
    ("valu-groups-B129-nomfma", D_BITS, W_BITS, 129, 5, 20, 4, 0.5, (NO_MFMA,), (0,)),
    # d_bias on both sides of its 8 x 1024 row stride
    ("dbias-8191", D_SPLIT, W_BITS, 8191, 1, 3, 5, 0.5, (), (0,)), ("dbias-8192", D_SPLIT, W_S1, 4096, 2, 3, 3, 0.5, (), (1,)),
    ("dbias-8193", D_SPLIT, W_BITS, 2731, 3, 3, 7, 0.5, (), (0,)), ("dbias-8192-N1", D_BYTE, W_BYTE, 8192, 1, 2, 8, 0.75, (), (1,)),
    # just inside the 160 KB of the data gradient: (39 x 1024 + 51 x 8) x 4 = 161 376 bytes
    ("lds-p0.5", D_BITS, W_BITS, 2, 39, 1024, 8, 0.5, (), (0,)), ("lds-p0.75", D_BYTE, W_BYTE, 2, 39, 1024, 8, 0.75, (), (1,)),
    ("lds-p0", D_PLAIN, W_PLAIN, 2, 39, 1024, 8, 0.0, (), (0,)),
    ("N128-p0.5", D_BITS, W_BITS, 2, 128, 70, 8, 0.5, (), (0,)), ("N128-p0.75", D_BYTE, W_BYTE, 2, 128, 70, 8, 0.75, (), (1,)),
    ("N65-p0", D_PLAIN, W_PLAIN, 2, 65, 100, 3, 0.0, (), (1,)), ("byte-knob", D_BYTE, W_BYTE, 3, 36, 310, 4, 0.5, (BYTE_KNOB,), (0, 1)),
    ("fused-p0.5", FUSED_T, None, 3, 36, 310, 4, 0.5, (FUSED,), (0, 1)), ("fused-p0", FUSED_F, None, 3, 36, 310, 4, 0.0, (FUSED,), (0, 1)),
    ("fused-p0.5-B513-L17", FUSED_T, None, 513, 5, 17, 2, 0.5, (FUSED,), (0, 1)), ("fused-p0-B513-L17", FUSED_F, None, 513, 5, 17, 3, 0.0, (FUSED,), (0, 1)),
    ("fused-p0.5-N33", FUSED_T, None, 5, 33, 49, 1, 0.5, (FUSED,), (1,)),
]
# every G of every VALU family (VQA_K2_MFMA=0 for G <= 4), N = 13: neither a multiple of 12 nor of 4
for _G in range(1, 9):
    _k = (NO_MFMA,) if _G <= 4 else ()
    BWD_CASES += [("G%d-p0.5" % _G, D_BITS, W_BITS, 2, 13, 70, _G, 0.5, _k, (_G & 1,)), ("G%d-p0.75" % _G, D_BYTE, W_BYTE, 2, 13, 70, _G, 0.75, _k, (1 - (_G & 1),)),
                  ("G%d-p0" % _G, D_PLAIN, W_PLAIN, 2, 13, 70, _G, 0.0, _k, (_G & 1,)), ("G%d-p0.5-B512" % _G, D_SPLIT, W_BITS, 512, 5, 20, _G, 0.5, _k, (1 - (_G & 1),))]


def check_bwd(ops, name, data, weight, B, N, L, G, p, knobs, gate, seed, via_word):
    host = operands(B, N, L, G, amplitude(B, N, L, G, keep_factor(p), True), bool(gate))
    refs = reference(host, p, seed, bit_layout_of(p, knobs), gate, True)[1:]
    rc, log, got = run_bwd(ops, [_in(t) for t in host], B, N, L, G, p, seed, via_word, gate)
    what = "%s gate=%d" % (name, gate)
    assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
    assert log == bwd_log(data, weight, B, N, L, G), (what, log)
    for key, have, want in zip(("d_vl", "d_ql", "d_w", "d_bias"), got, refs):
        assert_exact("%s %s" % (what, key), have, want)
    return got


@gpu
@pytest.mark.parametrize("case", BWD_CASES, ids=lambda c: c[0])
def test_backward_small_integers_are_exact(ops, lib_option, case):
    name, data, weight, B, N, L, G, p, knobs, gates = case
    set_knobs(lib_option, knobs)
    seed, via_word = case_seed(name)
    for gate in gates:
        check_bwd(ops, name, data, weight, B, N, L, G, p, knobs, gate, seed, via_word != bool(gate))


def test_sample_group_arithmetic():
    """what the group cases above rely on: 1, 2 and 3 samples per group, and a short last group"""
    assert [mfma_groups(B) for B in (255, 256, 257, 513)] == [(255, 1), (256, 1), (129, 2), (171, 3)]
    assert 129 * 2 - 257 == 1 and 171 * 3 - 513 == 0 and 170 * 3 < 513
    assert bounds(2, 128, 70, 8, 4, 3, 3, 3, 3, 3)[3] >= 2 ** 24 and amplitude(2, 128, 70, 8, 4, True) == 2
    assert (39 * 1024 + 51 * 8) * 4 == 161376 <= 160 * 1024 < (40 * 1024 + 52 * 8) * 4


@gpu
def test_every_form_gives_the_same_bits(ops, lib_option):
    """one shape and seed through every form that can take it (one-bit layout): with exact sums the results are identical, and a
    second call of the same form gives the same bits again"""
    B, N, L, G, p, seed = 256, 13, 100, 3, 0.5, 0xABCDEF0123
    host = operands(B, N, L, G, 3, True)
    dv = [_in(t) for t in host]
    knob_names = ("VQA_K2_MFMA", "VQA_K2_PK", "VQA_K2_WSTAGE", "VQA_K2_DATA_SPLIT", "VQA_K2_FUSED")
    fwd, bwd = [], []
    for form, knobs in ((FWD_MFMA_PK, ()), (FWD_MFMA_PK, ()), (FWD_MFMA_T, (NO_PK,)), (FWD_BITS, (NO_MFMA,))):
        for k in knob_names:
            lib_option(k, None)
        set_knobs(lib_option, knobs)
        rc, log, buf = run_fwd(ops, dv, B, N, L, G, p, seed, len(fwd) == 1)
        assert rc == 0 and log == [(form, fwd_grid(form, B, N, L))], (rc, log)
        fwd.append(_win(buf, (B, N, G), form))
    for data, weight, knobs in ((D_SPLIT, W_S1, ()), (D_SPLIT, W_S1, ()), (D_BITS, W_S1, (NO_SPLIT,)), (D_SPLIT, W_STAGED[True, 2], (HALVES,)),
                                (D_SPLIT, W_MFMA_PK, (UNSTAGED,)), (D_SPLIT, W_MFMA_T, (NO_PK,)), (D_SPLIT, W_BITS, (NO_MFMA,)),
                                (FUSED_T, None, (FUSED,))):
        for k in knob_names:
            lib_option(k, None)
        set_knobs(lib_option, knobs)
        rc, log, got = run_bwd(ops, dv, B, N, L, G, p, seed, len(bwd) == 1, 1)
        assert rc == 0 and log == bwd_log(data, weight, B, N, L, G), (rc, log)
        bwd.append(got)
    assert float(fwd[0].abs().max()) > 0 and all(float(t.abs().max()) > 0 for t in bwd[0])
    for other in fwd[1:]:
        assert _same_bits(fwd[0] + 0.0, other + 0.0)
    for other in bwd[1:]:
        for a, b in zip(bwd[0], other):
            assert _same_bits(a + 0.0, b + 0.0)
    assert_exact("logits", fwd[0], reference(host, p, seed, True, 1, False)[0])


# ======================================================================================================================= B
def oda_f32(vl, ql, w, bias, mask, dS):
    """the formulas of oracle/kernels_np.py in float32 with torch on the CPU; mask [B,N,N,L]"""
    B, N, L = vl.shape
    diff = vl[:, :, None, :] - vl[:, None, :, :]
    vq = (diff * ql[:, None, None, :] * mask).reshape(B, N, N * L)
    logits = vq @ w.t() + bias
    dw = torch.einsum("big,bik->gk", dS, vq)
    dvq = (dS @ w).view(B, N, N, L) * mask
    dd = dvq * ql[:, None, None, :]
    return logits, dd.sum(2) - dd.sum(1), (dvq * diff).sum((1, 2)), dw, dS.sum((0, 1))


@gpu
@pytest.mark.parametrize("B,N,L,G", [(2, 13, 70, 2), (3, 36, 310, 4), (2, 37, 100, 8)])
def test_non_dyadic_rate_against_float64(ops, measured, B, N, L, G):
    """p = 0.25: the byte-mask forward, data and weight kernels with random operands"""
    import oracle.kernels_np as knp
    p, seed = 0.25, (3 << 32) + 1000 * N + G
    gen = torch.Generator().manual_seed(97 * N + G)
    vl, ql = torch.randn(B, N, L, generator=gen).clamp_min(0.0), torch.randn(B, L, generator=gen).abs()
    w, bias = torch.randn(G, N * L, generator=gen) / (N * L) ** 0.5, 0.1 * torch.randn(G, generator=gen)
    dS = torch.randn(B, N, G, generator=gen)
    mask = host_mask_f32(p, seed, B, N, L, False)
    assert set(torch.unique(mask).tolist()) == {0.0, float(np.float32(256.0) / np.float32(192.0))}
    dv = [_in(t) for t in (vl, ql, w, bias, dS)]
    rc, log, buf = run_fwd(ops, dv, B, N, L, G, p, seed, False)
    assert rc == 0 and log == [(FWD_BYTE, fwd_grid(FWD_BYTE, B, N, L))], (rc, log)
    rc, blog, got = run_bwd(ops, dv, B, N, L, G, p, seed, True, 0)
    assert rc == 0 and blog == bwd_log(D_BYTE, W_BYTE, B, N, L, G), (rc, blog)
    m64 = mask.double().numpy().reshape(B, N, N * L)
    ref64 = (knp.object_difference_logits_fwd(vl.numpy(), ql.numpy(), w.numpy(), bias.numpy(), m64),
             *knp.object_difference_logits_bwd(vl.numpy(), ql.numpy(), w.numpy(), dS.numpy(), m64))
    ref32 = oda_f32(vl, ql, w, bias, mask, dS)
    bars = Bars(measured, "B%d N%d L%d G%d" % (B, N, L, G))
    for name, have, r64, r32 in zip(("logits", "d_vl", "d_ql", "d_w", "d_bias"), (_win(buf, (B, N, G), "logits"),) + got, ref64, ref32):
        bars.check(name, have, torch.from_numpy(np.ascontiguousarray(r64)), r32)
    bars.close()


# ======================================================================================================================= C
# (id, forward form, data form, weight form, B, p, knobs) at N = 13, L = 70, G = 2
ISOLATION_CASES = [
    ("mfma-p0", FWD_MFMA_F, D_PLAIN, W_S1F, 4, 0.0, ()), ("mfma-p0.5", FWD_MFMA_PK, D_BITS, W_S1, 4, 0.5, ()),
    ("nopk", FWD_MFMA_T, D_BITS, W_MFMA_T, 4, 0.5, (NO_PK,)), ("bits", FWD_BITS, D_BITS, W_BITS, 4, 0.5, (NO_MFMA,)),
    ("byte", FWD_BYTE, D_BYTE, W_BYTE, 4, 0.75, ()), ("plain", FWD_PLAIN, D_PLAIN, W_PLAIN, 4, 0.0, (NO_MFMA,)),
    ("split", FWD_MFMA_PK, D_SPLIT, W_S1, 256, 0.5, ()), ("fused-p0.5", FWD_MFMA_PK, FUSED_T, None, 4, 0.5, (FUSED,)),
    ("fused-p0", FWD_MFMA_F, FUSED_F, None, 4, 0.0, (FUSED,)),
]


@gpu
@pytest.mark.parametrize("case", ISOLATION_CASES, ids=lambda c: c[0])
def test_a_nan_stays_in_its_sample(ops, lib_option, case):
    """a NaN in vl of sample 1: logits, d_vl and d_ql of every other sample are bit for bit those of the clean run (d_w and d_bias
    sum over the samples; what the NaN becomes inside sample 1 depends on the mask layout and is not asserted)"""
    name, f_form, data, weight, B, p, knobs = case
    N, L, G = 13, 70, 2
    set_knobs(lib_option, knobs)
    seed, via_word = case_seed("nan-" + name)
    host = operands(B, N, L, G, 3, False)
    runs = []
    for dirty in (False, True):
        vl = host[0].to(F32)
        if dirty:
            vl[1, 3, 7] = NAN
        buf = torch.full((vl.numel() + 2 * PAD,), NAN, dtype=F32)
        buf[PAD:-PAD] = vl.reshape(-1)
        dv = [buf.to(dev())] + [_in(t) for t in host[1:]]
        rc, log, out = run_fwd(ops, dv, B, N, L, G, p, seed, via_word)
        assert rc == 0 and log == [(f_form, fwd_grid(f_form, B, N, L))], (name, rc, log)
        rc, blog, got = run_bwd(ops, dv, B, N, L, G, p, seed, via_word, 0)
        assert rc == 0 and blog == bwd_log(data, weight, B, N, L, G), (name, rc, blog)
        runs.append((_win(out, (B, N, G), "logits"), got[0], got[1]))
    others = [b for b in range(B) if b != 1]
    for key, clean, dirt in zip(("logits", "d_vl", "d_ql"), *runs):
        assert bool(torch.isfinite(clean).all()), (name, key)
        assert _same_bits(clean[others], dirt[others]), "%s %s: the NaN of sample 1 reached another sample" % (name, key)
    assert bool(torch.isnan(runs[1][0][1]).any()), "the NaN did not reach its own sample's logits"


@gpu
def test_refusals_launch_nothing(ops):
    """null pointers, a size <= 0, p outside [0, 1), a workspace one byte short: VQA_E_BADARG; G = 9, N = 129, L = 1025, B = 65536 and
    the backward at N = 40, L = 1024 (165 504 bytes of LDS): VQA_E_UNSUPPORTED.  An error text, no launch, the outputs untouched.
    Every buffer is as large as the refused call would have needed"""
    Lb = ops._lib.lib()
    n = 1 << 20
    src = torch.zeros(n, device=dev())
    outs = [_sentinel(n) for _ in range(5)]
    buf = (ctypes.c_ulonglong * 16)()
    ws_of = Lb.vqa_object_difference_attention_bwd_workspace_bytes

    def refused(code, fn, *args):
        Lb.vqa_launch_log_reset()
        assert fn(*args, None) == code, (fn.__name__, args, Lb.vqa_last_error())
        assert Lb.vqa_last_error() and Lb.vqa_launch_log(buf, 16) == 0, "a refused call launched a kernel"

    def fwd(B=2, N=5, L=8, G=2, p=0.5, null=None):
        ptrs = [_ptr(src)] * 4 + [_ptr(outs[0])]
        if null is not None:
            ptrs[null] = None
        return (Lb.vqa_object_difference_attention_fwd, *ptrs, p, 7, None, B, N, L, G)

    def bwd(B=2, N=5, L=8, G=2, p=0.5, null=None, short=0):
        ptrs = [_ptr(src)] * 4 + [_ptr(o) for o in outs]
        if null is not None:
            ptrs[null] = None
        need = ws_of(B, N, L, G)
        assert need <= 4 * n and max(B * N * L, G * N * L, 1) <= n
        return (Lb.vqa_object_difference_attention_bwd, *ptrs, (need or 4 * n) - short, p, 7, None, B, N, L, G, 0)

    def msk(B=2, N=5, L=8, p=0.5, null=False):
        assert B * N * N * L <= n
        return (Lb.vqa_object_difference_dropout_mask, None if null else _ptr(outs[0]), p, 7, None, B, N, L)

    for i in range(5):
        refused(E_BADARG, *fwd(null=i))
    for i in range(9):
        refused(E_BADARG, *bwd(null=i))
    refused(E_BADARG, *msk(null=True))
    for kw in (dict(B=0), dict(N=0), dict(L=-1), dict(p=-0.25), dict(p=1.0), dict(p=1.5)):
        refused(E_BADARG, *fwd(**kw))
        refused(E_BADARG, *bwd(**kw))
        refused(E_BADARG, *msk(**kw))
    refused(E_BADARG, *fwd(G=0))
    refused(E_BADARG, *bwd(G=0))
    refused(E_BADARG, *bwd(short=1))
    assert ws_of(0, 5, 8, 2) == 0 and ws_of(2, 5, 8, 0) == 0 and ws_of(2, 5, 8, 2) == 2 * 2 * 40 * 4
    for kw in (dict(G=9), dict(B=1, N=129), dict(B=1, L=1025), dict(B=65536, N=1, L=1, G=1)):
        refused(E_UNSUPPORTED, *fwd(**kw))
        refused(E_UNSUPPORTED, *bwd(**kw))
        if "G" not in kw or kw.get("B") == 65536:
            refused(E_UNSUPPORTED, *msk(**{k: v for k, v in kw.items() if k != "G"}))
    for p in (0.0, 0.5, 0.75):
        refused(E_UNSUPPORTED, *bwd(B=2, N=40, L=1024, G=8, p=p))
    assert b"LDS" in Lb.vqa_last_error()
    torch.cuda.synchronize()
    for t in outs:
        assert _untouched(t)


# ======================================================================================================================= D
def declared_forms():
    """every kernel expression a case above names (and asserts from the launch log)"""
    forms = {s for table in (FWD_CASES, BWD_CASES, ISOLATION_CASES) for case in table for s in case if isinstance(s, str) and "_kernel" in s}
    return forms | {MASK_K, REDUCE, DBIAS}      # test_exported_mask_*; the last two launches of every backward case (bwd_log)


def test_every_launch_site_is_declared():
    """a launch site added to (or renamed in) the file without a case here fails; so does a case whose form no longer exists.  The
    site inside the VQA_K2_STAGED macro counts through its four expansions, each of which the source must spell out"""
    path = os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc", "object_difference.hip")
    sites = launch_sites(path)
    assert len(sites) == 24, sites
    assert sites.count(STAGED_SITE) == 1
    text = re.sub(r"\s+", "", open(path).read())
    expansions = {W_STAGED[m, jh] for m in (True, False) for jh in (1, 2)
                  if "VQA_K2_STAGED(%s,%d)" % ("true" if m else "false", jh) in text}
    assert len(expansions) == 4
    sites = (set(sites) - {STAGED_SITE}) | expansions
    declared = declared_forms()
    assert sites - declared == set(), "launch sites that no case declares"
    assert declared - sites == set(), "declared forms that no launch site has"
