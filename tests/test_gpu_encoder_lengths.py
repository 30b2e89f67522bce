"""The length-aware question encoder on the GPU (include/vqa_mi355x.h and INTEGRATION.md section 2 state the contract):

  1  vqa_gemm_nt_split_batched_len / vqa_gru_gemm_bf16_len: row tiles that hold an active row carry the unmasked entry point's
     bits, row tiles without one are not written (the sentinel survives); tile heights from the _tile_rows queries
  2  vqa_gru_gates_{fwd,bwd}[_bf16]_len with NaN wherever an inactive row may not read: finite outputs that follow the state
     rule exactly, active rows bit for bit the unmasked kernels'
  3  BayesianGRU(length_aware=True): output and every gradient torch.equal to the default path's (derivable: an active row runs
     the same instructions on the same operands, the inactive steps' gradients are exact zeros either way), return_last=False
     against the CPU branch in float64, and what is launched
  4  cor2.Model(encoder_length_aware=True): logits and gradients torch.equal to the model without the switch; a replayed
     training step reads the counts of the batch it is given

Every operand is seeded and built on the CPU."""
import pytest
import torch

from kernel_harness import (BF, E_BADARG, F32, NAN, SENT, _bits, _call, _ptr, _same_bits, _sentinel, _untouched, dev, ops,
                            spy_launches)  # noqa: F401  (ops: the fixture)
from vqa_playground_pytorch_amd.encoder import BayesianGRU

pytestmark = pytest.mark.gpu
RTOL_MID = 2e-2            # tests/test_gpu_encoder_bf16.py: a bf16 intermediate, of the tensor's scale


# ---- 1. the products ---------------------------------------------------------------------------------------------------------
GEMM_T, GEMM_t = 6, 3
PATTERNS = ["sorted", "shuffled", "all_T", "all_1", "one_long"]


def _lens(pattern, M, gen):
    if pattern == "all_T":
        return torch.full((M,), GEMM_T, dtype=torch.int32)
    if pattern == "all_1":
        return torch.ones(M, dtype=torch.int32)
    if pattern == "one_long":                      # one unfinished row inside an otherwise finished tile (the last one)
        lens = torch.ones(M, dtype=torch.int32)
        lens[M - 5] = GEMM_T
        return lens
    lens = torch.randint(1, GEMM_T + 1, (M,), generator=gen, dtype=torch.int32)
    lens[:8] = GEMM_T                              # (the head of the batch is unfinished, its tail finished, when sorted)
    lens[-60:] = torch.randint(1, GEMM_t + 1, (60,), generator=gen, dtype=torch.int32)
    return lens.sort(descending=True).values if pattern == "sorted" else lens[torch.randperm(M, generator=gen)]


def _expected(ref, lens, BM):
    """ref [G,M,N] where a row's tile holds a row with lens > t, the sentinel elsewhere; -> (expected, number of skipped tiles)"""
    want, skipped = ref.clone(), 0
    for m0 in range(0, ref.shape[1], BM):
        if not bool((lens[m0:m0 + BM] > GEMM_t).any()):
            want[:, m0:m0 + BM] = SENT
            skipped += 1
    return want, skipped


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("NK", [64, 168])
@pytest.mark.parametrize("M", [64, 160, 304])
def test_split_gemm_len_skips_the_finished_row_tiles(ops, M, NK, pattern):
    G, N, K = 3, NK, NK
    L = ops._lib.lib()
    gen = torch.Generator().manual_seed(1000 * M + NK)
    a = torch.randn(G, M, K, generator=gen).to(dev())
    w = (torch.randn(G, N, K, generator=gen) / K ** 0.5).to(dev())
    lens = _lens(pattern, M, gen)
    lens_d = lens.to(dev())
    img = ops.split_weights(w)
    common = (_ptr(a), M * K, K, _ptr(img))
    tail = (M * N, N, None, 0, _ptr(w), w.stride(0), w.stride(1), 1, G, M, N, K)
    ref = _sentinel(G, M, N)
    rc, log0 = _call(ops, L.vqa_gemm_nt_split_batched, *common, _ptr(ref), *tail)
    assert rc == 0 and len(log0) == 1 and not bool((ref == SENT).any())
    got = _sentinel(G, M, N)
    rc, log = _call(ops, L.vqa_gemm_nt_split_batched_len, *common, _ptr(got), *tail, _ptr(lens_d), GEMM_t)
    assert rc == 0
    BM = L.vqa_gemm_nt_split_batched_tile_rows(G, M, N)
    assert BM in (112, 128, 144)
    want, skipped = _expected(ref, lens, BM)
    assert _same_bits(got, want), "%d of %d elements differ" % (int((_bits(got) != _bits(want)).sum()), got.numel())
    # the `_len` instantiation, with the unmasked launch's grid
    assert len(log) == 1 and log[0][1] == log0[0][1] and log[0][0] == log0[0][0].replace(">)", ",true>)"), (log, log0)
    if pattern == "all_T":
        assert skipped == 0 and _same_bits(got, ref)
    if pattern == "all_1":
        assert _untouched(got)
    if pattern == "one_long":
        assert skipped == -(-M // BM) - 1
    if pattern == "sorted" and M > BM:                # (the batch's tail of 60 finished rows covers the last tile)
        assert skipped >= 1, (M, BM, skipped)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("NK", [64, 168])
@pytest.mark.parametrize("M", [64, 160, 304])
def test_bf16_gemm_len_skips_the_finished_row_tiles(ops, M, NK, pattern):
    G, N, K = 3, NK, NK
    Kp = ops.pad_to(K)
    L = ops._lib.lib()
    gen = torch.Generator().manual_seed(2000 * M + NK)
    a = torch.zeros(G, M, Kp, dtype=BF)
    a[:, :, :K] = torch.randn(G, M, K, generator=gen).to(BF)
    w = torch.zeros(G, N, Kp, dtype=BF)
    w[:, :, :K] = (torch.randn(G, N, K, generator=gen) / K ** 0.5).to(BF)
    a, w = a.to(dev()), w.to(dev())
    lens = _lens(pattern, M, gen)
    lens_d = lens.to(dev())
    args = (_ptr(a), M * Kp, Kp, _ptr(w), N * Kp, Kp)
    tail = (M * N, N, G, M, N, K)
    ref = _sentinel(G, M, N)
    rc, log0 = _call(ops, L.vqa_gru_gemm_bf16, *args, _ptr(ref), *tail)
    assert rc == 0 and len(log0) == 1 and not bool((ref == SENT).any())
    got = _sentinel(G, M, N)
    rc, log = _call(ops, L.vqa_gru_gemm_bf16_len, *args, _ptr(got), *tail, _ptr(lens_d), GEMM_t)
    assert rc == 0
    BM = L.vqa_gru_gemm_bf16_tile_rows(M)
    assert BM == (64 if M <= 64 else 128)
    want, skipped = _expected(ref, lens, BM)
    assert _same_bits(got, want), "%d of %d elements differ" % (int((_bits(got) != _bits(want)).sum()), got.numel())
    assert len(log) == 1 and log[0][1] == log0[0][1] and log[0][0] == log0[0][0].replace(">)", ",true>)"), (log, log0)
    if pattern == "all_T":
        assert skipped == 0 and _same_bits(got, ref)
    if pattern == "all_1":
        assert _untouched(got)
    if pattern == "one_long":
        assert skipped == -(-M // BM) - 1
    if pattern == "sorted" and M > BM:
        assert skipped >= 1, (M, BM, skipped)


def test_len_entry_points_refuse_a_null_lens_before_any_launch(ops):
    L = ops._lib.lib()
    B, T, H, G = 64, 4, 64, 3
    f = torch.zeros(3 * B * T * H, device=dev())
    h = torch.zeros(3 * B * H, device=dev(), dtype=BF)
    p, q = _ptr(f), _ptr(h)
    calls = [
        (L.vqa_gemm_nt_split_batched_len, (p, B * H, H, p, p, B * H, H, None, 0, None, 0, 0, 0, G, B, H, H, None, 1)),
        (L.vqa_gru_gemm_bf16_len, (q, B * H, H, q, H * H, H, p, B * H, H, G, B, H, H, None, 1)),
        (L.vqa_gru_gates_fwd_len, (p, p, p, None, p, p, B * H, p, p, p, p, None, B, T, H, 1, 3)),
        (L.vqa_gru_gates_bwd_len, (p, p, p, None, p, p, p, p, p, p, B * H, p, p, None, B, T, H, 1, 3)),
        (L.vqa_gru_gates_fwd_bf16_len, (p, p, p, None, p, q, B * H, H, p, p, p, p, None, B, T, H, 1, 3)),
        (L.vqa_gru_gates_bwd_bf16_len, (p, p, p, None, p, p, p, p, p, q, B * H, H, p, p, None, B, T, H, 1, 3)),
    ]
    for fn, args in calls:
        rc, log = _call(ops, fn, *args)
        assert rc == E_BADARG and log == [], (fn.__name__, rc, log)


# ---- 2. the gate kernels -----------------------------------------------------------------------------------------------------
GT = 4


def _gate_case(B, H, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
    c = {"gi": r(3, B, GT, H), "a": r(3, B, H), "h_prev": 0.5 * r(B, H), "masks": (torch.rand(3, B, H, generator=gen) > 0.25).float() / 0.75,
         "saved": torch.stack([torch.sigmoid(r(B, H)), torch.sigmoid(r(B, H)), torch.tanh(r(B, H)), r(B, H)]),
         "d_out": r(B, H), "carry_in": r(B, H), "dhm": r(3, B, H)}
    c["lens"] = torch.tensor([(7 * b + 3) % GT + 1 for b in range(B)], dtype=torch.int32)         # 4, 3, 2, 1, 4, ...
    return c


def _len_instance(log, log0):
    """the `_len` entry (log) launched the LEN = true instantiation of the kernel whose LEN = false instantiation the plain entry
    (log0) launched, on the same grid"""
    plain = log0[0][0]
    return plain.endswith(",false>)") and log[0][0] == plain[:-len(",false>)")] + ",true>)" and log[0][1] == log0[0][1]


def _gates_fwd(ops, c, bf, t, af, a, lens):
    L = ops._lib.lib()
    B, H = c["h_prev"].shape
    ld = ops.pad_to(H) if bf else H
    d = {k: c[k].to(dev()) for k in ("gi", "h_prev", "masks")}
    a = a.to(dev())
    h_new, saved = _sentinel(B, H), _sentinel(4, B, H)
    hm = _sentinel(3, B, ld, dtype=BF if bf else F32)
    lens_d = lens.to(dev()) if lens is not None else None
    fn = getattr(L, "vqa_gru_gates_fwd" + ("_bf16" if bf else "") + ("_len" if lens is not None else ""))
    args = [_ptr(d["gi"]), _ptr(a), _ptr(d["h_prev"]), _ptr(d["masks"]), _ptr(h_new), _ptr(hm), B * ld] + ([ld] if bf else []) + \
           [_ptr(saved[k]) for k in range(4)] + ([_ptr(lens_d)] if lens is not None else []) + [B, GT, H, t, af]
    rc, log = _call(ops, fn, *args)
    assert rc == 0 and len(log) == 1, (rc, log)
    return h_new, hm, saved, log


@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [16, 168])
@pytest.mark.parametrize("B", [5, 160])
def test_gates_fwd_len_with_poisoned_inactive_rows(ops, B, H, bf, af):
    c = _gate_case(B, H, 31 * B + H)
    for t in range(GT):
        active = c["lens"] > t
        poisoned = c["a"].clone()
        poisoned[:, ~active] = NAN
        h_new, hm, saved, log = _gates_fwd(ops, c, bf, t, af, poisoned, c["lens"])
        ref_h, ref_hm, ref_saved, log0 = _gates_fwd(ops, c, bf, t, af, c["a"], None)
        # the LEN instantiation against the plain one of the same kernel, with the same grid
        assert _len_instance(log, log0), (log, log0)
        act = active.to(dev())
        for name, got, ref in (("h_new", h_new, ref_h), ("hm_next", hm[:, :, :H].transpose(0, 1), ref_hm[:, :, :H].transpose(0, 1)),
                               ("saved", saved.transpose(0, 1), ref_saved.transpose(0, 1))):
            assert _same_bits(got[act], ref[act]), "t=%d: %s of the active rows" % (t, name)
        assert bool(torch.isfinite(h_new).all()) and bool(torch.isfinite(hm[:, :, :H].float()).all())
        hp, m = c["h_prev"].to(dev()), c["masks"].to(dev())
        assert _same_bits(h_new[~act], hp[~act]), "t=%d: an inactive row's state moved" % t
        want_hm = (hp[None] * m).to(hm.dtype)
        assert _same_bits(hm[:, :, :H][:, ~act], want_hm[:, ~act]), "t=%d: hm_next of the inactive rows" % t
        assert _untouched(saved[:, ~act]), "t=%d: saved tensors of an inactive row were written" % t
        assert _untouched(hm[:, :, H:]), "t=%d: a store into the history's row pads" % t


def _gates_bwd(ops, c, bf, t, af, dhm, saved, lens):
    L = ops._lib.lib()
    B, H = c["h_prev"].shape
    ld = ops.pad_to(H) if bf else H
    last = t == GT - 1                                  # the last step has no carry and no dhm yet: null pointers, as ops passes them
    d = {k: c[k].to(dev()) for k in ("d_out", "carry_in", "masks", "h_prev")}
    dhm, saved = dhm.to(dev()), saved.to(dev())
    gz = _sentinel(3, B, ld, dtype=BF if bf else F32)
    d_gi, carry_out = _sentinel(3, B, GT, H), _sentinel(B, H)
    lens_d = lens.to(dev()) if lens is not None else None
    fn = getattr(L, "vqa_gru_gates_bwd" + ("_bf16" if bf else "") + ("_len" if lens is not None else ""))
    args = [_ptr(d["d_out"]), None if last else _ptr(d["carry_in"]), None if last else _ptr(dhm), _ptr(d["masks"])] + \
           [_ptr(saved[k]) for k in range(4)] + [_ptr(d["h_prev"]), _ptr(gz), B * ld] + ([ld] if bf else []) + [_ptr(d_gi), _ptr(carry_out)] + \
           ([_ptr(lens_d)] if lens is not None else []) + [B, GT, H, t, af]
    rc, log = _call(ops, fn, *args)
    assert rc == 0 and len(log) == 1, (rc, log)
    return gz, d_gi, carry_out, log


@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [16, 168])
@pytest.mark.parametrize("B", [5, 160])
def test_gates_bwd_len_with_poisoned_inactive_rows(ops, B, H, bf, af):
    c = _gate_case(B, H, 37 * B + H)
    for t in range(GT):
        active, active_next = c["lens"] > t, c["lens"] > t + 1
        dhm, saved = c["dhm"].clone(), c["saved"].clone()
        dhm[:, ~active_next] = NAN                     # a row inactive at t + 1 never reads dhm[b]
        saved[:, ~active] = NAN
        gz, d_gi, carry_out, log = _gates_bwd(ops, c, bf, t, af, dhm, saved, c["lens"])
        # the unmasked twin on clean operands: dhm[b] = 0 where the `_len` kernel leaves it out (x + 0 = x bit for bit, x != -0)
        dhm0 = c["dhm"].clone()
        dhm0[:, ~active_next] = 0.0
        ref_gz, ref_gi, ref_co, log0 = _gates_bwd(ops, c, bf, t, af, dhm0, c["saved"], None)
        # the LEN instantiation against the plain one of the same kernel, with the same grid
        assert _len_instance(log, log0), (log, log0)
        act = active.to(dev())
        for name, got, ref in (("gz", gz[:, :, :H].transpose(0, 1), ref_gz[:, :, :H].transpose(0, 1)),
                               ("d_gi", d_gi[:, :, t].transpose(0, 1), ref_gi[:, :, t].transpose(0, 1)), ("carry_out", carry_out, ref_co)):
            assert _same_bits(got[act], ref[act]), "t=%d: %s of the active rows" % (t, name)
            assert bool(torch.isfinite(got.float()).all()), "t=%d: %s is not finite" % (t, name)
        zero = torch.zeros(1, device=dev())
        assert bool((_bits(gz[:, :, :H][:, ~act]) == 0).all()), "t=%d: gz of an inactive row is not +0" % t
        assert bool((_bits(d_gi[:, :, t][:, ~act]) == _bits(zero)).all()), "t=%d: d_gi of an inactive row is not +0" % t
        want_co = c["d_out"].to(dev()) if t == GT - 1 else c["d_out"].to(dev()) + c["carry_in"].to(dev())
        assert _same_bits(carry_out[~act], want_co[~act]), "t=%d: carry_out of the inactive rows" % t
        other = [s for s in range(GT) if s != t]
        assert _untouched(d_gi[:, :, other]) and _untouched(gz[:, :, H:]), "t=%d: a store outside slot t / into the row pads" % t


@pytest.mark.parametrize("af", [1, 3], ids=["relu", "tanh"])
@pytest.mark.parametrize("bf", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("H", [16, 168])
@pytest.mark.parametrize("B", [5, 160])
def test_gates_len_with_every_row_active_equal_the_plain_entries(ops, B, H, bf, af):
    """the two instantiations of csrc/gru.hip's kernel pair share their arithmetic: with lens = T for every row, at every t, every
    output buffer of a `_len` entry is the plain entry's bit for bit, on all rows (sentinels outside the written slots included)"""
    c = _gate_case(B, H, 41 * B + H)
    full = torch.full((B,), GT, dtype=torch.int32)
    for t in range(GT):
        got = _gates_fwd(ops, c, bf, t, af, c["a"], full)
        ref = _gates_fwd(ops, c, bf, t, af, c["a"], None)
        assert _len_instance(got[3], ref[3]), (got[3], ref[3])
        for name, x, y in zip(("h_new", "hm_next", "saved"), got, ref):
            assert _same_bits(x, y), "forward t=%d: %s" % (t, name)
        got = _gates_bwd(ops, c, bf, t, af, c["dhm"], c["saved"], full)
        ref = _gates_bwd(ops, c, bf, t, af, c["dhm"], c["saved"], None)
        assert _len_instance(got[3], ref[3]), (got[3], ref[3])
        for name, x, y in zip(("gz", "d_gi", "carry_out"), got, ref):
            assert _same_bits(x, y), "backward t=%d: %s" % (t, name)


# ---- 3. BayesianGRU ----------------------------------------------------------------------------------------------------------
RENAME = {n: n + "_len" for n in ("gru_gates_fwd", "gru_gates_bwd", "gru_gates_fwd_bf16", "gru_gates_bwd_bf16", "gemm_nt_split_batched",
                                  "gru_gemm_bf16")}
GRU_SHAPES = [(160, 5, 12, 64), (160, 5, 12, 168), (5, 7, 12, 16)]


def _lengths(B, T, gen):
    """descending from T (the head of the batch) to 1, so the last row tile finishes early; one all-PAD row (0 -> runs T steps)"""
    n = torch.randint(1, T + 1, (B,), generator=gen).sort(descending=True).values
    n[0], n[-1] = T, 1
    if B > 64:
        n[-64:] = n[-64:].clamp(max=2)
    n[1] = 0
    return n


def _gru_pair(B, T, K, H, dtype, train, return_last=True, seed=3):
    torch.manual_seed(seed)
    off = BayesianGRU(K, H, dropout=0.25, af="tanh", compute_dtype=dtype, return_last=return_last)
    on = BayesianGRU(K, H, dropout=0.25, af="tanh", compute_dtype=dtype, return_last=return_last, length_aware=True)
    on.load_state_dict(off.state_dict())
    gen = torch.Generator().manual_seed(11)
    masks = [(torch.rand(B, 1, K, generator=gen) > 0.25).float() / 0.75 for _ in range(3)] + \
            [(torch.rand(B, H, generator=gen) > 0.25).float() / 0.75 for _ in range(3)]
    return off, on, masks, gen


def _inject(m, masks, device, train, dtype=F32):
    m.train(train)
    queue = [t.to(device=device, dtype=dtype) for t in masks]
    m._mask = (lambda like, q=queue: q.pop(0)) if train else (lambda like: None)


def _run(m, x, lengths, gy, device):
    xd = x.clone().to(device).requires_grad_()
    y = m(xd, lengths.to(device))
    y.backward(gy.to(device))
    return y.detach(), xd.grad, {n: p.grad.clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("dtype", [None, "bf16"], ids=["f32", "bf16"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("shape", GRU_SHAPES, ids=lambda s: "B%dT%dK%dH%d" % s)
def test_bayesian_gru_length_aware_equals_the_default_path(ops, monkeypatch, shape, train, dtype):
    B, T, K, H = shape
    off, on, masks, gen = _gru_pair(B, T, K, H, dtype, train)
    x, gy, lengths = torch.randn(B, T, K, generator=gen), torch.randn(B, H, generator=gen), _lengths(B, T, gen)
    seen = {}
    for name, m in (("off", off), ("on", on)):
        m.to(dev())
        _inject(m, masks, dev(), train)
        with monkeypatch.context() as mp:
            log = spy_launches(mp, ops)
            seen[name] = (_run(m, x, lengths, gy, dev()), list(log))
    (y0, gx0, gp0), log0 = seen["off"]
    (y1, gx1, gp1), log1 = seen["on"]
    assert torch.equal(y0, y1), "output"
    assert torch.equal(gx0, gx1), "input gradient"
    differ = [n for n in gp0 if not torch.equal(gp0[n], gp1[n])]
    assert not differ, differ
    assert all(bool(torch.isfinite(g).all()) for g in gp1.values()) and bool(torch.isfinite(on.all_hiddens).all())
    L = torch.where((lengths >= 1) & (lengths <= T), lengths, torch.full_like(lengths, T))
    idx = (L - 1).to(dev())
    held = on.all_hiddens[torch.arange(B, device=dev()), idx]                       # [B,H]: the last valid state
    past = (torch.arange(T)[None, :] >= L[:, None]).to(dev())                       # [B,T]
    assert torch.equal(on.all_hiddens[past], held[:, None, :].expand(B, T, H)[past]), "all_hiddens past the questions' ends"
    assert torch.equal(on.all_hiddens[~past], off.all_hiddens[~past]), "all_hiddens over the valid steps"
    # what was launched: the default's list with the gate and product launches replaced by their `_len` twins, nothing else
    assert not [n for n, _ in log0 if n.endswith("_len")], log0
    assert log1 == [(RENAME.get(n, n), s) for n, s in log0], (log0, log1)
    names1 = [n for n, _ in log1]
    sfx = "_bf16" if dtype else ""
    assert names1.count("gru_gates_fwd%s_len" % sfx) == T and names1.count("gru_gates_bwd%s_len" % sfx) == T and not set(names1) & set(RENAME)
    product = "gru_gemm_bf16_len" if dtype else "gemm_nt_split_batched_len"
    assert names1.count(product) == (2 * (T - 1) if (dtype or B >= 64) else 0), names1


@pytest.mark.parametrize("dtype", [None, "bf16"], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", GRU_SHAPES, ids=lambda s: "B%dT%dK%dH%d" % s)
def test_bayesian_gru_length_aware_all_steps_against_the_cpu_branch(ops, measured, shape, dtype):
    """return_last=False, training with injected masks: the [B,T,H] output (the last valid state past each end) and every gradient
    (d_out reaches the inactive steps here: the carry passes through them) against the torch-op branch in float64 -- fp32 at the
    bars of test_gpu_gru_sequence_matches_the_torch_path (1e-5; 1e-5 / 2e-5 of scale), bf16 at tests/test_gpu_encoder_bf16.py's
    2e-2 of scale."""
    B, T, K, H = shape
    _, gpu, masks, gen = _gru_pair(B, T, K, H, dtype, True, return_last=False)
    _, cpu, _, _ = _gru_pair(B, T, K, H, dtype, True, return_last=False)
    cpu.double()
    x, gy, lengths = torch.randn(B, T, K, generator=gen), torch.randn(B, T, H, generator=gen), _lengths(B, T, gen)
    _inject(cpu, masks, "cpu", True, torch.float64)
    yc, gxc, gpc = _run(cpu, x.double(), lengths, gy.double(), "cpu")
    gpu.to(dev())
    _inject(gpu, masks, dev(), True)
    yg, gxg, gpg = _run(gpu, x, lengths, gy, dev())
    tag = "B%dT%dH%d %s" % (B, T, H, dtype or "f32")
    if dtype is None:
        err = float((yg.cpu().double() - yc).abs().max())
        measured("%s out abs err" % tag, err, 1e-5)
        assert err <= 1e-5, err
        bars = {"x": 1e-5 * max(1.0, float(gxc.abs().max()))}
        bars.update({n: 2e-5 * max(float(g.abs().max()), 1e-6) for n, g in gpc.items()})
    else:
        err = float((yg.cpu().double() - yc).abs().max()) / float(yc.abs().max())
        measured("%s out err / scale" % tag, err, RTOL_MID)
        assert err <= RTOL_MID, err
        bars = {"x": RTOL_MID * float(gxc.abs().max())}
        bars.update({n: RTOL_MID * float(g.abs().max()) for n, g in gpc.items()})
    for n, got, ref in [("x", gxg, gxc)] + [(n, gpg[n], gpc[n]) for n in gpc]:
        e = float((got.cpu().double() - ref).abs().max())
        measured("%s d %s err" % (tag, n), e, bars[n])
        assert e <= bars[n], (n, e, bars[n])


# ---- 4. the model ------------------------------------------------------------------------------------------------------------
MB, MT, ANSWERS = 64, 6, 20
VOCAB = ["PAD"] + ["w%d" % i for i in range(MB * MT)]


def _model(length_aware, encoder_dtype=None):
    from vqa_playground_pytorch_amd import cor2
    torch.manual_seed(17)
    return cor2.Model(VOCAB, ANSWERS, seq2vec="skipthoughts", encoder_length_aware=length_aware, encoder_dtype=encoder_dtype).to(dev())


def _batch(seed, longest):
    """left-aligned token ids, 0 = PAD, lengths 1..longest and one all-PAD question; no word twice in the batch (the embedding's
    weight gradient adds the rows of a repeated word with atomics, in arrival order)"""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(MB, 36, 2048, generator=gen).abs()
    q = (1 + torch.randperm(len(VOCAB) - 1, generator=gen))[:MB * MT].view(MB, MT)
    n = torch.randint(1, longest + 1, (MB,), generator=gen)
    n[0], n[1], n[2] = longest, 1, 0
    q = q * (torch.arange(MT)[None, :] < n[:, None])
    a = torch.softmax(2.0 * torch.randn(MB, ANSWERS, generator=gen), dim=1)
    return {"v": v.to(dev()), "q_idxes": q.to(dev())}, a.to(dev())


@pytest.mark.parametrize("encoder_dtype", [None, "bf16"], ids=["f32", "bf16"])
@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
def test_cor2_with_the_length_aware_encoder_equals_the_model_without(train, encoder_dtype):
    from vqa_playground_pytorch_amd.trainer import kld_sum_loss
    sample, a = _batch(19, MT)
    out = []
    for length_aware in (False, True):
        model = _model(length_aware, encoder_dtype).train(train)
        assert model.seq2vec.length_aware is length_aware
        torch.manual_seed(23)                            # (the dropout seeds and the encoder's masks)
        logits = model(sample)
        kld_sum_loss(logits, a).backward()
        out.append((logits.detach(), {n: p.grad for n, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(out[0][0], out[1][0]), "logits"
    assert set(out[0][1]) == set(out[1][1])
    differ = [n for n in out[0][1] if not torch.equal(out[0][1][n], out[1][1][n])]
    assert not differ, differ


def test_replayed_step_reads_the_lengths_of_every_batch():
    """DataParallelTrainer, graph path, eval mode (no dropout: both sides deterministic): captured on a batch of SHORT questions, then
    replayed on long ones -- stale counts would freeze their states early.  Losses follow the kernel-by-kernel trainer fed the same
    batches (the bars of tests/test_gpu_region_counts.py::test_captured_step_reads_the_counts_of_every_batch)."""
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    warm = DataParallelTrainer.EAGER_STEPS_BEFORE_CAPTURE
    short, long_ = _batch(29, 2), _batch(31, MT)
    steps = [short] * (warm + 1) + [long_, short, long_]
    losses = {}
    for graph in (False, True):
        model = _model(True).eval()
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=graph)
        losses[graph] = [tuple(x.item() for x in tr.step(sample, a)) for sample, a in steps]
        if graph:
            assert tr._graph is not None, "the step was not captured"
    for (l0, n0), (l1, n1) in zip(losses[False], losses[True]):
        assert abs(l0 - l1) <= 1e-4 * abs(l0) and abs(n0 - n1) <= 1e-4 * max(abs(n0), 1e-6), (losses[False], losses[True])
    assert abs(losses[True][warm + 1][0] - losses[True][warm][0]) > 1e-3 * abs(losses[True][warm][0])      # (the batches do differ)
