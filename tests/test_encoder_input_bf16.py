"""The question encoder's opt-in mixed-precision INPUT side on the CPU (no GPU needed): the keyword and the environment switch, the
checkpoint surface, the built library's symbols, and BayesianGRU's torch-op branch against a float64 emulation of the arithmetic
contract written here (csrc/encoder_input_bf16.hip / INTEGRATION.md section 2 state it): xb_g = bf(x * mx_g), Wb_g = bf(W_ig),
gi_g = xb_g Wb_g^T + b_g, dgb = bf(d_gi) for the two products of the backward, d_b from the unrounded d_gi, straight-through
roundings.  The recurrent side's switch (compute_dtype) is independent: both of its values are run.

The bar for a result that passes through a bf16 intermediate is the project's 2e-2 of the tensor's scale (RTOL_MID of
tests/test_gpu_bf16.py, the bar of tests/test_encoder_bf16.py for the recurrent side)."""
import ctypes

import pytest
import torch

from vqa_playground_pytorch_amd import _lib, cor2, oda
from vqa_playground_pytorch_amd.encoder import BayesianGRU, SkipThoughts

RTOL_MID = 2e-2
BF = torch.bfloat16
VOCAB = ["PAD", "UNK"] + ["w%d" % i for i in range(38)]
ACCEPTED = [(None, torch.float32), (torch.float32, torch.float32), (BF, BF), ("bf16", BF), ("bfloat16", BF)]
REFUSED = ["fp16", "f32", torch.float16, torch.float64, 16, "BF16"]
NEW_SYMBOLS = ("vqa_embed_pack_bf16", "vqa_gemm_bf16_nt_f32_bias", "vqa_embed_grad")


# ---- the float64 emulation of the contract ----------------------------------------------------------------------------------------
def bf(x):
    return x.to(torch.float32).to(BF).to(torch.float64)


def same(x):
    return x


def emulate_sequence(gi, w, masks, af, d_out, rnd):
    """The recurrent part, forward and backward written out (tests/test_encoder_bf16.py): rnd = bf for compute_dtype=bfloat16."""
    _, B, T, H = gi.shape
    m = masks if masks is not None else torch.ones(3, B, H, dtype=torch.float64)
    wb = rnd(w)
    h = torch.zeros(B, H, dtype=torch.float64)
    hs, hms, rs, is_, ns, ans, pres = [], [], [], [], [], [], []
    for t in range(T):
        hm = rnd(h[None] * m) if t else torch.zeros(3, B, H, dtype=torch.float64)
        a = torch.einsum("gbk,gnk->gbn", hm, wb)
        r = torch.sigmoid(gi[0, :, t] + a[0])
        i = torch.sigmoid(gi[1, :, t] + a[1])
        pre = gi[2, :, t] + r * a[2]
        n = torch.relu(pre) if af == "relu" else torch.tanh(pre)
        hs.append(h)
        h = (1 - i) * n + i * h
        for lst, v in ((hms, hm), (rs, r), (is_, i), (ns, n), (ans, a[2]), (pres, pre)):
            lst.append(v)
    out = torch.stack(hs[1:] + [h])
    d_gi, d_w = torch.zeros_like(gi), torch.zeros_like(w)
    carry, dhm = torch.zeros(B, H, dtype=torch.float64), None
    for t in range(T - 1, -1, -1):
        dh = d_out[t] + carry
        if dhm is not None:
            dh = dh + (dhm * m).sum(0)
        r, i, n, an = rs[t], is_[t], ns[t], ans[t]
        dn = dh * (1 - i) * ((n > 0).double() if af == "relu" else 1 - n * n)
        dzr, dzi = dn * an * r * (1 - r), dh * (hs[t] - n) * i * (1 - i)
        d_gi[0, :, t], d_gi[1, :, t], d_gi[2, :, t] = dzr, dzi, dn
        gzb = rnd(torch.stack([dzr, dzi, dn * r]))
        d_w += torch.einsum("gbn,gbk->gnk", gzb, hms[t])
        dhm = torch.einsum("gbn,gnk->gbk", gzb, wb)
        carry = dh * i
    return out, d_gi, d_w, float(torch.stack(pres).abs().min())


def emulate_module(state, x, lengths, gy, in_masks, hid_masks, af, rnd_in, rnd_rec):
    """BayesianGRU.forward(x, lengths) and its backward for grad_output gy in float64 -> {'y', 'd_x', 'd_<parameter>'}, min |pre|.
    rnd_in = bf: the input side's contract, every rounding a line below; rnd_rec = bf: the recurrent side's."""
    d = {k: v.double() for k, v in state.items()}
    B, T, K = x.shape
    x = x.double()
    names = ("r", "i", "n")
    mx = [in_masks[g].double() if in_masks is not None else torch.ones(B, 1, K, dtype=torch.float64) for g in range(3)]
    xb = [rnd_in(x * mx[g]) for g in range(3)]                                            # xb_g = bf(e * mx_g)
    wb = [rnd_in(d["gru_cell.weight_i%s.weight" % c]) for c in names]                     # Wb_g = bf(W_ig)
    gi = torch.stack([xb[g] @ wb[g].t() + d["gru_cell.weight_i%s.bias" % names[g]] for g in range(3)])
    w = torch.stack([d["gru_cell.weight_h%s.weight" % c] for c in names])
    masks = torch.stack([hm.double() for hm in hid_masks]) if hid_masks is not None else None
    idx = (lengths.long() - 1) % T
    d_out = torch.zeros(T, B, w.shape[1], dtype=torch.float64)
    d_out[idx, torch.arange(B)] = gy.double()
    out, d_gi, d_w, min_pre = emulate_sequence(gi, w, masks, af, d_out, rnd_rec)
    res = {"y": out[idx, torch.arange(B)], "d_x": torch.zeros_like(x)}
    dgb = rnd_in(d_gi)                                                                    # dgb = bf(d_gi)
    for g, c in enumerate(names):
        res["d_gru_cell.weight_h%s.weight" % c] = d_w[g]
        res["d_gru_cell.weight_i%s.weight" % c] = torch.einsum("btn,btk->nk", dgb[g], xb[g])
        res["d_gru_cell.weight_i%s.bias" % c] = d_gi[g].sum((0, 1))                       # the UNROUNDED d_gi
        res["d_x"] += (dgb[g] @ wb[g]) * mx[g]
    return res, min_pre


# ---- keyword, environment, checkpoints, the built library -------------------------------------------------------------------------
@pytest.mark.parametrize("value,want", ACCEPTED, ids=[str(v) for v, _ in ACCEPTED])
def test_input_dtype_and_encoder_input_dtype_accept_the_five_spellings(value, want, monkeypatch):
    monkeypatch.delenv("VQA_ENCODER_INPUT_DTYPE", raising=False)
    monkeypatch.delenv("VQA_ENCODER_DTYPE", raising=False)
    gru = BayesianGRU(12, 16, input_dtype=value)
    assert gru.input_dtype == want and gru.compute_dtype == torch.float32          # a switch of its own
    enc = SkipThoughts(VOCAB, input_dtype=value)
    assert enc.input_dtype == want and enc.gru.input_dtype == want and enc.compute_dtype == torch.float32
    for M in (cor2.Model, oda.Model):
        model = M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype=value)
        assert model.seq2vec.gru.input_dtype == want and model.seq2vec.gru.compute_dtype == torch.float32
        both = M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype=value, encoder_dtype=BF)
        assert both.seq2vec.input_dtype == want and both.seq2vec.compute_dtype == BF


def test_the_default_is_the_fp32_input_side():
    assert BayesianGRU(12, 16).input_dtype == torch.float32 and SkipThoughts(VOCAB).input_dtype == torch.float32
    assert BayesianGRU(12, 16, compute_dtype=BF).input_dtype == torch.float32      # compute_dtype=bf16 still leaves the input side fp32


@pytest.mark.parametrize("value", REFUSED, ids=[str(v) for v in REFUSED])
def test_anything_else_is_a_value_error(value):
    for build in (lambda: BayesianGRU(12, 16, input_dtype=value), lambda: SkipThoughts(VOCAB, input_dtype=value)):
        with pytest.raises(ValueError, match="input_dtype must be None, torch.float32 or torch.bfloat16"):
            build()
    for M in (cor2.Model, oda.Model):
        with pytest.raises(ValueError, match="encoder_input_dtype must be None, torch.float32 or torch.bfloat16"):
            M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype=value)


@pytest.mark.parametrize("M", [cor2.Model, oda.Model], ids=["cor2", "oda"])
def test_encoder_input_dtype_next_to_a_module_or_the_vector_slot_is_refused(M):
    for seq2vec in ("vector", None, SkipThoughts(VOCAB)):
        with pytest.raises(ValueError, match="encoder_input_dtype"):
            M(VOCAB, 20, seq2vec=seq2vec, encoder_input_dtype=BF)
        M(VOCAB, 20, seq2vec=seq2vec)


@pytest.mark.parametrize("M", [cor2.Model, oda.Model], ids=["cor2", "oda"])
def test_the_environment_switch_is_read_where_the_encoder_is_built(M, monkeypatch):
    monkeypatch.delenv("VQA_ENCODER_INPUT_DTYPE", raising=False)
    monkeypatch.delenv("VQA_ENCODER_DTYPE", raising=False)
    assert M(VOCAB, 20, seq2vec="skipthoughts").seq2vec.input_dtype == torch.float32
    monkeypatch.setenv("VQA_ENCODER_INPUT_DTYPE", "bf16")
    enc = M(VOCAB, 20, seq2vec="skipthoughts").seq2vec
    assert enc.input_dtype == BF and enc.compute_dtype == torch.float32               # the other switch is not moved by it
    assert M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype=torch.float32).seq2vec.input_dtype == torch.float32   # the keyword wins
    M(VOCAB, 20, seq2vec="vector")                                                    # not an error: no encoder is built
    monkeypatch.setenv("VQA_ENCODER_INPUT_DTYPE", "f32")
    assert M(VOCAB, 20, seq2vec="skipthoughts").seq2vec.input_dtype == torch.float32
    assert M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype="bf16").seq2vec.input_dtype == BF                      # ... both ways
    monkeypatch.setenv("VQA_ENCODER_INPUT_DTYPE", "fp8")
    with pytest.raises(ValueError, match="VQA_ENCODER_INPUT_DTYPE"):
        M(VOCAB, 20, seq2vec="skipthoughts")
    monkeypatch.setenv("VQA_ENCODER_INPUT_DTYPE", "f32")
    monkeypatch.setenv("VQA_ENCODER_DTYPE", "bf16")
    enc = M(VOCAB, 20, seq2vec="skipthoughts").seq2vec
    assert enc.input_dtype == torch.float32 and enc.compute_dtype == BF


def test_state_dict_keys_are_the_same_with_the_mode_on_and_off():
    torch.manual_seed(3)
    off, on = SkipThoughts(VOCAB), SkipThoughts(VOCAB, input_dtype=BF, compute_dtype=BF)
    assert list(off.state_dict()) == list(on.state_dict())
    assert [n for n, _ in off.named_parameters()] == [n for n, _ in on.named_parameters()]
    assert [n for n, _ in on.named_buffers()] == []
    assert all(p.dtype == torch.float32 for p in on.parameters())                     # the masters stay fp32
    assert [[tuple(p.shape) for p in g] for g in off.gru.stack_groups()] == [[tuple(p.shape) for p in g] for g in on.gru.stack_groups()]
    on.load_state_dict(off.state_dict())
    q = torch.randint(1, len(VOCAB), (2, 4))
    on.eval()(q)                                                                      # a forward leaves no shadow behind in the module
    assert list(on.state_dict()) == list(off.state_dict()) and not list(on.named_buffers())
    for M in (cor2.Model, oda.Model):
        a = M(VOCAB, 20, seq2vec="skipthoughts")
        b = M(VOCAB, 20, seq2vec="skipthoughts", encoder_input_dtype=BF)
        assert list(a.state_dict()) == list(b.state_dict())


def test_the_built_library_exports_the_new_entry_points_under_abi_14():
    assert _lib.ABI_VERSION == 14
    handle = ctypes.CDLL(_lib.LIB_PATH)                       # the file `python __graft_entry__.py build` left beside the package
    for name in NEW_SYMBOLS:
        assert hasattr(handle, name), name
        assert name in _lib.SIGNATURES
    L = _lib.lib()
    assert L.vqa_version() == 14
    header = open(__import__("os").path.join(__import__("os").path.dirname(_lib._HERE), "include", "vqa_mi355x.h")).read()
    assert "#define VQA_ABI_VERSION 14" in header and all(name + "(" in header for name in NEW_SYMBOLS)


# ---- the CPU branch against the emulation ------------------------------------------------------------------------------------------
def _case(af, train):
    B, T, K, H = 5, 7, 12, 16
    torch.manual_seed(11)
    ref = BayesianGRU(K, H, dropout=0.25, af=af)
    gen = torch.Generator().manual_seed(31 + (af == "relu") + 2 * train)
    if af == "relu":
        # no relu decision on a knife edge (tests/test_encoder_bf16.py): |gi_n| >= 0.5 minus a small input term, a small
        # recurrent term; the test asserts min |pre| >= 0.05 on the emulation
        with torch.no_grad():
            c = ref.gru_cell
            sign = torch.where(torch.rand(H, generator=gen) < 0.5, -1.0, 1.0)
            c.weight_in.bias.copy_(sign * (0.5 + torch.randn(H, generator=gen).abs()))
            c.weight_in.weight.copy_(0.1 * torch.randn(H, K, generator=gen) / K ** 0.5)
            c.weight_hn.weight.copy_(0.1 * torch.randn(H, H, generator=gen) / H ** 0.5)
    x = torch.randn(B, T, K, generator=gen)
    lengths = torch.tensor([7, 1, 4, 6, 3])
    gy = torch.randn(B, H, generator=gen)
    masks = None
    if train:
        masks = [(torch.rand(B, 1, K, generator=gen) > 0.25).float() / 0.75 for _ in range(3)] + \
                [(torch.rand(B, H, generator=gen) > 0.25).float() / 0.75 for _ in range(3)]
    return ref, x, lengths, gy, masks


def _run_module(ref, x, lengths, gy, masks, af, train, **dtypes):
    m = BayesianGRU(ref.input_size, ref.hidden_size, dropout=0.25, af=af, **dtypes)
    m.load_state_dict(ref.state_dict())
    m.train(train)
    if train:
        queue = list(masks)
        m._mask = lambda like: queue.pop(0)
    xg = x.clone().requires_grad_()
    y = m(xg, lengths)
    y.backward(gy)
    res = {"y": y.detach(), "d_x": xg.grad}
    res.update({"d_" + n: p.grad for n, p in m.named_parameters()})
    return res


@pytest.mark.parametrize("compute_dtype", [None, BF], ids=["rec-f32", "rec-bf16"])
@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("af", ["relu", "tanh"])
def test_cpu_branch_honours_the_contract(af, train, compute_dtype):
    ref, x, lengths, gy, masks = _case(af, train)
    in_m, hid_m = (masks[:3], masks[3:]) if train else (None, None)
    rnd_rec = bf if compute_dtype == BF else same
    want, min_pre = emulate_module(ref.state_dict(), x, lengths, gy, in_m, hid_m, af, bf, rnd_rec)
    if af == "relu":
        assert min_pre >= 0.05, min_pre
    got = _run_module(ref, x, lengths, gy, masks, af, train, input_dtype=BF, compute_dtype=compute_dtype)
    off = _run_module(ref, x, lengths, gy, masks, af, train, compute_dtype=compute_dtype)
    off_again = _run_module(ref, x, lengths, gy, masks, af, train, compute_dtype=compute_dtype, input_dtype=None)
    assert set(got) == set(want) == set(off) and len(want) == 2 + 9
    differs = 0
    for k in want:
        err = float((got[k].double() - want[k]).abs().max()) / float(want[k].abs().max())
        print("[%s %s %s] %-34s bf16 input branch vs emulation %.3e" % (af, "train" if train else "eval", compute_dtype, k, err))
        assert err <= RTOL_MID, (k, err)
        assert torch.equal(off[k], off_again[k]), k           # input_dtype=None is not passing the keyword
        differs += int(not torch.equal(got[k], off[k]))
    assert not torch.equal(got["y"], off["y"]), "the bf16 input mode returned the fp32 input side's result"
    assert differs >= 9, differs


def test_token_ids_with_a_table_are_a_gpu_path_only():
    gru = BayesianGRU(12, 16, input_dtype=BF)
    with pytest.raises(ValueError, match="token ids with a table"):
        gru(torch.zeros(2, 3, dtype=torch.long), torch.tensor([3, 3]), table=torch.zeros(5, 12))
