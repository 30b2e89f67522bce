"""The length-aware question encoder on the CPU: the spellings of the switch, the torch-op branch of BayesianGRU under the contract
of INTEGRATION.md section 2 (a row past its question's end keeps its state), the golden of the reference's encoder with the switch
on, and the feed's question-length sort.  No GPU, no kernel launch."""
import os

import numpy as np
import pytest
import torch

import config.CoR2
import config.ODA
from oracle import seeded
from vqa_playground_pytorch_amd import _lib, cor2, feed, oda
from vqa_playground_pytorch_amd.encoder import BayesianGRU, SkipThoughts, encoder_length_aware_from

VOCAB = ["w%d" % i for i in range(9)]
IDX = [[3, 1, 4, 1, 5, 2], [2, 7, 0, 0, 0, 0], [8, 0, 0, 0, 0, 0], [1, 2, 3, 4, 0, 0]]          # tests/test_encoder.py's questions


# ---- the switch --------------------------------------------------------------------------------------------------------------
def test_switch_spellings_and_precedence(monkeypatch):
    monkeypatch.delenv("VQA_ENCODER_LENGTHS", raising=False)
    assert BayesianGRU(8, 16).length_aware is False and BayesianGRU(8, 16, length_aware=True).length_aware is True
    assert SkipThoughts(VOCAB).length_aware is False
    on = SkipThoughts(VOCAB, length_aware=True)
    assert on.length_aware is True and on.gru.length_aware is True
    assert encoder_length_aware_from(None) is False
    for impl in (cor2, oda):
        assert impl.Model(VOCAB, 10, seq2vec="skipthoughts").seq2vec.length_aware is False
        assert impl.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=True).seq2vec.length_aware is True
    monkeypatch.setenv("VQA_ENCODER_LENGTHS", "1")                      # read where the encoder is built
    assert encoder_length_aware_from(None) is True
    for impl in (cor2, oda):
        assert impl.Model(VOCAB, 10, seq2vec="skipthoughts").seq2vec.length_aware is True
        assert impl.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=False).seq2vec.length_aware is False   # the keyword wins
    assert SkipThoughts(VOCAB).length_aware is False                    # (the module itself takes the keyword only)
    monkeypatch.setenv("VQA_ENCODER_LENGTHS", "0")
    assert cor2.Model(VOCAB, 10, seq2vec="skipthoughts").seq2vec.length_aware is False
    assert cor2.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=True).seq2vec.length_aware is True


@pytest.mark.parametrize("bad", ["yes", "2", "", "true"])
def test_a_bad_environment_value_is_a_value_error(monkeypatch, bad):
    monkeypatch.setenv("VQA_ENCODER_LENGTHS", bad)
    with pytest.raises(ValueError, match="VQA_ENCODER_LENGTHS must be 0 or 1"):
        cor2.Model(VOCAB, 10, seq2vec="skipthoughts")
    assert cor2.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=True).seq2vec.length_aware is True    # not read then
    assert cor2.Model(VOCAB, 10, seq2vec="vector") is not None         # no encoder is built: not read


def test_the_keyword_is_checked(monkeypatch):
    monkeypatch.delenv("VQA_ENCODER_LENGTHS", raising=False)
    with pytest.raises(ValueError, match="encoder_length_aware must be None, True or False"):
        cor2.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=1)
    with pytest.raises(ValueError, match="encoder_length_aware configures the SkipThoughts encoder"):
        oda.Model(VOCAB, 10, seq2vec="vector", encoder_length_aware=True)


@pytest.mark.parametrize("cf", [config.CoR2, config.ODA])
def test_config_modules_forward_the_keyword(monkeypatch, cf):
    monkeypatch.delenv("VQA_ENCODER_LENGTHS", raising=False)
    assert cf.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=True).seq2vec.length_aware is True
    assert cf.Model(VOCAB, 10, seq2vec="skipthoughts").seq2vec.length_aware is False
    on = cf.Model(VOCAB, 10, seq2vec="skipthoughts", encoder_length_aware=True, encoder_dtype="bf16", encoder_input_dtype="bf16")
    assert (on.seq2vec.length_aware, on.seq2vec.compute_dtype, on.seq2vec.input_dtype) == (True, torch.bfloat16, torch.bfloat16)


def test_the_library_has_the_entry_points():
    names = ["vqa_gemm_nt_split_batched_len", "vqa_gemm_nt_split_batched_tile_rows", "vqa_gru_gemm_bf16_len", "vqa_gru_gemm_bf16_tile_rows",
             "vqa_gru_gates_fwd_len", "vqa_gru_gates_bwd_len", "vqa_gru_gates_fwd_bf16_len", "vqa_gru_gates_bwd_bf16_len"]
    L = _lib.lib()
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    for n in names[4:] + [names[0], names[2]]:
        assert "lens" in _lib.PARAMS[n] and _lib.PARAMS[n][-1] == "stream", n
        twin = n.replace("_len", "")
        assert [p for p in _lib.PARAMS[n] if p != "lens" and not (p == "t" and "gemm" in n)] == _lib.PARAMS[twin], n
    # the tile heights the launches pick (host-side queries: no GPU): the cost model of csrc/gru_gemm.hip at the training shape
    assert L.vqa_gemm_nt_split_batched_tile_rows(3, 512, 2400) == 112 and L.vqa_gemm_nt_split_batched_tile_rows(3, 4096, 2400) == 144
    assert (L.vqa_gru_gemm_bf16_tile_rows(64), L.vqa_gru_gemm_bf16_tile_rows(65)) == (64, 128)
    assert _lib.ABI_VERSION == 14


# ---- the torch-op branch -----------------------------------------------------------------------------------------------------
def _pair(K, H, af, dtype, in_dtype, return_last=True):
    torch.manual_seed(3)
    off = BayesianGRU(K, H, dropout=0.25, af=af, compute_dtype=dtype, input_dtype=in_dtype, return_last=return_last)
    on = BayesianGRU(K, H, dropout=0.25, af=af, compute_dtype=dtype, input_dtype=in_dtype, return_last=return_last, length_aware=True)
    on.load_state_dict(off.state_dict())
    return off, on


def _inject(modules, B, K, H, gen, train):
    masks = [(torch.rand(B, 1, K, generator=gen) > 0.25).float() / 0.75 for _ in range(3)] + \
            [(torch.rand(B, H, generator=gen) > 0.25).float() / 0.75 for _ in range(3)]
    for m in modules:
        m.train(train)
        queue = list(masks)
        m._mask = (lambda like, q=queue: q.pop(0)) if train else (lambda like: None)


LENGTHS = [7, 3, 1, 5, 7, 0]          # 0: an all-PAD row, which runs every step ((len - 1) % T picks the last)


@pytest.mark.parametrize("dtype,in_dtype", [(None, None), ("bf16", None), (None, "bf16"), ("bf16", "bf16")])
@pytest.mark.parametrize("af", ["relu", "tanh"])
@pytest.mark.parametrize("train", [False, True])
def test_torch_branch_returns_the_defaults_vector(train, af, dtype, in_dtype):
    """return_last=True: the vector is torch.equal to the default's (an active row computes what it computes without the switch);
    the gradients agree to tests/test_encoder.py's bars (1e-5 / 2e-5 of scale: the inactive steps' zero terms are summed in another
    order at most); all_hiddens holds the last valid state past each question's end; the all-PAD row behaves as length T."""
    B, T, K, H = 6, 7, 12, 16
    off, on = _pair(K, H, af, dtype, in_dtype)
    gen = torch.Generator().manual_seed(11)
    _inject((off, on), B, K, H, gen, train)
    x = torch.randn(B, T, K, generator=gen)
    lengths, gy = torch.tensor(LENGTHS), torch.randn(B, H, generator=gen)
    x0, x1 = x.clone().requires_grad_(), x.clone().requires_grad_()
    y0, y1 = off(x0, lengths), on(x1, lengths)
    assert torch.equal(y0, y1)
    L = torch.tensor([l if 1 <= l <= T else T for l in LENGTHS])
    for b in range(B):
        assert torch.equal(on.all_hiddens[b, :L[b]], off.all_hiddens[b, :L[b]]), b
        assert torch.equal(on.all_hiddens[b, L[b]:], on.all_hiddens[b, L[b] - 1].expand(T - int(L[b]), H)), b
    assert torch.equal(on.all_hiddens[5], off.all_hiddens[5])           # all-PAD: every step ran
    assert not torch.equal(on.all_hiddens[2], off.all_hiddens[2])       # (the default lets the state evolve over PAD embeddings)
    y0.backward(gy)
    y1.backward(gy)
    assert float((x1.grad - x0.grad).abs().max()) <= 1e-5 * max(1.0, float(x0.grad.abs().max()))
    for (n, p0), (_, p1) in zip(off.named_parameters(), on.named_parameters()):
        assert float((p1.grad - p0.grad).abs().max()) <= 2e-5 * max(float(p0.grad.abs().max()), 1e-6), n


def test_return_last_false_holds_the_last_valid_state():
    B, T, K, H = 6, 7, 12, 16
    off, on = _pair(K, H, "tanh", None, None, return_last=False)
    gen = torch.Generator().manual_seed(5)
    _inject((off, on), B, K, H, gen, False)
    x = torch.randn(B, T, K, generator=gen)
    y0, y1 = off(x, torch.tensor(LENGTHS)), on(x, torch.tensor(LENGTHS))
    assert y1.shape == (B, T, H)
    for b, l in enumerate(LENGTHS):
        l = l if 1 <= l <= T else T
        assert torch.equal(y1[b, :l], y0[b, :l]) and torch.equal(y1[b, l:], y1[b, l - 1].expand(T - l, H)), b
    assert torch.equal(on(x), off(x))                                   # no lengths: every row runs every step


def test_golden_still_matches_with_the_switch_on(golden_dir):
    """tests/test_encoder.py::test_encoder_matches_reference_golden with length_aware=True, at its tolerances -- except
    all_hiddens_norm, which the contract changes (the golden's states evolve past the questions' ends): it must match over the
    valid steps instead, where both hold the same values."""
    gold = np.load(os.path.join(golden_dir, "encoder.npz"))
    enc = SkipThoughts(VOCAB, af="relu", length_aware=True)
    seeded.load_state(enc, 91)
    ref = SkipThoughts(VOCAB, af="relu")
    seeded.load_state(ref, 91)
    enc.eval(), ref.eval()
    q = enc(torch.tensor(IDX))
    (q * torch.from_numpy(seeded.seeded_array((4, 2400), 92))).sum().backward()
    assert np.abs(q.detach().numpy() - gold["q"]).max() <= 1e-5 * np.abs(gold["q"]).max()
    assert torch.equal(q, ref(torch.tensor(IDX)))
    for b, l in enumerate([6, 2, 1, 4]):
        assert torch.equal(enc.gru.all_hiddens[b, :l], ref.gru.all_hiddens[b, :l])
    g = enc.embedding.weight.grad.numpy()
    assert np.abs(g - gold["g.embedding"]).max() <= 1e-4 * np.abs(gold["g.embedding"]).max()
    assert np.all(g[0] == 0)
    gn = enc.gru.gru_cell.weight_hn.weight.grad.double().norm().item()
    assert abs(gn - gold["g.weight_hn.norm"]) <= 1e-4 * gold["g.weight_hn.norm"]
    gb = enc.gru.gru_cell.weight_ir.bias.grad.numpy()
    assert np.abs(gb - gold["g.weight_ir.bias"]).max() <= 1e-4 * np.abs(gold["g.weight_ir.bias"]).max()


# ---- the feed ----------------------------------------------------------------------------------------------------------------
def _stores(tmp_path, N=5, D=8, n_img=9):
    rs = np.random.RandomState(0)
    feats = rs.standard_normal((n_img, N, D)).astype(np.float32)
    cnt = rs.randint(1, N + 1, n_img)
    for i, c in enumerate(cnt):
        feats[i, c:] = 0.0
    np.save(tmp_path / "padded.npy", feats)
    return feed.FeatureStore(tmp_path / "padded.npy", workers=2, counts=cnt), feats, cnt


def _qa(n_img, n=23, T=6):
    rs = np.random.RandomState(1)
    items = []
    for i in range(n):
        l = int(rs.randint(0, T + 1))                                   # 0: an all-PAD question sorts last
        items.append({"v_idx": (5 * i + 2) % n_img, "q_idxes": [int(t) for t in rs.randint(1, 9, l)] + [0] * (T - l), "q_id": 100 + i,
                      "a_10_idx": [((i * 7) % 20, 0.75), ((i * 7 + 1) % 20, 0.25)]})
    return items


def _records(batch, feats, N):
    """the batch as a sorted list of per-sample records (q_id, q_idxes, a, v rows): its multiset"""
    if "v_packed" in batch:
        lens = batch["v_len"].numpy().astype(np.int64)
        off = np.concatenate([[0], np.cumsum(lens)])
        v = np.zeros((len(lens), N, batch["v_packed"].shape[1]), np.float32)
        for b in range(len(lens)):
            v[b, :lens[b]] = batch["v_packed"][off[b]:off[b + 1]].numpy()
    else:
        v = batch["v"].numpy()
    rec = [(int(batch["q_id"][b]), tuple(batch["q_idxes"][b].tolist()), batch["a"][b].numpy().tobytes(), v[b].tobytes(),
            int(batch["v_len"][b])) for b in range(len(batch["q_id"]))]
    return sorted(rec)


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("shards", [1, 2])
@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True, seed=4, ring=5, prefetch=2, producers=2)], ids=["plain", "shuffle-prefetch"])
def test_store_batches_sorts_questions_inside_each_shard(tmp_path, kw, shards, packed):
    """23 records in batches of 8 (two full ones and a short one of 7): the same multiset of records per batch as unsorted, lengths
    non-increasing inside each shard's slice, the sort stable, packed rows following the new order"""
    store, feats, cnt = _stores(tmp_path)
    qa = _qa(9)
    plain = [{k: t.clone() for k, t in b.items()} for b in feed.store_batches(store, qa, 8, 20, pin=False, packed=packed, **kw)]
    got = [{k: t.clone() for k, t in b.items()}
           for b in feed.store_batches(store, qa, 8, 20, pin=False, packed=packed, sort_questions=True, shards=shards, **kw)]
    assert len(got) == len(plain) == 3
    q_len = {it["q_id"]: sum(1 for t in it["q_idxes"] if t) for it in qa}
    rows = {it["q_id"]: it["v_idx"] for it in qa}
    moved = 0
    for g, p in zip(got, plain):
        assert set(g) == set(p) and _records(g, feats, 5) == _records(p, feats, 5)
        B = len(g["q_id"])
        lens = (g["q_idxes"] != 0).sum(1).tolist()
        assert lens == [q_len[int(i)] for i in g["q_id"]]
        per = B // shards
        for r in range(shards):
            part = lens[r * per:(r + 1) * per]
            assert part == sorted(part, reverse=True), (r, part)
            ids, before = g["q_id"][r * per:(r + 1) * per].tolist(), p["q_id"][r * per:(r + 1) * per].tolist()
            assert sorted(ids) == sorted(before)                              # a rank keeps its records
            assert ids == sorted(before, key=lambda i: -q_len[i])             # stable: ties keep the feed's order
        assert g["v_len"].tolist() == [int(cnt[rows[int(i)]]) for i in g["q_id"]]
        if packed:      # the packed rows follow: sample b's rows are its image's real rows
            off = np.concatenate([[0], np.cumsum(g["v_len"].numpy())])
            for b, i in enumerate(g["q_id"].tolist()):
                assert np.array_equal(g["v_packed"][off[b]:off[b + 1]].numpy(), feats[rows[i], :cnt[rows[i]]])
            for r in range(shards):
                mine, theirs = feed.shard(g, r, shards), feed.shard(p, r, shards)
                assert _records(mine, feats, 5) == _records(theirs, feats, 5)
        moved += int(g["q_id"].tolist() != p["q_id"].tolist())
    assert moved                                                             # (the sort did something)


def test_sort_questions_refusals(tmp_path):
    store, _, _ = _stores(tmp_path)
    with pytest.raises(ValueError, match="shards must be >= 1"):
        next(iter(feed.store_batches(store, _qa(9), 8, 20, pin=False, sort_questions=True, shards=0)))
    vec = [{"v_idx": 0, "q_idxes": [0.5, 0.0, 1.0], "q_id": 1, "a_10_idx": [(1, 1.0)]}]
    with pytest.raises(ValueError, match="sort_questions=True"):
        next(iter(feed.store_batches(store, vec, 8, 20, pin=False, q_dtype=torch.float32, sort_questions=True)))
