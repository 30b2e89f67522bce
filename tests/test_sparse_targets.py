"""Sparse answer targets without a GPU: the format (ops.densify against the reference's loop, datasets.py:963-969), the feed
serving the pairs as they are (collate / store_batches(answers="sparse") densify to bitwise the dense batch), metrics.topk_hits
on a pair, and the CPU trainer stepping from a pair -- KLD and BCE exactly as from the densified target, CE on labels it draws."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from vqa_playground_pytorch_amd import _lib, feed, metrics, ops
from vqa_playground_pytorch_amd.trainer import DataParallelTrainer

NEW_SYMBOLS = ("vqa_sparse_loss_workspace_bytes", "vqa_kld_sum_loss_sparse", "vqa_kld_sum_loss_sparse_hits", "vqa_bce_mean_loss_sparse",
               "vqa_bce_mean_loss_sparse_hits", "vqa_ce_mean_loss_sampled", "vqa_ce_mean_loss_sampled_hits")


def reference_dense(a_idx, a_val, C):
    """datasets.py:963-969 per row: a = zeros; for c_id, c_prob in pairs: a[c_id] = c_prob -- ids outside [0, C) skipped."""
    out = np.zeros((len(a_idx), C), np.float32)
    for b, (ids, vals) in enumerate(zip(a_idx.tolist(), a_val.tolist())):
        for c_id, c_prob in zip(ids, vals):
            if 0 <= c_id < C:
                out[b, c_id] = np.float32(c_prob)
    return torch.from_numpy(out)


def pairs_case(B, C, K, seed=0):
    """Rows of every kind the format names: random pairs, all padding, a single pair, a duplicated id whose later value differs,
    an id at C - 1, an id >= C, a pair with value 0 and one with value 1.0."""
    g = torch.Generator().manual_seed(seed)
    a_idx = torch.randint(0, C, (B, K), generator=g).to(torch.int32)
    a_val = torch.rand(B, K, generator=g)
    a_idx[torch.rand(B, K, generator=g) < 0.3] = -1
    special = [(-1,) * K, (C - 1,) + (-1,) * (K - 1), (0, 0) + (-1,) * (K - 2) if K > 1 else (0,),
               (C, C + 5) + (C - 1,) * (K - 2) if K > 1 else (C,)]
    for b, ids in enumerate(special[:B]):
        a_idx[b] = torch.tensor(ids, dtype=torch.int32)
    if B > 4:
        a_val[4, 0] = 0.0
        a_idx[4, 0] = C // 2
    if B > 5:
        a_val[5, K - 1] = 1.0
        a_idx[5, K - 1] = C // 3
    return a_idx, a_val


@pytest.mark.parametrize("B,C,K", [(8, 7, 1), (8, 7, 4), (40, 300, 10), (9, 2000, 16)])
def test_densify_is_the_references_loop(B, C, K):
    a_idx, a_val = pairs_case(B, C, K, seed=B + C + K)
    assert torch.equal(ops.densify(a_idx, a_val, C), reference_dense(a_idx, a_val, C))
    live = ops.live_pairs(a_idx, C)
    assert live.shape == (B, K) and not live[0].any()                                  # the all-padding row
    if K > 1:
        assert live[2].tolist()[:2] == [False, True]                                     # the later of a duplicated id counts


def test_new_symbols_are_bound_and_refuse_bad_arguments_without_a_gpu():
    h = _lib.lib()
    assert h.vqa_version() == 14 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(h, name), name
    assert h.vqa_sparse_loss_workspace_bytes(512, 0) == 512 * 4 and h.vqa_sparse_loss_workspace_bytes(512, 5) == 512 * 8
    assert h.vqa_sparse_loss_workspace_bytes(0, 5) == 0
    p, big = 16, 1 << 20     # never dereferenced: the checks come first
    calls = ((h.vqa_kld_sum_loss_sparse, (p, p, p), (p, p), ()), (h.vqa_bce_mean_loss_sparse, (p, p, p), (p, p), (0.5,)),
             (h.vqa_ce_mean_loss_sampled, (p, p, p, p), (p, p), (0.5, 1, None, 0)))
    for fn, head, out, tail in calls:
        assert fn(*head, *out, *tail, p, big, 4, 4097, 10, None) == -2 and b"4097" in h.vqa_last_error()
        assert fn(*head, *out, *tail, p, big, 4, 300, 17, None) == -1 and b"K=17" in h.vqa_last_error()
        assert fn(*head, *out, *tail, p, big, 4, 300, 0, None) == -1
        assert fn(*head, *out, *tail, p, big, 0, 300, 10, None) == -1
        assert fn(*head, *out, *tail, None, big, 4, 300, 10, None) == -1                 # null workspace
        assert fn(*head, *out, *tail, p, 4 * 4 - 1, 4, 300, 10, None) == -1              # workspace too small
        for hole in range(len(head)):                                                    # null logits / a_idx / a_val / labels_out
            args = list(head)
            args[hole] = None
            assert fn(*args, *out, *tail, p, big, 4, 300, 10, None) == -1
        assert fn(*head, None, p, *tail, p, big, 4, 300, 10, None) == -1                 # null loss
    assert h.vqa_kld_sum_loss_sparse_hits(p, p, p, p, p, None, 5, p, big, 4, 300, 10, None) == -1     # null hits
    assert h.vqa_bce_mean_loss_sparse_hits(p, p, p, p, p, p, 17, 0.5, p, big, 4, 300, 10, None) == -1  # kmax over 16
    assert h.vqa_ce_mean_loss_sampled_hits(p, p, p, p, p, p, p, 5, 0.5, 1, None, 0, p, 4 * 8 - 1, 4, 300, 10, None) == -1
    assert h.vqa_ce_mean_loss_sampled(p, p, p, p, p, p, 0.5, 1, 20, 0, p, big, 4, 300, 10, None) == -2  # misaligned seed word


def test_every_wrapper_refuses_bad_dtype_shape_and_k():
    z = torch.zeros(4, 10)
    a_idx, a_val = torch.zeros(4, 3, dtype=torch.int32), torch.zeros(4, 3)
    wrappers = (lambda *a: ops.kld_sum_loss_and_grad_sparse(*a), lambda *a: ops.kld_sum_loss_and_grad_sparse_hits(*a, 5),
                lambda *a: ops.bce_mean_loss_and_grad_sparse(*a), lambda *a: ops.bce_mean_loss_and_grad_sparse_hits(*a, 5),
                lambda *a: ops.ce_mean_loss_and_grad_sampled(*a, seed=1), lambda *a: ops.ce_mean_loss_and_grad_sampled_hits(*a, 5, seed=1))
    bad = ((z, a_idx.long(), a_val), (z, a_idx, a_val.double()), (z.double(), a_idx, a_val), (z, a_idx[:, :2], a_val),
           (z, a_idx[:3], a_val[:3]), (z[0], a_idx, a_val), (z, a_idx[:, :0], a_val[:, :0]),
           (z, torch.zeros(4, 17, dtype=torch.int32), torch.zeros(4, 17)), (z, a_idx[0], a_val[0]))
    for fn in wrappers:
        for args in bad:
            with pytest.raises(ValueError):
                fn(*args)
    with pytest.raises(ValueError):
        ops.densify(a_idx.long(), a_val, 10)
    with pytest.raises(ValueError):
        ops.densify(torch.zeros(4, 17, dtype=torch.int32), torch.zeros(4, 17), 10)
    with pytest.raises(_lib.VqaLibraryError):            # well-formed CPU tensors: the kernels have no CPU fallback
        ops.kld_sum_loss_and_grad_sparse(z, a_idx, a_val)


# ---- the feed ------------------------------------------------------------------------------------------------------------------
def records(n, C=20, T=6, seed=0, most=5):
    """Reference-style records with 1 .. `most` pairs each, a duplicated id in some and a record with a single pair."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        k = 1 if i == 1 else 1 + rs.randint(most)
        ids = rs.choice(C, size=k, replace=True)
        p = rs.dirichlet(np.ones(k))
        out.append({"v": rs.standard_normal((4, 8)).astype(np.float32), "v_idx": int(rs.randint(11)), "q_idxes": [1 + i, 2, 0, 0, 0, 0][:T],
                    "q_id": 100 + i, "a_10_idx": [(int(c), float(x)) for c, x in zip(ids, p)]})
    return out


def _store(tmp_path, n_img=11, N=4, D=8, seed=3):
    feats = np.random.RandomState(seed).standard_normal((n_img, N, D)).astype(np.float32)
    np.save(tmp_path / "feats.npy", feats)
    return feed.FeatureStore(tmp_path / "feats.npy", workers=1)


@pytest.mark.parametrize("n", [7, 1])
def test_collate_sparse_densifies_to_the_dense_batch(n):
    its = records(n)
    dense, sparse = feed.collate(its, 20), feed.collate(its, 20, answers="sparse")
    assert "a" not in sparse and sparse["a_idx"].dtype == torch.int32 and sparse["a_val"].dtype == torch.float32
    K = max(len(it["a_10_idx"]) for it in its)
    assert sparse["a_idx"].shape == sparse["a_val"].shape == (n, K)
    assert torch.equal(ops.densify(sparse["a_idx"], sparse["a_val"], 20), dense["a"])
    for i, it in enumerate(its):                                                         # record order, -1 / 0 padding
        k = len(it["a_10_idx"])
        assert sparse["a_idx"][i, :k].tolist() == [c for c, _ in it["a_10_idx"]] and (sparse["a_idx"][i, k:] == -1).all()
        assert (sparse["a_val"][i, k:] == 0).all()
    assert all(torch.equal(dense[k], sparse[k]) for k in ("v", "q_idxes", "q_id"))
    assert torch.equal(feed.shard(sparse, 1, n)["a_idx"], sparse["a_idx"][1:2]) if n > 1 else True
    with pytest.raises(ValueError):
        feed.collate(its, 20, answers="csr")


@pytest.mark.parametrize("batch_size", [4, 5, 11])
def test_store_batches_sparse_densifies_to_the_dense_batches(tmp_path, batch_size):
    store = _store(tmp_path)
    its = records(11, seed=2)
    table = feed.qa_table(store, its, 20, require_answers=True)
    dense = [{k: v.clone() for k, v in b.items()} for b in feed.store_batches(store, table, batch_size, 20, shuffle=True, seed=5, pin=False)]
    sparse = [{k: v.clone() for k, v in b.items()}
              for b in feed.store_batches(store, table, batch_size, 20, shuffle=True, seed=5, pin=False, answers="sparse")]
    assert len(dense) == len(sparse) == -(-11 // batch_size)
    K = max(len(it["a_10_idx"]) for it in its)
    for d, s in zip(dense, sparse):
        assert "a" not in s and s["a_idx"].shape == s["a_val"].shape == (d["a"].size(0), K)     # K is the TABLE's largest count
        assert s["a_idx"].dtype == torch.int32 and s["a_val"].dtype == torch.float32
        assert torch.equal(ops.densify(s["a_idx"], s["a_val"], 20), d["a"])
        assert all(torch.equal(d[k], s[k]) for k in ("v", "q_idxes", "q_id"))
    assert dense[-1]["a"].size(0) == 11 - batch_size * (len(dense) - 1)                          # the short last batch
    # background assembly and the prefetcher path keep the two keys
    pre = list(feed.DevicePrefetcher(feed.store_batches(store, table, batch_size, 20, shuffle=True, seed=5, pin=False, answers="sparse",
                                                        prefetch=1, ring=3), "cpu"))
    assert [sorted(b) for b in pre] == [sorted(s) for s in sparse]
    with pytest.raises(ValueError):
        next(feed.store_batches(store, table, batch_size, 20, answers="coo"))


def test_feed_refuses_what_it_cannot_serve_sparse(tmp_path):
    store = _store(tmp_path)
    its = records(4)
    many = copy.deepcopy(its)
    many[2]["a_10_idx"] = [(i, 1.0 / 17) for i in range(17)]
    with pytest.raises(ValueError, match="17"):
        feed.collate(many, 20, answers="sparse")
    with pytest.raises(ValueError, match="17"):
        next(feed.store_batches(store, many, 2, 20, pin=False, answers="sparse"))
    assert next(feed.store_batches(store, many, 2, 20, pin=False))["a"].shape == (2, 20)         # dense serves them as before
    sixteen = copy.deepcopy(its)
    sixteen[0]["a_10_idx"] = [(i, 1.0 / 16) for i in range(16)]
    assert feed.collate(sixteen, 20, answers="sparse")["a_idx"].shape == (4, 16)
    given_dense = [dict({k: v for k, v in it.items() if k != "a_10_idx"}, a=np.zeros(20, np.float32)) for it in its]
    with pytest.raises(ValueError, match="dense 'a'"):
        feed.collate(given_dense, 20, answers="sparse")
    with pytest.raises(ValueError, match="dense 'a'"):
        next(feed.store_batches(store, given_dense, 2, 20, pin=False, answers="sparse"))
    empty = copy.deepcopy(its)
    empty[3]["a_10_idx"] = []
    with pytest.raises(ValueError, match="q_id 103"):
        feed.qa_table(store, empty, 20, require_answers=True)
    table = feed.qa_table(store, empty, 20)                                                      # not required: an all-padding row
    b = next(feed.store_batches(store, table, 4, 20, pin=False, answers="sparse"))
    assert (b["a_idx"][3] == -1).all() and not ops.densify(b["a_idx"], b["a_val"], 20)[3].any()


def test_topk_hits_takes_the_sparse_pair():
    a_idx, a_val = pairs_case(40, 300, 10, seed=4)
    z = torch.randn(40, 300, generator=torch.Generator().manual_seed(1))
    want = metrics.topk_hits(z, ops.densify(a_idx, a_val, 300), 5)
    assert torch.equal(metrics.topk_hits(z, (a_idx, a_val), 5), want)
    assert torch.equal(metrics.topk_hits(z, {"a_idx": a_idx, "a_val": a_val, "q_id": None}, 5), want)


# ---- the trainer on the CPU ----------------------------------------------------------------------------------------------------
class Tiny(nn.Module):       # the model of tests/test_trainer_gloo.py
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(12, 16)
        self.b = nn.Linear(16, 9)

    def forward(self, sample):
        return self.b(torch.tanh(self.a(sample["x"])))


def _batches(steps=3, B=6, C=9, K=4):
    g = torch.Generator().manual_seed(11)
    out = []
    for s in range(steps):
        a_idx, a_val = pairs_case(B, C, K, seed=20 + s)
        a_val = a_val.clamp(min=0.05)
        a_val[4, 0] = 0.0
        out.append(({"x": torch.randn(B, 12, generator=g)}, a_idx, a_val))
    return out


@pytest.mark.parametrize("loss", ["KLD", "BCE"])
def test_cpu_steps_from_a_sparse_target_equal_steps_from_the_densified_one(loss):
    torch.manual_seed(0)
    model = Tiny()
    ta = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, loss=loss, topk=(1, 5))
    tb = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, loss=loss, topk=(1, 5))
    for sample, a_idx, a_val in _batches():
        la, na = ta.step(sample, {"a_idx": a_idx, "a_val": a_val})
        lb, nb = tb.step(sample, ops.densify(a_idx, a_val, 9))
        assert torch.equal(la, lb) and torch.equal(na, nb)
        assert torch.equal(ta.last_hits, tb.last_hits) and ta.last_labels is None
    for p, q in zip(ta.model.parameters(), tb.model.parameters()):
        assert torch.equal(p, q)


def test_cpu_ce_draws_live_labels_and_steps_on_them():
    torch.manual_seed(0)
    model = Tiny()
    ta = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, loss="CE", topk=(1, 5))
    tb = DataParallelTrainer(copy.deepcopy(model), lr=1e-2, loss="CE", topk=(1, 5))
    seen = set()
    for sample, a_idx, a_val in _batches():
        keep = ops.densify(a_idx, a_val, 9).sum(1) > 0              # rows with a positive pair (CE's labels must be real classes)
        sample, a_idx, a_val = {"x": sample["x"][keep]}, a_idx[keep], a_val[keep]
        la, _ = ta.step(sample, {"a_idx": a_idx, "a_val": a_val})
        labels = ta.last_labels
        assert labels.dtype == torch.int64 and labels.shape == (a_idx.size(0),)
        dense = ops.densify(a_idx, a_val, 9)
        assert (dense.gather(1, labels[:, None]) > 0).all()          # live ids with positive probability
        seen.update(labels.tolist())
        lb, _ = tb.step(sample, labels)
        assert torch.equal(la, lb) and torch.equal(ta.last_hits, tb.last_hits)
    assert len(seen) > 1
    for p, q in zip(ta.model.parameters(), tb.model.parameters()):
        assert torch.equal(p, q)
    # a row without a positive pair: label -1, nothing added to loss or gradient, never a hit
    sample, a_idx, a_val = _batches(1)[0]
    a_idx[0] = -1
    before = [p.detach().clone() for p in ta.model.parameters()]
    loss, _ = ta.step(sample, {"a_idx": a_idx, "a_val": a_val})
    assert ta.last_labels[0].item() == -1 and torch.isfinite(loss)
    rest = torch.arange(1, 6)
    logits = Tiny.forward(types.SimpleNamespace(a=lambda x: torch.nn.functional.linear(x, before[0], before[1]),
                                                b=lambda x: torch.nn.functional.linear(x, before[2], before[3])), sample)
    want = torch.nn.functional.cross_entropy(logits[rest], ta.last_labels[rest], reduction="sum") / 6
    assert torch.allclose(loss, want, rtol=1e-6, atol=0)
    assert ta.last_hits[-1].item() <= 5


def test_from_config_samplingans_steps_from_the_sparse_feed(tmp_path):
    store = _store(tmp_path)
    its = records(8, C=9, seed=6)
    for it in its:
        it["q_idxes"] = np.random.RandomState(it["q_id"]).standard_normal(12).astype(np.float32)

    class FromFeed(Tiny):
        def forward(self, sample):
            return super().forward({"x": sample["q_idxes"]})

    torch.manual_seed(0)
    tr = DataParallelTrainer.from_config(FromFeed(), types.SimpleNamespace(lr=1e-2, samplingans=True), topk=(1,))
    assert tr.loss_kind == "CE"
    n = 0
    for batch in feed.store_batches(store, feed.qa_table(store, its, 9, q_dtype=torch.float32, require_answers=True), 4, 9, pin=False,
                                    q_dtype=torch.float32, answers="sparse"):
        loss, _ = tr.step(batch, batch)                              # the two keys are picked out of the batch dict
        dense = ops.densify(batch["a_idx"], batch["a_val"], 9)
        assert torch.isfinite(loss) and (dense.gather(1, tr.last_labels[:, None]) > 0).all()
        assert len(tr.accuracy()) == 1
        n += 1
    assert n == 2
