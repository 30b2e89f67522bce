"""Per-sample region counts ('v_len'), the parts that need no GPU: the four `_len_` entry points of K3 exist in the header, the
binding and the library and refuse NULL pointers; the feed serves the counts of a FeatureStore as 'v_len' for the right images;
the models validate (CoR2) or refuse (ODA) them before anything is launched.  The kernels themselves and the model-level contract
(alpha exactly 0 on the padding, padding invisible to every output and gradient) are tests/test_gpu_region_counts.py: the layers
have no CPU path to run them on."""
import os
import re

import numpy as np
import pytest
import torch

from kernel_harness import forbid_launches
from vqa_playground_pytorch_amd import CoR2Model, ODAModel, _lib, feed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["vqa_softmax_attention_pool_len_fwd", "vqa_softmax_attention_pool_len_bwd",
           "vqa_softmax_attention_pool_len_fwd_bf16", "vqa_softmax_attention_pool_len_bwd_bf16"]


def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "vqa_mi355x.h"), encoding="utf-8") as fh:
        header = fh.read()
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
        # (logits / alpha, v, lens, ...): the third argument is the counts pointer in all four
        assert len(_lib.SIGNATURES[name][1]) == (14 if "_fwd" in name else 16), name
    assert L.vqa_version() == 14 == _lib.ABI_VERSION
    assert "#define VQA_ABI_VERSION 14" in header


@pytest.mark.parametrize("name", ENTRIES)
def test_null_pointers_are_refused_without_a_gpu(name):
    L = _lib.lib()
    fn = getattr(L, name)
    if "_fwd" in name:
        rc = fn(None, None, None, None, None, None, 0.0, 0, None, 2, 3, 8, 1, None)
    else:
        rc = fn(None, None, None, None, None, None, None, None, 0.0, 0, None, 2, 3, 8, 1, None)
    assert rc == -1
    assert b"null pointer" in L.vqa_last_error()


# ---- feed -------------------------------------------------------------------------------------------------------------------
N_IMG, N, D = 11, 4, 8


def _store(tmp_path, counts="file"):
    rs = np.random.RandomState(3)
    feats = rs.standard_normal((N_IMG, N, D)).astype(np.float32)
    cnt = (np.arange(N_IMG) * 3) % N + 1                       # 1..N, every value taken
    for i, c in enumerate(cnt):
        feats[i, c:] = 0.0                                      # the store is zero-padded
    np.save(tmp_path / "f.npy", feats)
    np.save(tmp_path / "counts.npy", cnt)
    if counts == "file":
        counts = tmp_path / "counts.npy"
    elif counts == "array":
        counts = cnt
    return feed.FeatureStore(tmp_path / "f.npy", workers=2, counts=counts), feats, cnt


def _qa(n=23):
    return [{"v_idx": (5 * i + 2) % N_IMG, "q_idxes": [i, 1, 0], "q_id": i, "a_10_idx": [((i * 7) % 20, 1.0)]} for i in range(n)]


@pytest.mark.parametrize("how", ["file", "array"])
@pytest.mark.parametrize("kw", [dict(shuffle=False), dict(shuffle=True, seed=4), dict(shuffle=True, ring=5, prefetch=2)],
                         ids=["plain", "shuffle", "shuffle-prefetch"])
def test_store_batches_serve_the_counts_of_the_right_images(tmp_path, how, kw):
    """23 records in batches of 4: five full batches and a last one of 3.  Every row's 'v_len' is the count of ITS image -- found
    again through q_id -> record -> image -- and the regions beyond it are the store's zeros."""
    st, feats, cnt = _store(tmp_path, how)
    qa = _qa()
    seen = 0
    for batch in feed.store_batches(st, qa, 4, 20, pin=False, **kw):
        b = batch["v"].size(0)
        assert batch["v_len"].dtype == torch.int32 and batch["v_len"].shape == (b,)
        for r in range(b):
            img = qa[int(batch["q_id"][r])]["v_idx"]
            assert int(batch["v_len"][r]) == int(cnt[img])
            assert np.array_equal(batch["v"][r].numpy(), feats[img])
            assert not batch["v"][r, int(cnt[img]):].any()
        seen += b
    assert seen == 23 and b == 3
    assert torch.equal(next(iter(feed.store_batches(st, qa, 23, 20, pin=False)))["v_len"],
                       torch.from_numpy(cnt[[q["v_idx"] for q in qa]].astype(np.int32)))


def test_a_store_without_counts_serves_no_v_len(tmp_path):
    st, _, _ = _store(tmp_path, None)
    assert st.counts is None
    assert "v_len" not in next(iter(feed.store_batches(st, _qa(), 4, 20, pin=False)))


@pytest.mark.parametrize("bad", [0, N + 1, -1])
def test_counts_outside_1_to_n_raise(tmp_path, bad):
    _, _, cnt = _store(tmp_path)
    wrong = cnt.copy()
    wrong[5] = bad
    with pytest.raises(ValueError):
        feed.FeatureStore(tmp_path / "f.npy", counts=wrong)
    with pytest.raises(ValueError):
        feed.FeatureStore(tmp_path / "f.npy", counts=cnt[:-1])
    with pytest.raises(ValueError):
        feed.FeatureStore(tmp_path / "f.npy", counts=cnt.astype(np.float32))


def test_collate_and_shard_carry_v_len():
    rs = np.random.RandomState(0)
    items = [{"v": rs.standard_normal((N, D)).astype(np.float32), "q_idxes": [1, 2, 0], "q_id": i, "v_len": 1 + i % N,
              "a_10_idx": [(i, 1.0)]} for i in range(6)]
    batch = feed.collate(items, 20)
    assert batch["v_len"].dtype == torch.int32 and batch["v_len"].tolist() == [1, 2, 3, 4, 1, 2]
    assert "v_len" not in feed.collate([{k: x for k, x in it.items() if k != "v_len"} for it in items], 20)
    for bad in (0, N + 1):
        with pytest.raises(ValueError):
            feed.collate([dict(items[0], v_len=bad)], 20)
    parts = [feed.shard(batch, r, 3) for r in range(3)]
    assert [p["v_len"].tolist() for p in parts] == [[1, 2], [3, 4], [1, 2]]
    assert all(torch.equal(p["v"], batch["v"][2 * r:2 * r + 2]) for r, p in enumerate(parts))


def test_device_prefetcher_passes_v_len_through_on_the_cpu(tmp_path):
    st, _, _ = _store(tmp_path)
    plain = [b["v_len"].clone() for b in feed.store_batches(st, _qa(), 4, 20, pin=False)]
    got = [b["v_len"].clone() for b in feed.DevicePrefetcher(feed.store_batches(st, _qa(), 4, 20, pin=False), "cpu")]
    assert len(got) == len(plain) and all(torch.equal(a, b) for a, b in zip(got, plain))


# ---- models -----------------------------------------------------------------------------------------------------------------
def _sample(B=3, regions=36):
    return {"v": torch.zeros(B, regions, 2048), "q_idxes": torch.zeros(B, 2400)}


@pytest.mark.parametrize("dtype", [torch.int32, torch.int64])
@pytest.mark.parametrize("bad", [0, 37, -3])
def test_cor2_refuses_host_counts_outside_1_to_n_before_anything_runs(bad, dtype, monkeypatch):
    """the validation sits in front of every layer: with all of ops' launches made to fail the ValueError still comes first"""
    from vqa_playground_pytorch_amd import ops
    forbid_launches(monkeypatch, ops)
    model = CoR2Model(["PAD", "UNK"], 50).eval()
    monkeypatch.setattr(model.compress_v, "forward", lambda *a, **k: pytest.fail("a layer ran"))
    with pytest.raises(ValueError, match="1..36"):
        model(dict(_sample(), v_len=torch.tensor([36, bad, 1], dtype=dtype)))
    with pytest.raises(ValueError, match="v_len"):
        model(dict(_sample(), v_len=torch.tensor([36, 1], dtype=dtype)))            # [B - 1]
    with pytest.raises(ValueError, match="v_len"):
        model(dict(_sample(), v_len=torch.tensor([36.0, 1.0, 2.0])))               # not integers


def test_region_counts_become_int32_and_keep_valid_values():
    from vqa_playground_pytorch_amd import ops
    got = ops.region_counts(torch.tensor([1, 36, 20], dtype=torch.int64), 36, torch.device("cpu"))
    assert got.dtype == torch.int32 and got.tolist() == [1, 36, 20]
    same = torch.tensor([5, 6], dtype=torch.int32)
    assert ops.region_counts(same, 6, torch.device("cpu")).data_ptr() == same.data_ptr()


def test_oda_refuses_v_len():
    model = ODAModel(["PAD", "UNK"], 50).eval()
    with pytest.raises(ValueError, match="v_len"):
        model(dict(_sample(), v_len=torch.tensor([36, 36, 36], dtype=torch.int32)))


def test_trainer_and_evaluator_count_v_len_among_the_model_inputs():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    with_len = dict(_sample(), v_len=torch.ones(3, dtype=torch.int32), a=None, q_id=None)
    assert DataParallelTrainer._model_keys(with_len) == {"v", "q_idxes", "v_len"}
    assert DataParallelTrainer._model_keys(_sample()) == {"v", "q_idxes"}
    assert tuple(Evaluator._model_keys(with_len)) == ("v", "q_idxes", "v_len")
    assert tuple(Evaluator._model_keys(_sample())) == ("v", "q_idxes")
