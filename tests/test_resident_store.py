"""The device-resident region store, the parts that need no GPU: the two entry points in the header, the binding and the library;
ops.gather_regions on CPU tensors against FeatureStore.gather (and gather_packed + ops.unpack_regions) in its three dtype forms;
feed.DeviceFeatureStore(device="cpu") -- layouts, compaction, the host validation, the capacity refusal; store_batches(resident=)
against the host path; the 'v_idx' key through collate, shard, the model's attribute and the trainer's / evaluator's key sets.
Every comparison is exact: the feature copies rows, it computes nothing.  The kernel, the models, the captured step, the
prefetcher's copies and the evaluator are tests/test_gpu_resident_store.py."""
import os
import re

import numpy as np
import pytest
import torch

from vqa_playground_pytorch_amd import CoR2Model, ODAModel, _lib, feed, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, BF = torch.float32, torch.bfloat16
FORMS = [(F32, F32), (BF, BF), (BF, F32)]          # (the store's dtype, the gather's out_dtype)
N_IMG, N, D = 7, 5, 8
IDX = [0, 6, 3, 3, 1, 6, 0, 2]                     # duplicates, 0 and n_img - 1 among them


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """{'padded', 'counts', 'ragged'}: a padded store, the same array with counts (padding zeroed; a -0.0 among the real values)
    and the ragged store of its real rows; the array; the counts.  Built once, never changed."""
    root = tmp_path_factory.mktemp("resident")
    rs = np.random.RandomState(3)
    full = rs.standard_normal((N_IMG, N, D)).astype(np.float32)
    full[2, 0, 1] = -0.0
    cnt = np.array([1, N, 3, 2, N, 4, 1])
    feats = full.copy()
    for i, c in enumerate(cnt):
        feats[i, c:] = 0.0
    np.save(root / "full.npy", full)
    np.save(root / "padded.npy", feats)
    np.save(root / "rows.npy", np.concatenate([feats[i, :c] for i, c in enumerate(cnt)]))
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    names = ["img%d.jpg" % i for i in range(N_IMG)]
    return {"padded": feed.FeatureStore(root / "full.npy", names=names, workers=2),
            "counts": feed.FeatureStore(root / "padded.npy", names=names, workers=2, counts=cnt),
            "ragged": feed.FeatureStore(root / "rows.npy", names=names, workers=2, offsets=offsets, regions=N),
            "root": root, "full": full, "feats": feats, "cnt": cnt, "offsets": offsets}


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "vqa_mi355x.h"), encoding="utf-8") as fh:
        header = fh.read()
    L = _lib.lib()
    for name, nargs in (("vqa_gather_regions", 14), ("vqa_gather_regions_supported", 5)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs == len(_lib.PARAMS[name]), name
        assert hasattr(L, name), name
    assert list(_lib.PARAMS["vqa_gather_regions"]) == ["rows", "total_rows", "starts", "counts", "n_img", "idx", "out", "v_len_out", "B",
                                                        "N", "D", "in_bf16", "out_bf16", "stream"]
    assert L.vqa_version() == 14 == _lib.ABI_VERSION
    assert "#define VQA_ABI_VERSION 14" in header
    with open(os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc", "Makefile"), encoding="utf-8") as fh:
        assert "region_gather.hip" in fh.read()


def test_supported_truth_table():
    S = _lib.lib().vqa_gather_regions_supported
    for in_bf16, out_bf16 in ((0, 0), (1, 1), (1, 0)):
        assert S(512, 36, 2048, in_bf16, out_bf16) == 1 and S(1, 1, 8, in_bf16, out_bf16) == 1
        assert S(128, 100, 12, in_bf16, out_bf16) == 0 and S(128, 100, 4, in_bf16, out_bf16) == 0          # D % 8
        for B_, N_, D_ in ((0, 36, 8), (-1, 36, 8), (2, 0, 8), (2, 36, 0), (2, -3, 8)):                     # positive sizes
            assert S(B_, N_, D_, in_bf16, out_bf16) == 0, (B_, N_, D_)
    assert S(128, 100, 2048, 0, 1) == 0                                         # fp32 rows are not narrowed


def test_null_pointers_are_bad_arguments():
    """no device memory is needed to be refused: every required pointer NULL in turn (the others are never dereferenced, nothing is
    launched on a refusal), then a non-positive size"""
    import ctypes
    L = _lib.lib()
    some = ctypes.c_void_p(4096)
    for missing in range(4):
        rows, starts, idx, out = (None if k == missing else some for k in range(4))
        assert L.vqa_gather_regions(rows, 35, starts, None, 7, idx, out, None, 2, 5, 8, 0, 0, None) == -1, missing
        assert b"null pointer" in L.vqa_last_error()
    for B_, n_img, total in ((0, 7, 35), (2, 0, 35), (2, 7, 0)):
        assert L.vqa_gather_regions(some, total, some, None, n_img, some, some, None, B_, 5, 8, 0, 0, None) == -1
        assert b"must be positive" in L.vqa_last_error()
    assert L.vqa_gather_regions(some, 35, some, None, 7, some, some, None, 2, 5, 12, 0, 0, None) == -2        # D % 8
    assert L.vqa_gather_regions(some, 35, some, None, 7, some, some, None, 2, 5, 8, 0, 1, None) == -2         # fp32 -> bf16
    assert L.vqa_gather_regions(ctypes.c_void_p(4100), 35, some, None, 7, some, some, None, 2, 5, 8, 0, 0, None) == -2   # alignment


# ---- ops.gather_regions on the CPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["padded", "counts", "ragged"])
@pytest.mark.parametrize("compact", [True, False], ids=["compact", "as-is"])
def test_gather_regions_equals_the_host_gather(stores, kind, compact):
    store, cnt = stores[kind], stores["cnt"]
    idx = torch.tensor(IDX, dtype=torch.int32)
    for dt_store, dt_out in FORMS:
        what = (kind, compact, dt_store, dt_out)
        ds = feed.DeviceFeatureStore(store, "cpu", dtype=dt_store, compact=compact, chunk_bytes=1)    # (chunks of one image)
        v, v_len = ops.gather_regions(ds, idx, dt_out)
        assert v.shape == (len(IDX), N, D) and v.dtype == dt_out, what
        if kind == "ragged":
            want = None
        else:
            want = store.gather(IDX, torch.empty(len(IDX), N, D, dtype=dt_store)).to(dt_out)       # (bf16 -> fp32: exact)
            assert _same_bits(v, want), what
        if kind != "padded":
            packed, lens = torch.zeros(len(IDX) * N, D, dtype=dt_store), torch.zeros(len(IDX), dtype=torch.int32)
            store.gather_packed(IDX, packed, lens)
            assert _same_bits(v, ops.unpack_regions(packed, lens, len(IDX), dt_out)), what
            assert v_len.dtype == torch.int32 and v_len.tolist() == cnt[IDX].tolist() == lens.tolist(), what
            pad = torch.arange(N)[None, :] >= v_len[:, None].long()
            assert bool((_bits(v)[pad] == 0).all()), (what, "the padding is not +0.0")
            assert ops.gather_regions(ds, idx, dt_out, want_len=False)[1] is None
        else:
            assert v_len is None and ds.counts is None, what
        assert _same_bits(ops.gather_regions(ds, idx.long(), dt_out)[0], v), (what, "int64 indices")
        assert _same_bits(ops.gather_regions(ds, torch.tensor([9] + IDX, dtype=torch.int32)[1:], dt_out)[0], v), (what, "a slice")


def test_gather_regions_keeps_a_negative_zero_of_the_store_and_pads_with_positive_zero(stores):
    ds = feed.DeviceFeatureStore(stores["counts"], "cpu")
    v, v_len = ops.gather_regions(ds, torch.tensor([2, 0], dtype=torch.int32))
    assert _bits(v)[0, 0, 1].item() == -2 ** 31                      # the -0.0 the store holds is a real value: copied
    assert v_len.tolist() == [3, 1] and bool((_bits(v)[0, 3:] == 0).all()) and bool((_bits(v)[1, 1:] == 0).all())


def test_gather_regions_refusals(stores):
    ds = feed.DeviceFeatureStore(stores["counts"], "cpu")
    with pytest.raises(IndexError):
        ops.gather_regions(ds, torch.tensor([0, N_IMG], dtype=torch.int32))
    with pytest.raises(IndexError):
        ops.gather_regions(ds, torch.tensor([-1, 0]))
    with pytest.raises(ValueError):
        ops.gather_regions(ds, torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError):
        ops.gather_regions(ds, torch.tensor([[0, 1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="cast by the model"):
        ops.gather_regions(ds, torch.tensor([0], dtype=torch.int32), BF)                  # fp32 rows are never narrowed here


# ---- DeviceFeatureStore ------------------------------------------------------------------------------------------------------
def test_device_store_fields_and_compaction(stores):
    cnt, R = stores["cnt"], int(stores["cnt"].sum())
    compact = feed.DeviceFeatureStore(stores["counts"], "cpu", dtype=BF)
    assert compact.rows.shape == (R, D) and compact.rows.dtype == BF, "compact=True holds only the real rows"
    assert compact.starts.tolist() == stores["offsets"][:-1].tolist() and compact.counts.tolist() == cnt.tolist()
    assert compact.starts.dtype == torch.int64 and compact.counts.dtype == torch.int32
    assert compact.nbytes == R * D * 2 + N_IMG * 12 and len(compact) == N_IMG and compact.sample_shape == (N, D)
    assert compact.index("img4.jpg") == 4 and compact.name_to_idx is stores["counts"].name_to_idx
    as_is = feed.DeviceFeatureStore(stores["counts"], "cpu", compact=False)
    assert as_is.rows.shape == (N_IMG * N, D) and as_is.starts.tolist() == [i * N for i in range(N_IMG)]
    assert _same_bits(as_is.rows, torch.from_numpy(stores["feats"]).view(-1, D))
    ragged = feed.DeviceFeatureStore(stores["ragged"], "cpu", dtype=BF)
    assert _same_bits(ragged.rows, compact.rows) and ragged.starts.tolist() == compact.starts.tolist()
    plain = feed.DeviceFeatureStore(stores["padded"], "cpu")
    assert plain.counts is None and plain.nbytes == N_IMG * N * D * 4 + N_IMG * 8
    assert _same_bits(plain.rows, torch.from_numpy(stores["full"]).view(-1, D))
    with pytest.raises(KeyError):
        plain.index("nope.jpg")
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        feed.DeviceFeatureStore(stores["padded"], "cpu", dtype=torch.float16)


def test_device_store_validates_the_layout_on_the_host(stores):
    """FeatureStore checks what it is given; DeviceFeatureStore checks again what it is about to rely on, so a store whose arrays
    were changed behind its back is refused before a byte is uploaded"""
    root, cnt, offsets = stores["root"], stores["cnt"], stores["offsets"]

    def ragged():
        return feed.FeatureStore(root / "rows.npy", offsets=offsets, regions=N)

    def padded():
        return feed.FeatureStore(root / "padded.npy", counts=cnt)
    s = ragged()
    s._starts[N_IMG - 1] += 1                                  # the last image's rows would end one row past the array
    with pytest.raises(ValueError, match="the store holds %d" % int(cnt.sum())):
        feed.DeviceFeatureStore(s, "cpu")
    s = ragged()
    s._starts[0] = -1
    with pytest.raises(ValueError, match="owns rows -1"):
        feed.DeviceFeatureStore(s, "cpu")
    for bad, compact in ((0, True), (0, False), (N + 1, True), (N + 1, False)):
        s = padded()
        s.counts[3] = bad
        with pytest.raises(ValueError, match="image 3 has region count %d outside 1..%d" % (bad, N)):
            feed.DeviceFeatureStore(s, "cpu", compact=compact)
    with pytest.raises(ValueError, match="do not pass counts="):
        feed.FeatureStore(root / "rows.npy", offsets=offsets, regions=N, counts=cnt)
    feed._check_store_layout("ok", offsets[:-1], cnt, N, int(cnt.sum()))
    with pytest.raises(ValueError):
        feed._check_store_layout("short", offsets[:-1], cnt, N, int(cnt.sum()) - 1)
    with pytest.raises(ValueError):
        feed._check_store_layout("no counts", [0, 5, 11], None, 5, 15)       # the last image: rows 11..16 of 15


def test_device_store_capacity_refusal_names_both_numbers(stores):
    with pytest.raises(ValueError) as e:
        feed.DeviceFeatureStore(stores["counts"], "cpu", reserve_bytes=1 << 60)
    need = int(stores["cnt"].sum()) * D * 4 + N_IMG * 12
    assert "needs %d bytes" % need in str(e.value) and "%d reserved" % (1 << 60) in str(e.value) and " free" in str(e.value)
    assert feed.DeviceFeatureStore(stores["counts"], "cpu", reserve_bytes=0).nbytes == need
    assert feed.DeviceFeatureStore.DEFAULT_RESERVE_BYTES == 8 << 30 and "8 GiB" in feed.DeviceFeatureStore.__doc__


# ---- store_batches(resident=), collate, shard --------------------------------------------------------------------------------
def _qa(n=23):
    return [{"img_filename": "img%d.jpg" % ((5 * i + 2) % N_IMG), "q_idxes": [1] * (1 + i % 3) + [0] * (3 - i % 3), "q_id": 100 + i,
             "a_10_idx": [((i * 7) % 20, 0.75), ((i * 7 + 1) % 20, 0.25)]} for i in range(n)]


def _clone(batches):
    return [{k: t.clone() for k, t in b.items()} for b in batches]


@pytest.mark.parametrize("answers", ["dense", "sparse"])
@pytest.mark.parametrize("kw", [{}, {"sort_questions": True, "shards": 2}, {"prefetch": 2, "producers": 2, "ring": 5}],
                         ids=["plain", "sorted-2-shards", "prefetch"])
def test_store_batches_resident_yields_the_host_paths_batches_without_regions(stores, answers, kw):
    host_store = stores["counts"]
    ds = feed.DeviceFeatureStore(host_store, "cpu")
    qa, B = _qa(), 8
    common = dict(shuffle=True, seed=4, pin=False, answers=answers, epochs=2, **kw)
    host = _clone(feed.store_batches(host_store, qa, B, 20, **common))
    table = feed.qa_table(host_store, qa, 20)
    order = [np.random.RandomState(4 + e).permutation(len(qa)) for e in range(2)]
    for store_arg in (host_store, ds):
        got = _clone(feed.store_batches(store_arg, qa, B, 20, resident=ds, **common))
        assert [b["q_id"].numel() for b in got] == [8, 8, 7, 8, 8, 7]                    # the short last batch of each epoch
        for i, (g, h) in enumerate(zip(got, host)):
            assert set(g) == (set(h) - {"v", "v_len"}) | {"v_idx"}, sorted(g)
            for k in g:
                if k != "v_idx":
                    assert torch.equal(g[k], h[k]), (i, k)
            ids = g["q_id"].numpy() - 100                                                 # (the record of each row)
            assert g["v_idx"].dtype == torch.int32 and g["v_idx"].tolist() == table.rows[ids].tolist(), i
            assert sorted(ids.tolist()) == sorted(order[i // 3][(i % 3) * B:(i % 3) * B + B].tolist()), i
            v, v_len = ops.gather_regions(ds, g["v_idx"])
            assert _same_bits(v, h["v"]) and torch.equal(v_len, h["v_len"]), (i, "the gather rebuilds the host path's regions")


def test_store_batches_resident_allocates_nothing_of_region_size(stores):
    ds = feed.DeviceFeatureStore(stores["counts"], "cpu")
    B, T = 8, 4
    batches = list(feed.store_batches(None, _qa(), B, 20, resident=ds, pin=False, ring=3))
    slots = {}
    for b in batches:
        for k, t in b.items():
            if k != "q_id":                                            # ('q_id' is made per batch, not a slot tensor)
                slots[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
    per_slot = B * 4 + B * T * 8 + B * 20 * 4                          # 'v_idx' int32, 'q_idxes' int64, 'a' fp32 -- and nothing else
    assert len(slots) == 3 * 3 and sum(slots.values()) == 3 * per_slot, slots
    assert per_slot < B * N * D * 4, "the test's own sizes: a region slot would have been larger than all the others together"
    assert all("v" not in b and "v_packed" not in b and "v_len" not in b for b in batches)


def test_store_batches_resident_refusals(stores):
    ds = feed.DeviceFeatureStore(stores["counts"], "cpu")
    with pytest.raises(ValueError, match="resident"):
        next(feed.store_batches(stores["counts"], _qa(), 8, 20, resident=ds, packed=True, pin=False))
    with pytest.raises(ValueError, match="resident"):
        next(feed.store_batches(stores["counts"], _qa(), 8, 20, resident=ds, region_dtype=BF, pin=False))
    with pytest.raises(IndexError):
        next(feed.store_batches(None, [{"v_idx": N_IMG, "q_idxes": [1], "q_id": 0}], 8, 20, resident=ds, pin=False))


def test_shard_and_collate_carry_v_idx(stores):
    ds = feed.DeviceFeatureStore(stores["counts"], "cpu")
    batch = next(feed.store_batches(None, _qa(), 8, 20, resident=ds, pin=False))
    for rank in (0, 1):
        part = feed.shard(batch, rank, 2)
        assert set(part) == set(batch) and all(torch.equal(part[k], batch[k][rank * 4:rank * 4 + 4]) for k in batch)
    assert feed.shard(batch, 0, 1) is batch
    items = [{"v_idx": i, "q_idxes": [1, 2, 0], "q_id": 7 + i, "a_10_idx": [(i, 1.0)]} for i in (3, 0, 6)]
    got = feed.collate(items, 20)
    assert set(got) == {"v_idx", "q_idxes", "q_id", "a"} and got["v_idx"].dtype == torch.int32 and got["v_idx"].tolist() == [3, 0, 6]
    assert got["a"][2, 6] == 1.0 and got["q_id"].tolist() == [10, 7, 13]
    with pytest.raises(ValueError):
        feed.collate(items, 20, packed=True)


# ---- model, trainer, evaluator -----------------------------------------------------------------------------------------------
def test_an_attached_store_is_no_part_of_the_models_state(stores):
    big = type("Store", (), {"sample_shape": (36, 2048), "counts": None})()
    for model in (CoR2Model(["PAD", "UNK"], 20), ODAModel(["PAD", "UNK"], 20)):
        keys, n_params, n_buffers = set(model.state_dict()), len(list(model.parameters())), len(list(model.buffers()))
        assert model.region_store is None
        assert model.use_region_store(big) is model and model.region_store is big
        assert set(model.state_dict()) == keys and len(list(model.parameters())) == n_params and len(list(model.buffers())) == n_buffers
        assert big not in list(model.modules()) and "region_store" not in model._modules and "region_store" not in model._buffers
        model.use_region_store(None)
        assert model.region_store is None
    small = feed.DeviceFeatureStore(stores["counts"], "cpu")                  # N = 5, D = 8: fits neither model
    with pytest.raises(ValueError, match="does not fit"):
        CoR2Model(["PAD", "UNK"], 20).use_region_store(small)
    with pytest.raises(ValueError, match="does not fit"):
        ODAModel(["PAD", "UNK"], 20, regions=36).use_region_store(type("Store", (), {"sample_shape": (100, 2048), "counts": None})())


def test_v_idx_needs_a_store_and_excludes_the_other_region_keys():
    model = CoR2Model(["PAD", "UNK"], 20)
    idx, q = torch.zeros(2, dtype=torch.int32), torch.zeros(2, 2400)
    with pytest.raises(ValueError, match="use_region_store"):
        model({"v_idx": idx, "q_idxes": q})
    model.use_region_store(type("Store", (), {"sample_shape": (36, 2048), "counts": None})())
    for key, t in (("v", torch.zeros(2, 36, 2048)), ("v_packed", torch.zeros(72, 2048)), ("v_len", torch.ones(2, dtype=torch.int32))):
        with pytest.raises(ValueError, match="not both"):
            model({"v_idx": idx, key: t, "q_idxes": q})
    oda = ODAModel(["PAD", "UNK"], 20)
    oda.use_region_store(type("Store", (), {"sample_shape": (36, 2048), "counts": torch.ones(3, dtype=torch.int32)})())
    with pytest.raises(ValueError, match="region_counts=True"):
        oda({"v_idx": idx, "q_idxes": q})


def test_model_keys_of_trainer_and_evaluator():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    t = torch.zeros(1)
    batch = {"v_idx": t, "q_idxes": t, "q_id": t, "a": t}
    assert DataParallelTrainer._model_keys(batch) == {"v_idx", "q_idxes"}
    assert set(Evaluator._model_keys(batch)) == {"v_idx", "q_idxes"} and len(Evaluator._model_keys(batch)) == 2
    assert DataParallelTrainer._model_keys({"v_idx": t, "q": t}) == {"v_idx", "q"}
    assert DataParallelTrainer._model_keys({"v": t, "q_idxes": t, "v_len": t}) == {"v", "q_idxes", "v_len"}        # as before
    assert set(Evaluator._model_keys({"v_packed": t, "q_idxes": t, "v_len": t})) == {"v_packed", "q_idxes", "v_len"}
