"""Packed (ragged) region batches, the parts that need no GPU: the ragged FeatureStore and the packed gather (native and numpy,
fp32 and bf16), store_batches / collate / shard with packed=True against their padded forms, the refusals, ops.unpack_regions on
CPU tensors against a numpy restatement of the format, and the new entry points in the header, the binding and the library.
Every comparison is exact: the feature copies, it computes nothing.  The kernel, the models, the trainer, the prefetcher's copies
and the evaluator are tests/test_gpu_packed_regions.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from kernel_harness import forbid_launches
from vqa_playground_pytorch_amd import CoR2Model, ODAModel, _lib, feed, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -12345.0


def unpack_np(packed, lens, N):
    """the format, restated: sample b's rows are packed[off[b] : off[b] + lens[b]], off the exclusive prefix sum; zeros behind"""
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    out = np.zeros((len(lens), N) + packed.shape[1:], dtype=packed.dtype)
    for b, (o, n) in enumerate(zip(off, lens)):
        out[b, :n] = packed[o:o + n]
    return out


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _stores(tmp_path, N, D, n_img=9, seed=0):
    """a random padded store with counts (1 and N among them, padding zeroed) and the ragged store that holds the same rows"""
    rs = np.random.RandomState(seed)
    feats = rs.standard_normal((n_img, N, D)).astype(np.float32)
    cnt = rs.randint(1, N + 1, n_img)
    cnt[1], cnt[n_img - 2] = 1, N
    for i, c in enumerate(cnt):
        feats[i, c:] = 0.0
    rows = np.concatenate([feats[i, :c] for i, c in enumerate(cnt)])
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    np.save(tmp_path / "padded.npy", feats)
    np.save(tmp_path / "rows.npy", rows)
    np.save(tmp_path / "offsets.npy", offsets)
    padded = feed.FeatureStore(tmp_path / "padded.npy", workers=3, counts=cnt)
    ragged = feed.FeatureStore(tmp_path / "rows.npy", workers=3, offsets=tmp_path / "offsets.npy", regions=N)
    return padded, ragged, feats, cnt


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_bound_and_exported():
    with open(os.path.join(ROOT, "include", "vqa_mi355x.h"), encoding="utf-8") as fh:
        header = fh.read()
    L = _lib.lib()
    for name, nargs in (("vqa_unpack_regions", 9), ("vqa_unpack_regions_supported", 5), ("vqa_host_gather_ragged", 14)):
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(L, name), name
    assert L.vqa_version() == 14 == _lib.ABI_VERSION
    assert "#define VQA_ABI_VERSION 14" in header
    assert L.vqa_unpack_regions_supported(128, 100, 2048, 1, 0) == 1
    assert L.vqa_unpack_regions_supported(128, 100, 12, 0, 0) == 0          # D % 8
    assert L.vqa_unpack_regions_supported(128, 100, 2048, 0, 1) == 0        # fp32 rows are not narrowed
    assert L.vqa_unpack_regions(None, None, None, 2, 3, 8, 0, 0, None) == -1 and b"null pointer" in L.vqa_last_error()
    with open(os.path.join(ROOT, "vqa_playground_pytorch_amd", "csrc", "Makefile"), encoding="utf-8") as fh:
        assert "region_unpack.hip" in fh.read()


# ---- gathers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,D", [(5, 8), (5, 2048), (36, 8), (36, 2048)])
def test_gather_packed_unpacks_to_the_padded_gather(tmp_path, N, D, dtype):
    padded, ragged, feats, cnt = _stores(tmp_path, N, D)
    idx = [8, 1, 7, 7, 0, 3, 1]                     # images 1 (one row) and 7 (N rows) among them, a repeat
    want = padded.gather(idx, torch.empty(len(idx), N, D, dtype=dtype))          # (the store is zero-padded)
    R = int(cnt[idx].sum())
    results = []
    for store in (ragged, padded):
        for native in (True, False):
            out = torch.full((len(idx) * N + 3, D), SENT, dtype=dtype)
            v_len = torch.full((len(idx) + 2,), -7, dtype=torch.int32)
            assert store.gather_packed(idx, out, v_len, native=native) == R
            assert v_len[:len(idx)].tolist() == cnt[idx].tolist() and v_len[len(idx):].tolist() == [-7, -7]
            assert torch.equal(_bits(out[R:]), _bits(torch.full_like(out[R:], SENT))), "rows from R on were written"
            got = unpack_np(out[:R].view(torch.int16 if dtype == torch.bfloat16 else torch.int32).numpy(), cnt[idx], N)
            assert np.array_equal(got, _bits(want).numpy()), (store.ragged, native)
            results.append(_bits(out).clone())
    assert all(torch.equal(results[0], r) for r in results[1:]), "native and numpy, ragged and padded: the same bytes"


def test_gather_packed_with_one_worker_and_an_exact_capacity(tmp_path):
    _, ragged, feats, cnt = _stores(tmp_path, 5, 8)
    one = feed.FeatureStore(tmp_path / "rows.npy", workers=1, offsets=np.load(tmp_path / "offsets.npy"), regions=5)
    assert len(one) == 9 and one.sample_shape == (5, 8) and one.counts.tolist() == cnt.tolist()
    idx = list(range(9))
    out, v_len = torch.empty(int(cnt.sum()), 8), torch.empty(9, dtype=torch.int32)
    assert one.gather_packed(idx, out, v_len) == int(cnt.sum())
    assert np.array_equal(unpack_np(out.numpy(), cnt, 5), feats)


# ---- store_batches, collate, shard -------------------------------------------------------------------------------------------
def _qa(n_img, n=23):
    return [{"v_idx": (5 * i + 2) % n_img, "q_idxes": [i, 1, 0], "q_id": i,
             "a_10_idx": [((i * 7) % 20, 0.75), ((i * 7 + 1) % 20, 0.25)]} for i in range(n)]


def _same_batch(packed, padded, N):
    assert "v" not in packed and packed["v_packed"].shape == (padded["v"].size(0) * N, padded["v"].size(2))
    assert packed["v_packed"].dtype == padded["v"].dtype
    for k in padded:
        if k != "v":
            assert torch.equal(packed[k], padded[k]) and packed[k].dtype == padded[k].dtype, k
    assert set(packed) == set(padded) - {"v"} | {"v_packed"}
    R = int(packed["v_len"].sum())
    unpacked = unpack_np(_bits(packed["v_packed"][:R]).numpy(), packed["v_len"].numpy(), N)
    assert np.array_equal(unpacked, _bits(padded["v"]).numpy())
    assert torch.equal(_bits(ops.unpack_regions(packed["v_packed"], packed["v_len"], packed["v_len"].numel())), _bits(padded["v"]))


@pytest.mark.parametrize("answers", ["dense", "sparse"])
@pytest.mark.parametrize("kw", [dict(), dict(shuffle=True, seed=4), dict(shuffle=True, seed=2, ring=5, prefetch=2, producers=2),
                                dict(region_dtype=torch.bfloat16)], ids=["plain", "shuffle", "prefetch-producers", "bf16"])
def test_store_batches_packed_equal_the_padded_batches(tmp_path, kw, answers):
    """23 records in batches of 4: five full batches and a short one of 3, from the ragged store and from the padded one"""
    N = 5
    padded, ragged, _, _ = _stores(tmp_path, N, 8)
    qa = _qa(len(padded))
    want = [{k: t.clone() for k, t in b.items()} for b in feed.store_batches(padded, qa, 4, 20, pin=False, answers=answers, **kw)]
    assert [b["v"].size(0) for b in want] == [4, 4, 4, 4, 4, 3]
    for store in (ragged, padded):
        got = [{k: t.clone() for k, t in b.items()}
               for b in feed.store_batches(store, qa, 4, 20, pin=False, answers=answers, packed=True, **kw)]
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _same_batch(g, w, N)
    # through the prefetcher on the CPU: passed through as they are
    got = list(feed.DevicePrefetcher(feed.store_batches(ragged, qa, 4, 20, pin=False, answers=answers, packed=True, ring=4, **{
        k: v for k, v in kw.items() if k != "ring"}), "cpu", depth=2))
    _same_batch(got[-1], want[-1], N)


def test_collate_packed_equals_the_padded_collate():
    rs = np.random.RandomState(1)
    N, D = 5, 8
    lens = [1, 5, 3, 2, 5, 4]
    items = []
    for i, n in enumerate(lens):
        v = rs.standard_normal((N, D)).astype(np.float32)
        v[n:] = 0.0
        items.append({"v": v, "v_len": n, "q_idxes": [1, 2, 0], "q_id": i, "a_10_idx": [(i, 1.0)]})
    want = feed.collate(items, 20)
    _same_batch(feed.collate(items, 20, packed=True), want, N)                                   # padded 'v' + 'v_len'
    ragged = [{k: (x[:it["v_len"]] if k == "v" else x) for k, x in it.items() if k != "v_len"} for it in items]
    _same_batch(feed.collate(ragged, 20, packed=True, regions=N), want, N)                       # ragged 'v' [n_i, D]
    _same_batch(feed.collate(ragged, 20, packed=True, regions=N, answers="sparse"), feed.collate(items, 20, answers="sparse"), N)
    with pytest.raises(ValueError):
        feed.collate(ragged, 20, packed=True)                       # ragged items without N
    with pytest.raises(ValueError):
        feed.collate(ragged, 20, packed=True, regions=4)            # an item with 5 rows
    with pytest.raises(ValueError):
        feed.collate([dict(items[0], v_len=0)], 20, packed=True)


@pytest.mark.parametrize("world", [2, 4])
def test_shard_of_a_packed_batch(tmp_path, world):
    N = 5
    padded, ragged, _, _ = _stores(tmp_path, N, 8)
    qa = _qa(len(padded), 8)
    whole = next(iter(feed.store_batches(padded, qa, 8, 20, pin=False)))
    packed = next(iter(feed.store_batches(ragged, qa, 8, 20, pin=False, packed=True)))
    assert feed.shard(packed, 0, 1) is packed
    for r in range(world):
        part, want = feed.shard(packed, r, world), feed.shard(whole, r, world)
        assert part["v_packed"].size(0) == (8 // world) * N
        assert part["v_packed"].data_ptr() == packed["v_packed"].data_ptr() + int(packed["v_len"][:r * 8 // world].sum()) * 8 * 4
        _same_batch(part, want, N)


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_ragged_store_refusals(tmp_path):
    _, ragged, _, cnt = _stores(tmp_path, 5, 8)
    rows, off = tmp_path / "rows.npy", np.load(tmp_path / "offsets.npy")
    swapped = off.copy()
    swapped[3], swapped[4] = off[4], off[3]
    zero = off.copy()
    zero[2] = zero[1]                                     # image 1 without a row
    for bad, regions in ((swapped, 5), (zero, 5), (off, 4), (off[:-1], 5), (off + 1, 5), (off.astype(np.float32), 5), (off, None)):
        with pytest.raises(ValueError):
            feed.FeatureStore(rows, offsets=bad, regions=regions)
    short = off.copy()
    short[-1] -= 1                                        # offsets[-1] != the row count
    with pytest.raises(ValueError):
        feed.FeatureStore(rows, offsets=short, regions=5)
    with pytest.raises(ValueError):
        feed.FeatureStore(rows, offsets=off, regions=5, counts=cnt)
    with pytest.raises(ValueError):
        feed.FeatureStore(tmp_path / "padded.npy", offsets=off, regions=5)          # a [n_img, N, D] array with offsets
    with pytest.raises(ValueError):
        ragged.gather([0], torch.empty(1, 5, 8))
    with pytest.raises(ValueError):
        next(iter(feed.store_batches(ragged, _qa(9), 4, 20, pin=False)))
    plain = feed.FeatureStore(tmp_path / "padded.npy")
    with pytest.raises(ValueError):
        next(iter(feed.store_batches(plain, _qa(9), 4, 20, pin=False, packed=True)))


@pytest.mark.parametrize("native", [True, False])
def test_gather_packed_checks_before_it_copies(tmp_path, native):
    _, ragged, _, cnt = _stores(tmp_path, 5, 8)
    out, v_len = torch.full((10, 8), SENT), torch.zeros(4, dtype=torch.int32)
    for bad in ([0, 9], [-1]):
        with pytest.raises(IndexError):
            ragged.gather_packed(bad, out, v_len, native=native)
    idx = [7, 7, 7]                                        # 15 rows into 10
    with pytest.raises(ValueError):
        ragged.gather_packed(idx, out, v_len, native=native)
    with pytest.raises(ValueError):
        ragged.gather_packed([0], torch.empty(10, 9), v_len, native=native)
    with pytest.raises(ValueError):
        ragged.gather_packed([0, 1, 2, 3, 4], out, v_len, native=native)            # v_len_out too short
    assert bool((out == SENT).all()) and not v_len.any()


def test_the_native_gather_checks_its_own_arguments(tmp_path):
    """the C entry point is pointer arithmetic over what it is given: it range-checks all of it itself, before the first byte"""
    L = _lib.lib()
    rows = np.arange(6 * 8, dtype=np.float32).reshape(6, 8)
    starts, counts = np.array([0, 2, 5], np.int64), np.array([2, 3, 1], np.int32)
    out, v_len, total = np.full((4, 8), SENT, np.float32), np.zeros(3, np.int32), ctypes.c_long(-1)

    def call(starts=starts, counts=counts, idx=(0, 1), cap=4, store_rows=6):
        idx = np.asarray(idx, np.int64)
        return L.vqa_host_gather_ragged(rows.ctypes.data, store_rows, 8, starts.ctypes.data, counts.ctypes.data, 3, idx.ctypes.data,
                                        idx.size, out.ctypes.data, cap, v_len.ctypes.data, ctypes.addressof(total), 0, 2)
    assert call(idx=(0, 3)) == -1 and call(idx=(-1,)) == -1                        # an index outside the store
    assert call(idx=(0, 1, 2)) == -1                                               # R = 6 above the capacity of 4
    assert call(starts=np.array([0, 4, 5], np.int64)) == -1                        # rows 4 .. 7 of a store of 6
    assert call(starts=np.array([-1, 2, 5], np.int64)) == -1
    assert call(counts=np.array([2, -3, 1], np.int32)) == -1
    assert call(store_rows=4) == -1
    assert (out == SENT).all() and total.value == -1
    assert L.vqa_host_gather_ragged(None, 6, 8, None, None, 3, None, 0, None, 4, None, None, 0, 2) == -1
    assert call(idx=(2, 0)) == 0 and total.value == 3 and v_len.tolist() == [1, 2, 0]
    assert np.array_equal(out[:3], rows[[5, 0, 1]]) and (out[3] == SENT).all()


def _packed_sample(B=3, regions=36):
    return {"v_packed": torch.zeros(B * regions, 2048), "v_len": torch.full((B,), 2, dtype=torch.int32), "q_idxes": torch.zeros(B, 2400)}


def test_models_refuse_malformed_packed_batches_before_anything_runs(monkeypatch):
    forbid_launches(monkeypatch, ops)
    model = CoR2Model(["PAD", "UNK"], 50).eval()
    monkeypatch.setattr(model.compress_v, "forward", lambda *a, **k: pytest.fail("a layer ran"))
    s = _packed_sample()
    with pytest.raises(ValueError, match="not both"):
        model(dict(s, v=torch.zeros(3, 36, 2048)))
    with pytest.raises(ValueError, match="v_len"):
        model({k: t for k, t in s.items() if k != "v_len"})
    with pytest.raises(ValueError, match="1..36"):
        model(dict(s, v_len=torch.tensor([36, 37, 1], dtype=torch.int32)))
    with pytest.raises(ValueError, match="v_packed"):
        model(dict(s, v_packed=torch.zeros(3 * 36 + 1, 2048)))                      # not B * N rows
    with pytest.raises(ValueError, match="v_packed"):
        model(dict(s, v_packed=torch.zeros(3, 36, 2048)))                           # not [B*N, D]
    oda = ODAModel(["PAD", "UNK"], 50).eval()
    with pytest.raises(ValueError, match="region_counts=True"):
        oda(s)
    with pytest.raises(ValueError, match="region_counts=True"):
        oda({k: t for k, t in s.items() if k != "v_len"})
    for bad in (dict(s, v=torch.zeros(3, 36, 2048)), {k: t for k, t in s.items() if k != "v_len"}):
        with pytest.raises(ValueError):
            feed.shard(bad, 0, 2)


def test_trainer_and_evaluator_count_v_packed_among_the_model_inputs():
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    s = dict(_packed_sample(), a=None, q_id=None)
    assert DataParallelTrainer._model_keys(s) == {"v_packed", "q_idxes", "v_len"}
    assert tuple(Evaluator._model_keys(s)) == ("v_packed", "q_idxes", "v_len")


# ---- ops.unpack_regions on the CPU -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,D", [(1, 1, 8), (2, 36, 8), (7, 5, 16), (65, 3, 8)])
def test_unpack_regions_on_cpu_tensors_is_the_numpy_restatement(B, N, D):
    rs = np.random.RandomState(B * 100 + N)
    for lens in (np.full(B, N), np.ones(B, np.int64), rs.randint(1, N + 1, B)):
        R = int(lens.sum())
        packed = np.full((B * N, D), np.nan, np.float32)               # rows from R on: never read, so no NaN comes out
        packed[:R] = rs.standard_normal((R, D))
        want = unpack_np(packed[:R], lens, N)
        v_len = torch.from_numpy(lens.astype(np.int32))
        got = ops.unpack_regions(torch.from_numpy(packed), v_len, B)
        assert got.dtype == torch.float32 and np.array_equal(got.numpy().view(np.int32), want.view(np.int32))
        half = torch.from_numpy(packed).to(torch.bfloat16)
        want_bf = torch.from_numpy(want).to(torch.bfloat16)
        assert torch.equal(_bits(ops.unpack_regions(half, v_len, B)), _bits(want_bf))
        assert torch.equal(_bits(ops.unpack_regions(half, v_len, B, torch.float32)), _bits(want_bf.float()))
    with pytest.raises(ValueError):
        ops.unpack_regions(torch.zeros(B * N, D), v_len, B, torch.bfloat16)        # fp32 rows are not narrowed here
    with pytest.raises(ValueError):
        ops.unpack_regions(torch.zeros(2 * N + 1, D), torch.ones(2, dtype=torch.int32), 2)      # not 2 * N rows
    with pytest.raises(ValueError):
        ops.unpack_regions(torch.zeros(B * N, D), v_len.long(), B)
