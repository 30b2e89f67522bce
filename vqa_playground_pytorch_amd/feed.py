"""Host -> device feed for the hot path: the sample wire format of the reference's loader (datasets.py:893-977) and an
asynchronous, double-buffered H2D prefetcher.

The reference yields dict batches ``{'v' [B,36,2048] fp32, 'q_idxes' [B,26] int64 (0 = PAD, left aligned), 'q_id',
'a' [B,num_ans] fp32 soft targets}`` from a ``DataLoader(pin_memory=True)`` (datasets.py:975-977) and moves them to the
GPU synchronously inside the step (train.py:54-57).  At 100 k samples/s the 151 MB of region features per 512-sample
batch is the next bottleneck (PCIe Gen5 x16: ~2.5-3 ms per batch), so here the copy of batch t+1 runs on its own HIP
stream from pinned staging buffers while batch t trains.

`FeatureStore` + `store_batches` are the part in front of that: the reference keeps the region features of ALL images in one
HDF5 file (`size,rcnn_arch,224.hy`, dataset 'att' [n_img,36,2048] float32, datasets.py:367,405-412) next to a text file with one
image file name per row (`.txt`, utils.py:452-454; row i names feature i, datasets.py:570-571) and indexes it per sample
(`outer.data['img']['feature'][visual_index]`, datasets.py:912-913).  h5py is not part of this image, so the store here is the
SAME array as a raw `.npy` file opened with numpy.memmap (tools/hy_to_npy.py converts wherever h5py exists; a contiguous HDF5
dataset is this byte range already, `FeatureStore(..., offset=)` opens it in place when the offset is known): a batch is
gathered row by row straight into a pinned staging buffer, in a few threads (one memcpy stream tops out near 10 GB/s, a
512-sample batch is 151 MB), and handed to `DevicePrefetcher`.
"""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch


def soft_target(a_10_idx, num_ans, out=None):
    """datasets.py:963-969: dense soft-answer vector; ``a_10_idx`` = [(answer id, probability), ...]."""
    a = out if out is not None else torch.zeros(num_ans, dtype=torch.float32)
    a.zero_()
    for c_id, c_prob in a_10_idx:
        a[c_id] = c_prob
    return a


MC_CANDIDATES = 50
MAX_PAIRS = 16         # (answer id, probability) pairs per question a sparse answer target holds (the loss kernels' limit)


def _check_answers(answers):
    if answers not in ("dense", "sparse"):
        raise ValueError("answers=%r: 'dense' or 'sparse'" % (answers,))
    return answers == "sparse"


def _pair_width(most):
    """K of a sparse answer target whose longest pair list has `most` entries."""
    if most > MAX_PAIRS:
        raise ValueError("a question with %d (answer id, probability) pairs: a sparse answer target holds at most %d" % (most, MAX_PAIRS))
    return max(1, int(most))


def _check_count(count, regions, what):
    if not 1 <= count <= regions:
        raise ValueError("%s: region count %d outside 1..%d" % (what, count, regions))
    return count


def _check_packed_keys(batch):
    if "v_packed" in batch:
        if "v" in batch:
            raise ValueError("a batch carries its regions padded ('v') or packed ('v_packed'), not both")
        if "v_len" not in batch:
            raise ValueError("'v_packed' needs 'v_len': the region counts are what delimits the samples' rows")


def collate(items, num_ans, pin=False, answers="dense", packed=False, regions=None):
    """List of reference-style items {'v' [36,2048], 'q_idxes' [T], 'q_id', 'a_10_idx' or 'a', optionally 'a_mc_idx', optionally
    'v_len' = the number of real (not padding) rows of 'v'} -> one batch dict of
    contiguous host tensors (optionally pinned), the layout Model.forward and the trainer expect.  answers="sparse": instead of the
    dense 'a' [B,num_ans] the pairs of 'a_10_idx' as they are, in record order -- 'a_idx' int32 [B,K] and 'a_val' float32 [B,K], K the
    batch's largest pair count, shorter rows padded with -1 / 0 (ops.densify defines the format; the trainer takes the two keys).
    packed=True: a packed region batch -- 'v_packed' [B*N, D] (the items' real rows back to back in a capacity-sized buffer, the
    rest left unwritten) and 'v_len' instead of 'v'.  The items carry ragged 'v' [n_i, D] (then `regions` = N is given), or padded
    'v' [N, D] plus 'v_len' (N from the shape unless given).
    Items for a device-resident store (DeviceFeatureStore) carry 'v_idx', their image's index, and no 'v': the batch then holds
    'v_idx' int32 [B] and no region tensor (this is the one place that key needs a case of its own: it stands where 'v' is built)."""
    sparse = _check_answers(answers)
    B = len(items)
    resident = "v" not in items[0] and "v_idx" in items[0]
    if resident and packed:
        raise ValueError("collate: items with 'v_idx' and no 'v' name rows of a resident store; packed=True does not apply")
    v0 = torch.as_tensor(items[0]["v"]) if not resident else None
    mk = (lambda *s, dtype: torch.empty(*s, dtype=dtype).pin_memory()) if pin else (lambda *s, dtype: torch.empty(*s, dtype=dtype))
    if resident:
        regions_part = {"v_idx": mk(B, dtype=torch.int32)}
        for i, it in enumerate(items):
            regions_part["v_idx"][i] = int(it["v_idx"])
    elif packed:
        if regions is None and "v_len" not in items[0]:
            raise ValueError("collate(packed=True): ragged items need regions= (the capacity N per sample)")
        N = int(v0.shape[0] if regions is None else regions)
        lens = [_check_count(int(it["v_len"]) if "v_len" in it else int(torch.as_tensor(it["v"]).shape[0]), N, "item %d" % i)
                for i, it in enumerate(items)]
        regions_part = {"v_packed": mk(B * N, v0.shape[1], dtype=torch.float32)}
    else:
        regions_part = {"v": mk(B, *v0.shape, dtype=torch.float32)}
    batch = {**regions_part,
             "q_idxes": mk(B, len(items[0]["q_idxes"]), dtype=torch.long),
             "q_id": torch.tensor([int(it.get("q_id", i)) for i, it in enumerate(items)], dtype=torch.long)}
    has_a = "a" in items[0] or "a_10_idx" in items[0]
    if sparse and has_a:
        if any("a_10_idx" not in it for it in items):
            raise ValueError("answers='sparse' needs every item's 'a_10_idx' pairs: a dense 'a' cannot be served sparse")
        K = _pair_width(max(len(it["a_10_idx"]) for it in items))
        batch["a_idx"], batch["a_val"] = mk(B, K, dtype=torch.int32), mk(B, K, dtype=torch.float32)
        batch["a_idx"].fill_(-1)
        batch["a_val"].zero_()
        for i, it in enumerate(items):
            for j, (c_id, c_prob) in enumerate(it["a_10_idx"]):
                if not 0 <= int(c_id) < num_ans:
                    raise IndexError("collate: answer id outside [0, %d)" % num_ans)
                batch["a_idx"][i, j], batch["a_val"][i, j] = int(c_id), float(c_prob)
        has_a = False
    if has_a:
        batch["a"] = mk(B, num_ans, dtype=torch.float32)
    if "a_mc_idx" in items[0]:
        # MultipleChoice candidates, padded with -1 to MC_CANDIDATES per question (datasets.py:948)
        batch["a_mc_idx"] = torch.full((B, MC_CANDIDATES), -1, dtype=torch.long)
        for i, it in enumerate(items):
            mc = torch.as_tensor(it["a_mc_idx"], dtype=torch.long).reshape(-1)
            if mc.numel() > MC_CANDIDATES:
                raise ValueError("item %d has %d multiple-choice candidates, more than %d" % (i, mc.numel(), MC_CANDIDATES))
            batch["a_mc_idx"][i, :mc.numel()] = mc
    if packed:
        batch["v_len"] = mk(B, dtype=torch.int32)
        off = 0
        for i, (it, n) in enumerate(zip(items, lens)):
            v = torch.as_tensor(it["v"], dtype=torch.float32)
            if v.shape[0] < n or v.shape[1:] != v0.shape[1:]:
                raise ValueError("item %d: 'v' %s does not hold %d rows of %d" % (i, tuple(v.shape), n, v0.shape[1]))
            batch["v_packed"][off:off + n].copy_(v[:n])
            batch["v_len"][i] = n
            off += n
    elif "v_len" in items[0] and not resident:
        # per-item region counts (adaptive features padded to the store's N): int32 [B], what cor2.Model reads as sample['v_len']
        batch["v_len"] = mk(B, dtype=torch.int32)
        for i, it in enumerate(items):
            batch["v_len"][i] = _check_count(int(it["v_len"]), v0.shape[0], "item %d" % i)
    for i, it in enumerate(items):
        if not packed and not resident:
            batch["v"][i].copy_(torch.as_tensor(it["v"], dtype=torch.float32))
        batch["q_idxes"][i].copy_(torch.as_tensor(it["q_idxes"], dtype=torch.long))
        if has_a:
            if "a" in it:
                batch["a"][i].copy_(torch.as_tensor(it["a"], dtype=torch.float32))
            else:
                soft_target(it["a_10_idx"], num_ans, out=batch["a"][i])
    return batch


def shard(batch, rank, world):
    """Rank r's contiguous slice [r*B/P, (r+1)*B/P) of every tensor of a global batch (SURVEY 8e partitioning).  A packed batch
    ('v_packed' + 'v_len'): the rank's samples start at row off[r*B/P] of the global buffer (off = the exclusive prefix sum of
    'v_len') and its 'v_packed' is the view of (B/P)*N rows from there -- a capacity again, of which the rank's own sum of counts
    is meaningful; it cannot run past the global buffer, since off[b] <= b*N.  (DataParallelTrainer.shard is per tensor and
    cannot do this: packed batches are sharded here.)  'v_idx' of a resident-store batch is a dim-0 tensor like 'q_idxes' and is
    sliced like it: no case of its own."""
    _check_packed_keys(batch)
    if world == 1:
        return batch
    out = {}
    for k, t in batch.items():
        if k == "v_packed":
            B = batch["v_len"].size(0)
            per, N = B // world, t.size(0) // B
            start = int(batch["v_len"][:rank * per].sum())
            out[k] = t[start:start + per * N]
            continue
        per = t.size(0) // world
        out[k] = t[rank * per:(rank + 1) * per]
    return out


class DevicePrefetcher:
    """Iterates device-resident batches; the H2D copies of the next batch overlap the consumer's work on the current
    one.  ``depth`` staging slots are allocated once in pinned host memory and once on the device (no per-batch
    allocation), copies run on a dedicated stream, and each yielded batch is handed to the consumer's stream with an
    event wait -- the consumer never blocks the host.  A resident-store batch ('v_idx' int32 [B] instead of region rows,
    store_batches(resident=)) needs no case here: the key is staged and copied like 'q_idxes', 4 bytes per sample."""

    def __init__(self, batches, device, depth=2):
        self.it = iter(batches)
        self.device = torch.device(device)
        self.depth = depth
        self.cuda = self.device.type == "cuda"
        self.stream = torch.cuda.Stream(self.device) if self.cuda else None
        self.slots = []          # [{'host': {...}, 'dev': {...}, 'ready': Event, 'free': Event}]
        self.queue = []
        self.n = 0

    def _slot(self, batch):
        if len(self.slots) < self.depth:
            s = {"host": {},   # pinned staging, allocated lazily and only for sources that are not page-locked
                 "dev": {k: torch.empty_like(t, device=self.device) for k, t in batch.items()} if self.cuda else None,
                 "ready": torch.cuda.Event() if self.cuda else None,
                 "free": torch.cuda.Event() if self.cuda else None}
            self.slots.append(s)
            return s
        s = self.slots[self.n % self.depth]
        if self.cuda:
            s["free"].synchronize()      # the consumer finished with this slot's previous batch
        return s

    def _issue(self):
        try:
            batch = next(self.it)
        except StopIteration:
            return False
        if not self.cuda:
            self.queue.append((None, batch))
            return True
        s = self._slot(batch)
        self.n += 1
        # The slots are sized by the first batch.  The reference's DataLoader has no drop_last (datasets.py:975), so the
        # last batch of an epoch is shorter: it is staged into / yielded as the leading rows of the slot buffers (a plain
        # copy_ would raise on the size mismatch -- or, for a remainder of ONE sample, silently broadcast it).
        # A packed batch's 'v_packed' is a capacity buffer of which the first R = sum(v_len) rows mean something: only those are
        # staged and copied (R from the host-side 'v_len', in hand here) -- the padding never crosses the bus; the device slot is
        # allocated at capacity and yielded whole (what lies behind row R there is never read).
        _check_packed_keys(batch)
        live = int(batch["v_len"].sum()) if "v_packed" in batch else None
        if live is not None and live > batch["v_packed"].size(0):
            raise ValueError("prefetcher: 'v_len' sums to %d rows, 'v_packed' holds %d" % (live, batch["v_packed"].size(0)))
        src, dev, copies = {}, {}, {}
        for k, t in batch.items():
            full = s["dev"][k]
            if t.shape[1:] != full.shape[1:] or t.dtype != full.dtype or t.size(0) > full.size(0):
                full = s["dev"][k] = torch.empty_like(t, device=self.device)      # a larger / differently shaped batch
                s["host"].pop(k, None)
            b = t.size(0)
            if t.is_pinned():
                src[k] = t                              # already page-locked (DataLoader(pin_memory=True)): DMA from it
            else:
                if k not in s["host"] or s["host"][k].shape[1:] != t.shape[1:] or s["host"][k].size(0) < b:
                    s["host"][k] = torch.empty_like(t).pin_memory()
                stage = s["host"][k].narrow(0, 0, b)
                rows = b if k != "v_packed" else live
                stage.narrow(0, 0, rows).copy_(t.narrow(0, 0, rows))     # pageable -> pinned staging slot (a host memcpy: ~10 GB/s)
                src[k] = stage
            dev[k] = full.narrow(0, 0, b) if b != full.size(0) else full
            copies[k] = (dev[k], src[k]) if k != "v_packed" else (dev[k].narrow(0, 0, live), src[k].narrow(0, 0, live))
        with torch.cuda.stream(self.stream):
            for k in batch:
                if dev[k].shape != src[k].shape:
                    raise RuntimeError("prefetcher: staging shape %s does not match the batch %s"
                                       % (tuple(dev[k].shape), tuple(src[k].shape)))
                self._copy(k, *copies[k])
            s["ready"].record(self.stream)
        self.queue.append((s, dev))
        return True

    def _copy(self, key, dst, src):
        """one host -> device copy of a batch entry, on the copy stream (the views say how many bytes cross the bus)"""
        dst.copy_(src, non_blocking=True)

    def __iter__(self):
        for _ in range(self.depth):
            if not self._issue():
                break
        while self.queue:
            s, dev = self.queue.pop(0)
            if s is not None:
                torch.cuda.current_stream(self.device).wait_event(s["ready"])
            yield dev
            if s is not None:
                s["free"].record(torch.cuda.current_stream(self.device))
            self._issue()


class FeatureStore:
    """The reference's region-feature store (datasets.py:367,405-412: dataset 'att' [n_img,N,D] float32 of the `.hy` file; row i
    belongs to the image named on line i of the `.txt` beside it, datasets.py:570-571) as a read-only memory map.

    path: a `.npy` file holding the array (numpy.load(mmap_mode="r")), or any file that holds it as one contiguous float32 block
    at byte `offset` with `shape` given (a contiguous HDF5 dataset, a raw dump).  names: the `.txt` path or a list of image file
    names; `name_to_idx` is the reference's dict of the same name.  gather(indices, out) copies rows into `out` (a pinned host
    tensor [B,N,D] fp32, or bf16 -- then the rows are rounded on the way, half the PCIe bytes for the bf16 path) with `workers`
    threads; nothing is read until a row is asked for (the file stays on disk / in the page cache, like the reference's
    h5py handle with load_mem=None, datasets.py:565-566).  counts: the images' region counts (1..N each, ValueError otherwise) for a
    store of zero-padded adaptive features; store_batches then serves them as 'v_len'.

    offsets: the RAGGED store, the form adaptive features usually come in -- `path` then holds [total_rows, D] float32, the images'
    rows back to back with no padding, and offsets (a `.npy` path or an array) n_img + 1 non-decreasing int64 values with
    offsets[-1] == total_rows: image i owns rows offsets[i] .. offsets[i+1].  regions= gives N, the most rows an image may have
    (every count must lie in 1..N); counts are the differences of offsets, sample_shape stays (N, D) and len() is the image count.
    Such a store serves packed batches (gather_packed, store_batches(packed=True)); so does a padded store with counts=, whose
    gather then takes the first `count` rows of every image."""

    def __init__(self, path, names=None, shape=None, offset=0, workers=4, counts=None, offsets=None, regions=None):
        if shape is None:
            self.features = np.load(path, mmap_mode="r")
        else:
            self.features = np.memmap(path, dtype=np.float32, mode="r", offset=int(offset), shape=tuple(int(x) for x in shape))
        self.ragged = offsets is not None
        if self.ragged:
            counts = self._open_ragged(path, offsets, regions, counts)
        elif self.features.ndim != 3 or self.features.dtype != np.float32:
            raise ValueError("feature store %s: expected a float32 [n_img, regions, dim] array, got %s %s"
                             % (path, self.features.dtype, self.features.shape))
        else:
            self._n_img, self._sample_shape = self.features.shape[0], tuple(self.features.shape[1:])
            self._starts = None        # (a padded store's row starts, i * N: built when it first serves a packed batch)
        if isinstance(names, (str, os.PathLike)):
            with open(names, encoding="utf-8") as fh:                          # utils.file2data(..., 'txt'): utils.py:452-454
                names = fh.read().split("\n")[:-1]
        self.idx_to_name = list(names) if names is not None else None
        self.name_to_idx = {n: i for i, n in enumerate(self.idx_to_name)} if names is not None else None
        if self.idx_to_name is not None and len(self.idx_to_name) != self._n_img:
            raise ValueError("feature store %s: %d names for %d feature rows" % (path, len(self.idx_to_name), self._n_img))
        # counts (optional): a `.npy` path or an array of [n_img] integers, the number of real regions of every image (adaptive
        # bottom-up features: 10..100 boxes).  The rows beyond an image's count are handed out as the file holds them, so the
        # store must be ZERO-PADDED there (the models only ask for finite values; zeros are the contract).
        self.counts = None
        if counts is not None:
            c = np.load(counts) if isinstance(counts, (str, os.PathLike)) else np.asarray(counts)
            if c.ndim != 1 or c.shape[0] != self._n_img or not np.issubdtype(c.dtype, np.integer):
                raise ValueError("feature store %s: counts must be %d integers, got %s %s" % (path, self._n_img, c.dtype, c.shape))
            if c.size and (c.min() < 1 or c.max() > self._sample_shape[0]):
                raise ValueError("feature store %s: region counts %d..%d outside 1..%d"
                                 % (path, int(c.min()), int(c.max()), self._sample_shape[0]))
            self.counts = np.ascontiguousarray(c.astype(np.int32))
        self.workers = max(1, int(workers))
        self._pool = ThreadPoolExecutor(self.workers) if self.workers > 1 else None
        self._lock = threading.Lock()

    def _open_ragged(self, path, offsets, regions, counts):
        """checks of the ragged form -> the counts (the differences of offsets)"""
        if counts is not None:
            raise ValueError("feature store %s: offsets= already says the counts; do not pass counts= as well" % path)
        if regions is None or int(regions) < 1:
            raise ValueError("feature store %s: a ragged store needs regions= (N, the most rows an image may have)" % path)
        if self.features.ndim != 2 or self.features.dtype != np.float32:
            raise ValueError("feature store %s: with offsets= expected a float32 [total_rows, dim] array, got %s %s"
                             % (path, self.features.dtype, self.features.shape))
        o = np.load(offsets) if isinstance(offsets, (str, os.PathLike)) else np.asarray(offsets)
        if o.ndim != 1 or o.size < 2 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError("feature store %s: offsets must be n_img + 1 integers, got %s %s" % (path, o.dtype, o.shape))
        o = np.ascontiguousarray(o.astype(np.int64))
        if o[0] != 0 or o[-1] != self.features.shape[0]:
            raise ValueError("feature store %s: offsets run %d..%d, the array holds %d rows" % (path, int(o[0]), int(o[-1]), self.features.shape[0]))
        if (np.diff(o) < 0).any():
            raise ValueError("feature store %s: offsets must not decrease" % path)
        self._n_img, self._sample_shape = o.size - 1, (int(regions), int(self.features.shape[1]))
        self._starts = np.ascontiguousarray(o[:-1])
        return np.diff(o)                  # (1..N each: checked with the counts of a padded store)

    def __len__(self):
        return self._n_img

    def populate(self):
        """Map every page of the store into this process now (MADV_POPULATE_READ where the kernel has it, else one read per 4 KiB
        page).  A cold mapping pays a minor page fault per page on first touch -- 72 per sample, under the process's mmap lock, so
        a 16-thread gather of 512 cold rows takes 60-90 ms instead of 2 (measured, tools/feed_host_profile.py); a store that fits
        RAM is worth populating once, a larger one lives with first-touch faults like the reference's h5py reads do."""
        mm = getattr(self.features, "_mmap", None)
        try:
            if mm is None:
                raise OSError
            mm.madvise(22)                                     # MADV_POPULATE_READ (Linux >= 5.14)
        except (OSError, ValueError, AttributeError):
            flat = self.features.reshape(-1)
            step = 1 << 20                                     # 4 MiB of floats per slice: one element per page is read
            total = 0.0
            for lo in range(0, flat.size, step * 256):
                total += float(flat[lo:lo + step * 256:1024].sum())
        return self

    @property
    def sample_shape(self):
        return self._sample_shape

    def index(self, img_filename):
        """datasets.py:912: `outer.data['img']['name_to_idx'][item_vqa['img_filename']]` (KeyError for an unknown image)."""
        return self.name_to_idx[img_filename]

    def gather(self, indices, out):
        """out[r] = feature[indices[r]] (rows of N x D floats), fp32 or rounded to bf16 (nearest even), on `workers` threads."""
        if self.ragged:
            raise ValueError("gather: a ragged store (offsets=) holds no padded rows; it serves packed batches (gather_packed)")
        idx = np.asarray(indices, dtype=np.int64)
        if idx.ndim != 1 or out.shape[0] < idx.size or tuple(out.shape[1:]) != self.sample_shape:
            raise ValueError("gather: out %s does not take %d rows of %s" % (tuple(out.shape), idx.size, self.sample_shape))
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError("gather: feature index out of range [0, %d)" % len(self))
        n = idx.size
        if out.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("gather: out must be float32 or bfloat16")
        if n == 0:
            return out[:0]
        # ONE native call for the batch (csrc/feed_host.hip: `workers` threads, memcpy or round-to-nearest-even to bf16): a ctypes call
        # drops the GIL once, where a numpy.take per worker thread took and returned it per call -- next to a training loop that holds
        # the GIL for milliseconds at a time that was 9-19 ms per batch instead of 2-3 (tools/feed_bench.py --store)
        if self.features.flags["C_CONTIGUOUS"] and out.is_contiguous():
            from . import _lib
            try:
                L_ = _lib.lib()
            except _lib.VqaLibraryError:
                L_ = None
            if L_ is not None:
                idx = np.ascontiguousarray(idx)
                _lib.check(L_.vqa_host_gather_rows(self.features.ctypes.data, len(self), int(np.prod(self.sample_shape)), idx.ctypes.data, n,
                                                   out.data_ptr(), int(out.dtype == torch.bfloat16), self.workers), "host_gather_rows")
                return out[:n]
        # (no library: numpy, one take per worker thread; bf16 through torch's conversion)
        dst = out.numpy() if out.dtype == torch.float32 else np.empty((n,) + self.sample_shape, dtype=np.float32)

        def copy(lo, hi):
            if hi > lo:
                np.take(self.features, idx[lo:hi], axis=0, out=dst[lo:hi], mode="clip")   # (range-checked above; mode="raise" buffers `out`)
        if self._pool is None or n < 2 * self.workers:
            copy(0, n)
        else:
            step = -(-n // self.workers)
            list(self._pool.map(lambda lo: copy(lo, min(lo + step, n)), range(0, n, step)))
        if out.dtype == torch.bfloat16:
            out[:n].copy_(torch.from_numpy(dst[:n]))
        return out[:n]


    def gather_packed(self, indices, out, v_len_out, native=True):
        """The packed form of gather: the real rows of images `indices`, back to back, into out [capacity, D] (a pinned host tensor,
        fp32, or bf16 -- rounded to nearest even on the way), their counts into v_len_out (int32, at least len(indices) long).
        -> R, the number of rows written; rows of `out` from R on are left as they are.  A ragged store copies offsets[i] ..
        offsets[i+1], a padded store with counts= the first counts[i] rows of image i.  ONE native call for the batch
        (csrc/feed_host.hip, vqa_host_gather_ragged: the destination prefix sum once, the copy split over `workers` threads by
        bytes); native=False, or no library: the same in numpy.  Everything is range-checked before a byte is copied: the indices
        (IndexError), R against the capacity (ValueError)."""
        if self.counts is None:
            raise ValueError("gather_packed: the store has no region counts (FeatureStore(counts=) or (offsets=, regions=))")
        idx = np.ascontiguousarray(np.asarray(indices, dtype=np.int64))
        N, D = self.sample_shape
        if idx.ndim != 1 or out.dim() != 2 or out.shape[1] != D or not out.is_contiguous():
            raise ValueError("gather_packed: out %s is not a contiguous [capacity, %d] buffer" % (tuple(out.shape), D))
        if out.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("gather_packed: out must be float32 or bfloat16")
        if v_len_out.dtype != torch.int32 or v_len_out.dim() != 1 or v_len_out.numel() < idx.size or not v_len_out.is_contiguous():
            raise ValueError("gather_packed: v_len_out must be a contiguous int32 tensor of at least %d entries" % idx.size)
        if idx.size and (idx.min() < 0 or idx.max() >= len(self)):
            raise IndexError("gather_packed: feature index out of range [0, %d)" % len(self))
        lens = self.counts[idx]
        R = int(lens.sum(dtype=np.int64))
        if R > out.shape[0]:
            raise ValueError("gather_packed: the batch has %d rows, out holds %d" % (R, out.shape[0]))
        if self._starts is None:
            with self._lock:
                if self._starts is None:
                    self._starts = np.arange(len(self), dtype=np.int64) * N
        if idx.size == 0:
            return 0
        rows = self.features.reshape(-1, D)          # (a view: the padded store's [n_img * N, D])
        L_ = None
        if native and rows.flags["C_CONTIGUOUS"]:
            from . import _lib
            try:
                L_ = _lib.lib()
            except _lib.VqaLibraryError:
                L_ = None
        if L_ is not None:
            import ctypes
            total = ctypes.c_long(0)
            _lib.check(L_.vqa_host_gather_ragged(rows.ctypes.data, rows.shape[0], D, self._starts.ctypes.data, self.counts.ctypes.data,
                                                 len(self), idx.ctypes.data, idx.size, out.data_ptr(), out.shape[0],
                                                 v_len_out.data_ptr(), ctypes.addressof(total), int(out.dtype == torch.bfloat16),
                                                 self.workers), "host_gather_ragged")
            return int(total.value)
        v_len_out.numpy()[:idx.size] = lens
        src = np.concatenate([np.arange(s, s + n) for s, n in zip(self._starts[idx], lens)])
        if out.dtype == torch.float32:
            np.take(rows, src, axis=0, out=out.numpy()[:R], mode="clip")       # (range-checked above)
        else:
            out[:R].copy_(torch.from_numpy(rows[src]))
        return R


def _check_store_layout(what, starts, counts, regions, total_rows):
    """The invariant vqa_gather_regions relies on, for every image: 0 <= starts[i], counts[i] in 1..N (N without counts) and
    starts[i] + counts[i] <= total_rows.  ValueError naming the first image that breaks it."""
    starts = np.asarray(starts, dtype=np.int64)
    c = np.asarray(counts, dtype=np.int64) if counts is not None else np.full(starts.shape, int(regions), np.int64)
    if starts.ndim != 1 or c.shape != starts.shape or starts.size < 1:
        raise ValueError("%s: starts %s and counts %s must be [n_img], n_img >= 1" % (what, starts.shape, c.shape))
    bad = (c < 1) | (c > regions)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("%s: image %d has region count %d outside 1..%d" % (what, i, int(c[i]), regions))
    bad = (starts < 0) | (starts + c > total_rows)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError("%s: image %d owns rows %d..%d, the store holds %d" % (what, i, int(starts[i]), int(starts[i] + c[i]), total_rows))


def _free_bytes(device):
    """bytes the device can still hand out: HIP's figure for a GPU (memory torch has cached but not in use is not counted), the
    available physical memory for the CPU"""
    if device.type == "cuda":
        return int(torch.cuda.mem_get_info(device)[0])
    try:
        return int(os.sysconf("SC_AVPHYS_PAGES")) * int(os.sysconf("SC_PAGE_SIZE"))
    except (ValueError, OSError, AttributeError):
        return 1 << 62


class DeviceFeatureStore:
    """A FeatureStore uploaded ONCE into device memory: a batch then names its images ('v_idx' int32 [B], 2 KB at B = 512) and the
    device gathers their rows out of HBM (ops.gather_regions, csrc/region_gather.hip) -- no host gather, no pinned region slots,
    no host -> device copy of region rows in the step.  The reference's feature file for VQA v2 train+val is 36.4 GB as fp32 and
    18.2 GB as bf16 (123 287 x 36 x 2048); an MI355X has 288 GB.

    store: a FeatureStore of any form -- padded, padded with counts=, or ragged (offsets=).  dtype: float32, or bfloat16 -- then
    the rows are rounded on the way up, by store.gather / store.gather_packed, i.e. the round-to-nearest-even of the bf16
    transport (store_batches(region_dtype=torch.bfloat16)): an fp32 model widens them in the gather, exactly.  fp32 rows are never
    narrowed on the device.  compact=True: a padded store that has counts is uploaded as its real rows only, back to back (the
    ragged layout); compact=False keeps its padded layout.  The upload runs in chunks through ONE pinned staging buffer of
    chunk_bytes (two halves: the host gather of one chunk overlaps the copy of the other); there is never a second full copy in
    host memory.

    Fields: rows [total_rows, D] (dtype), starts int64 [n_img] (the first row of image i), counts int32 [n_img] or None (every
    image has N rows) -- tensors on `device`; sample_shape (N, D), len() = n_img, nbytes (the three tensors), upload_seconds;
    index(img_filename) / name_to_idx / idx_to_name are the host store's.  device="cpu" keeps the tensors on the host: the same
    class for host tests and gloo runs.

    Checked once, on the host, before anything is uploaded (ValueError): 0 <= starts[i], every count in 1..N and
    starts[i] + counts[i] <= total_rows -- for the host store's layout and for the one built here.  The gather kernel clamps the
    index and the count it reads and relies on this for the rest.  Capacity: construction raises ValueError naming both numbers
    when nbytes exceeds the device's free memory minus reserve_bytes -- what is kept free for the model, its activations and
    the captured graphs' pools.  reserve_bytes defaults to 8 GiB on a GPU and to 0 on the CPU."""

    DEFAULT_RESERVE_BYTES = 8 << 30

    def __init__(self, store, device, dtype=torch.float32, compact=True, chunk_bytes=256 << 20, reserve_bytes=None):
        self.device = torch.device(device)
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("DeviceFeatureStore: dtype must be float32 or bfloat16, got %s" % (dtype,))
        N, D = (int(x) for x in store.sample_shape)
        n_img = len(store)
        self.sample_shape, self._n_img, self.dtype = (N, D), n_img, dtype
        self.name_to_idx, self.idx_to_name = store.name_to_idx, getattr(store, "idx_to_name", None)
        # the host store's own layout, as its gathers will read it
        src_rows = int(store.features.shape[0]) * (1 if store.ragged else N)
        src_starts = store._starts if store.ragged else np.arange(n_img, dtype=np.int64) * N
        _check_store_layout("DeviceFeatureStore: the host store", src_starts, store.counts, N, src_rows)
        self.packed_upload = store.counts is not None and (store.ragged or bool(compact))
        if self.packed_upload:
            c64 = store.counts.astype(np.int64)
            starts = np.cumsum(c64) - c64
            total_rows = int(c64.sum())
        else:
            starts, total_rows = src_starts, n_img * N
        counts = store.counts
        _check_store_layout("DeviceFeatureStore", starts, counts, N, total_rows)
        item = torch.empty((), dtype=dtype).element_size()
        self.nbytes = total_rows * D * item + n_img * 8 + (n_img * 4 if counts is not None else 0)
        reserve = (self.DEFAULT_RESERVE_BYTES if self.device.type == "cuda" else 0) if reserve_bytes is None else int(reserve_bytes)
        free = _free_bytes(self.device)
        if self.nbytes > free - reserve:
            raise ValueError("DeviceFeatureStore: the store needs %d bytes, %s has %d free minus %d reserved = %d"
                             % (self.nbytes, self.device, free, reserve, free - reserve))
        import time
        t0 = time.perf_counter()
        self.rows = torch.empty(total_rows, D, dtype=dtype, device=self.device)
        self.starts = torch.from_numpy(np.ascontiguousarray(starts, dtype=np.int64)).to(self.device)
        self.counts = torch.from_numpy(np.ascontiguousarray(counts, dtype=np.int32)).to(self.device) if counts is not None else None
        self._upload(store, starts, max(int(chunk_bytes), 2 * N * D * item))
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        self.upload_seconds = time.perf_counter() - t0

    def _upload(self, store, starts, chunk_bytes):
        N, D = self.sample_shape
        n_img, cuda = self._n_img, self.device.type == "cuda"
        half_rows = chunk_bytes // 2 // (D * self.rows.element_size())          # (>= N: one image always fits a half)
        stage = torch.empty(2, half_rows, D, dtype=self.dtype)
        if cuda:
            stage = stage.pin_memory()
        lens = torch.empty(half_rows, dtype=torch.int32) if self.packed_upload else None
        done = [None, None]
        end = np.append(starts[1:], self.rows.size(0)) if self.packed_upload else None      # image i's rows end at end[i]
        lo = k = 0
        while lo < n_img:
            if self.packed_upload:
                hi = max(lo + 1, int(np.searchsorted(end, starts[lo] + half_rows, side="right")))
            else:
                hi = min(n_img, lo + half_rows // N)
            half = stage[k % 2]
            if done[k % 2] is not None:
                done[k % 2].synchronize()                # the copy that last read this half has finished
            ids = np.arange(lo, hi, dtype=np.int64)
            if self.packed_upload:
                r = store.gather_packed(ids, half, lens)
                r0 = int(starts[lo])
            else:
                store.gather(ids, half[:(hi - lo) * N].view(hi - lo, N, D))
                r, r0 = (hi - lo) * N, lo * N
            self.rows[r0:r0 + r].copy_(half[:r], non_blocking=cuda)
            if cuda:
                done[k % 2] = torch.cuda.Event()
                done[k % 2].record()
            lo, k = hi, k + 1

    def __len__(self):
        return self._n_img

    def index(self, img_filename):
        """FeatureStore.index: the row of an image file name (KeyError for an unknown image)."""
        return self.name_to_idx[img_filename]


class _QaTable:
    """The per-question records turned into arrays ONCE (the reference keeps dicts and pays Python per sample per epoch in its
    DataLoader workers): feature rows, the question matrix, ids, and the soft answers as CSR (datasets.py:963-969: a[c_id] = c_prob,
    the last pair of a duplicated id wins)."""

    def __init__(self, store, qa_items, num_ans, q_dtype, require_answers=False):
        n = len(qa_items)
        self.rows = np.fromiter((it["v_idx"] if "v_idx" in it else store.index(it["img_filename"]) for it in qa_items), np.int64, n)
        self.q_ids = np.fromiter((int(it.get("q_id", i)) for i, it in enumerate(qa_items)), np.int64, n)
        q_np = {torch.long: np.int64, torch.float32: np.float32, torch.float64: np.float64}.get(q_dtype, np.float32)
        self.q = np.asarray([np.asarray(it["q_idxes"]) for it in qa_items]).astype(q_np, copy=False)
        self.kind = "dense" if "a" in qa_items[0] else ("soft" if "a_10_idx" in qa_items[0] else None)
        if self.kind == "dense":
            self.a = np.asarray([np.asarray(it["a"], dtype=np.float32) for it in qa_items])
        elif self.kind == "soft":
            counts = np.fromiter((len(it["a_10_idx"]) for it in qa_items), np.int64, n)
            if require_answers and n and counts.min() == 0:
                i = int(np.argmin(counts))                         # the reference: assert item_vqa['a_10_idx'] (datasets.py:953, :962)
                raise ValueError("record %d (q_id %s) has an empty 'a_10_idx': a training record needs at least one answer pair"
                                 % (i, qa_items[i].get("q_id", i)))
            self.max_pairs = int(counts.max()) if n else 0
            self.ptr = np.concatenate([[0], np.cumsum(counts)])
            flat = [pair for it in qa_items for pair in it["a_10_idx"]]
            self.cols = np.fromiter((int(c) for c, _ in flat), np.int64, len(flat))
            self.vals = np.fromiter((float(p) for _, p in flat), np.float32, len(flat))
            if len(flat) and (self.cols.min() < 0 or self.cols.max() >= num_ans):
                raise IndexError("store_batches: answer id outside [0, %d)" % num_ans)

    def fill_answers(self, a, ids):
        dst = a.numpy()
        if self.kind == "dense":
            dst[...] = self.a[ids]
            return
        dst.fill(0.0)
        lo, hi = self.ptr[ids], self.ptr[ids + 1]
        counts = hi - lo
        if counts.sum():
            rows = np.repeat(np.arange(len(ids)), counts)
            src = np.concatenate([np.arange(x, y) for x, y in zip(lo, hi)]) if len(ids) else np.zeros(0, np.int64)
            dst[rows, self.cols[src]] = self.vals[src]        # (in order: the last pair of a duplicated id wins, as in the reference's loop)

    def pair_width(self):
        """K of the sparse answer target this table serves (its largest pair count); ValueError when it cannot serve one."""
        if self.kind != "soft":
            raise ValueError("answers='sparse' needs records with 'a_10_idx' pairs: a dense 'a' cannot be served sparse")
        return _pair_width(self.max_pairs)

    def padded_pairs(self):
        """The CSR as two padded arrays [n,K] (ids int32, -1 where a row has no pair; values float32, 0 there), built once: a
        batch's sparse target is then two row gathers."""
        if getattr(self, "_pairs", None) is None:
            K, n = self.pair_width(), len(self.rows)
            counts = np.diff(self.ptr)
            rows = np.repeat(np.arange(n), counts)
            within = np.arange(len(self.cols)) - np.repeat(self.ptr[:-1], counts)
            pidx, pval = np.full((n, K), -1, np.int32), np.zeros((n, K), np.float32)
            pidx[rows, within] = self.cols
            pval[rows, within] = self.vals
            self._pairs = (pidx, pval)
        return self._pairs

    def fill_pairs(self, a_idx, a_val, ids):
        """The pairs of records `ids` as they are, in record order, into a_idx int32 / a_val float32 [b,K]; padding -1 / 0."""
        pidx, pval = self.padded_pairs()
        a_idx.numpy()[...] = pidx[ids]
        a_val.numpy()[...] = pval[ids]


def qa_table(store, qa_items, num_ans, q_dtype=torch.long, require_answers=False):
    """The array form of the per-question records that store_batches works on; build it once, pass it instead of the list.
    require_answers=True: a record with an empty 'a_10_idx' raises ValueError naming it (the reference's training loader asserts the
    same per item, datasets.py:953, :962)."""
    return _QaTable(store, qa_items, num_ans, q_dtype, require_answers)


def _sorted_by_question_length(ids, q, shards):
    """ids [b] reordered by descending count of non-zero tokens of q[ids], stably, inside each of the `shards` contiguous b // shards
    slices (what `shard` hands to a rank); rows behind the last whole slice, which no rank receives, are sorted among themselves."""
    ids = np.asarray(ids)
    n = (q[ids] != 0).sum(axis=1)
    per = len(ids) // shards
    bounds = [r * per for r in range(shards)] + [shards * per, len(ids)] if per else [0, len(ids)]
    parts = [lo + np.argsort(-n[lo:hi], kind="stable") for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
    return ids[np.concatenate(parts)] if parts else ids


def store_batches(store, qa_items, batch_size, num_ans, shuffle=False, seed=0, pin=True, region_dtype=torch.float32, ring=3,
                  q_dtype=torch.long, prefetch=0, epochs=1, producers=1, answers="dense", packed=False, sort_questions=False,
                  shards=1, resident=None):
    """The reference's loader (datasets.py:893-977: `Inner.__getitem__` + DataLoader(batch_size, shuffle, pin_memory=True), no
    drop_last) over a FeatureStore: yields batch dicts {'v' [B,N,D], 'q_idxes' [B,T], 'q_id' [B], 'a' [B,num_ans]} of host tensors.
    qa_items: the reference's per-question records -- 'img_filename' (or 'v_idx'), 'q_idxes', 'q_id', 'a_10_idx' [(answer id,
    probability), ...] (or a dense 'a'; neither for test splits).  The staging tensors come from a ring of `ring` pinned sets reused
    in turn (a yielded batch stays valid until `ring - 1 - prefetch` further batches have been drawn; DevicePrefetcher(depth) needs
    ring >= depth + prefetch + 1).  region_dtype = torch.bfloat16 stores the regions rounded to bf16 (the transport format: half the
    PCIe bytes; the fp32 path widens them exactly on the device).  q_dtype: torch.long for token ids (the reference), a float type when
    'q_idxes' holds precomputed question vectors (the models' identity-encoder slot).  The records are turned into arrays once
    per call (`qa_table(...)` does it ahead of time: pass its result as qa_items to reuse it over epochs).  prefetch > 0: batches are assembled by a
    background thread, up to `prefetch` ahead of the consumer (the DataLoader's worker processes, as one thread: numpy and torch
    release the GIL in the copies that dominate); producers > 1: that many threads, each assembling whole batches, delivered in
    order.  epochs: passes over the records (None: for ever), each with its own shuffle
    (seed + epoch) -- ONE generator for a whole run keeps its pinned staging ring (page-locking 160 MB per slot takes tens of
    milliseconds: a generator per epoch would pay that again every time).  answers="sparse": instead of 'a' the batches carry the pairs
    as they are, 'a_idx' int32 [B,K] and 'a_val' float32 [B,K] in the same staging ring (K = the table's largest pair count, at most
    16; shorter rows padded with -1 / 0, pairs in record order): no dense [B,num_ans] row is allocated, filled or copied, the
    trainer computes its loss from the pairs (ops.densify defines the format).  Records given with a dense 'a' cannot be served sparse.
    A store with region counts (FeatureStore(counts=...)) adds 'v_len' int32 [B] to every batch, from the same staging ring.
    packed=True (a store with counts, padded or ragged): instead of 'v' the batches carry 'v_packed', the ring slot's capacity
    tensor [batch_size*N, D] of which the first sum(v_len) rows are the samples' real rows back to back (the rest is whatever the
    slot held: nothing reads it) -- the padding is neither gathered nor, through DevicePrefetcher, copied to the device; the
    models unpack it there (ops.unpack_regions).  The short last batch yields the leading B_last*N rows.
    sort_questions=True (token-id questions): each batch's record ids are reordered by descending question length (its count of
    non-zero tokens) BEFORE anything is gathered -- a stable sort, so every key of the batch follows, packed rows included -- for
    the length-aware question encoder, whose products skip row tiles that hold no unfinished question (SkipThoughts(length_aware=
    True)).  shards=P: the sort happens inside each of the P contiguous B/P slices that `shard` hands to a rank, so ranks keep equal
    work.  Which records make up a batch does not change, and order inside a batch does not change the training sum.
    resident=DeviceFeatureStore: the region rows already live on the device, so the batches carry 'v_idx' int32 [B] -- the image
    of each sample, from the same staging ring -- instead of 'v' / 'v_packed' / 'v_len': no region staging tensor is allocated and
    no gather runs here; the model the store is attached to (RegionQuestionModel.use_region_store) gathers on the device and takes
    the counts from the store.  Everything else (sort_questions, shards, answers, prefetch, producers) works as above; `store` may
    be the host store the resident one was built from, or the resident store itself.  With packed=True or a region_dtype other
    than float32 it raises ValueError: how the rows are laid out and stored was decided when the store was uploaded."""
    sparse = _check_answers(answers)
    if int(shards) < 1:
        raise ValueError("store_batches: shards must be >= 1, got %r" % (shards,))
    if resident is not None:
        if packed or region_dtype != torch.float32:
            raise ValueError("store_batches(resident=): no region rows are shipped, so packed=True / region_dtype= do not apply "
                             "(the resident store's layout and dtype were chosen when it was uploaded)")
        store = resident
    if packed and store.counts is None:
        raise ValueError("store_batches(packed=True) needs a store with region counts (FeatureStore(counts=) or (offsets=, regions=))")
    if resident is None and not packed and getattr(store, "ragged", False):
        raise ValueError("store_batches: a ragged store (offsets=) serves packed batches only: pass packed=True")
    n = len(qa_items.rows) if isinstance(qa_items, _QaTable) else len(qa_items)

    def order_of(epoch):
        o = np.arange(n)
        if shuffle:
            np.random.RandomState(seed + epoch).shuffle(o)
        return o
    table = qa_items if isinstance(qa_items, _QaTable) else _QaTable(store, qa_items, num_ans, q_dtype)
    T = table.q.shape[1]
    if resident is not None and n and (table.rows.min() < 0 or table.rows.max() >= len(resident)):
        raise IndexError("store_batches(resident=): feature index out of range [0, %d)" % len(resident))
    if sort_questions and table.q.dtype.kind not in "iu":
        raise ValueError("store_batches(sort_questions=True) sorts by the count of non-zero token ids: it needs q_dtype=torch.long")
    has_a = table.kind is not None
    K = table.padded_pairs()[0].shape[1] if sparse and has_a else 0       # (built here, before any producer thread runs)
    mk = (lambda *s, dtype: torch.empty(*s, dtype=dtype).pin_memory()) if pin else (lambda *s, dtype: torch.empty(*s, dtype=dtype))
    slots = []

    slot_lock = threading.Lock()

    def assemble(k, job):
        order, lo = job
        ids = order[lo:lo + batch_size]
        b = len(ids)
        if sort_questions:
            ids = _sorted_by_question_length(ids, table.q, int(shards))
        with slot_lock:
            while len(slots) <= k:
                v_shape = (batch_size * store.sample_shape[0], store.sample_shape[1]) if packed else (batch_size, *store.sample_shape)
                slots.append({"v": mk(*v_shape, dtype=region_dtype) if resident is None else None,
                              "v_idx": mk(batch_size, dtype=torch.int32) if resident is not None else None,
                              "q_idxes": mk(batch_size, T, dtype=q_dtype),
                              "a": mk(batch_size, num_ans, dtype=torch.float32) if has_a and not sparse else None,
                              "a_idx": mk(batch_size, K, dtype=torch.int32) if K else None,
                              "a_val": mk(batch_size, K, dtype=torch.float32) if K else None,
                              "v_len": mk(batch_size, dtype=torch.int32) if store.counts is not None and resident is None else None})
        s = slots[k]
        if resident is not None:
            batch = {"v_idx": s["v_idx"][:b]}
            batch["v_idx"].numpy()[...] = table.rows[ids]
        elif packed:
            store.gather_packed(table.rows[ids], s["v"], s["v_len"])
            batch = {"v_packed": s["v"][:b * store.sample_shape[0]], "v_len": s["v_len"][:b]}
        else:
            batch = {"v": store.gather(table.rows[ids], s["v"])}
        batch.update({"q_idxes": s["q_idxes"][:b], "q_id": torch.from_numpy(table.q_ids[ids])})
        batch["q_idxes"].numpy()[...] = table.q[ids]
        if store.counts is not None and not packed and resident is None:
            batch["v_len"] = s["v_len"][:b]
            batch["v_len"].numpy()[...] = store.counts[table.rows[ids]]
        if K:
            batch["a_idx"], batch["a_val"] = s["a_idx"][:b], s["a_val"][:b]
            table.fill_pairs(batch["a_idx"], batch["a_val"], ids)
        elif has_a:
            batch["a"] = s["a"][:b]
            table.fill_answers(batch["a"], ids)
        return batch

    def jobs():
        epoch = 0
        while epochs is None or epoch < epochs:
            order = order_of(epoch)
            for lo in range(0, n, batch_size):
                yield order, lo
            epoch += 1
    ring = max(1, ring)
    if prefetch <= 0:
        for j, job in enumerate(jobs()):
            yield assemble(j % ring, job)
        return
    if ring < prefetch + 2:
        raise ValueError("store_batches: ring=%d is too small for prefetch=%d (a slot would be refilled while still in use)" % (ring, prefetch))
    from collections import deque
    ex = ThreadPoolExecutor(max(1, int(producers)))
    window, it = deque(), enumerate(jobs())

    def submit_next():
        try:
            j, job = next(it)
        except StopIteration:
            return False
        window.append(ex.submit(assemble, j % ring, job))
        return True
    try:
        for _ in range(prefetch):
            if not submit_next():
                break
        while window:
            fut = window.popleft()
            batch = fut.result()
            submit_next()
            yield batch
    finally:
        for fut in window:
            fut.cancel()
        ex.shutdown(wait=True)
