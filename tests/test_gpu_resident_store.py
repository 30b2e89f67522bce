"""The device-resident region store on the GPU: vqa_gather_regions (csrc/region_gather.hip) through the C ABI, and 'v_idx' through
the models, the trainer's captured step, the prefetcher's copies and the evaluator.  The feature copies rows and widens bf16
exactly, so every comparison here is of bits.

  A  the kernel's three forms against the host restatement, padded-with-gaps and ragged layouts, with and without counts; padding
     comes back +0.0, v_len_out holds the counts, nothing outside the two output windows is touched, no NaN of the store's guards,
     of its gap rows or of the pre-filled window survives; one launch whose grid depends on (B, N, D) alone; out-of-range indices
     and counts in device memory give the result of the clamped values; refusals launch nothing.
  B  CoR2Model (fp32 B 64 x N 36, bf16 B 16 x N 100), ODAModel(region_counts=True) and the default ODAModel on a 'v_idx' batch
     with an attached store against the same batch materialised as padded 'v' (+ 'v_len'): logits, loss, alphas, every parameter
     gradient, eval and train mode; a bf16 store against the padded bf16 transport.
  C  a batch without 'v_idx' launches the same with a store attached as without.
  D  DataParallelTrainer(graph=True) fed by store_batches(resident=) + DevicePrefetcher against the same records host-fed padded
     and against the resident steps launched kernel by kernel; what the prefetcher copies; the evaluator."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import reference_faithful as RF
from oracle import seeded
from kernel_harness import (BF, E_BADARG, E_UNSUPPORTED, F32, NAN, PAD, _bits, _call, _ceil, _out, _ptr, _same_bits, _untouched, _win,
                            dev, ops, spy_launches)  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

FORMS = [(F32, F32), (BF, BF), (BF, F32)]
KERNEL = "(gather_regions_kernel<%s>)"          # <true>: bf16 rows widened to fp32; <false>: the two copying forms
TARGET_WGS, THREADS = 1024, 256
N_IMG = 7                           # fewer images than samples: indices repeat
# D = 8: one 16-byte unit per bf16 row, every B (1, 2, across a wave, across 256) with every N (1, a multiple and a non-multiple of
# the row chunk, 100); D = 2048 (the models' rows: 256 units a row) where the chunking of a sample's rows changes and where a thread
# runs the pipelined passes (a chunk of more than 4 rows), the single-unit tail and the zero fill in one launch
SHAPES = [(B, N, 8) for B in (1, 2, 65, 257) for N in (1, 36, 37, 100)] + \
         [(1, 1, 2048), (1, 37, 2048), (2, 100, 2048), (65, 37, 2048), (257, 36, 2048)]
GUARD_IMAGES_BEHIND = 3
V_LEN_PAD = 4                       # int32 entries (16 bytes) of sentinel in front of and behind the v_len_out window
V_LEN_SENT = -7


def _grid(B, N):
    chunks = min(_ceil(TARGET_WGS, B), N)
    rows = _ceil(N, chunks)
    return B * _ceil(N, rows) * THREADS


def _counts(n, N, kind, rs):
    if kind == "full":
        return np.full(n, N, np.int64)
    if kind == "ones":
        return np.ones(n, np.int64)
    if kind == "random":
        return rs.randint(1, N + 1, n)
    lens = np.ones(n, np.int64)
    lens[n // 2] = N                # one image with every row, every other with one
    return lens


def gather_host(rows, starts, counts, idx, N):
    """the contract, restated on the host: out[b, r] = rows[starts[i] + r] for r < c, +0.0 behind; i and c clamped"""
    n_img = len(starts)
    out = torch.zeros(len(idx), N, rows.size(1), dtype=rows.dtype)
    lens = []
    for b, i in enumerate(idx):
        i = min(max(int(i), 0), n_img - 1)
        c = N if counts is None else min(max(int(counts[i]), 0), N)
        out[b, :c] = rows[int(starts[i]):int(starts[i]) + c]
        lens.append(c)
    return out, lens


class _Store:
    """A store in ONE device allocation that an unclamped index or count would still stay inside: a guard image of NaN rows in
    front, the n_img images (padded layout: N rows each, NaN in every row behind an image's count; ragged: the real rows back to
    back), GUARD_IMAGES_BEHIND NaN images behind.  starts / counts carry guard entries too -- in front (what idx = -1 would read)
    and behind (idx = n_img ..) -- that name those NaN images.  `rows_host` [total_rows, D]: the declared rows, NaN in the gaps."""

    def __init__(self, source, counts, N, D, dt, ragged, null_counts=False):
        n_img = N_IMG
        c = np.full(n_img, N, np.int64) if counts is None else np.asarray(counts, np.int64)
        self.starts_host = (np.cumsum(c) - c) if ragged else np.arange(n_img, dtype=np.int64) * N
        self.total_rows = int(c.sum()) if ragged else n_img * N
        rows = torch.full((self.total_rows, D), NAN, dtype=dt)
        for i in range(n_img):
            s = int(self.starts_host[i])
            rows[s:s + int(c[i])] = source[i, :int(c[i])].to(dt)
        self.rows_host, self.counts_host, self.N, self.D, self.dt = rows, (None if null_counts else c), N, D, dt
        front, behind = N, GUARD_IMAGES_BEHIND * N                     # guard rows
        buf = torch.full(((front + self.total_rows + behind) * D,), NAN, dtype=dt)
        buf[front * D:(front + self.total_rows) * D] = rows.reshape(-1)
        self.buf, self.rows_off = buf.to(dev()), front * D
        assert (self.rows_off * buf.element_size()) % 16 == 0
        # guard entries: 2 int64 / 4 int32 in front (16 bytes: the declared arrays stay aligned), GUARD_IMAGES_BEHIND behind
        guard_starts = [self.total_rows + k * N for k in range(GUARD_IMAGES_BEHIND)]
        self.starts_buf = torch.tensor([-N, -N] + list(self.starts_host) + guard_starts, dtype=torch.int64).to(dev())
        self.counts_buf = torch.tensor([N] * 4 + list(c) + [N] * GUARD_IMAGES_BEHIND, dtype=torch.int32).to(dev())

    def args(self, rows_off=0, starts_off=0, counts_off=0):
        counts = None if self.counts_host is None else _ptr(self.counts_buf, 4 + counts_off)
        return _ptr(self.buf, self.rows_off + rows_off), self.total_rows, _ptr(self.starts_buf, 2 + starts_off), counts, N_IMG


def _nan_window(n, dt):
    buf = _out(n, dt)
    buf[PAD:PAD + n] = NAN
    return buf


def _run(ops, store, idx_d, B, N, D, dt_out, out_off=PAD, want_len=True, idx_off=0, len_off=V_LEN_PAD, **offs):
    buf = _nan_window(B * N * D, dt_out)
    lens = torch.full((max(B, 1) + 2 * V_LEN_PAD,), V_LEN_SENT, dtype=torch.int32, device=dev())
    rc, log = _call(ops, ops._lib.lib().vqa_gather_regions, *store.args(**offs), _ptr(idx_d, idx_off), _ptr(buf, out_off),
                    _ptr(lens, len_off) if want_len else None, B, N, D, int(store.dt == BF), int(dt_out == BF))
    return rc, log, buf, lens


def _v_len(lens, B, what):
    """-> the v_len_out window as a list; asserts that nothing around it changed"""
    got = lens[V_LEN_PAD:V_LEN_PAD + B].tolist()
    rest = lens[:V_LEN_PAD].tolist() + lens[V_LEN_PAD + B:].tolist()
    assert rest == [V_LEN_SENT] * len(rest), (what, "a store outside the v_len_out window")
    return got


def _indices(B, rs):
    idx = rs.randint(0, N_IMG, B)
    idx[0] = N_IMG - 1
    idx[B - 1] = 0 if B > 1 else idx[B - 1]
    return idx


def _kernel_case(ops, B, N, D):
    rs = np.random.RandomState(B * 1000 + N + D)
    source = torch.randn(N_IMG, N, D, generator=torch.Generator().manual_seed(B + N + D))
    idx = _indices(B, rs)
    idx_d = torch.from_numpy(idx.astype(np.int32)).to(dev())
    grids = set()
    cases = [(ragged, kind) for ragged in (False, True) for kind in ("full", "ones", "random", "one-long")] + [(False, None)]
    for ragged, kind in cases:
        counts = None if kind is None else _counts(N_IMG, N, kind, rs)
        for dt_in, dt_out in FORMS:
            what = "B=%d N=%d D=%d %s %s %s->%s" % (B, N, D, "ragged" if ragged else "padded", kind or "counts=NULL", dt_in, dt_out)
            store = _Store(source, counts, N, D, dt_in, ragged, null_counts=kind is None)
            rc, log, buf, lens = _run(ops, store, idx_d, B, N, D, dt_out)
            assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
            name = KERNEL % str((dt_in, dt_out) == (BF, F32)).lower()
            assert log == [(name, _grid(B, N))], (what, log)
            grids.add(log[0][1])
            got = _win(buf, (B, N, D), what).cpu()
            want, want_len = gather_host(store.rows_host, store.starts_host, store.counts_host, idx, N)
            want = want.to(dt_out)                                  # (bf16 -> fp32: exact)
            assert not bool(torch.isnan(got.float()).any()), (what, "a NaN of the guards, of a gap row or of the pre-filled window")
            assert _same_bits(got, want), (what, "differs from the host restatement (a -0.0 on the padding counts)")
            assert _v_len(lens, B, what) == want_len, what
            if kind in ("full", None) and (dt_in, dt_out) == (BF, F32):
                rows_d = store.rows_host.view(N_IMG, N, D)[idx].to(dev())
                assert _same_bits(got, ops.widen_bf16(rows_d).cpu()), (what, "not the bits of widen_bf16")
            if kind == "random":
                rc2, log2, buf2, lens2 = _run(ops, store, idx_d, B, N, D, dt_out, want_len=False)
                assert rc2 == 0 and log2 == log and _same_bits(_win(buf2, (B, N, D), what).cpu(), got), (what, "second run")
                assert lens2.tolist() == [V_LEN_SENT] * lens2.numel(), (what, "v_len_out = NULL and something was written")
    assert len(grids) == 1, ("the grid depends on the counts or the layout", B, N, D, grids)


@pytest.mark.parametrize("B,N,D", SHAPES, ids=["B%d-N%d-D%d" % s for s in SHAPES])
def test_gather_kernel_against_the_host_restatement(ops, B, N, D):
    _kernel_case(ops, B, N, D)


@pytest.mark.parametrize("ragged", [False, True], ids=["padded", "ragged"])
def test_gather_kernel_clamps_the_indices_and_counts_it_reads(ops, ragged):
    """Indices outside [0, n_img) and counts outside 0..N in DEVICE memory (the host ones are refused by ops.image_indices and by
    DeviceFeatureStore): the result is that of the clamped values.  The allocation is built so that the unclamped reads would stay
    inside it -- starts[-1], starts[n_img ..], counts[-1], counts[n_img ..] are guard entries that name NaN images, in front of
    and behind the declared rows -- and show up as NaN or as a wrong count; nothing here reads outside an allocation."""
    B, N, D = 8, 4, 16
    source = torch.randn(N_IMG, N, D, generator=torch.Generator().manual_seed(9))
    counts = np.array([2, 4, 1, 3, 4, 1, 3])
    idx = np.array([-1, N_IMG, N_IMG + 2, 3, 1, 4, 2, 5])
    for dt_in, dt_out in FORMS:
        store = _Store(source, counts, N, D, dt_in, ragged)
        idx_d = torch.from_numpy(idx.astype(np.int32)).to(dev())
        want, want_len = gather_host(store.rows_host, store.starts_host, counts, idx, N)
        rc, log, buf, lens = _run(ops, store, idx_d, B, N, D, dt_out)
        assert rc == 0 and len(log) == 1
        got = _win(buf, (B, N, D), "clamped indices").cpu()
        assert not bool(torch.isnan(got.float()).any()) and _same_bits(got, want.to(dt_out)), (dt_in, dt_out)
        assert _v_len(lens, B, "clamped indices") == want_len == [2, 3, 3, 3, 4, 4, 1, 1]
        if ragged:
            continue                # (a ragged image's rows end where the next one's begin: only a padded store can hold a count of 0)
        given = np.array([0, N + 2, -3, 3, N + 1, 1, 0])       # in device memory: 0, over N, negative
        store.counts_buf[4:4 + N_IMG] = torch.from_numpy(given.astype(np.int32)).to(dev())
        padded_rows = torch.full((N_IMG * N, D), NAN, dtype=dt_in)
        clamped = np.clip(given, 0, N)
        for i, c in enumerate(clamped):
            padded_rows[i * N:i * N + c] = source[i, :c].to(dt_in)          # (every row of the padded layout up to the clamped count)
        store.buf[store.rows_off:store.rows_off + N_IMG * N * D] = padded_rows.reshape(-1).to(dev())
        want, want_len = gather_host(padded_rows, store.starts_host, clamped, idx, N)
        rc, log, buf, lens = _run(ops, store, idx_d, B, N, D, dt_out)
        assert rc == 0 and len(log) == 1
        got = _win(buf, (B, N, D), "clamped counts").cpu()
        assert not bool(torch.isnan(got.float()).any()) and _same_bits(got, want.to(dt_out)), (dt_in, dt_out)
        assert _v_len(lens, B, "clamped counts") == want_len == [0, 0, 0, 3, 4, 4, 0, 1]


def test_gather_kernel_refusals_launch_nothing(ops):
    L = ops._lib.lib()
    B, N, D = 2, 3, 16
    store = _Store(torch.randn(N_IMG, N, D), np.array([3, 1, 2, 3, 1, 2, 3]), N, D, F32, ragged=False)
    idx_d = torch.tensor([3, 1, 0, 0, 0, 0], dtype=torch.int32, device=dev())

    def refused(code, B_=B, D_=D, dt_out=F32, **kw):
        rc, log, buf, lens = _run(ops, store, idx_d, B_, N, D_, dt_out, **kw)
        assert rc == code and log == [], (rc, log, L.vqa_last_error(), kw)
        assert lens.tolist() == [V_LEN_SENT] * lens.numel()
        buf[PAD:PAD + B_ * N * D_] = -12345.0
        assert _untouched(buf)
    refused(E_UNSUPPORTED, D_=12)                                   # D % 8
    refused(E_UNSUPPORTED, rows_off=1)                              # each pointer 4 bytes off a 16-byte boundary
    refused(E_UNSUPPORTED, counts_off=1)
    refused(E_UNSUPPORTED, idx_off=1)
    refused(E_UNSUPPORTED, out_off=PAD + 1)
    refused(E_UNSUPPORTED, len_off=V_LEN_PAD + 1)
    refused(E_UNSUPPORTED, dt_out=BF)                               # fp32 rows are not narrowed
    refused(E_BADARG, B_=0)
    out = _out(B * N * D)
    rows, total, starts, counts, n_img = store.args()
    good = [rows, total, starts, counts, n_img, _ptr(idx_d), _ptr(out, PAD), None]
    rc, log = _call(ops, L.vqa_gather_regions, rows, total, ctypes.c_void_p(store.starts_buf.data_ptr() + 16 + 4), counts, n_img,
                    _ptr(idx_d), _ptr(out, PAD), None, B, N, D, 0, 0)
    assert rc == E_UNSUPPORTED and log == []                        # starts 4 bytes off
    for missing in (0, 2, 5, 6):                                    # rows, starts, idx, out
        args = list(good)
        args[missing] = None
        rc, log = _call(ops, L.vqa_gather_regions, *args, B, N, D, 0, 0)
        assert rc == E_BADARG and log == [] and b"null pointer" in L.vqa_last_error(), missing
    for k, v in ((1, 0), (4, 0)):                                   # total_rows, n_img
        args = list(good)
        args[k] = v
        rc, log = _call(ops, L.vqa_gather_regions, *args, B, N, D, 0, 0)
        assert rc == E_BADARG and log == [], k
    assert _untouched(out)
    rc, log = _call(ops, L.vqa_gather_regions, *good, B, N, D, 0, 0)        # (and the same arguments, whole, are served)
    assert rc == 0 and len(log) == 1


# ---- stores for the wrapper, the models and the step ---------------------------------------------------------------------------
def _host_store(root, name, n_img, N, seed, counts=True):
    """a padded FeatureStore [n_img, N, 2048] of bf16-exact values, zero-padded behind its counts (1 and N among them)"""
    from vqa_playground_pytorch_amd import feed
    rs = np.random.RandomState(seed)
    feats = torch.from_numpy(rs.standard_normal((n_img, N, 2048)).astype(np.float32)).to(BF).float().numpy()
    cnt = None
    if counts:
        cnt = rs.randint(1, N + 1, n_img)
        cnt[0], cnt[1] = 1, N
        for i, c in enumerate(cnt):
            feats[i, c:] = 0.0
    np.save(root / (name + ".npy"), feats)
    return feed.FeatureStore(root / (name + ".npy"), workers=2, counts=cnt)


@pytest.fixture(scope="module")
def host_stores(tmp_path_factory):
    """built once, never changed: {36: 40 images with counts, 100: 12 images with counts, 'plain': 12 images x 36 without}"""
    root = tmp_path_factory.mktemp("resident")
    return {36: _host_store(root, "n36", 40, 36, 7), 100: _host_store(root, "n100", 12, 100, 8),
            "plain": _host_store(root, "plain", 12, 36, 9, counts=False)}


def test_ops_gather_regions_on_the_device(ops, monkeypatch, host_stores):
    """the wrapper: one logged launch per call, the CPU definition's bits, int64 and a misaligned slice of indices served, a host
    index out of range refused, a device one clamped"""
    from vqa_playground_pytorch_amd import feed
    host = host_stores[100]
    idx = torch.tensor([5, 11, 0, 0, 3, 11, 7], dtype=torch.int32)
    for dt_in, dt_out in FORMS:
        for compact in (True, False):
            ds, ds_cpu = (feed.DeviceFeatureStore(host, d, dtype=dt_in, compact=compact, chunk_bytes=3 << 20) for d in (dev(), "cpu"))
            assert ds.rows.is_cuda and ds.starts.is_cuda and ds.counts.is_cuda and _same_bits(ds.rows.cpu(), ds_cpu.rows), "chunked upload"
            want, want_len = ops.gather_regions(ds_cpu, idx, dt_out)
            with monkeypatch.context() as m:
                seen = spy_launches(m, ops)
                got, got_len = ops.gather_regions(ds, idx, dt_out)                     # host indices: checked, moved
                assert [n for n, _ in seen] == ["gather_regions"]
                again = ops.gather_regions(ds, idx.long().to(dev()), dt_out)[0]        # int64 on the device
                sliced = ops.gather_regions(ds, torch.cat([idx[:1], idx]).to(dev())[1:], dt_out, want_len=False)   # 4 bytes off
                assert [n for n, _ in seen] == ["gather_regions"] * 3 and sliced[1] is None
            assert got.shape == (7, 100, 2048) and _same_bits(got.cpu(), want) and torch.equal(got_len.cpu(), want_len)
            assert _same_bits(again, got) and _same_bits(sliced[0], got)
            assert _same_bits(want, host.gather(idx.tolist(), torch.empty(7, 100, 2048, dtype=dt_in)).to(dt_out))
    with pytest.raises(IndexError):
        ops.gather_regions(ds, torch.tensor([0, 12]))
    wild = ops.gather_regions(ds, torch.tensor([-5, 12], device=dev()))
    assert _same_bits(wild[0], ops.gather_regions(ds, torch.tensor([0, 11]))[0]) and wild[1].tolist() == [1, int(host.counts[11])]


def test_device_store_refuses_what_does_not_fit_the_device(host_stores):
    from vqa_playground_pytorch_amd import feed
    free = torch.cuda.mem_get_info(dev())[0]
    with pytest.raises(ValueError, match="needs [0-9]+ bytes.* free minus %d reserved" % free):
        feed.DeviceFeatureStore(host_stores["plain"], dev(), reserve_bytes=free)


# ================================================================================================================================ B
def _alphas(model):
    out = {}
    for k, x in model.alpha_dict.items():
        out[k] = torch.cat(list(x), -1).detach().clone() if isinstance(x, (list, tuple)) else x.detach().clone()
    return out


def _fwd_bwd(model, sample, a, train):
    model.train(train)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)                    # (the fused masks' seeds are drawn from torch's CPU generator)
    logits = model(sample)
    loss = RF.kld_sum_loss(logits, a)
    loss.backward()
    return logits.detach().clone(), loss.detach().clone(), _alphas(model), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _assert_same_run(got, want, what):
    assert _same_bits(got[0], want[0]), (what, "logits")
    assert _same_bits(got[1], want[1]), (what, "loss")
    assert set(got[2]) == set(want[2]) and all(_same_bits(got[2][k], want[2][k]) for k in want[2]), (what, "alphas")
    differ = [n for n in want[3] if not _same_bits(got[3][n], want[3][n])]
    assert not differ, (what, differ)
    assert all(bool(torch.isfinite(g).all()) for g in got[3].values()), what


def _model_batch(host, B, nans, seed):
    """-> (idx [B] with repeats, image 0 (one row) and image 1 (N rows) among them; the materialised padded v; v_len or None; q; a)"""
    rs = np.random.RandomState(seed)
    idx = rs.randint(0, len(host), B)
    idx[0], idx[1], idx[B - 1] = 0, 1, len(host) - 1
    N = host.sample_shape[0]
    v = host.gather(idx, torch.empty(B, N, 2048)).clone()
    v_len = torch.from_numpy(host.counts[idx]) if host.counts is not None else None
    _, q, a = seeded.seeded_inputs(B, regions=1, answers=nans, seed=seed)
    return torch.from_numpy(idx.astype(np.int32)), v, v_len, torch.from_numpy(q).to(dev()), torch.from_numpy(a).to(dev())


MODELS = [("cor2", F32, 64, 36), ("cor2", BF, 16, 100), ("oda-counts", F32, 64, 36), ("oda", F32, 64, "plain")]


@pytest.mark.parametrize("name,dt,B,key", MODELS, ids=["cor2-f32-B64-N36", "cor2-bf16-B16-N100", "oda-counts-B64-N36", "oda-default-B64-N36"])
def test_models_on_a_resident_store_equal_the_padded_batch(host_stores, name, dt, B, key):
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel, feed
    nans, host = 300, host_stores[key]
    if name == "cor2":
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans, compute_dtype=dt), 0).to(dev())
    else:
        model = seeded.load_state(ODAModel(["PAD", "UNK"], nans, regions=36, region_counts=name == "oda-counts"), 0).to(dev())
    idx, v, v_len, q, a = _model_batch(host, B, nans, seed=31)
    keys_before = set(model.state_dict())
    for store_dt in ((F32, BF) if name == "cor2" else (F32,)):
        # an fp32 model on a bf16 store: the padded bf16 transport; a bf16 model on an fp32 store: the padded fp32 'v' it casts
        ds = feed.DeviceFeatureStore(host, dev(), dtype=store_dt)
        assert model.use_region_store(ds) is model and set(model.state_dict()) == keys_before
        padded = {"v": v.to(store_dt).to(dev()), "q_idxes": q}
        if v_len is not None:
            padded["v_len"] = v_len.to(dev())
        for indices in (idx, idx.to(dev()), idx.long().to(dev())):        # host (checked), device, int64
            for train in (False, True):
                want = _fwd_bwd(model, padded, a, train)
                got = _fwd_bwd(model, {"v_idx": indices, "q_idxes": q}, a, train)
                _assert_same_run(got, want, (name, str(dt), str(store_dt), "train" if train else "eval", indices.device.type))
    model.use_region_store(None)
    with pytest.raises(ValueError, match="use_region_store"):
        model({"v_idx": idx.to(dev()), "q_idxes": q})


def test_models_refuse_a_store_or_batch_that_does_not_fit(host_stores):
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel, feed
    with_counts = feed.DeviceFeatureStore(host_stores[36], dev())
    idx, v, v_len, q, a = _model_batch(host_stores[36], 4, 50, seed=3)
    oda = ODAModel(["PAD", "UNK"], 50).eval().to(dev()).use_region_store(with_counts)
    with pytest.raises(ValueError, match="region_counts=True"):                     # the default ODA model: its existing refusal
        oda({"v_idx": idx.to(dev()), "q_idxes": q})
    with pytest.raises(ValueError, match="does not fit"):
        ODAModel(["PAD", "UNK"], 50, regions=36).use_region_store(feed.DeviceFeatureStore(host_stores[100], dev()))
    cor2 = CoR2Model(["PAD", "UNK"], 50).eval().to(dev()).use_region_store(with_counts)
    for key, t in (("v", v), ("v_len", v_len)):
        with pytest.raises(ValueError, match="not both"):
            cor2({"v_idx": idx.to(dev()), key: t.to(dev()), "q_idxes": q})
    with pytest.raises(IndexError):
        cor2({"v_idx": torch.tensor([0, 1, 2, 40]), "q_idxes": q})


# ================================================================================================================================ C
def _launch_names(monkeypatch, model, sample, a):
    from vqa_playground_pytorch_amd import ops as o
    with monkeypatch.context() as m:
        seen = spy_launches(m, o)
        torch.manual_seed(5)
        model.zero_grad(set_to_none=True)
        RF.kld_sum_loss(model(sample), a).backward()
        torch.cuda.synchronize()
    return [name for name, _ in seen]


def test_a_batch_without_v_idx_launches_the_same_with_and_without_a_store(monkeypatch, host_stores):
    from vqa_playground_pytorch_amd import CoR2Model, feed
    host = host_stores[36]
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], 300), 0).train().to(dev())
    idx, v, v_len, q, a = _model_batch(host, 64, 300, seed=31)
    ds, ds_bf = feed.DeviceFeatureStore(host, dev()), feed.DeviceFeatureStore(host, dev(), dtype=BF)
    packed = torch.zeros(64 * 36, 2048)
    host.gather_packed(idx.tolist(), packed, torch.zeros(64, dtype=torch.int32))
    forms = {"padded": {"v": v.to(dev()), "q_idxes": q}, "padded+len": {"v": v.to(dev()), "v_len": v_len.to(dev()), "q_idxes": q},
             "bf16": {"v": v.to(BF).to(dev()), "v_len": v_len.to(dev()), "q_idxes": q},
             "packed": {"v_packed": packed.to(dev()), "v_len": v_len.to(dev()), "q_idxes": q}}
    detached = {k: _launch_names(monkeypatch, model, s, a) for k, s in forms.items()}
    model.use_region_store(ds)
    attached = {k: _launch_names(monkeypatch, model, s, a) for k, s in forms.items()}
    assert attached == detached and all("gather_regions" not in names for names in detached.values())
    assert detached["bf16"] == ["widen_bf16"] + detached["padded+len"] and detached["packed"] == ["unpack_regions"] + detached["padded+len"]
    # the 'v_idx' batch: the one gather launch in front of the masked launches -- also where it widens (one launch, not two)
    assert _launch_names(monkeypatch, model, {"v_idx": idx.to(dev()), "q_idxes": q}, a) == ["gather_regions"] + detached["padded+len"]
    model.use_region_store(ds_bf)
    assert _launch_names(monkeypatch, model, {"v_idx": idx.to(dev()), "q_idxes": q}, a) == ["gather_regions"] + detached["padded+len"]


# ================================================================================================================================ D
NANS = 300


def _records(n, n_img=40, seed=2):
    rs = np.random.RandomState(seed)
    return [{"v_idx": int(rs.randint(n_img)), "q_idxes": rs.standard_normal(2400).astype(np.float32), "q_id": 1000 + i,
             "a_10_idx": [(int(c), 0.25) for c in rs.choice(NANS, 4, replace=False)]} for i in range(n)]


def _feed(host, ds, qa, B, depth=2, spy=None):
    from vqa_playground_pytorch_amd import feed
    pre = feed.DevicePrefetcher(feed.store_batches(host, qa, B, NANS, q_dtype=F32, resident=ds, ring=depth + 2), dev(), depth=depth)
    if spy is not None:
        real = pre._copy
        pre._copy = lambda key, dst, src: (spy.append((key, src.numel() * src.element_size())), real(key, dst, src))[1]
    return pre


def _train(host, ds, qa, B, capture=True, spy=None):
    """six full steps over the prefetcher's two device slots + one short last batch -> per-step (loss, norm, replayed, the batch's
    'v_idx' if it has one), the parameters after the six steps and after the last one, the trainer"""
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    torch.manual_seed(21)
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).train().to(dev()).use_region_store(ds)
    tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True, adopt_inputs=True, input_slots=2)
    if not capture:
        tr.EAGER_STEPS_BEFORE_CAPTURE = 10 ** 9         # never captures: every step is launched kernel by kernel
    steps, after_six = [], None
    for i, b in enumerate(_feed(host, ds, qa, B, spy=spy)):
        sample = {k: b[k] for k in b if k in ("v", "v_idx", "v_len", "q_idxes")}
        replay = tr._graph is not None and b["a"].shape == tr._graph["target"].shape and tr._slot_of(sample, b["a"]) is not None
        seen = (b["v_idx"].data_ptr(), b["v_idx"].tolist()) if "v_idx" in b else None
        loss, norm = tr.step(sample, b["a"])
        steps.append((loss.detach().clone(), norm.detach().clone(), replay, seen))
        if i == 5:
            after_six = [p.detach().clone() for p in model.parameters()]
    return steps, after_six, [p.detach().clone() for p in model.parameters()], tr


def test_captured_step_on_resident_batches_equals_host_fed_and_eager(host_stores):
    """B 64 x N 36, fp32, train mode, a store with counts.  'v_idx' batches through the captured step against (a) the same records
    host-fed as padded 'v' + 'v_len', captured too, and (b) the resident steps launched kernel by kernel by the same trainer code
    with the replay's device-side seed and step scalars (a trainer that never captures): losses, gradient norms and parameters
    bit for bit.  The replays read 'v_idx' out of the prefetcher's two device slots, whose contents change from batch to batch:
    equality with (a) on every step says each replay followed its own indices.  The last batch is short (24 samples): it runs
    kernel by kernel in (a) and in the resident run alike, and matches."""
    from vqa_playground_pytorch_amd import feed
    host = host_stores[36]
    ds = feed.DeviceFeatureStore(host, dev())
    B = 64
    qa = _records(6 * B + 24)
    copied = []
    got, got_six, got_end, tr = _train(host, ds, qa, B, spy=copied)
    assert len(got) == 7
    warm = tr.EAGER_STEPS_BEFORE_CAPTURE
    assert tr._graph is not None and len(tr._slots) == 2, "the resident step was not captured on both ring slots"
    for s in tr._slots:
        assert set(s["sample"]) == {"v_idx", "q_idxes"} and s["sample"]["v_idx"].shape == (B,) and s["sample"]["v_idx"].dtype == torch.int32
        assert sum(t.numel() * t.element_size() for t in s["sample"].values()) == B * (4 + 2400 * 4), "a region-sized tensor in the slot"
    assert [r for _, _, r, _ in got] == [False] * (warm + 1) + [True] * (5 - warm) + [False], "steps after the warm-up are replays"
    seen = [s for _, _, _, s in got[:6]]
    assert len({p for p, _ in seen}) == 2, "the prefetcher's two device slots"
    for i, (p, ix) in enumerate(seen):
        if got[i][2]:           # a replay: the slot's 'v_idx' held other indices at every earlier step, the capture among them
            earlier = [jx for q, jx in seen[:i] if q == p]
            assert earlier and all(jx != ix for jx in earlier), ("step %d replayed the indices its slot was captured with" % i)
    # what crossed the bus: per batch 'v_idx' (4 bytes a sample), the question vectors, the targets, the ids -- no region rows
    per_sample = 4 + 2400 * 4 + NANS * 4 + 8
    assert sorted({k for k, _ in copied}) == ["a", "q_id", "q_idxes", "v_idx"]
    assert sum(n for _, n in copied) == (6 * B + 24) * per_sample and per_sample < 2048 * 4 * 2
    want, want_six, want_end, tr_p = _train(host, None, qa, B)
    assert all("v" in s["sample"] and "v_len" in s["sample"] for s in tr_p._slots)
    assert [r for _, _, r, _ in want] == [r for _, _, r, _ in got]
    # each forward graph holds ONE gather node: phase by phase the captured graphs have the padded run's kernel nodes, but for
    # the phase that reads the regions, which has one more
    extra = {k: tr.graph_nodes[k]["kernel"] - tr_p.graph_nodes[k]["kernel"] for k in tr_p.graph_nodes}
    assert set(tr.graph_nodes) == set(tr_p.graph_nodes) and sorted(extra.values()) == [0] * (len(extra) - 1) + [1], extra
    for i, ((l0, n0, _, _), (l1, n1, _, _)) in enumerate(zip(got, want)):
        assert _same_bits(l0, l1) and _same_bits(n0, n1), ("resident against host-fed padded, step %d" % i, l0, l1, n0, n1)
    assert all(_same_bits(x, y) for x, y in zip(got_six, want_six)) and all(_same_bits(x, y) for x, y in zip(got_end, want_end))
    # (the six full steps: the short last batch draws its dropout seed on the host in a capturing trainer, on the device in this one)
    eager, eager_six, _, tr_e = _train(host, ds, qa, B, capture=False)
    assert tr_e._graph is None and not any(r for _, _, r, _ in eager)
    for i, ((l0, n0, _, _), (l1, n1, _, _)) in enumerate(zip(got[:6], eager[:6])):
        assert _same_bits(l0, l1) and _same_bits(n0, n1), ("replayed against kernel by kernel, step %d" % i, l0, l1, n0, n1)
    assert all(_same_bits(x, y) for x, y in zip(got_six, eager_six))


def test_a_switch_between_padded_and_resident_batches_runs_kernel_by_kernel(host_stores):
    from vqa_playground_pytorch_amd import CoR2Model, feed
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    host = host_stores[36]
    ds = feed.DeviceFeatureStore(host, dev())
    idx, v, v_len, q, a = _model_batch(host, 8, NANS, seed=4)
    forms = {"v": {"v": v.to(dev()), "v_len": v_len.to(dev()), "q_idxes": q}, "v_idx": {"v_idx": idx.to(dev()), "q_idxes": q}}
    out = {}
    for first in ("v", "v_idx"):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).eval().to(dev()).use_region_store(ds)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
        other = "v_idx" if first == "v" else "v"
        losses = [tr.step(forms[first], a)[0].clone() for _ in range(tr.EAGER_STEPS_BEFORE_CAPTURE + 1)]
        assert tr._graph is not None and first in tr._graph["sample"] and other not in tr._graph["sample"]
        losses.append(tr.step(forms[other], a)[0].clone())          # the other form: not the captured keys -> kernel by kernel
        losses.append(tr.step(forms[first], a)[0].clone())          # ... and the graph still serves the form it holds
        out[first] = losses
    assert all(bool(torch.isfinite(x)) for x in out["v"] + out["v_idx"])
    assert all(_same_bits(x, y) for x, y in zip(out["v"], out["v_idx"])), "the same batch, as rows or as indices: the same steps"


def test_evaluator_on_resident_batches_gives_the_padded_run(host_stores):
    from vqa_playground_pytorch_amd import CoR2Model, feed
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    host = host_stores[36]
    ds = feed.DeviceFeatureStore(host, dev())
    B = 8
    qa = _records((Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 2) * B + 3, seed=6)
    out = {}
    for resident in (None, ds):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).to(dev()).use_region_store(ds)
        ev = Evaluator(model, graph=True)
        steps = []
        for b in feed.store_batches(host, qa, B, NANS, q_dtype=F32, resident=resident, pin=False):
            steps.append({k: t.clone() for k, t in ev.step(b).items() if t is not None})
        assert ev._graph is not None and ("v_idx" in ev._graph["inputs"]) == (resident is not None)
        assert ("v" in ev._graph["inputs"]) == (resident is None) and ("v_len" in ev._graph["inputs"]) == (resident is None)
        run = Evaluator(model, graph=True).run(feed.store_batches(host, qa, B, NANS, q_dtype=F32, resident=resident, pin=False))
        out[resident is not None] = (steps, run)
    assert len(out[True][0]) == Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 3
    for plain, got in zip(out[False][0], out[True][0]):
        assert set(plain) == set(got) and all(_same_bits(plain[k], got[k]) if plain[k].is_floating_point() else torch.equal(plain[k], got[k])
                                              for k in plain), "answers and scores"
    assert out[True][1] == out[False][1] and out[True][1][1] is not None
