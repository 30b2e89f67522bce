"""Packed (ragged) region batches on the GPU: vqa_unpack_regions (csrc/region_unpack.hip) through the C ABI, and 'v_packed' through
the models, the trainer's captured step, the prefetcher's copies and the evaluator.  The feature copies rows and widens bf16
exactly, so every comparison here is of bits.

  A  the kernel's three forms against the host restatement of the format; padding comes back +0.0, nothing outside the output window
     is touched, no NaN of the packed buffer's dead rows or of the pre-filled window survives; one launch whose grid depends on
     (B, N, D) alone; refusals launch nothing.
  B  CoR2Model (fp32 B 64 x N 36, bf16 B 16 x N 100) and ODAModel(region_counts=True) on a packed batch against the same batch
     padded: logits, loss, alphas, every parameter gradient, eval and train mode; bf16 transport against a padded bf16 'v'.
  C  a batch without 'v_packed' launches what it launched before this feature existed.
  D  DataParallelTrainer(graph=True) fed by store_batches(packed=True) + DevicePrefetcher against the same steps padded and against
     the packed steps launched kernel by kernel; the prefetcher copies R rows; the evaluator."""
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
KERNEL = "(unpack_regions_kernel<%s,%s>)"
TARGET_WGS, THREADS = 1024, 256
# D = 8: one 16-byte unit per bf16 row, every B (1, 2, across a wave, across a 256-thread workgroup of the prefix sum) with every N
# (1, a multiple and a non-multiple of the row chunk, 100); D = 2048 (the models' rows: 256 units, two per thread) where the chunking
# of a sample's rows changes: one sample (N chunks), two, B = 65 (N = 37: chunks of 3 rows, the last one short) and B = 257 (4 chunks)
SHAPES = [(B, N, 8) for B in (1, 2, 65, 257) for N in (1, 36, 37, 100)] + \
         [(1, 1, 2048), (1, 37, 2048), (2, 36, 2048), (2, 100, 2048), (65, 37, 2048), (257, 36, 2048)]
MULTI_PASS = (1031, 3, 8)          # every thread of the prefix sum takes more than four counts


def _grid(B, N):
    chunks = min(_ceil(TARGET_WGS, B), N)
    rows = _ceil(N, chunks)
    return B * _ceil(N, rows) * THREADS


def _counts(B, N, kind, rs):
    if kind == "full":
        return np.full(B, N, np.int64)
    if kind == "ones":
        return np.ones(B, np.int64)
    if kind == "random":
        return rs.randint(1, N + 1, B)
    lens = np.ones(B, np.int64)
    lens[B // 2] = N                # one sample with every row, every other with one
    return lens


def unpack_host(packed, lens, N):
    """the format, restated on the host: out[b, i] = packed[off[b] + i] for i < lens[b], off the exclusive prefix sum; +0.0 behind"""
    lens = torch.as_tensor(lens, dtype=torch.int64)
    off = torch.cumsum(lens, 0) - lens
    i = torch.arange(N)
    real = i[None, :] < lens[:, None]
    rows = torch.where(real, off[:, None] + i[None, :], 0)
    out = packed[rows.reshape(-1)].view(len(lens), N, packed.size(1)).clone()
    out[~real] = 0.0
    return out


def _packed_buffer(rows_host, B, N, dt):
    """device buffer of B*N rows with NaN in front, behind, and in every row from R on; the R real rows PAD elements in"""
    R, D = rows_host.shape
    buf = torch.full((B * N * D + 2 * PAD,), NAN, dtype=dt)
    buf[PAD:PAD + R * D] = rows_host.reshape(-1)
    return buf.to(dev())


def _nan_window(n, dt):
    buf = _out(n, dt)
    buf[PAD:PAD + n] = NAN
    return buf


def _run(ops, packed_d, lens_d, B, N, D, dt_in, dt_out, packed_off=PAD, out_off=PAD):
    buf = _nan_window(B * N * D, dt_out)
    rc, log = _call(ops, ops._lib.lib().vqa_unpack_regions, _ptr(packed_d, packed_off), _ptr(lens_d), _ptr(buf, out_off), B, N, D,
                    int(dt_in == BF), int(dt_out == BF))
    return rc, log, buf


def _kernel_case(ops, B, N, D, kinds=("full", "ones", "random", "one-long")):
    rs = np.random.RandomState(B * 1000 + N + D)
    gen = torch.Generator().manual_seed(B + N + D)
    source = torch.randn(B * N, D, generator=gen)
    grids = set()
    for kind in kinds:
        lens = _counts(B, N, kind, rs)
        R = int(lens.sum())
        lens_d = torch.from_numpy(lens.astype(np.int32)).to(dev())
        for dt_in, dt_out in FORMS:
            what = "B=%d N=%d D=%d %s %s->%s" % (B, N, D, kind, dt_in, dt_out)
            rows = source[:R].to(dt_in)
            packed_d = _packed_buffer(rows, B, N, dt_in)
            rc, log, buf = _run(ops, packed_d, lens_d, B, N, D, dt_in, dt_out)
            assert rc == 0, (what, rc, ops._lib.lib().vqa_last_error())
            name = KERNEL % (str(dt_in == BF).lower(), str(dt_out == BF).lower())
            assert log == [(name, _grid(B, N))], (what, log)
            grids.add(log[0][1])
            got = _win(buf, (B, N, D), what).cpu()
            want = unpack_host(rows, lens, N).to(dt_out)          # (bf16 -> fp32: exact)
            assert not bool(torch.isnan(got.float()).any()), (what, "a NaN of the dead rows or of the pre-filled window came through")
            assert _same_bits(got, want), (what, "differs from the host restatement (a -0.0 on the padding counts)")
            if kind == "full":
                assert _same_bits(got.view(B * N, D), rows.to(dt_out)), what
                if (dt_in, dt_out) == (BF, F32):
                    assert _same_bits(got, ops.widen_bf16(rows.to(dev())).view(B, N, D).cpu()), (what, "not the bits of widen_bf16")
            if kind == "random":
                rc2, log2, buf2 = _run(ops, packed_d, lens_d, B, N, D, dt_in, dt_out)
                assert rc2 == 0 and log2 == log and _same_bits(_win(buf2, (B, N, D), what).cpu(), got), (what, "second run")
    assert len(grids) == 1, ("the grid depends on the counts", B, N, D, grids)


@pytest.mark.parametrize("B,N,D", SHAPES, ids=["B%d-N%d-D%d" % s for s in SHAPES])
def test_unpack_kernel_against_the_host_restatement(ops, B, N, D):
    _kernel_case(ops, B, N, D)


def test_unpack_kernel_prefix_sum_over_many_passes(ops):
    _kernel_case(ops, *MULTI_PASS, kinds=("random", "one-long"))


def test_unpack_kernel_clamps_the_counts_it_reads(ops):
    """counts outside 0..N in DEVICE memory (the host ones are refused by ops.region_counts): clamped, so the rows read stay inside
    the B*N of the buffer and the result is that of the clamped counts"""
    B, N, D = 5, 4, 8
    given = np.array([9, -3, 2, 4, 1000000])
    lens = np.clip(given, 0, N)
    rows = torch.randn(int(lens.sum()), D, generator=torch.Generator().manual_seed(1))
    rc, log, buf = _run(ops, _packed_buffer(rows, B, N, F32), torch.from_numpy(given.astype(np.int32)).to(dev()), B, N, D, F32, F32)
    assert rc == 0 and len(log) == 1
    assert _same_bits(_win(buf, (B, N, D), "clamped").cpu(), unpack_host(rows, lens, N))


def test_unpack_kernel_refusals_launch_nothing(ops):
    L = ops._lib.lib()
    B, N, D = 2, 3, 16
    lens_d = torch.tensor([3, 1], dtype=torch.int32, device=dev())
    packed_d = _packed_buffer(torch.randn(4, D), B, N, F32)

    def refused(code, *args, **kw):
        rc, log, buf = _run(ops, *args, **kw)
        assert rc == code and log == [], (rc, log, L.vqa_last_error())
        buf[PAD:PAD + B * N * D] = -12345.0
        assert _untouched(buf)
    refused(E_UNSUPPORTED, packed_d, lens_d, B, N, 12, F32, F32)                    # D % 8
    refused(E_UNSUPPORTED, packed_d, lens_d, B, N, D, F32, F32, packed_off=PAD + 1)     # packed 4 bytes off a 16-byte boundary
    refused(E_UNSUPPORTED, packed_d, lens_d, B, N, D, F32, F32, out_off=PAD + 1)        # out 4 bytes off
    refused(E_UNSUPPORTED, packed_d, lens_d, B, N, D, F32, BF)                      # fp32 rows are not narrowed
    refused(E_BADARG, packed_d, lens_d, 0, N, D, F32, F32)
    out = _out(B * N * D)
    for args in ((None, _ptr(lens_d), _ptr(out, PAD)), (_ptr(packed_d, PAD), None, _ptr(out, PAD)), (_ptr(packed_d, PAD), _ptr(lens_d), None)):
        rc, log = _call(ops, L.vqa_unpack_regions, *args, B, N, D, 0, 0)
        assert rc == E_BADARG and log == []
    rc, log = _call(ops, L.vqa_unpack_regions, _ptr(packed_d, PAD), ctypes.c_void_p(lens_d.data_ptr() + 4), _ptr(out, PAD), 1, N, D, 0, 0)
    assert rc == E_UNSUPPORTED and log == []                                        # lens 4 bytes off
    assert _untouched(out)


def test_ops_unpack_regions_on_the_device(ops):
    """the wrapper: one logged launch, the CPU definition's bits, a misaligned slice of counts served"""
    B, N, D = 6, 5, 2048
    lens = torch.tensor([9, 9, 5, 1, 3, 2, 5, 4], dtype=torch.int32)
    rows = torch.randn(B * N, D, generator=torch.Generator().manual_seed(2)).to(BF)
    v_len = lens.to(dev())[2:]                          # 8 bytes off a 16-byte boundary
    for dt_in, dt_out in FORMS:
        got = ops.unpack_regions(rows.to(dt_in).to(dev()), v_len, B, dt_out)
        assert got.shape == (B, N, D) and _same_bits(got.cpu(), ops.unpack_regions(rows.to(dt_in), lens[2:], B, dt_out))
    with pytest.raises(ValueError):
        ops.unpack_regions(rows.float().to(dev()), lens[2:], B)              # counts on another device


# ================================================================================================================================ B
def _batch(B, N, nans, seed):
    """-> (padded v [B,N,2048] with zeros behind the counts, packed rows [B*N, 2048] whose dead rows are NaN, v_len, q, a), host"""
    rs = np.random.RandomState(seed)
    v_len = rs.randint(1, N + 1, size=B)
    v_len[min(3, B - 1)], v_len[B - 2] = 1, N
    v, q, a = seeded.seeded_inputs(B, regions=N, answers=nans, seed=seed)
    v = torch.from_numpy(v).to(BF).float()             # (bf16-exact rows: the bf16 transport carries the same values)
    packed = torch.full((B * N, 2048), NAN)
    off = 0
    for b, n in enumerate(v_len):
        v[b, n:] = 0.0
        packed[off:off + n] = v[b, :n]
        off += n
    return v, packed, torch.from_numpy(v_len.astype(np.int32)), torch.from_numpy(q), torch.from_numpy(a)


def _alphas(model):
    out = {}
    for k, x in model.alpha_dict.items():
        out[k] = torch.cat(list(x), -1).detach().clone() if isinstance(x, (list, tuple)) else x.detach().clone()
    return out


def _fwd_bwd(model, regions, q, a, v_len, train):
    model.train(train)
    model.zero_grad(set_to_none=True)
    torch.manual_seed(5)                    # (the fused masks' seeds are drawn from torch's CPU generator)
    logits = model(dict(regions, q_idxes=q.to(dev()), v_len=v_len))
    loss = RF.kld_sum_loss(logits, a.to(dev()))
    loss.backward()
    return logits.detach().clone(), loss.detach().clone(), _alphas(model), {n: p.grad.detach().clone() for n, p in model.named_parameters()}


def _assert_same_run(got, want, what):
    assert _same_bits(got[0], want[0]), (what, "logits")
    assert _same_bits(got[1], want[1]), (what, "loss")
    assert set(got[2]) == set(want[2]) and all(_same_bits(got[2][k], want[2][k]) for k in want[2]), (what, "alphas")
    differ = [n for n in want[3] if not _same_bits(got[3][n], want[3][n])]
    assert not differ, (what, differ)
    assert all(bool(torch.isfinite(g).all()) for g in got[3].values()), what


MODELS = [("cor2", F32, 64, 36), ("cor2", BF, 16, 100), ("oda", F32, 64, 36)]


@pytest.mark.parametrize("name,dt,B,N", MODELS, ids=["cor2-f32-B64-N36", "cor2-bf16-B16-N100", "oda-f32-B64-N36"])
def test_models_on_a_packed_batch_equal_the_padded_batch(name, dt, B, N):
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel
    nans = 300
    if name == "cor2":
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], nans, compute_dtype=dt), 0).to(dev())
    else:
        model = seeded.load_state(ODAModel(["PAD", "UNK"], nans, regions=N, region_counts=True), 0).to(dev())
    v, packed, v_len, q, a = _batch(B, N, nans, seed=31)
    for counts in (v_len, v_len.to(dev())):             # host counts (validated) and device counts
        for train in (False, True):
            for transport in ((F32, BF) if name == "cor2" else (F32,)):
                want = _fwd_bwd(model, {"v": v.to(transport).to(dev())}, q, a, counts, train)
                got = _fwd_bwd(model, {"v_packed": packed.to(transport).to(dev())}, q, a, counts, train)
                _assert_same_run(got, want, (name, str(dt), "train" if train else "eval", str(transport), counts.device.type))


def test_default_oda_model_refuses_a_packed_batch():
    from vqa_playground_pytorch_amd import ODAModel
    model = ODAModel(["PAD", "UNK"], 50).eval().to(dev())
    v, packed, v_len, q, a = _batch(4, 36, 50, seed=3)
    with pytest.raises(ValueError, match="region_counts=True"):
        model({"v_packed": packed.to(dev()), "v_len": v_len, "q_idxes": q.to(dev())})
    with pytest.raises(ValueError, match="region_counts=True"):
        model({"v_packed": packed.to(dev()), "q_idxes": q.to(dev())})


# ================================================================================================================================ C
# The ops-level launches (ops._launch's names, in order) of one CoR2Model forward + backward on a padded batch, B 64 x N 36, fp32,
# train mode, recorded on the commit before packed batches existed: without 'v_len' and with it.
_PARENT_UNMASKED = [
    "dropout_groups_fwd", "grouped_gemm", "grouped_epilogue", "grouped_gemm", "grouped_epilogue", "linear_act_fwd_split",
    "lowrank_bilinear_fusion_fwd", "attention_logits_fwd", "softmax_attention_pool_drop_fwd", "bias_act", "gate_product_fwd",
    "relation_linear_fwd_split", "lowrank_bilinear_fusion_fwd", "attention_logits_fwd", "softmax_attention_pool_fwd",
    "relation_apply_fwd", "bias_act", "grouped_gemm", "grouped_epilogue", "grouped_epilogue", "grouped_gemm",
    "grouped_epilogue", "grouped_gemm", "grouped_epilogue", "grouped_epilogue", "grouped_gemm", "grouped_epilogue",
    "act_bwd_colsum", "relation_apply_bwd", "softmax_attention_pool_bwd", "attention_logits_bwd", "lowrank_bilinear_fusion_bwd",
    "relation_linear_dw_split", "relation_projection_dgrad_split", "gate_product_bwd", "act_bwd_colsum",
    "softmax_attention_pool_drop_bwd", "attention_logits_bwd", "lowrank_bilinear_fusion_bwd", "linear_act_dw_split",
    "grouped_epilogue", "grouped_gemm", "grouped_epilogue", "grouped_gemm"]
_K3_MASKED = {"softmax_attention_pool_drop_fwd": "softmax_attention_pool_len_fwd",
              "softmax_attention_pool_fwd": "softmax_attention_pool_len_fwd",
              "softmax_attention_pool_bwd": "softmax_attention_pool_len_bwd",
              "softmax_attention_pool_drop_bwd": "softmax_attention_pool_len_bwd"}
PARENT_LAUNCHES = {False: _PARENT_UNMASKED, True: [_K3_MASKED.get(name, name) for name in _PARENT_UNMASKED]}      # (K3 alone differs)


def _launch_names(monkeypatch, sample, a):
    from vqa_playground_pytorch_amd import CoR2Model, ops as o
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], 300), 0).train().to(dev())
    with monkeypatch.context() as m:
        seen = spy_launches(m, o)
        torch.manual_seed(5)
        RF.kld_sum_loss(model(sample), a).backward()
        torch.cuda.synchronize()
    return [name for name, _ in seen]


def test_a_padded_batch_launches_what_it_launched_before(monkeypatch):
    for with_len in (False, True):
        _padded_and_packed_launches(monkeypatch, with_len)


def _padded_and_packed_launches(monkeypatch, with_len):
    v, packed, v_len, q, a = _batch(64, 36, 300, seed=31)
    sample = {"v": v.to(dev()), "q_idxes": q.to(dev())}
    if with_len:
        sample["v_len"] = v_len.to(dev())
    names = _launch_names(monkeypatch, sample, a.to(dev()))
    assert "unpack_regions" not in names
    assert names == PARENT_LAUNCHES[with_len], names
    packed_names = _launch_names(monkeypatch, {"v_packed": packed.to(dev()), "v_len": v_len.to(dev()), "q_idxes": q.to(dev())}, a.to(dev()))
    if with_len:                            # the packed batch: the one unpack launch in front of the same launches
        assert packed_names == ["unpack_regions"] + names
    bf16 = dict(sample, v=sample["v"].to(BF))         # bf16 transport, padded: still widened by widen_bf16
    assert _launch_names(monkeypatch, bf16, a.to(dev())) == ["widen_bf16"] + names
    if with_len:                            # ... and packed: the unpack launch does the widening (one launch, not two)
        packed_bf = {"v_packed": packed.to(BF).to(dev()), "v_len": v_len.to(dev()), "q_idxes": q.to(dev())}
        assert _launch_names(monkeypatch, packed_bf, a.to(dev())) == ["unpack_regions"] + names


# ================================================================================================================================ D
N_IMG, NANS = 40, 300


@pytest.fixture(scope="module")
def stores(tmp_path_factory):
    """a padded store with counts (zero-padded, bf16-exact values) and the ragged store of the same rows; built once, never changed"""
    from vqa_playground_pytorch_amd import feed
    root = tmp_path_factory.mktemp("packed")
    rs = np.random.RandomState(7)
    feats = torch.from_numpy(rs.standard_normal((N_IMG, 36, 2048)).astype(np.float32)).to(BF).float().numpy()
    cnt = rs.randint(1, 37, N_IMG)
    cnt[0], cnt[1] = 1, 36
    for i, c in enumerate(cnt):
        feats[i, c:] = 0.0
    np.save(root / "padded.npy", feats)
    np.save(root / "rows.npy", np.concatenate([feats[i, :c] for i, c in enumerate(cnt)]))
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    padded = feed.FeatureStore(root / "padded.npy", workers=2, counts=cnt)
    ragged = feed.FeatureStore(root / "rows.npy", workers=2, offsets=offsets, regions=36)
    return padded, ragged


def _records(n, seed=2):
    rs = np.random.RandomState(seed)
    return [{"v_idx": int(rs.randint(N_IMG)), "q_idxes": rs.standard_normal(2400).astype(np.float32), "q_id": 1000 + i,
             "a_10_idx": [(int(c), 0.25) for c in rs.choice(NANS, 4, replace=False)]} for i in range(n)]


def _feed(store, qa, B, packed, depth=2, **kw):
    from vqa_playground_pytorch_amd import feed
    return feed.DevicePrefetcher(feed.store_batches(store, qa, B, NANS, q_dtype=F32, packed=packed, ring=depth + 2, **kw), dev(), depth=depth)


def _train(store, qa, B, packed, capture=True):
    """six full steps over the prefetcher's two device slots + one short last batch -> per-step (loss, norm, replayed), the
    parameters after the six steps and after the last one, the trainer"""
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    torch.manual_seed(21)
    model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).train().to(dev())
    tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True, adopt_inputs=True, input_slots=2)
    if not capture:
        tr.EAGER_STEPS_BEFORE_CAPTURE = 10 ** 9         # never captures: every step is launched kernel by kernel
    steps, after_six = [], None
    for i, b in enumerate(_feed(store, qa, B, packed)):
        sample = {k: b[k] for k in b if k in ("v", "v_packed", "v_len", "q_idxes")}
        replay = tr._graph is not None and b["a"].shape == tr._graph["target"].shape and tr._slot_of(sample, b["a"]) is not None
        loss, norm = tr.step(sample, b["a"])
        steps.append((loss.detach().clone(), norm.detach().clone(), replay))
        if i == 5:
            after_six = [p.detach().clone() for p in model.parameters()]
    return steps, after_six, [p.detach().clone() for p in model.parameters()], tr


def test_captured_step_on_packed_batches_equals_padded_and_eager(stores):
    """B 64 x N 36, fp32, train mode, counts that differ in every batch.  Packed batches through the captured step against (a) the
    same steps on padded batches, captured too, and (b) the packed steps launched kernel by kernel by the same trainer code with the
    replay's device-side seed and step scalars (a trainer that never captures): losses, gradient norms and parameters bit for bit.
    The last batch is short (24 samples): it runs kernel by kernel in (a) and in the packed run alike, and matches."""
    padded, ragged = stores
    B = 64
    qa = _records(6 * B + 24)
    got, got_six, got_end, tr = _train(ragged, qa, B, packed=True)
    assert len(got) == 7
    warm = tr.EAGER_STEPS_BEFORE_CAPTURE
    assert tr._graph is not None and len(tr._slots) == 2, "the packed step was not captured on both ring slots"
    assert all("v_packed" in s["sample"] and "v_len" in s["sample"] and "v" not in s["sample"] for s in tr._slots)
    assert tr._slots[0]["sample"]["v_packed"].shape == (B * 36, 2048)
    assert [r for _, _, r in got] == [False] * (warm + 1) + [True] * (5 - warm) + [False], "steps after the warm-up are replays"
    want, want_six, want_end, tr_p = _train(padded, qa, B, packed=False)
    assert [r for _, _, r in want] == [r for _, _, r in got]
    for i, ((l0, n0, _), (l1, n1, _)) in enumerate(zip(got, want)):
        assert _same_bits(l0, l1) and _same_bits(n0, n1), ("packed against padded, step %d" % i, l0, l1, n0, n1)
    assert all(_same_bits(x, y) for x, y in zip(got_six, want_six)) and all(_same_bits(x, y) for x, y in zip(got_end, want_end))
    eager, eager_six, _, tr_e = _train(ragged, qa, B, packed=True, capture=False)
    assert tr_e._graph is None and not any(r for _, _, r in eager)
    for i, ((l0, n0, _), (l1, n1, _)) in enumerate(zip(got[:6], eager[:6])):
        assert _same_bits(l0, l1) and _same_bits(n0, n1), ("replayed against kernel by kernel, step %d" % i, l0, l1, n0, n1)
    assert all(_same_bits(x, y) for x, y in zip(got_six, eager_six))


def test_a_switch_between_padded_and_packed_batches_runs_kernel_by_kernel(stores):
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    v, packed, v_len, q, a = (t.to(dev()) for t in _batch(8, 36, NANS, seed=4))
    out = {}
    for first in ("v", "v_packed"):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).eval().to(dev())
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
        forms = {"v": {"v": v, "v_len": v_len, "q_idxes": q}, "v_packed": {"v_packed": packed, "v_len": v_len, "q_idxes": q}}
        other = "v_packed" if first == "v" else "v"
        losses = [tr.step(forms[first], a)[0].clone() for _ in range(tr.EAGER_STEPS_BEFORE_CAPTURE + 1)]
        assert tr._graph is not None and first in tr._graph["sample"] and other not in tr._graph["sample"]
        losses.append(tr.step(forms[other], a)[0].clone())          # the other form: not the captured keys -> kernel by kernel
        losses.append(tr.step(forms[first], a)[0].clone())          # ... and the graph still serves the form it holds
        out[first] = losses
    assert all(bool(torch.isfinite(x)) for x in out["v"] + out["v_packed"])
    assert _same_bits(out["v"][0], out["v_packed"][0])               # (the first step: same parameters, same batch)


@pytest.mark.parametrize("dt", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("pin", [True, False], ids=["pinned", "staged"])
def test_prefetcher_copies_the_real_rows_only(stores, dt, pin):
    from vqa_playground_pytorch_amd import feed
    _, ragged = stores
    B, D = 16, 2048
    qa = _records(3 * B + 5)
    host, copies = [], []

    def keep(batches):
        for b in batches:
            host.append({k: t.clone() for k, t in b.items()})
            yield b
    pre = feed.DevicePrefetcher(keep(feed.store_batches(ragged, qa, B, NANS, q_dtype=F32, packed=True, ring=4, pin=pin, region_dtype=dt)),
                                dev(), depth=2)
    real = pre._copy
    pre._copy = lambda key, dst, src: (copies.append((key, tuple(src.shape), tuple(dst.shape), src.element_size(), src.is_pinned())),
                                       real(key, dst, src))[1]
    for i, b in enumerate(pre):
        h = host[i]
        R = int(h["v_len"].sum())
        assert b["v_packed"].is_cuda and b["v_packed"].dtype == dt and b["v_packed"].shape == h["v_packed"].shape
        assert b["v_packed"].shape[0] == h["v_len"].numel() * 36, "the yielded tensor is the capacity"
        assert _same_bits(b["v_packed"][:R].cpu(), h["v_packed"][:R])
        assert torch.equal(b["v_len"].cpu(), h["v_len"]) and torch.equal(b["q_id"].cpu(), h["q_id"])
    shapes = [c for c in copies if c[0] == "v_packed"]
    assert len(shapes) == len(host) == 4
    for c, h in zip(shapes, host):
        R = int(h["v_len"].sum())
        assert c[1] == (R, D) and c[2] == (R, D) and c[4], c             # R rows from a page-locked source into R rows
        assert c[1][0] * c[1][1] * c[3] == R * D * (2 if dt == BF else 4)
    assert len(pre.slots) == 2 and all(s["dev"]["v_packed"].shape == (B * 36, D) for s in pre.slots)


def test_evaluator_on_packed_batches_gives_the_padded_run(stores):
    from vqa_playground_pytorch_amd import CoR2Model, feed
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    padded, ragged = stores
    B = 8
    qa = _records((Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 2) * B + 3, seed=6)
    out = {}
    for packed, store in ((False, padded), (True, ragged)):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS), 0).to(dev())
        ev = Evaluator(model, graph=True)
        steps = []
        for b in feed.store_batches(store, qa, B, NANS, q_dtype=F32, packed=packed, pin=False):
            steps.append({k: t.clone() for k, t in ev.step(b).items() if t is not None})
        assert ev._graph is not None and ("v_packed" in ev._graph["inputs"]) == packed and "v_len" in ev._graph["inputs"]
        run = Evaluator(model, graph=True).run(feed.store_batches(store, qa, B, NANS, q_dtype=F32, packed=packed, pin=False))
        out[packed] = (steps, run)
    assert len(out[True][0]) == Evaluator.EAGER_STEPS_BEFORE_CAPTURE + 3
    for plain, got in zip(out[False][0], out[True][0]):
        assert set(plain) == set(got) and all(_same_bits(plain[k], got[k]) if plain[k].is_floating_point() else torch.equal(plain[k], got[k])
                                              for k in plain), "answers and scores"
    assert out[True][1] == out[False][1] and out[True][1][1] is not None
