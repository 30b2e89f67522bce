#!/usr/bin/env python3
"""PCIe-inclusive rate of the CoR2 training step: batches start in (pinned) host memory and are streamed through
feed.DevicePrefetcher while the hipGraph-replayed step runs.  NOT the headline number (bench.py times inputs resident
in HBM); it sizes the feed path of SURVEY 8f row 4.   python tools/feed_bench.py [--steps 30]

    python tools/feed_bench.py --packed [--counts full|uniform|both] [--parent-tree DIR] [--blocks 4] [--steps 20]

--packed: packed (ragged) region batches against padded ones, as ONE JSON line on stdout.  Two shapes: f32 (B = 512, N = 36, fp32
model) and bf16 (B = 128, N = 100, compute_dtype = bfloat16, the shape adaptive features are padded to); counts `full` (every
sample N rows: packed cannot win, same bytes plus a pass) and `uniform` (10..N).  For each:
  unpack_us    vqa_unpack_regions in its three forms beside vqa_widen_bf16 at the same size, microseconds per launch
  gather_ms    the host gather of one batch into pinned staging, dense (vqa_host_gather_rows) against ragged, fp32 and bf16
  fed          samples/s of the captured step fed from a FeatureStore through store_batches + DevicePrefetcher, padded
               ('v' + 'v_len') against packed ('v_packed' + 'v_len'), fp32 and bf16 transport
  step_ms      the captured step on resident inputs, 'v_packed' + 'v_len' against 'v' + 'v_len'
Forms alternate in blocks inside one process; a figure is the median of its blocks, and the blocks are in the record.
--parent-tree DIR: a checkout of the parent commit with its library built; its padded 'v' + 'v_len' step is then timed too, in
child processes that alternate with this tree's.

    python tools/feed_bench.py --resident [--store N_IMG] [--blocks 4] [--steps 30] [--iters 50]

--resident: the device-resident region store (feed.DeviceFeatureStore) against the host feeds, as ONE JSON line on stdout, from one
process in alternating blocks.  The store is the synthetic one of --store N_IMG (default 4096 images x 36 x 2048).
  upload       seconds and nbytes of DeviceFeatureStore(store), fp32 and bf16
  gather_us    vqa_gather_regions in its three forms beside vqa_unpack_regions at the same (B, N, D), B 512 x N 36 and
               B 128 x N 100, microseconds per launch (every sample N rows: the same bytes move)
  fed          samples/s of the captured B 512 x N 36 fp32 step: fed by store_batches(resident=) ('v_idx' batches, fp32 and bf16
               store), fed from the memory-mapped host store with fp32 and bf16 transport, and on rotating batches that are
               already on the device (no feed at all)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:            # (--packed --parent-tree: this file, run on the parent checkout's package)
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from vqa_playground_pytorch_amd import CoR2Model, feed  # noqa: E402
from vqa_playground_pytorch_amd.trainer import DataParallelTrainer  # noqa: E402


PACKED_CONFIGS = {"f32": dict(B=512, N=36, dtype="float32", n_img=1024), "bf16": dict(B=128, N=100, dtype="bfloat16", n_img=512)}
NANS, D = 2000, 2048


def _median(blocks, digits=4):
    return {"median": round(statistics.median(blocks), digits), "min": round(min(blocks), digits), "max": round(max(blocks), digits),
            "blocks": [round(x, digits) for x in blocks]}


def _alternate(forms, blocks):
    """forms: {name: callable -> one figure}; the order reversed every other block -> {name: median / range / blocks}"""
    out = {name: [] for name in forms}
    for i in range(blocks):
        for name in (list(forms) if i % 2 == 0 else list(reversed(list(forms)))):
            out[name].append(forms[name]())
    return {name: _median(v) for name, v in out.items()}


def _gpu_ms(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _counts_of(n, N, kind):
    import numpy as np
    if kind == "full":
        return np.full(n, N, np.int64)
    return np.random.RandomState(17).randint(min(10, N), N + 1, n)


def _packed_of(v, lens):
    """padded [B,N,D] + counts -> the packed capacity buffer [B*N, D] (rows from sum(lens) on stay zero)"""
    out = torch.zeros(v.size(0) * v.size(1), v.size(2), dtype=v.dtype)
    out[:int(lens.sum())] = torch.cat([v[b, :int(n)] for b, n in enumerate(lens)])
    return out


def _unpack_us(cfg, kinds, args, dev):
    from vqa_playground_pytorch_amd import ops
    B, N = cfg["B"], cfg["N"]
    rows = torch.randn(B * N, D, generator=torch.Generator().manual_seed(3))
    forms = {"widen_bf16": lambda x=rows.to(torch.bfloat16).to(dev): ops.widen_bf16(x)}
    for kind in kinds:
        lens = torch.from_numpy(_counts_of(B, N, kind).astype("int32")).to(dev)
        for name, dt_in, dt_out in (("f32", torch.float32, torch.float32), ("bf16", torch.bfloat16, torch.bfloat16),
                                    ("bf16_to_f32", torch.bfloat16, torch.float32)):
            forms["%s_%s" % (name, kind)] = lambda x=rows.to(dt_in).to(dev), lens=lens, dt_out=dt_out: ops.unpack_regions(x, lens, B, dt_out)
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return _alternate({k: (lambda fn=fn: 1e3 * _gpu_ms(fn, args.iters)) for k, fn in forms.items()}, args.blocks)


def _store_for(cfg, kind, workers):
    import numpy as np
    path = "/tmp/feed_bench_store_%dx%d.npy" % (cfg["n_img"], cfg["N"])
    if not os.path.exists(path):
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(cfg["n_img"], cfg["N"], D))
        rs = np.random.RandomState(0)
        for lo in range(0, cfg["n_img"], 128):
            mm[lo:lo + 128] = rs.standard_normal((min(128, cfg["n_img"] - lo), cfg["N"], D)).astype(np.float32)
        mm.flush()
        del mm
    return feed.FeatureStore(path, workers=workers, counts=_counts_of(cfg["n_img"], cfg["N"], kind)).populate()


def _gather_ms(cfg, kinds, args):
    import numpy as np
    B, N = cfg["B"], cfg["N"]
    idx = np.random.RandomState(5).randint(cfg["n_img"], size=B)
    forms = {}
    for kind in kinds:
        store = _store_for(cfg, kind, args.workers)
        for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            dense, ragged = torch.empty(B, N, D, dtype=dt).pin_memory(), torch.empty(B * N, D, dtype=dt).pin_memory()
            v_len = torch.empty(B, dtype=torch.int32)
            if kind == kinds[0]:
                forms["dense_" + name] = lambda store=store, out=dense: store.gather(idx, out)
            forms["ragged_%s_%s" % (name, kind)] = lambda store=store, out=ragged, v_len=v_len: store.gather_packed(idx, out, v_len)

    def timed(fn):
        t0 = time.perf_counter()
        for _ in range(5):
            fn()
        return 1e3 * (time.perf_counter() - t0) / 5
    for fn in forms.values():
        fn()
    return _alternate({k: (lambda fn=fn: timed(fn)) for k, fn in forms.items()}, args.blocks)


def _model(cfg, dev):
    return CoR2Model(["PAD"], NANS, compute_dtype=getattr(torch, cfg["dtype"])).to(dev).train()


def _fed(cfg, kinds, args, dev):
    """samples/s, padded against packed, per transport and count distribution"""
    import numpy as np
    B, depth = cfg["B"], 3
    rec = {}
    for kind in kinds:
        store = _store_for(cfg, kind, args.workers)
        rs = np.random.RandomState(1)
        qa = feed.qa_table(store, [{"v_idx": int(rs.randint(cfg["n_img"])), "q_idxes": rs.standard_normal(2400).astype(np.float32), "q_id": i,
                                    "a_10_idx": [(int(c), 0.1) for c in rs.choice(NANS, 10, replace=False)]} for i in range(B * 8)],
                             NANS, q_dtype=torch.float32)
        for transport, vdt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            forms, loaders = {}, []
            for packed in (False, True):
                tr = DataParallelTrainer(_model(cfg, dev), graph=True, adopt_inputs=True, input_slots=depth)
                loader = feed.store_batches(store, qa, B, NANS, shuffle=True, seed=0, pin=True, region_dtype=vdt, ring=depth + 2 * args.producers + 2,
                                            q_dtype=torch.float32, prefetch=2 * args.producers, epochs=None, producers=args.producers, packed=packed)
                loaders.append(loader)
                for _ in range(depth + 2 * args.producers + 2):      # every ring slot page-locked now: a producer thread that
                    next(loader)                                     # pins memory during a capture would invalidate it
                pre = feed.DevicePrefetcher(iter(()), dev, depth=depth)
                key = "v_packed" if packed else "v"

                def run(n, tr=tr, pre=pre, loader=loader, key=key):
                    pre.it = (next(loader) for _ in range(n))
                    t0 = time.perf_counter()
                    for b in pre:
                        tr.step({key: b[key], "v_len": b["v_len"], "q_idxes": b["q_idxes"]}, b["a"])
                    torch.cuda.synchronize()
                    return B * n / (time.perf_counter() - t0)
                run(4 + 2 * depth)                      # warm-up + one graph per device slot
                assert tr._graph is not None and len(tr._slots) == depth, "the fed step was not captured on every slot"
                forms["packed" if packed else "padded"] = lambda run=run: run(args.steps)
            rec["%s_%s" % (transport, kind)] = _alternate(forms, args.blocks)
            for loader in loaders:
                loader.close()
            del forms
            torch.cuda.empty_cache()
    return rec


def _step_ms(cfg, kinds, args, dev, packed_forms):
    """the captured step on resident inputs: padded 'v' + 'v_len', and (this tree) 'v_packed' + 'v_len'"""
    B, N = cfg["B"], cfg["N"]
    gen = torch.Generator().manual_seed(9)
    v, q = torch.randn(B, N, D, generator=gen), torch.randn(B, 2400, generator=gen)
    a = torch.softmax(torch.randn(B, NANS, generator=gen), 1).to(dev)
    forms, captured = {}, {}
    for kind in kinds:
        lens = torch.from_numpy(_counts_of(B, N, kind).astype("int32"))
        samples = {"padded_" + kind: {"v": v.to(dev), "v_len": lens.to(dev), "q_idxes": q.to(dev)}}
        if packed_forms:
            samples["packed_" + kind] = {"v_packed": _packed_of(v, lens).to(dev), "v_len": lens.to(dev), "q_idxes": q.to(dev)}
        for name, sample in samples.items():
            tr = DataParallelTrainer(_model(cfg, dev), lr=2e-5, clip=0.25, graph=True)
            forms[name] = lambda tr=tr, sample=sample: tr.step(sample, a)
            for _ in range(DataParallelTrainer.EAGER_STEPS_BEFORE_CAPTURE + 2):
                forms[name]()
            captured[name] = tr._graph is not None
    rec = _alternate({k: (lambda fn=fn: _gpu_ms(fn, args.steps)) for k, fn in forms.items()}, args.blocks)
    rec["captured"] = captured
    return rec


def _unpack_vs_gather_us(B, N, n_img, args, dev):
    """vqa_gather_regions against vqa_unpack_regions, every sample N rows, the three dtype forms; the store holds n_img images"""
    from types import SimpleNamespace
    from vqa_playground_pytorch_amd import ops
    gen = torch.Generator().manual_seed(3)
    idx = torch.randint(n_img, (B,), generator=gen).to(torch.int32).to(dev)
    lens = torch.full((B,), N, dtype=torch.int32, device=dev)
    starts = (torch.arange(n_img, dtype=torch.int64) * N).to(dev)
    forms = {}
    for name, dt_in, dt_out in (("f32", torch.float32, torch.float32), ("bf16", torch.bfloat16, torch.bfloat16),
                                ("bf16_to_f32", torch.bfloat16, torch.float32)):
        rows = torch.randn(n_img * N, D, device=dev).to(dt_in)
        store = SimpleNamespace(rows=rows, starts=starts, counts=None, sample_shape=(N, D))
        counted = SimpleNamespace(rows=rows, starts=starts, counts=torch.full((n_img,), N, dtype=torch.int32, device=dev), sample_shape=(N, D))
        forms["gather_" + name] = lambda store=store, dt_out=dt_out: ops.gather_regions(store, idx, dt_out)
        forms["gather_counts_" + name] = lambda store=counted, dt_out=dt_out: ops.gather_regions(store, idx, dt_out)
        forms["unpack_" + name] = lambda x=rows[:B * N], dt_out=dt_out: ops.unpack_regions(x, lens, B, dt_out)
    for fn in forms.values():
        fn()
    torch.cuda.synchronize()
    return _alternate({k: (lambda fn=fn: 1e3 * _gpu_ms(fn, args.iters)) for k, fn in forms.items()}, args.blocks)


def resident_main(args):
    import numpy as np
    assert torch.cuda.is_available(), "feed_bench.py --resident measures on a GPU"
    dev = torch.device("cuda:0")
    n_img, B, N, depth = args.store or 4096, args.batch, 36, args.depth
    cfg = dict(n_img=n_img, N=N)
    path = "/tmp/feed_bench_store_%dx%d.npy" % (n_img, N)
    if not os.path.exists(path):
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(n_img, N, D))
        rs = np.random.RandomState(0)
        for lo in range(0, n_img, 128):
            mm[lo:lo + 128] = rs.standard_normal((min(128, n_img - lo), N, D)).astype(np.float32)
        mm.flush()
        del mm
    store = feed.FeatureStore(path, workers=args.workers).populate()
    rec = {"n_img": n_img, "B": B, "N": N, "steps": args.steps, "blocks": args.blocks, "upload": {}, "gather_us": {}}
    resident = {}
    for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        resident[name] = feed.DeviceFeatureStore(store, dev, dtype=dt)
        again = feed.DeviceFeatureStore(store, dev, dtype=dt)          # (the second upload: staging pages and file pages warm)
        rec["upload"][name] = {"nbytes": again.nbytes, "first_s": round(resident[name].upload_seconds, 3), "second_s": round(again.upload_seconds, 3),
                               "second_GBps": round(again.nbytes / again.upload_seconds / 1e9, 2)}
        del again
    rec["gather_us"]["B512xN36"] = _unpack_vs_gather_us(512, 36, 1024, args, dev)
    rec["gather_us"]["B128xN100"] = _unpack_vs_gather_us(128, 100, 512, args, dev)
    torch.cuda.empty_cache()
    rs = np.random.RandomState(1)
    qa = feed.qa_table(store, [{"v_idx": int(rs.randint(n_img)), "q_idxes": rs.standard_normal(2400).astype(np.float32), "q_id": i,
                                "a_10_idx": [(int(c), 0.1) for c in rs.choice(NANS, 10, replace=False)]} for i in range(B * 8)],
                         NANS, q_dtype=torch.float32)
    forms, loaders = {}, []
    ring = depth + 2 * args.producers + 2
    feeds = [("resident_f32", dict(resident=resident["f32"]), "v_idx"), ("resident_bf16", dict(resident=resident["bf16"]), "v_idx"),
             ("host_f32", dict(region_dtype=torch.float32), "v"), ("host_bf16", dict(region_dtype=torch.bfloat16), "v")]
    for name, kw, key in feeds:
        model = CoR2Model(["PAD"], NANS).to(dev).train().use_region_store(kw.get("resident"))
        tr = DataParallelTrainer(model, graph=True, adopt_inputs=True, input_slots=depth)
        loader = feed.store_batches(store, qa, B, NANS, shuffle=True, seed=0, pin=True, ring=ring, q_dtype=torch.float32,
                                    prefetch=2 * args.producers, epochs=None, producers=args.producers, **kw)
        loaders.append(loader)
        for _ in range(ring):                               # every ring slot page-locked before anything is captured
            next(loader)
        pre = feed.DevicePrefetcher(iter(()), dev, depth=depth)

        def run(n, tr=tr, pre=pre, loader=loader, key=key):
            pre.it = (next(loader) for _ in range(n))
            t0 = time.perf_counter()
            for b in pre:
                tr.step({key: b[key], "q_idxes": b["q_idxes"]}, b["a"])
            torch.cuda.synchronize()
            return B * n / (time.perf_counter() - t0)
        run(4 + 2 * depth)                                  # warm-up + one graph per device slot
        assert tr._graph is not None and len(tr._slots) == depth, "the fed step (%s) was not captured on every slot" % name
        forms[name] = lambda run=run: run(args.steps)
    # no feed at all: `depth` batches that are already on the device, in turn (what bench.py's step time stands for)
    gen = torch.Generator().manual_seed(9)
    rotating = [({"v": torch.randn(B, N, D, generator=gen).to(dev), "q_idxes": torch.randn(B, 2400, generator=gen).to(dev)},
                 torch.softmax(torch.randn(B, NANS, generator=gen), 1).to(dev)) for _ in range(depth)]
    tr = DataParallelTrainer(CoR2Model(["PAD"], NANS).to(dev).train(), graph=True, adopt_inputs=True, input_slots=depth)

    def rotate(n, tr=tr):
        t0 = time.perf_counter()
        for i in range(n):
            tr.step(*rotating[i % depth])
        torch.cuda.synchronize()
        return B * n / (time.perf_counter() - t0)
    rotate(4 + 2 * depth)
    assert tr._graph is not None and len(tr._slots) == depth, "the rotating step was not captured on every slot"
    forms["rotating_on_device"] = lambda: rotate(args.steps)
    rec["fed"] = _alternate({k: fn for k, fn in forms.items()}, args.blocks)
    for name in rec["fed"]:
        rec["fed"][name] = {k: (round(v) if not isinstance(v, list) else [round(x) for x in v]) for k, v in rec["fed"][name].items()}
    for loader in loaders:
        loader.close()
    print(json.dumps(rec))


def packed_child(args):
    assert torch.cuda.is_available(), "feed_bench.py --packed measures on a GPU"
    dev = torch.device("cuda:0")
    kinds = ["full", "uniform"] if args.counts == "both" else [args.counts]
    has_packed = hasattr(feed.FeatureStore, "gather_packed")
    rec = {"tree": ROOT, "packed_forms": has_packed, "counts": kinds}
    for name, cfg in PACKED_CONFIGS.items():
        rec[name] = {"step_ms": _step_ms(cfg, kinds, args, dev, has_packed)}
        if has_packed and not args.step_only:
            rec[name].update(unpack_us=_unpack_us(cfg, kinds, args, dev), gather_ms=_gather_ms(cfg, kinds, args), fed=_fed(cfg, kinds, args, dev))
    print(json.dumps(rec))


def packed_main(args):
    if args.child:
        return packed_child(args)
    me = os.path.abspath(__file__)
    common = ["--packed", "--child", "--counts", args.counts, "--blocks", str(args.blocks), "--steps", str(args.steps), "--iters", str(args.iters),
              "--workers", str(args.workers), "--producers", str(args.producers)]
    runs = [("this", me, ROOT, [])]
    if args.parent_tree:      # the parent has no --packed: this file runs there on the parent's package, the step alone
        parent = os.path.abspath(args.parent_tree)
        runs += [("parent", me, parent, ["--step-only", "--tree", parent]), ("this_step", me, ROOT, ["--step-only"]),
                 ("parent", me, parent, ["--step-only", "--tree", parent])]
    out = {}
    for name, script, cwd, extra in runs:
        done = subprocess.run([sys.executable, script] + common + extra, check=True, stdout=subprocess.PIPE, text=True, cwd=cwd)
        out.setdefault(name, []).append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--packed", action="store_true", help="packed (ragged) region batches against padded ones: see the module docstring")
    ap.add_argument("--resident", action="store_true", help="the device-resident region store against the host feeds: see the module docstring")
    ap.add_argument("--counts", choices=["full", "uniform", "both"], default="both")
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--step-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--depth", type=int, default=3, help="device slots of the prefetcher = input slots of the trainer (a step graph per "
                    "slot reads it in place); 2: the host waits for step t before it may refill the slot step t + 2 reads")
    ap.add_argument("--copy", action="store_true", help="the trainer copies every batch into its own graph input buffers (round 5's form)")
    ap.add_argument("--store", type=int, default=0, metavar="N_IMG",
                    help="feed from a feed.FeatureStore of N_IMG synthetic images (a .npy under /tmp, memory-mapped) through "
                         "feed.store_batches: the per-sample row gather into pinned staging is part of what is timed")
    ap.add_argument("--workers", type=int, default=8, help="gather threads of the FeatureStore")
    ap.add_argument("--producers", type=int, default=2, help="threads that assemble whole batches ahead of the consumer")
    ap.add_argument("--switch-interval", type=float, default=0.0, help="sys.setswitchinterval (seconds; 0 = leave Python's 5 ms): how "
                    "long the trainer's thread may keep the GIL while the producer thread waits for it")
    ap.add_argument("--transport", choices=["f32", "bf16"], default="f32",
                    help="bf16: the regions cross PCIe as bf16 (half the bytes) and are widened on the device (ops.widen_bf16); the step is the fp32 one")
    ap.add_argument("--answers", choices=["dense", "sparse"], default="dense",
                    help="sparse: the answers cross as (id, probability) pairs (a_idx / a_val [B,K]) and the loss is computed from them; "
                         "no dense [B,2000] target is built, copied or read")
    args = ap.parse_args()
    if args.packed:
        return packed_main(args)
    if args.resident:
        return resident_main(args)
    if args.switch_interval > 0:
        sys.setswitchinterval(args.switch_interval)
    dev = torch.device("cuda:0")
    B = args.batch
    torch.manual_seed(0)
    vdt = torch.bfloat16 if args.transport == "bf16" else torch.float32
    host = [{"v": torch.randn(B, 36, 2048).to(vdt).pin_memory(), "q_idxes": torch.randn(B, 2400).pin_memory(),
             "a": torch.softmax(torch.randn(B, 2000), 1).pin_memory()} for _ in range(3)]
    akeys = ("a",)
    if args.answers == "sparse":
        akeys = ("a_idx", "a_val")
        for h in host:
            del h["a"]
            h["a_idx"] = torch.stack([torch.randperm(2000)[:10] for _ in range(B)]).to(torch.int32).pin_memory()
            h["a_val"] = torch.softmax(torch.randn(B, 10), 1).pin_memory()
    target = (lambda b: b["a"]) if args.answers == "dense" else (lambda b: {"a_idx": b["a_idx"], "a_val": b["a_val"]})
    store = qa = None
    if args.store:
        import numpy as np
        path = "/tmp/feed_bench_store_%d.npy" % args.store
        if not os.path.exists(path):
            mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.float32, shape=(args.store, 36, 2048))
            rs = np.random.RandomState(0)
            for lo in range(0, args.store, 256):
                mm[lo:lo + 256] = rs.standard_normal((min(256, args.store - lo), 36, 2048)).astype(np.float32)
            mm.flush()
            del mm
        store = feed.FeatureStore(path, workers=args.workers).populate()     # (steady state: no first-touch page faults in the timed region)
        rs = np.random.RandomState(1)
        qa = [{"v_idx": int(rs.randint(args.store)), "q_idxes": rs.standard_normal(2400).astype(np.float32), "q_id": i,
               "a_10_idx": [(int(c), 0.1) for c in rs.choice(2000, 10, replace=False)]} for i in range(B * 8)]
        qa = feed.qa_table(store, qa, 2000, q_dtype=torch.float32)          # the records as arrays, once
    model = CoR2Model(["PAD"], 2000).to(dev).train()
    tr = DataParallelTrainer(model, graph=True) if args.copy else \
        DataParallelTrainer(model, graph=True, adopt_inputs=True, input_slots=args.depth)

    stats = {}

    def stream(n):
        if store is not None:        # the reference loader's batches from the memory-mapped store (question vectors stand in for ids)
            loader = feed.store_batches(store, qa, B, 2000, shuffle=True, seed=0, pin=True, region_dtype=vdt, ring=args.depth + 2 * args.producers + 2,
                                        q_dtype=torch.float32, prefetch=2 * args.producers, epochs=None, producers=args.producers,
                                        answers=args.answers)
            waited = 0.0
            for _ in range(n):
                t_w = time.perf_counter()
                b = next(loader)
                waited += time.perf_counter() - t_w
                yield dict({"v": b["v"], "q_idxes": b["q_idxes"]}, **{k: b[k] for k in akeys})
            loader.close()
            stats["producer_wait_ms_per_batch"] = 1e3 * waited / max(n, 1)
            return
        for i in range(n):
            yield host[i % len(host)]

    pre = feed.DevicePrefetcher(stream(4 + 2 * args.depth), dev, depth=args.depth)
    slots = []
    for b in pre:                                         # warm-up + graph capture (one graph per device slot, each replayed once)
        tr.step({"v": b["v"], "q_idxes": b["q_idxes"]}, target(b))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    # (the timed stream goes through the SAME prefetcher object's device slots: a fresh one would allocate new slots, i.e. new graphs)
    pre.it = iter(stream(args.steps))
    for b in pre:
        tr.step({"v": b["v"], "q_idxes": b["q_idxes"]}, target(b))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if stats:
        print("  the consumer waited %.2f ms per batch for the producer thread" % stats["producer_wait_ms_per_batch"])
    # raw H2D rate of one batch for reference
    d = torch.empty_like(host[0]["v"], device=dev)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(10):
        d.copy_(host[0]["v"], non_blocking=True)
    torch.cuda.synchronize()
    h2d = 10 * host[0]["v"].numel() * host[0]["v"].element_size() / (time.perf_counter() - t1) / 1e9
    print("host-fed (%s transport, %s answers, %s%s): %.1f samples/s (%.3f ms/step, graph=%s); pinned H2D of v alone: %.1f GB/s"
          % (args.transport, args.answers, "copied into the graph's buffers" if args.copy else "%d slots read in place" % args.depth,
             ", FeatureStore of %d images, %d gather threads" % (args.store, args.workers) if args.store else "", B * args.steps / dt, 1e3 * dt / args.steps, tr._graph is not None, h2d))


if __name__ == "__main__":
    main()
