"""Forward-only throughput and the cost of top-k hits in the train step, as ONE JSON line on stdout.

    python tools/eval_bench.py [--batch 512] [--iters 50] [--step-blocks 6] [--step-block 20]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o step -- python tools/eval_bench.py --skip-eval

eval:  samples/s of Evaluator.step (eval-mode forward under no_grad + top-5 predictions + hits) for CoR2 (2000 answers) and
       ODA (3000 answers), fp32, one resident batch: kernel by kernel ("eager") and replayed as one hipGraph ("graph").
step:  CoR2 train step (graph-replayed, as bench.py runs it) with topk=None and topk=(1, 5), timed in alternating blocks on
       the same GPU, so drift of the clock hits both alike; ms per step of each (median of the blocks) and their difference.
bench.py is the headline measurement and is unchanged; this tool only covers what it does not: the evaluation path."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def build(cls, nans, dev):
    from oracle import seeded
    from vqa_playground_pytorch_amd import CoR2Model, ODAModel
    model = {"cor2": CoR2Model, "oda": ODAModel}[cls](["PAD", "UNK"], nans)
    return seeded.load_state(model, 0).to(dev)


def inputs(B, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, 36, 2048, generator=g).to(dev)
    q = torch.randn(B, 2400, generator=g).to(dev)
    a = torch.softmax(2.0 * torch.randn(B, C, generator=g), 1).to(dev)
    return {"v": v, "q_idxes": q}, a


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def eval_rates(args, dev):
    from vqa_playground_pytorch_amd.evaluate import Evaluator
    out = {}
    for cls, nans in (("cor2", 2000), ("oda", 3000)):
        model = build(cls, nans, dev).eval()
        sample, a = inputs(args.batch, nans, dev, 1)
        batch = dict(sample, a=a)
        rec = {}
        for form, graph in (("eager", False), ("graph", True)):
            ev = Evaluator(model, graph=graph, k=5)
            for _ in range(args.warmup):
                ev.step(batch)
            if graph and ev._graph is None:
                raise RuntimeError("%s: the evaluation was not captured" % cls)
            ms = timed(lambda: ev.step(batch), args.iters)
            rec[form] = {"ms": round(ms, 4), "samples_per_s": round(args.batch / ms * 1e3, 1)}
        if cls == "cor2":
            rec["graph_nodes"] = ev.graph_nodes
        out[cls] = rec
        del model, ev
        torch.cuda.empty_cache()
    return out


def step_cost(args, dev):
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    sample, a = inputs(args.batch, 2000, dev, 2)
    trainers = {}
    for name, topk in (("none", None), ("top5", (1, 5))):
        torch.manual_seed(0)
        tr = DataParallelTrainer(build("cor2", 2000, dev).train(), lr=2e-5, clip=0.25, graph=True, adopt_inputs=True, topk=topk)
        for _ in range(args.warmup):
            tr.step(sample, a)
        if tr._graph is None:
            raise RuntimeError("%s: the step was not captured" % name)
        trainers[name] = tr
    blocks = {name: [] for name in trainers}
    for i in range(args.step_blocks):
        order = list(trainers) if i % 2 == 0 else list(reversed(list(trainers)))
        for name in order:
            tr = trainers[name]
            blocks[name].append(timed(lambda: tr.step(sample, a), args.step_block))
    med = {name: statistics.median(v) for name, v in blocks.items()}
    acc = trainers["top5"].accuracy()
    return {"ms_per_step": {k: round(v, 5) for k, v in med.items()},
            "blocks_ms": {k: [round(x, 5) for x in v] for k, v in blocks.items()},
            "added_us": round((med["top5"] - med["none"]) * 1e3, 2),
            "added_pct": round(100.0 * (med["top5"] - med["none"]) / med["none"], 3),
            "last_acc": [round(x, 3) for x in acc]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--step-blocks", type=int, default=6)
    ap.add_argument("--step-block", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="eval throughput only")
    ap.add_argument("--skip-eval", action="store_true", help="the two step forms only (e.g. under rocprofv3 --kernel-trace --stats, "
                    "which then lists kld_rows_kernel<false> and kld_rows_kernel<true> side by side)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "eval_bench needs a GPU"
    dev = torch.device("cuda:0")
    rec = {"tool": "eval_bench", "batch": args.batch, "dtype": "f32"}
    if not args.skip_eval:
        rec["eval"] = eval_rates(args, dev)
    if not args.skip_step:
        rec["step"] = step_cost(args, dev)
    print(json.dumps(rec, separators=(",", ":")))


if __name__ == "__main__":
    main()
