"""The length-aware question encoder (SkipThoughts(length_aware=True)) next to the default one inside the replayed CoR2 train step,
as ONE JSON line on stdout.

    python tools/encoder_len_bench.py [--batch 512] [--rounds 4] [--iters 20]

The workload is bench.py --encoder's: the graph-replayed CoR2 + SkipThoughts step at T = 26.  The switch goes off / on in
alternating blocks inside one process and one call (the order reversed every other round), because two boxes, or two calls on one
box, differ by several per cent: a pair from two calls is not evidence.  Three length profiles per compute dtype (fp32 and
compute_dtype=bf16 of the encoder):

  all_26     every question has all 26 tokens: nothing can be skipped, "on" pays only its votes and predicates
  uniform    lengths uniform in 5..26, unsorted (bench.py's own draw): a row tile is skipped once ALL its rows are done
  sorted     the same draw sorted descending (what feed.store_batches(sort_questions=True) hands over)

Per profile: every block's ms per step, the medians, `off_spread_ms` (max - min of the repeated off-blocks: what the box does to
the same work) and `gain_ms` = median off - median on; `on_within_off_spread` / `on_faster_than_spread` say how the gain compares
to that spread.  No threshold is applied: the record is the result."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T = 26


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def profiles(B, vocab, seed):
    """{name: q_idxes int64 [B,T]}: left-aligned token ids, 0 = PAD"""
    gen = torch.Generator().manual_seed(seed)
    lengths = torch.randint(5, T + 1, (B,), generator=gen)
    words = torch.randint(1, vocab, (B, T), generator=gen)
    cut = lambda n: words * (torch.arange(T)[None, :] < n[:, None])      # noqa: E731
    return {"all_26": cut(torch.full((B,), T)), "uniform": cut(lengths), "sorted": cut(lengths.sort(descending=True).values)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=4, help="off/on pairs of blocks per profile")
    ap.add_argument("--iters", type=int, default=20, help="replayed steps per block")
    ap.add_argument("--answers", type=int, default=2000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_len_bench needs a GPU"
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    dev = torch.device("cuda:0")
    B, C = args.batch, args.answers
    vocab = ["PAD", "UNK"] + ["w%d" % i for i in range(14998)]
    qs = profiles(B, len(vocab), 6)
    gen = torch.Generator().manual_seed(5)
    v = torch.randn(B, 36, 2048, generator=gen).to(dev)
    a = torch.softmax(2.0 * torch.randn(B, C, generator=gen), 1).to(dev)
    rec = {"tool": "encoder_len_bench", "batch": B, "T": T, "rounds": args.rounds, "iters": args.iters, "dtypes": {}}
    for dtype in ("f32", "bf16"):
        steps = {}
        for name, on in (("off", False), ("on", True)):
            torch.manual_seed(1234)
            model = CoR2Model(vocab, C, seq2vec="skipthoughts", encoder_dtype=None if dtype == "f32" else dtype,
                              encoder_length_aware=on).to(dev).train()
            # resident inputs (adopt_inputs): each trainer owns its q_idxes tensor, overwritten in place per profile -- the replayed
            # graph reads the tokens, and with them the lengths, from it
            sample = {"v": v, "q_idxes": qs["uniform"].to(dev).clone()}
            tr = DataParallelTrainer(model, lr=1e-4, clip=0.25, graph=True, adopt_inputs=True)
            for _ in range(6):
                tr.step(sample, a)
            torch.cuda.synchronize()
            if tr._graph is None:
                raise RuntimeError("%s %s: the step was not captured" % (dtype, name))
            steps[name] = (sample, lambda tr=tr, sample=sample: tr.step(sample, a))
        out = {}
        for prof, q in qs.items():
            for sample, fn in steps.values():
                sample["q_idxes"].copy_(q)
                for _ in range(2):
                    fn()
            torch.cuda.synchronize()
            blocks = {"off": [], "on": []}
            for r in range(args.rounds):
                for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
                    blocks[name].append(timed(steps[name][1], args.iters))
            off, on = statistics.median(blocks["off"]), statistics.median(blocks["on"])
            spread = max(blocks["off"]) - min(blocks["off"])
            out[prof] = {"off_blocks_ms": [round(x, 4) for x in blocks["off"]], "on_blocks_ms": [round(x, 4) for x in blocks["on"]],
                         "off_ms": round(off, 4), "on_ms": round(on, 4), "off_spread_ms": round(spread, 4), "gain_ms": round(off - on, 4),
                         "on_within_off_spread": bool(abs(off - on) <= spread), "on_faster_than_spread": bool(off - on > spread),
                         "samples_per_s": {"off": round(B / off * 1e3, 1), "on": round(B / on * 1e3, 1)}}
        rec["dtypes"][dtype] = out
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(rec, separators=(",", ":")))


if __name__ == "__main__":
    main()
