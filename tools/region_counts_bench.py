"""Per-sample region counts ('v_len'): what the masked K3 kernels and a masked train step cost, as ONE JSON line on stdout.

    python tools/region_counts_bench.py [--parent-tree DIR] [--rounds 2] [--blocks 6]

Two configurations: f32 (B = 512, N = 36, fp32: the headline shape) and bf16 (B = 128, N = 100, compute_dtype = bfloat16: BASELINE
configs[4], the shape adaptive features are padded to).  For each:

k3     vqa_softmax_attention_pool_drop_{fwd,bwd} (unmasked) next to vqa_softmax_attention_pool_len_{fwd,bwd} with every count N
       (`full`) and with counts drawn uniformly from 10..N (`uniform`: mean about N / 2) -- D = 2048, G = 4, p = 0.5, `first`, d_v
       and d_alpha_ext asked for, as CoR2's first attention calls them; us per launch, device events around `iters` launches
step   the graph-replayed CoR2 train step (DataParallelTrainer(graph=True), train mode) without 'v_len', with every count N and
       with the uniform counts; ms per step

Everything is timed in alternating blocks inside one process (the order reversed every other block); a figure is the median of its
blocks and the blocks are in the record.  --parent-tree DIR: a checkout of the parent commit with its library built.  The same
measurement (the forms that tree has: unmasked K3, the step without 'v_len') then runs on that tree too, in child processes that
alternate with this tree's, `rounds` times each, in the same call on the same GPU -- the record holds both sides."""
import argparse
import ctypes
import inspect
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"f32": dict(B=512, N=36, dtype="float32"), "bf16": dict(B=128, N=100, dtype="bfloat16")}
D, G, P_DROP, NANS = 2048, 4, 0.5, 2000


def timed(fn, iters):
    import torch
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(forms, blocks, iters, warmup):
    """forms: {name: callable} -> {name: {"ms": median, "blocks_ms": [...]}}, the order reversed every other block"""
    import torch
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in forms}
    for i in range(blocks):
        for name in (list(forms) if i % 2 == 0 else list(reversed(list(forms)))):
            out[name].append(timed(forms[name], iters))
    return {name: {"ms": round(statistics.median(v), 5), "blocks_ms": [round(x, 5) for x in v]} for name, v in out.items()}


def counts(B, N, kind, dev):
    import torch
    if kind == "full":
        return torch.full((B,), N, dtype=torch.int32, device=dev)
    gen = torch.Generator().manual_seed(17)
    return torch.randint(min(10, N), N + 1, (B,), generator=gen).to(torch.int32).to(dev)


def k3(cfg, masked, args, dev):
    import torch
    from vqa_playground_pytorch_amd import _lib, ops
    L = _lib.lib()
    B, N = cfg["B"], cfg["N"]
    dt = getattr(torch, cfg["dtype"])
    sfx = "_bf16" if dt == torch.bfloat16 else ""
    gen = torch.Generator().manual_seed(3)
    logits = (3.0 * torch.randn(B, N, G, generator=gen)).to(dev)
    v = torch.randn(B, N, D, generator=gen).to(dt).to(dev)
    d_pooled, d_first, d_ext = (torch.randn(*s, generator=gen).to(dev) for s in ((B, G, D), (B, D), (B, N, G)))
    alpha, pooled, first = torch.empty(B, N, G, device=dev), torch.empty(B, G, D, device=dev), torch.empty(B, D, device=dev)
    d_logits, d_v = torch.empty(B, N, G, device=dev), torch.empty_like(v)
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    tail = (P_DROP, 7, None, B, N, D, G)

    def call(fn, *a):
        _lib.check(fn(*a, *tail, ops._stream()), "k3")

    fwd, bwd = {}, {}
    f_u, b_u = getattr(L, "vqa_softmax_attention_pool_drop_fwd" + sfx), getattr(L, "vqa_softmax_attention_pool_drop_bwd" + sfx)
    fwd["unmasked"] = lambda: call(f_u, p(logits), p(v), p(alpha), p(pooled), p(first))
    bwd["unmasked"] = lambda: call(b_u, p(alpha), p(v), p(d_pooled), p(d_first), p(d_ext), p(d_logits), p(d_v))
    rec = {}
    if masked:
        f_m, b_m = getattr(L, "vqa_softmax_attention_pool_len_fwd" + sfx), getattr(L, "vqa_softmax_attention_pool_len_bwd" + sfx)
        for kind in ("full", "uniform"):
            lens = counts(B, N, kind, dev)
            rec["mean_count_" + kind] = float(lens.float().mean())
            fwd[kind] = lambda lens=lens: call(f_m, p(logits), p(v), p(lens), p(alpha), p(pooled), p(first))
            bwd[kind] = lambda lens=lens: call(b_m, p(alpha), p(v), p(lens), p(d_pooled), p(d_first), p(d_ext), p(d_logits), p(d_v))
    rec["fwd"] = alternate(fwd, args.blocks, args.iters, 5)
    fwd["unmasked"]()         # (alpha for every backward form: a masked backward never reads its rows beyond the count)
    rec["bwd"] = alternate(bwd, args.blocks, args.iters, 5)
    return rec


def step(cfg, masked, args, dev):
    import torch
    from oracle import seeded
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    B, N = cfg["B"], cfg["N"]
    v, q, a = (torch.from_numpy(x).to(dev) for x in seeded.seeded_inputs(B, regions=N, answers=NANS, seed=9))
    forms, rec = {}, {}
    for kind in (("none", "full", "uniform") if masked else ("none",)):
        model = seeded.load_state(CoR2Model(["PAD", "UNK"], NANS, compute_dtype=getattr(torch, cfg["dtype"])), 0).train().to(dev)
        tr = DataParallelTrainer(model, lr=2e-5, clip=0.25, graph=True)
        sample = {"v": v, "q_idxes": q}
        if kind != "none":
            sample["v_len"] = counts(B, N, kind, dev)
        forms[kind] = lambda tr=tr, sample=sample: tr.step(sample, a)
        for _ in range(DataParallelTrainer.EAGER_STEPS_BEFORE_CAPTURE + 2):
            forms[kind]()
        rec["captured_" + kind] = tr._graph is not None
    rec.update(alternate(forms, args.blocks, max(args.iters // 5, 5), 3))
    return rec


def child(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from vqa_playground_pytorch_amd import ops
    assert torch.cuda.is_available(), "region_counts_bench.py measures on a GPU"
    dev = torch.device("cuda:0")
    masked = "lens" in inspect.signature(ops.softmax_attention_pool_drop).parameters
    rec = {"tree": os.path.abspath(args.tree), "masked_forms": masked}
    for name, cfg in CONFIGS.items():
        rec[name] = {"k3_us": k3(cfg, masked, args, dev), "step_ms": step(cfg, masked, args, dev)}
        for side in ("fwd", "bwd"):          # (kernel figures in microseconds)
            for form in rec[name]["k3_us"][side].values():
                form["us"] = round(form.pop("ms") * 1e3, 2)
                form["blocks_us"] = [round(x * 1e3, 2) for x in form.pop("blocks_ms")]
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--tree", default=ROOT)
    args = ap.parse_args()
    if args.child:
        return child(args)
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(args.parent_tree))] if args.parent_tree else [])
    out = {name: [] for name, _ in trees}
    for r in range(args.rounds):
        for name, tree in (trees if r % 2 == 0 else trees[::-1]):
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--blocks", str(args.blocks),
                                   "--iters", str(args.iters)], check=True, stdout=subprocess.PIPE, text=True, cwd=tree)
            out[name].append(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
