"""Per-sample region counts for ODA: what the masked K2 kernels and a masked ODA train step cost, as ONE JSON line on stdout.

    python tools/oda_region_counts_bench.py [--parent-tree DIR] [--rounds 2] [--blocks 6]

The sibling of tools/region_counts_bench.py (CoR2 / K3), written the same way and sharing its helpers.  ODA shape: B = 512, N = 36,
L = 310, G = 4, p = 0.5.

k2     vqa_object_difference_attention_{fwd,bwd} (unmasked) next to vqa_object_difference_attention_len_{fwd,bwd} with every count
       N (`full`) and with counts drawn uniformly from 10..N (`uniform`); gate_dvl = 1 as the model calls it; us per launch, device
       events around `iters` launches
step   the graph-replayed ODA train step (DataParallelTrainer(graph=True), train mode) of oda.Model(region_counts=True) without
       'v_len', with every count N and with the uniform counts; ms per step.  On a tree without the option (the parent commit) the
       default model's step without the key.

Everything is timed in alternating blocks inside one process (the order reversed every other block); a figure is the median of its
blocks and the blocks are in the record.  --parent-tree DIR: a checkout of the parent commit with its library built; the forms that
tree has then run on it too, in child processes that alternate with this tree's, `rounds` times each, in the same call on the
same GPU -- the record holds both sides."""
import argparse
import ctypes
import inspect
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from region_counts_bench import NANS, alternate, counts  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N, L, G, P_DROP = 512, 36, 310, 4, 0.5


def k2(masked, args, dev):
    import torch
    from vqa_playground_pytorch_amd import _lib, ops
    Lb = _lib.lib()
    gen = torch.Generator().manual_seed(3)
    vl = torch.randn(B, N, L, generator=gen).clamp_min(0.0).to(dev)
    ql = torch.randn(B, L, generator=gen).abs().to(dev)
    w = (torch.randn(G, N * L, generator=gen) / (N * L) ** 0.5).to(dev)
    bias, dS = torch.randn(G, generator=gen).to(dev), torch.randn(B, N, G, generator=gen).to(dev)
    logits, d_vl, d_ql, d_w, d_bias = (torch.empty_like(t) for t in (dS, vl, ql, w, bias))
    p = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    tail = (P_DROP, 7, None, B, N, L, G)

    def ws_of(query):
        nbytes = query(B, N, L, G)
        return torch.empty(nbytes // 4, device=dev), nbytes

    def call(fn, *a):
        _lib.check(fn(*a, ops._stream()), "k2")

    ws_u, nb_u = ws_of(Lb.vqa_object_difference_attention_bwd_workspace_bytes)
    fwd = {"unmasked": lambda: call(Lb.vqa_object_difference_attention_fwd, p(vl), p(ql), p(w), p(bias), p(logits), *tail)}
    bwd = {"unmasked": lambda: call(Lb.vqa_object_difference_attention_bwd, p(vl), p(ql), p(w), p(dS), p(d_vl), p(d_ql), p(d_w),
                                    p(d_bias), p(ws_u), nb_u, *tail, 1)}
    rec = {}
    if masked:
        ws_m, nb_m = ws_of(Lb.vqa_object_difference_attention_len_bwd_workspace_bytes)
        for kind in ("full", "uniform"):
            lens = counts(B, N, kind, dev)
            rec["mean_count_" + kind] = float(lens.float().mean())
            rec["mean_pairs_" + kind] = float((lens.float() ** 2).mean()) / (N * N)
            fwd[kind] = lambda lens=lens: call(Lb.vqa_object_difference_attention_len_fwd, p(vl), p(ql), p(w), p(bias), p(lens),
                                               p(logits), *tail)
            bwd[kind] = lambda lens=lens: call(Lb.vqa_object_difference_attention_len_bwd, p(vl), p(ql), p(w), p(dS), p(lens),
                                               p(d_vl), p(d_ql), p(d_w), p(d_bias), p(ws_m), nb_m, *tail, 1)
    rec["fwd"] = alternate(fwd, args.blocks, args.iters, 5)
    rec["bwd"] = alternate(bwd, args.blocks, args.iters, 5)
    return rec


def step(masked, args, dev):
    import torch
    from oracle import seeded
    from vqa_playground_pytorch_amd import ODAModel
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    v, q, a = (torch.from_numpy(x).to(dev) for x in seeded.seeded_inputs(B, regions=N, answers=NANS, seed=9))
    forms, rec = {}, {}
    for kind in (("none", "full", "uniform") if masked else ("none",)):
        kw = dict(region_counts=True) if masked else {}
        model = seeded.load_state(ODAModel(["PAD", "UNK"], NANS, **kw), 0).train().to(dev)
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
    assert torch.cuda.is_available(), "oda_region_counts_bench.py measures on a GPU"
    dev = torch.device("cuda:0")
    masked = "lens" in inspect.signature(ops.object_difference_attention).parameters
    rec = {"tree": os.path.abspath(args.tree), "masked_forms": masked, "k2_us": k2(masked, args, dev), "step_ms": step(masked, args, dev)}
    for side in ("fwd", "bwd"):          # (kernel figures in microseconds)
        for form in rec["k2_us"][side].values():
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
