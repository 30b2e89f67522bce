"""The question encoder's mixed-precision modes next to the fp32 one, as ONE JSON line on stdout.

    python tools/encoder_bf16_bench.py [--batch 512] [--blocks 6] [--skip-step]

Everything is timed on one GPU in one call, in alternating blocks (fp32, bf16, bf16+in, bf16+in, bf16, fp32, ...), so drift of the
clock hits all sides alike; every figure is the median of its blocks, the blocks themselves are in the record.  The encoder and the
step are timed in three modes: f32, bf16 (compute_dtype=bf16: the recurrent products) and bf16_in (compute_dtype=bf16 plus
input_dtype=bf16: the input side too, csrc/encoder_input_bf16.hip).

product   the per-step recurrent product 3 x [B,2400] x [2400,2400]^T: vqa_gemm_nt_split_batched (fp32 operands, six bf16
          partial products) and vqa_gru_gemm_bf16 (one bf16 product), us per launch and TFLOP/s of the 2 G M N K operations
dw        the recurrent weight gradient over all T*B rows: three vqa_gemm_tn_split against three vqa_gemm_bf16_tn
encoder   SkipThoughts forward + backward alone (B x 26 tokens, lengths 5..26, training mode), ms
step      the graph-replayed CoR2 train step with the encoder in it (bench.py --encoder's workload), ms per step
input     per-launch times (KernelTimer: an event pair around each launch) of what the encoder's input side launches over its
          B*T rows in the bf16 and bf16_in modes: the split engine's products, or the three new kernels and the bf16 products
history   bytes of one [3,T,B,.] GEMM-operand history before and after
bench.py --encoder is the headline measurement and is unchanged (VQA_ENCODER_DTYPE=bf16 selects the mode there; its line does
not say which encoder ran)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

H, T = 2400, 26


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def alternate(forms, blocks, iters, warmup=3):
    """forms: {name: callable} -> {name: [ms per call of each block]}, the order reversed every other block"""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in forms}
    for i in range(blocks):
        for name in (list(forms) if i % 2 == 0 else list(reversed(list(forms)))):
            out[name].append(timed(forms[name], iters))
    return out


def summary(blocks, flops=None):
    rec = {}
    for name, v in blocks.items():
        med = statistics.median(v)
        rec[name] = {"ms": round(med, 5), "blocks_ms": [round(x, 5) for x in v]}
        if flops:
            rec[name]["tflops"] = round(flops / med / 1e9, 1)
    names = list(blocks)
    for a, b in zip(names, names[1:]):
        rec["ratio_%s_over_%s" % (a, b)] = round(rec[a]["ms"] / rec[b]["ms"], 3)
        rec["ranges_overlap_%s_%s" % (a, b)] = bool(min(blocks[a]) <= max(blocks[b]) and min(blocks[b]) <= max(blocks[a]))
    return rec


def product(args, dev):
    from vqa_playground_pytorch_amd import _lib, ops
    B, Hp = args.batch, ops.pad_to(H)
    gen = torch.Generator().manual_seed(1)
    a = torch.randn(3, B, H, generator=gen).to(dev)
    w = (torch.randn(3, H, H, generator=gen) / H ** 0.5).to(dev)
    c32, c16 = torch.empty(3, B, H, device=dev), torch.empty(3, B, H, device=dev)
    img = ops.split_weights(w)
    ab = torch.zeros(3, B, Hp, device=dev, dtype=torch.bfloat16)
    ab[:, :, :H] = a
    wb = ops.pack_bf16(w, torch.zeros(3, H, Hp, device=dev, dtype=torch.bfloat16), H * Hp, Hp, 1, zero_fill=False)
    forms = {"f32_split": lambda: ops.gemm_nt_split_batched(a, 0, B * H, H, img, c32, None, w, False, 3, B, H, H),
             "bf16": lambda: ops.gru_gemm_bf16(ab, 0, B * Hp, Hp, wb, H * Hp, Hp, c16, 3, B, H, H)}
    rec = summary(alternate(forms, args.blocks, args.iters), 2.0 * 3 * B * H * H)
    ref = torch.bmm(a.double(), w.double().transpose(1, 2))
    rec["max_err_over_scale"] = {"f32_split": float((c32.double() - ref).abs().max() / ref.abs().max()),
                                 "bf16": float((c16.double() - ref).abs().max() / ref.abs().max())}
    # the weight gradient over all T*B rows, three gates
    M = T * B
    torch.manual_seed(7)
    g32, x32 = torch.randn(3, M, H, device=dev), torch.randn(3, M, H, device=dev)
    g16, x16 = (torch.zeros(3, M, Hp, device=dev, dtype=torch.bfloat16) for _ in range(2))
    g16[:, :, :H], x16[:, :, :H] = g32, x32
    d32, d16 = torch.empty(3, H, H, device=dev), torch.empty(3, H, H, device=dev)
    L = _lib.lib()
    ws_bytes = L.vqa_gemm_bf16_tn_workspace_bytes(M, H, H)
    ws = torch.empty((ws_bytes + 3) // 4, device=dev)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)      # noqa: E731

    def dw32():
        for g in range(3):
            if not ops.gemm_tn_split(g32, g * M * H, H, x32, g * M * H, H, d32[g], M, H, H):
                raise RuntimeError("vqa_gemm_tn_split refused the encoder's shape")

    def dw16():
        for g in range(3):
            ops._launch("gemm_bf16_tn", (M, H, H), L.vqa_gemm_bf16_tn, p(g16, 2 * g * M * Hp), Hp, p(x16, 2 * g * M * Hp), Hp, p(d16[g]),
                        p(ws), ws_bytes, M, H, H)

    return rec, summary(alternate({"f32_split": dw32, "bf16": dw16}, args.blocks, max(args.iters // 4, 3)), 2.0 * 3 * M * H * H)


def tokens(B, vocab, dev, seed):
    gen = torch.Generator().manual_seed(seed)
    lengths = torch.randint(5, T + 1, (B,), generator=gen)
    q = torch.randint(1, vocab, (B, T), generator=gen) * (torch.arange(T)[None, :] < lengths[:, None])
    return q.to(dev)


MODES = (("f32", None, None), ("bf16", torch.bfloat16, None), ("bf16_in", torch.bfloat16, torch.bfloat16))
INPUT_KERNELS = ("embed_pack_bf16", "gemm_bf16_nt_f32_bias", "embed_grad", "gemm_bf16_tn", "gru_gemm_bf16", "pack_bf16", "column_sum",
                 "gemm_nt_split_batched", "gemm_tn_split", "bias_act", "act_bwd_colsum")


def encoder(args, dev):
    from vqa_playground_pytorch_amd import ops
    from vqa_playground_pytorch_amd.encoder import SkipThoughts
    vocab = ["PAD", "UNK"] + ["w%d" % i for i in range(14998)]
    q = tokens(args.batch, len(vocab), dev, 2)
    gy = torch.randn(args.batch, H, generator=torch.Generator().manual_seed(3)).to(dev)
    forms = {}
    for name, dtype, in_dtype in MODES:
        torch.manual_seed(4)
        m = SkipThoughts(vocab, af="relu", compute_dtype=dtype, input_dtype=in_dtype).to(dev).train()

        def run(m=m):
            for prm in m.parameters():
                prm.grad = None
            m(q).backward(gy)
        forms[name] = run
    rec = summary(alternate(forms, args.blocks, max(args.iters // 10, 2), warmup=2))
    # per-launch times of the input side's launches (those over all B*T rows), three passes each
    M, launches = args.batch * T, {}
    for name in ("bf16", "bf16_in"):
        timer = ops.KernelTimer(INPUT_KERNELS)
        ops.set_kernel_timer(timer)
        for _ in range(3):
            forms[name]()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        launches[name] = {"%s %s" % (k, list(shape)): {"launches_per_pass": n // 3, "us": round(ms * 1e3, 1)}
                          for (k, shape), (n, ms) in sorted(timer.summary().items()) if M in shape or (args.batch in shape and T in shape)}
    return rec, launches


def step(args, dev):
    from vqa_playground_pytorch_amd import CoR2Model
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer
    vocab = ["PAD", "UNK"] + ["w%d" % i for i in range(14998)]
    B, C = args.batch, 2000
    gen = torch.Generator().manual_seed(5)
    sample = {"v": torch.randn(B, 36, 2048, generator=gen).to(dev), "q_idxes": tokens(B, len(vocab), dev, 6)}
    a = torch.softmax(2.0 * torch.randn(B, C, generator=gen), 1).to(dev)
    forms, nodes = {}, {}
    for name, dtype, in_dtype in MODES:
        torch.manual_seed(1234)
        model = CoR2Model(vocab, C, seq2vec="skipthoughts", encoder_dtype=dtype or torch.float32,
                          encoder_input_dtype=in_dtype or torch.float32).to(dev).train()
        tr = DataParallelTrainer(model, lr=1e-4, clip=0.25, graph=True, adopt_inputs=True)
        for _ in range(6):
            tr.step(sample, a)
        torch.cuda.synchronize()
        if tr._graph is None:
            raise RuntimeError("%s: the step was not captured" % name)
        nodes[name] = tr.graph_nodes
        forms[name] = lambda tr=tr: tr.step(sample, a)
    rec = summary(alternate(forms, args.blocks, max(args.iters // 5, 3), warmup=2))
    for name, _, _ in MODES:
        rec[name]["samples_per_s"] = round(B / rec[name]["ms"] * 1e3, 1)
    rec["graph_nodes"] = nodes
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--iters", type=int, default=50, help="launches per block of the per-step product (the longer forms run fewer)")
    ap.add_argument("--skip-step", action="store_true", help="leave the replayed CoR2 step out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "encoder_bf16_bench needs a GPU"
    dev = torch.device("cuda:0")
    from vqa_playground_pytorch_amd import ops
    B, Hp = args.batch, ops.pad_to(H)
    rec = {"tool": "encoder_bf16_bench", "batch": B, "T": T, "H": H}
    rec["product"], rec["dw"] = product(args, dev)
    rec["encoder_fwd_bwd"], rec["input"] = encoder(args, dev)
    if not args.skip_step:
        rec["step"] = step(args, dev)
    rec["history_bytes"] = {"f32": 3 * T * B * H * 4, "bf16": 3 * T * B * Hp * 2}
    print(json.dumps(rec, separators=(",", ":")))


if __name__ == "__main__":
    main()
