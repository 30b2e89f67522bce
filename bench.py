#!/usr/bin/env python3
"""Headline benchmark: VQA samples/sec of one CoR2 training step (forward + KLD-sum loss + backward +
flat-gradient sum-all-reduce + clip 0.25 + Adam), batch 512 per GPU, 36x2048 regions, 2400-d question,
fp32, dropout active -- BASELINE.json configs[1] (N=1) / configs[3] (N=8, global batch 4096).

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 --master-addr 127.0.0.1 \
        --master-port 29500 bench.py --gpus 8 --steps 20 --warmup 5

Rank 0 prints ONE compact JSON line (< 2000 bytes: `compact_line`) on stdout: the contract fields, the configuration
and, for N > 1, `distributed`.  A plain run does only what that line needs: set up, warm up, time the K steps, write
`--dump-outputs`, print.  `--full` adds everything measured in runs of its own, after the timed region: `roofline`,
`cpu_baseline`, `resident_inputs` and one small record per sub-benchmark on the line; `roofline_all` (EVERY timed op
of the step, C-ABI launches and library GEMMs, with its work model), the counters behind `mfma_busy_pct`,
`step_coverage` and the full sub-records in the full record.  The full record goes to `bench_detail.json` in the
working directory (`--detail-file`) and to stderr.  Inputs are synthetic and resident in HBM before the timed
region.  The `roofline` object is for the hand-written op with the largest share of the step (mean duration x
launches), timed live with HIP events on the launch stream.  `cpu_baseline` times the oracle's reference-faithful
torch-CPU port (oracle/reference_faithful.py) on a bounded sample on the host cores.  `--dump-outputs DIR` also writes
what the last timed step computed as DIR/<name>.npy (seeded inputs: two builds compare output for output).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from vqa_playground_pytorch_amd import _srchash  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
MFMA_F32_PEAK_TF = 157.3   # dense fp32 MFMA peak (v_mfma_f32_32x32x2_f32)
MFMA_BF16_PEAK_TF = 2500.0 # dense bf16 MFMA peak (v_mfma_f32_32x32x16_bf16), no sparsity
MFMA_SPLIT_PEAK_TF = MFMA_BF16_PEAK_TF / 6.0   # an fp32 product on the split engine = six bf16 partial products: 416.7 TFLOP/s of
                                               # fp32 GEMM FLOPs is what the bf16 pipe can deliver (csrc/gemm_f32_split.hpp)

BATCH, REGIONS, FEAT, QDIM, ANSWERS = 512, 36, 2048, 2400, 2000
ROTATE = 4                 # resident batches the timed steps visit in turn (4 x 151 MB > the 256 MB Infinity Cache)
LOW, HID, GLIMPSES, RANK = 310, 510, 4, 2


K4_FOLDED = os.environ.get("VQA_K4_FORM", "auto") != "engine"
EVIDENCE_TAG = "r06"      # profiles/<tag>_pmc_traffic[_<cfg>].json / <tag>_pmc_mfma[_<cfg>].json: rocprofv3 --pmc passes of this command


def work_of(name, shape):
    """(bound, algorithmic work per launch) of one timed op -- bytes for "hbm", FLOPs for "mfma" / "valu" -- from the
    shape its wrapper in ops.py reports (SURVEY.md 8d per-sample figures x the samples of the launch).
    None: no model (the op is still listed with its time)."""
    bf16 = name.endswith("_bf16")
    base = name[:-5] if bf16 else name
    fv, f = (2 if bf16 else 4), 4        # bytes per element of the region tensors / of everything else
    s = shape
    if base == "lowrank_bilinear_fusion_fwd":
        B, N, L, H, R = s[:5]
        return "mfma", B * (2 * R * N * L * H + 2 * R * N * H)
    if base == "lowrank_bilinear_fusion_bwd":
        B, N, L, H, R, dx = s[:6]
        return "mfma", B * (2 * R * N * L * H) * (2 if dx else 1)                    # dW1 (+ dx) contractions
    if base in ("linear_act_fwd", "linear_act_fwd_split"):
        M, K, N = s[:3]
        return "mfma", 2 * M * K * N                                                  # the fp32 GEMM's FLOPs on either engine
    if base in ("linear_act_dw_split", "relation_linear_dw_split"):
        M, K, N = s[:3]
        return "mfma", 2 * M * K * N
    if base == "relation_linear_fwd_split":                                           # K1 -> K5 in one kernel: the projection's FLOPs
        B, N, D, L = s[:4]                                                            # (the relation step's 2 N D per sample ride along)
        return "mfma", 2 * B * N * D * L
    if base == "linear_act_bwd":
        M, K, N, _drop, dx = s[:5]
        return "mfma", 2 * M * K * N * (2 if dx else 1)                              # dW (+ dx)
    if base in ("relation_projection_dgrad", "relation_projection_dgrad_split"):
        B, N, D, L = s[:4]
        return "mfma", 2 * B * N * D * L                                              # the data-gradient contraction
    if base == "gemm_nt_split_batched":                                               # the question encoder's per-step / input products
        G, M, N, K = s[:4]
        return "mfma", 2 * G * M * N * K
    if base == "gemm_tn_split":                                                        # ... and its weight gradients (one gate per call)
        M, N1, N2 = s[:3]
        return "mfma", 2 * M * N1 * N2
    if base in ("grouped_gemm", "grouped_gemm_split"):                                    # K6: every GEMM of a phase of the
        return "mfma", s[2]                                                               # [B,.] layers (head.py), FLOPs summed
    if base == "grouped_epilogue":
        return "hbm", s[2] * f                                                            # slabs read + outputs written
    if base == "library_gemm":
        M, N, K = s[:3]
        return "mfma", 2 * M * N * K
    if base in ("gemm_bf16_nt", "gemm_bf16_tn"):
        return "mfma", 2 * s[0] * s[1] * s[2]
    if base == "object_difference_attention_fwd":
        B, N, L, G = s[:4]
        return "valu", B * 2 * G * N * N * L                                         # 2 flop per (mask element, glimpse)
    if base == "object_difference_attention_bwd":
        B, N, L, G = s[:4]
        return "valu", B * 4 * G * N * N * L                                         # data pass + weight pass
    if base == "relation_apply_fwd":
        B, N, D = s[:3]
        return "hbm", B * (2 * N * D * fv + 2 * D * f)                               # v in, dropped v2 out
    if base == "relation_apply_bwd":
        B, N, D, _drop, dv = s[:5]
        return "hbm", B * ((2 + (1 if dv else 0)) * N * D * fv + 3 * D * f)          # v, g in; d_t, d_c2 (, d_v) out
    if base == "pairwise_relation_reduce_fwd":
        B, N, D = s[:3]
        return "hbm", B * (2 * N * D * fv + (2 * D + N) * f)                         # 606 352 B/sample at fp32
    if base == "pairwise_relation_reduce_bwd":
        B, N, D, dv, gb = s[:5]
        return "hbm", B * ((2 + (1 if dv else 0) + (1 if gb else 0)) * N * D * fv + (4 * D + 2 * N) * f)
    if base in ("softmax_attention_pool_fwd", "softmax_attention_pool_drop_fwd"):
        B, N, D, G = s[:4]
        return "hbm", B * (N * D * fv + (2 * N * G + G * D) * f)                     # 328 832 B/sample at fp32
    if base in ("softmax_attention_pool_bwd", "softmax_attention_pool_drop_bwd"):
        B, N, D, G, dv = s[:5]
        return "hbm", B * ((1 + (1 if dv else 0)) * N * D * fv + (G * D + 3 * N * G) * f)
    if base == "attention_logits_fwd":
        M, K, G = s[:3]
        return "hbm", M * (K * fv + G * f)
    if base == "attention_logits_bwd":
        M, K, G, _drop, dx = s[:5]
        return "hbm", M * ((1 + (1 if dx else 0)) * K * fv + G * f)
    if base == "kld_sum_loss":
        B, C, need = s[:3]
        return "hbm", B * C * f * (3 if need else 2)
    if base == "grad_norm_clip_coef":
        return "hbm", s[0] * f
    if base in ("adam_step", "adam_step_dyn"):
        return "hbm", s[0] * 7 * f                                                   # p, g, m, v in; p, m, v out
    if base == "column_sum":
        return "hbm", s[0] * s[1] * fv
    if base == "bias_act":
        G, B, A = s[:3]
        return "hbm", 2 * G * B * A * f
    if base == "act_bwd_colsum":
        G, B, A = s[:3]
        return "hbm", 3 * G * B * A * f
    if base == "rank_product_fwd":
        B, R, H = s[:3]
        return "hbm", (2 * R + 1) * B * H * f
    if base == "rank_product_bwd":
        B, R, H = s[:3]
        return "hbm", (4 * R + 1) * B * H * f
    return None


# HBM-side traffic per launch from the PMC passes of this same command (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE in
# separate runs, kernel by kernel, KiB units; profiles/<tag>_pmc_traffic.json, built by tools/pmc_table.py).  FETCH_SIZE
# under-reports 16-byte-per-lane streaming reads by exactly 2x on gfx950 (MI355X_MICROARCH.md, HBM section); the multiplier
# is stated per kernel.  Counters cannot be collected inside the driver's own run of this file (no profiler is attached
# there): the table is the committed evidence of the same command, and `traffic_source` says so in the output line.
PMC_KERNELS = {  # C-ABI entry -> kernel-name prefixes of its dominant device kernel (the first one found at the launch's grid)
    "lowrank_bilinear_fusion_fwd": ["vqa::bilinear_fold_rt_kernel<true", "vqa::bilinear_fold_kernel<true"],
    "linear_act_fwd": ["vqa::rt::gemm_nt_kernel<9, 5, 1, 2, 2"],
    "linear_act_bwd": ["vqa::rt::gemm_tn_kernel<5, 2"],
    "linear_act_fwd_split": ["vqa::sp::gemm_nt_kernel<9, 5, 1, 2, 2"],
    "linear_act_dw_split": ["vqa::sp::gemm_tn_shared_kernel<5", "vqa::sp::gemm_tn_kernel<5, 2"],
    "relation_projection_dgrad_split": ["vqa::relation_dgrad_split_kernel"],
    "relation_linear_fwd_split": ["vqa::sp::gemm_nt_kernel<9, 5, 1, 2, 2"],
    "relation_linear_dw_split": ["vqa::sp::gemm_tn_shared_kernel<5"],
    "gemm_nt_split_batched": ["vqa::gemm_nt_batched_kernel"], "gemm_tn_split": ["vqa::sp::gemm_tn_shared_kernel<5"],
    "lowrank_bilinear_fusion_bwd": ["vqa::bilinear_dw_rt_kernel"],
    "relation_projection_dgrad": ["vqa::relation_dgrad_kernel"],
    "attention_logits_fwd": ["vqa::attention_logits_fwd_kernel"],
    "attention_logits_bwd": ["vqa::attention_logits_bwd_kernel"],
    "relation_apply_fwd": ["vqa::relation_apply_fwd_kernel"],
    "relation_apply_bwd": ["vqa::relation_apply_bwd_kernel"],
    "pairwise_relation_reduce_fwd": ["vqa::pairwise_fwd"],
    "pairwise_relation_reduce_bwd": ["vqa::pairwise_bwd_stream_kernel"],
    "softmax_attention_pool_fwd": ["vqa::attention_pool_fwd_kernel"],
    "softmax_attention_pool_bwd": ["vqa::attention_pool_bwd_fused_kernel", "vqa::attention_pool_bwd_stream_kernel"],
    "softmax_attention_pool_drop_fwd": ["vqa::attention_pool_fwd_kernel"],
    "softmax_attention_pool_drop_bwd": ["vqa::attention_pool_bwd_fused_kernel", "vqa::attention_pool_bwd_stream_kernel"],
    "grouped_gemm": ["vqa::grouped_gemm_kernel"],
    "grouped_gemm_split": ["vqa::grouped_gemm_split_kernel"],
    "grouped_epilogue": ["vqa::grouped_epilogue_kernel"],
    "object_difference_attention_fwd": ["vqa::oda_fwd"],
    "object_difference_attention_bwd": ["vqa::oda_bwd_data", "vqa::oda_bwd_weight"],
    "adam_step_dyn": ["vqa::adam_kernel"], "adam_step": ["vqa::adam_kernel"],
    "kld_sum_loss": ["vqa::kld_rows_kernel"],
    "gemm_bf16_nt": ["vqa::gemm_bf16_nt_kernel"], "gemm_bf16_tn": ["vqa::gemm_bf16_tn_kernel"],
    "lowrank_bilinear_fusion_fwd_bf16": ["vqa::bilinear_fold_bf16_kernel", "vqa::bilinear_fwd2_bf16_kernel"],
    "lowrank_bilinear_fusion_bwd_bf16": ["vqa::gemm_bf16_tn_kernel", "vqa::gemm_bf16_nt_kernel"],
}
STALE = "stale"            # a counter row whose kernel sources have changed since it was collected: reported, never printed as data
FETCH_MULT = 2.0           # FETCH_SIZE under-counts 16-byte-per-lane streaming reads by 2x on gfx950 (MI355X_MICROARCH.md)
_tables = {}


def evidence_cfg(B, regions, bf16, model="cor2"):
    """Which committed counter tables belong to a run: "" = the headline configuration (CoR2 and ODA heads at B = 512, N = 36,
    fp32, both engines: one table), "bf16_n100_b128" = one rank's share of configs[4], "oda_attention" = configs[2]'s op alone;
    None = no counters were collected at this shape."""
    if model == "oda-attention":
        return "oda_attention" if (B, regions) == (BATCH, REGIONS) else None
    if bf16:
        return "bf16_n100_b128" if (B, regions) == (128, 100) else None
    return "" if (B, regions) == (BATCH, REGIONS) else None


def _evidence(kind, cfg=""):
    key = (kind, cfg)
    if key not in _tables:
        path = os.path.join(ROOT, "profiles", "%s_pmc_%s%s.json" % (EVIDENCE_TAG, kind, "_" + cfg if cfg else ""))
        _tables[key] = json.load(open(path)) if os.path.exists(path) else {}
    return _tables[key]


def _norm_kernel(text):
    for junk in (" ", "(", ")", "vqa::", "rt::"):
        text = text.replace(junk, "")
    return text


def pmc_row(table, name, grids):
    """The counter-table row of the dominant device kernel behind one C-ABI launch: keys are "<kernel>|grid=<work-items>"
    (tools/pmc_table.py), and a row only counts when its grid is one the launch really used (`grids`: the library's launch
    log, ops.KernelTimer.grids: ((work-items, kernel expression at the launch site), ...)) -- the same kernel at another
    shape is another row; of several template instances at that grid the one the launch site names wins.  None when there
    is no such row."""
    if not table or name not in PMC_KERNELS or not grids:
        return None
    sizes = {g for g, _ in grids}
    texts = [_norm_kernel(t).rstrip(">") for _, t in grids if t]
    for prefix in PMC_KERNELS[name]:
        hits = []
        for key, row in table.items():
            kernel, _, grid = key.partition("|grid=")
            if kernel.startswith(prefix) and grid.isdigit() and int(grid) in sizes:
                hits.append((key, row))
        if hits:
            exact = [h for h in hits if any("<" in t and _norm_kernel(h[0].split("|")[0]).startswith(t) for t in texts)]
            key, row = (exact or hits)[0]
            # round 6: a row is evidence only for the code it was measured on -- its `source` stamp (the fingerprint of the
            # files that define the kernel, written by tools/pmc_table.py / pmc_mfma.py) must equal the tree's
            return dict(row, key=key, stale=_srchash.row_is_stale(key, row))
    return None


def trace_ms(grids, cfg=""):
    """The duration of an op in the committed rocprofv3 --kernel-trace of the REPLAYED step (profiles/<tag>_trace[_<cfg>].json,
    tools/by_grid.py): the medians of the device kernels its C-ABI call launched (library's launch log: identifier + grid),
    summed, in ms -- printed next to the event-timed `mean_ms` of the kernel-by-kernel pass, which brackets launch gaps too and
    reads ~10 % high.  None when a kernel has no row or a row's source stamp differs from the tree's."""
    key = ("trace", cfg)
    if key not in _tables:
        path = os.path.join(ROOT, "profiles", "%s_trace%s.json" % (EVIDENCE_TAG, "_" + cfg if cfg else ""))
        _tables[key] = json.load(open(path)) if os.path.exists(path) else {}
    table = _tables[key]
    if not table or not grids:
        return None
    total = 0.0
    for grid, text in grids:
        ident = _srchash.kernel_identifier(_norm_kernel(text or ""))
        rows = [(k, r) for k, r in table.items() if not k.startswith("__") and k.endswith("|grid=%d" % grid)
                and _srchash.kernel_identifier(k) == ident]
        want = _norm_kernel(text or "").rstrip(">")          # of several template instances at that grid: the one the launch site names
        exact = [(k, r) for k, r in rows if "<" in want and _norm_kernel(k.split("|")[0]).startswith(want)]
        rows = exact or rows
        if not rows or any(_srchash.row_is_stale(k, r) for k, r in rows):
            return None
        n = sum(r["launches"] for _, r in rows)
        total += sum(r["median_us"] * r["launches"] for _, r in rows) / max(n, 1)
    return round(total * 1e-3, 5)


def pmc_traffic(name, grids, cfg=""):
    """HBM bytes per launch (FETCH_SIZE x 2 + WRITE_SIZE, KiB counters) of the dominant kernel behind an op, or None."""
    row = pmc_row(_evidence("traffic", cfg), name, grids)
    if row is None:
        return None
    if row["stale"]:
        return STALE
    return int((row["FETCH_SIZE_KiB"] * FETCH_MULT + row["WRITE_SIZE_KiB"]) * 1024.0)


def pmc_mfma(name, grids, cfg=""):
    """Counter-backed matrix-pipe occupancy of the kernel behind an op: SQ_VALU_MFMA_BUSY_CYCLES / SQ_BUSY_CYCLES and the
    MFMA instruction count (profiles/<tag>_pmc_mfma[_<cfg>].json, tools/pmc_mfma.py), or None."""
    return pmc_row(_evidence("mfma", cfg), name, grids)


def roofline_entry(name, shape, launches, mean_ms, B, regions=REGIONS, bf16=False, grids=(), model_name="cor2"):
    model = work_of(name, shape)
    if model is not None and model[1] is None:
        model = None
    cfg = evidence_cfg(B, regions, bf16, model_name)
    entry = {"kernel": name, "shape": list(shape), "launches": launches, "mean_ms": round(mean_ms, 5)}
    if model is None:
        entry.update({"bound": None, "achieved": None, "peak": None, "unit": None, "frac": None, "traffic": None})
        return entry
    bound, work = model
    sec = max(mean_ms, 1e-9) * 1e-3
    if bound == "hbm":
        achieved, peak, unit = work / sec / 1e9, HBM_PEAK_GBS, "GB/s"
    elif name.endswith("_bf16") or name.startswith("gemm_bf16"):
        achieved, peak, unit = work / sec / 1e12, MFMA_BF16_PEAK_TF, "TFLOP/s"
    elif name.endswith("_split") or "_split_" in name:
        achieved, peak, unit = work / sec / 1e12, round(MFMA_SPLIT_PEAK_TF, 1), "TFLOP/s"
    else:  # "mfma" and "valu" share the fp32 peak on gfx950 (157.3 TFLOP/s for both pipes)
        achieved, peak, unit = work / sec / 1e12, MFMA_F32_PEAK_TF, "TFLOP/s"
    # (the ODA head at B = 512 runs K2 / K3 at the shapes of the attention-op benchmark: their rows live in that table)
    cfgs = [] if cfg is None else [cfg] + (["oda_attention"] if model_name == "oda" and cfg == "" else [])
    traffic = next((t for t in (pmc_traffic(name, grids, c) for c in cfgs) if t is not None), None)
    if traffic == STALE:
        traffic, entry["traffic_stale"] = None, True
    entry.update({"bound": bound, "achieved": round(achieved, 2), "peak": peak, "unit": unit,
                  "frac": round(achieved / peak, 4), "traffic": traffic})
    if name == "lowrank_bilinear_fusion_fwd" and K4_FOLDED and regions <= 112 and len(shape) >= 5 and shape[1] > 1:
        # `achieved` prices the kernel at SURVEY 8d's algorithmic FLOPs (R GEMMs per fusion).  The rank-folded kernel
        # executes 1/R of them on the matrix core, plus the padding of a sample to whole 16-region blocks and of L / H to
        # the 16-wide chunk / 64-wide tile: state what the MFMA pipe really ran as well.
        nb = {1: 1, 2: 2, 3: 3, 4: 5, 5: 5, 6: 7, 7: 7}[(regions + 15) // 16]
        executed = 2.0 * shape[0] * (nb * 16) * ((LOW + 1 + 15) // 16 * 16) * ((HID + 63) // 64 * 64)
        entry["form"] = "rank-folded (csrc/bilinear_folded.hip)"
        entry["mfma_flops_executed"] = int(executed)
        entry["mfma_executed_tflops"] = round(executed / sec / 1e12, 2)
    busy = next((t for t in (pmc_mfma(name, grids, c) for c in cfgs) if t is not None), None)
    if busy is not None and busy["stale"]:
        entry["traffic_stale"] = True
    elif busy is not None:
        if busy.get("mfma_busy_pct") is not None:
            entry["mfma_busy_pct"] = busy.get("mfma_busy_pct")
        if busy.get("valu_issue_pct_min") is not None:
            entry["valu_issue_pct_min"] = busy.get("valu_issue_pct_min")
        entry["mfma_counters"] = {k: busy[k] for k in busy if k.startswith("SQ_") or k in ("launches", "key")}
    if grids:
        entry["device_kernels"] = [[t, g] for g, t in grids]
        t_ms = next((t for t in (trace_ms(grids, c) for c in cfgs) if t is not None), None)
        if t_ms is not None:
            entry["trace_ms"] = t_ms
    return entry


def step_table(timer, steps_timed, B, regions, bf16, model_name="cor2"):
    """Every timed op of the per-kernel pass as a roofline entry, sorted by its share of the step."""
    entries = [roofline_entry(name, shape, n, ms, B, regions, bf16, timer.grids.get((name, shape), ()), model_name)
               for (name, shape), (n, ms) in timer.summary().items()]
    for e in entries:
        e["ms_per_step"] = round(e["mean_ms"] * e["launches"] / max(steps_timed, 1), 5)
    entries.sort(key=lambda e: -e["ms_per_step"])
    return entries


def roofline_record(timer, args, B, bf16, graphed, ms_step):
    """--full, a training step: `roofline`, `traffic_source`, `step_coverage` and `roofline_all` from the per-kernel pass."""
    steps_timed = min(args.steps, 10) if (graphed or not args.no_graph) else args.steps
    entries = step_table(timer, steps_timed, B, args.regions, bf16, args.model)
    # `roofline` = the hand-written OP that takes the largest share of the step -- its launches summed over every shape
    # it runs at (linear_act_fwd runs once with and once without the in-register dropout mask: two entries of
    # roofline_all, one op) -- not a favourite; library GEMMs (hipBLASLt through torch) are listed in roofline_all with
    # their time and rate as well
    ours = [e for e in entries if e["bound"] is not None and e["kernel"] != "library_gemm"]
    by_op = {}
    for e in ours:
        by_op.setdefault(e["kernel"], []).append(e)
    dominant = None
    if by_op:
        name, group = max(by_op.items(), key=lambda kv: sum(e["ms_per_step"] for e in kv[1]))
        launches = sum(e["launches"] for e in group)
        total_ms = sum(e["mean_ms"] * e["launches"] for e in group)
        work = sum(e["achieved"] * e["mean_ms"] * e["launches"] for e in group)        # (rate x time = work, per entry)
        lead = max(group, key=lambda e: e["ms_per_step"])
        dominant = {"bound": lead["bound"], "achieved": round(work / total_ms, 2), "peak": lead["peak"], "unit": lead["unit"],
                    "frac": round(work / total_ms / lead["peak"], 4),
                    "traffic": lead["traffic"], "kernel": name, "mean_ms": round(total_ms / launches, 5),
                    "launches": launches, "ms_per_step": round(sum(e["ms_per_step"] for e in group), 5),
                    "shapes": [e["shape"] for e in group],
                    "device_kernels": lead.get("device_kernels", PMC_KERNELS.get(name, []))}
        for k in ("mfma_busy_pct", "valu_issue_pct_min", "traffic_stale"):
            if k in lead:
                dominant[k] = lead[k]
        if all("trace_ms" in e for e in group):      # the same op in the committed trace of the replayed step, launch-weighted
            dominant["trace_ms"] = round(sum(e["trace_ms"] * e["launches"] for e in group) / launches, 5)
    else:
        dominant = dict(entries[0])
    kernel_ms = sum(e["ms_per_step"] for e in entries)
    lib_ms = sum(e["ms_per_step"] for e in entries if e["kernel"] == "library_gemm")
    return {
        "roofline": dominant,
        "traffic_source": "profiles/%s_pmc_traffic.json: rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this command "
                          "(committed evidence; no profiler is attached in this run)" % EVIDENCE_TAG,
        # how much of the step the per-kernel table accounts for (its durations come from the kernel-by-kernel pass,
        # ms_per_step from the replayed graphs; the rest is framework glue: small element-wise kernels, copies, gaps)
        "step_coverage": {"timed_ops_ms": round(kernel_ms, 3), "of_ms_per_step": round(kernel_ms / ms_step, 3),
                          "library_gemm_ms": round(lib_ms, 3), "hand_written_ms": round(kernel_ms - lib_ms, 3)},
        "roofline_all": entries,
    }


COMPACT_LIMIT = 2000        # bytes: the driver keeps a 2000-character tail of stdout and parses the last line of it


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def compact_line(full):
    """The ONE stdout line: the driver-contract fields and the configuration (+ `distributed` for N > 1; with --full also
    `roofline`, `cpu_baseline`, `resident_inputs` and one small record per sub-benchmark, each when the full result holds
    it), built from the full result and kept under COMPACT_LIMIT bytes -- the
    record that outgrew the harness in round 3 (21 KB, `parsed: null`) cannot happen again: optional parts are dropped,
    last first, until the line fits (tests/test_bench_line.py)."""
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                        "vs_baseline", "dtype", "data"))
    cfg = full.get("config", {})
    line["config"] = _pick(cfg, ("workload", "global_batch", "parallelism", "launch", "relation_mode", "f32_products", "inputs"))
    if cfg.get("warmup_run"):
        line["config"]["warmup_run"] = str(cfg["warmup_run"]).split(" (")[0]
    line["config"]["workload"] = str(line["config"].get("workload", ""))[:130]
    if full.get("roofline") is not None:
        line["roofline"] = _pick(full["roofline"], ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "mean_ms",
                                                    "launches", "mfma_busy_pct", "valu_issue_pct_min", "traffic_stale", "trace_ms"))
    if full.get("cpu_baseline") is not None:
        cb = full["cpu_baseline"]
        line["cpu_baseline"] = _pick(cb, ("value", "unit", "cores", "kind", "host_cores", "sweep"))
        line["cpu_baseline"]["sample"] = str(cb.get("sample", ""))[:90]
    if full.get("resident_inputs") is not None:
        line["resident_inputs"] = _pick(full["resident_inputs"], ("value", "ms_per_step", "batches"))
    if full.get("distributed") is not None:
        line["distributed"] = _pick(full["distributed"], ("nranks", "backend", "allreduce_payload_bytes", "allreduce_ms_alone",
                                                          "allreduce_busbw_GBs", "overlap", "schedules"))
    if full.get("sub_records"):
        subs = {}
        for tag, rec in full["sub_records"].items():
            if "error" in rec:
                subs[tag] = {"error": str(rec["error"])[:80]}
            else:
                roof = rec.get("roofline") or {}
                subs[tag] = dict(_pick(rec, ("value", "ms_per_step", "dtype")), kernel=str(roof.get("kernel"))[:28], frac=roof.get("frac"))
                if subs[tag].get("dtype") == "f32":
                    del subs[tag]["dtype"]              # (only a sub-record in another arithmetic says so)
        line["sub_records"] = subs
    line["detail"] = full.get("detail_file")
    if len(json.dumps(line)) >= COMPACT_LIMIT:           # first the long texts, then whole optional parts (a hard guarantee)
        line["config"]["workload"] = line["config"]["workload"][:120]
        if "cpu_baseline" in line:
            line["cpu_baseline"]["sample"] = line["cpu_baseline"]["sample"][:100]
    if len(json.dumps(line)) >= COMPACT_LIMIT:
        for rec in line.get("sub_records", {}).values():
            if rec.get("kernel"):
                rec["kernel"] = str(rec["kernel"])[:24]
    for optional in ("detail", "sub_records", "resident_inputs", "distributed"):
        if len(json.dumps(line)) < COMPACT_LIMIT:
            break
        line.pop(optional, None)
    return line


def emit(full, detail_path):
    """Full result -> `detail_path` (and stderr); compact line -> stdout, the last thing printed."""
    full["detail_file"] = os.path.basename(detail_path) if detail_path else None
    text = json.dumps(full)
    if detail_path:
        try:
            with open(detail_path, "w") as fh:
                fh.write(text + "\n")
        except OSError as e:          # a read-only working directory must not cost the record
            print("bench.py: cannot write %s: %s" % (detail_path, e), file=sys.stderr)
            full["detail_file"] = None
    print(text, file=sys.stderr, flush=True)
    line = json.dumps(compact_line(full))
    assert len(line) < COMPACT_LIMIT, "compact line is %d bytes" % len(line)
    print(line, flush=True)


DUMP_LIMIT = 64 * 10 ** 6     # --dump-outputs: bytes on disk in all, the .npy headers (128 bytes a file) included


def sample_outputs(arrays, limit=DUMP_LIMIT):
    """name -> array as float32 (float64 stays float64).  Everything is kept whole while it fits `limit`; otherwise every
    array longer than one common cap is cut to `cap` of its elements, flat indices drawn without replacement by a generator
    seeded 0 and kept in order: the same elements in every run and every build, the same positions in a parameter and its
    gradient."""
    import numpy as np
    out = {}
    for name, a in arrays.items():
        a = np.asarray(a)
        out[name] = np.asarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32, order="C")   # (0-d stays 0-d)
    budget = limit - 128 * len(out)

    def size(cap):
        return sum(min(a.size, cap) * a.itemsize for a in out.values())

    longest = max((a.size for a in out.values()), default=0)
    if size(longest) <= budget:
        return out
    lo, hi = 0, longest                  # the largest cap that fits
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if size(mid) <= budget else (lo, mid - 1)
    for name, a in out.items():
        if a.size > lo:
            out[name] = a.reshape(-1)[np.sort(np.random.default_rng(0).choice(a.size, lo, replace=False))]
    return out


def write_outputs(directory, arrays):
    """`sample_outputs(arrays)` -> directory/<name>.npy."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    kept = sample_outputs(arrays)
    for name, a in kept.items():
        np.save(os.path.join(directory, name + ".npy"), a)
    print("bench.py: %d arrays, %.1f MB -> %s" % (len(kept), sum(a.nbytes for a in kept.values()) / 1e6, directory),
          file=sys.stderr, flush=True)


def step_outputs(trainer, model, loss, gnorm):
    """What a training step hands its caller, on the host: the loss and the global gradient norm it returns, every parameter
    after the Adam update and the (summed) gradient the update used."""
    grad_of = {id(p): g for p, g in zip(trainer.flat.params, trainer.flat.g_views)}
    out = {"loss": loss.detach().double().cpu().numpy(), "grad_norm": gnorm.detach().double().cpu().numpy()}
    for name, p in model.named_parameters():
        out["param." + name] = p.detach().float().cpu().numpy()
        if id(p) in grad_of:
            out["grad." + name] = grad_of[id(p)].float().cpu().numpy()
    return out


def cpu_baseline_worker(batch, threads, budget_s):
    """Runs in a child process (no GPU): CoR2 fwd+bwd of the oracle's reference-faithful torch-CPU port."""
    from oracle import reference_faithful as RF
    from oracle import seeded
    torch.set_num_threads(threads)
    model = RF.CoR2Oracle(ANSWERS).train()
    v, q, a = (torch.from_numpy(x) for x in seeded.seeded_inputs(batch, answers=ANSWERS, seed=3))

    def one():
        model.zero_grad(set_to_none=True)
        RF.kld_sum_loss(model({"v": v, "q": q}), a).backward()

    one()  # warm-up
    steps, t0 = 0, time.perf_counter()
    while steps < 2 or (time.perf_counter() - t0 < budget_s and steps < 50):
        one()
        steps += 1
    dt = (time.perf_counter() - t0) / steps
    print(json.dumps({"value": round(batch / dt, 2), "unit": "samples/s", "cores": threads, "kind": "port",
                      "sample": "CoR2 fwd+bwd, dropout on, batch %d x %d steps; reference-faithful torch-CPU port; %d threads of %d cores"
                                % (batch, steps, threads, os.cpu_count() or 1)}))


def _cpu_baseline_start(batch, threads, budget_s):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--cpu-baseline-worker", str(batch), str(threads), str(budget_s)]
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", OMP_NUM_THREADS=str(threads))
    return subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT)


def _cpu_baseline_collect(proc, batch, threads, hard_timeout_s):
    import subprocess
    try:
        out, err = proc.communicate(timeout=hard_timeout_s)
        line = [ln for ln in out.splitlines() if ln.startswith("{")]
        if proc.returncode == 0 and line:
            return json.loads(line[-1])
        return {"value": None, "unit": "samples/s", "cores": threads, "kind": "port",
                "sample": "failed: rc=%d %s" % (proc.returncode, err[-200:])}
    except subprocess.TimeoutExpired:
        proc.kill()             # (the exact child started above)
        proc.communicate()
        return {"value": None, "unit": "samples/s", "cores": threads, "kind": "port",
                "sample": "did not finish 3 steps of batch %d within %.0f s" % (batch, hard_timeout_s)}


class CpuBaseline:
    """The reference cannot travel to the GPU box; time its op-for-op torch-CPU port (validated against the
    reference's golden vectors in tests/) on the host cores.  Bounded: child processes (no GPU) with a hard timeout, so a
    slow host can never stall the benchmark; run after every GPU measurement of the invocation (beside the GPU
    sub-records they slowed the host-bound graph replays of the short ODA step by 12 %).  A sweep over 16 / 32 / 64 threads,
    one after the other (the reference's thousands of tiny per-sample ops get slower with more: all 256 cores of the pool's
    hosts did not finish three steps in 45 s in round 4); the best one is `value`, the others are reported next to it."""
    THREADS = (16, 32, 64)

    def __init__(self, batch=16, budget_s=8.0):
        self.batch, self.budget_s = batch, budget_s
        self.cores = os.cpu_count() or 1
        self.sweep = sorted({min(t, self.cores) for t in self.THREADS})

    def result(self, hard_timeout_s=60.0):
        runs = [_cpu_baseline_collect(_cpu_baseline_start(self.batch, t, self.budget_s), self.batch, t, hard_timeout_s)
                for t in self.sweep]
        ok = [r for r in runs if r.get("value")]
        best = dict(max(ok, key=lambda r: r["value"]) if ok else runs[0])
        best["host_cores"] = self.cores
        best["sweep"] = {str(r["cores"]): r["value"] for r in runs}
        best["all_runs"] = [{"cores": r["cores"], "value": r["value"], "sample": r["sample"]} for r in runs]
        return best


# The other single-GPU BASELINE configs, attached to the headline line by --full as sub-records (each a child run of this file
# on the same GPU, after the headline's timed region): SURVEY 8d config 3 (the ODA attention op), the ODA head at batch 512
# (configs[2]), the CoR2 step with the relation step's forward on the pairwise kernel, and one rank's share of configs[4].
SUB_RECORDS = [
    ("oda_b512", ["--model", "oda"]),
    ("oda_attention_b512", ["--model", "oda-attention"]),
    ("cor2_pairwise_b512", ["--relation-mode", "0"]),
    ("cor2_bf16_n100_b128", ["--dtype", "bf16", "--regions", "100", "--batch", "128"]),
    # the headline config with the tall projections on the fp32 MFMA engine (v_mfma_f32_16x16x4_f32) instead of the split engine
    # (the default: fp32 in, fp32 accumulate, fp32 out; error against float64 of the fp32 MFMA engine's size, tests/test_gpu_split.py)
    ("cor2_fp32_mfma_b512", ["--f32-products", "mfma"]),
]


def run_sub_records(steps, warmup, detail_path, timeout_s=150.0):
    """Child runs of this file; each prints its own compact line and writes its full record next to ours."""
    import subprocess
    out = {}
    stem = os.path.splitext(detail_path or os.path.join(os.getcwd(), "bench_detail.json"))[0]
    for tag, extra in SUB_RECORDS:
        child_detail = "%s_%s.json" % (stem, tag)
        cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
               "--full", "--no-cpu-baseline", "--no-sub-records", "--detail-file", child_detail] + extra
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout_s, cwd=ROOT)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line:
                out[tag] = {"error": "rc=%d %s" % (r.returncode, r.stderr[-300:])}
                continue
            try:
                full = json.load(open(child_detail))
            except (OSError, ValueError):
                full = json.loads(line[-1])
            keep = ("metric", "value", "unit", "ms_per_step", "dtype", "steps", "warmup", "roofline", "step_coverage",
                    "final_loss", "final_grad_norm")
            rec = {k: full[k] for k in keep if k in full}
            rec["workload"] = full.get("config", {}).get("workload")
            rec["launch"] = full.get("config", {}).get("launch")
            rec["command"] = "bench.py " + " ".join(extra)
            rec["detail_file"] = os.path.basename(child_detail)
            rec["wall_s"] = round(time.perf_counter() - t0, 1)
            out[tag] = rec
        except subprocess.TimeoutExpired:
            out[tag] = {"error": "did not finish within %.0f s" % timeout_s}
    return out


def launch_ranks(args):
    """`bench.py --gpus N` started WITHOUT a launcher: start the N ranks here (torch.distributed.run as a child process,
    before this process has touched the GPU), relay their output and exit with their code.  Fails loudly when the node
    has fewer than N GPUs -- never a silent one-GPU measurement."""
    import socket
    import subprocess
    rehearsal = os.environ.get("VQA_ONE_GPU_REHEARSAL") == "1"
    n_dev = torch.cuda.device_count()           # (counting devices does not initialise the GPU)
    if n_dev < args.gpus and not rehearsal:
        raise SystemExit("bench.py --gpus %d: only %d GPU(s) visible on this node; refusing to measure fewer ranks than asked"
                         % (args.gpus, n_dev))
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    rc = subprocess.run(cmd, env=env, cwd=ROOT).returncode
    raise SystemExit(rc)


def bench_oda_attention(args, world, rank, dev, ops):
    """the ODA attention op alone.  Given the compressed regions v_low [B,N,310], the compressed
    question q_low [B,310], the regions v [B,N,2048] and the attention filter (4, N*310): logits (K2, dropout 0.5 in the
    kernel) -> softmax over regions + pooling (K3), forward + backward with a fixed upstream gradient.  No optimizer."""
    torch.manual_seed(100 + rank)
    B, N = args.batch, args.regions
    w = (torch.randn(GLIMPSES, N * LOW, device=dev) / (N * LOW) ** 0.5).requires_grad_()
    bias = torch.zeros(GLIMPSES, device=dev, requires_grad=True)
    sets = []      # ROTATE input sets visited in turn (the 151 MB of regions per set then come from HBM); --no-rotate: one
    for _ in range(1 if args.no_rotate else ROTATE):
        sets.append((torch.relu(torch.randn(B, N, LOW, device=dev)).requires_grad_(),
                     torch.relu(torch.randn(B, LOW, device=dev)).requires_grad_(),
                     torch.randn(B, N, FEAT, device=dev), torch.randn(B, GLIMPSES, FEAT, device=dev)))

    def step(seed):
        vl, ql, v, g_pooled = sets[seed % len(sets)]
        for t in (vl, ql, w, bias):
            t.grad = None
        logits = ops.object_difference_attention(vl, ql, w, bias, 0.5, seed)
        alpha, pooled = ops.softmax_attention_pool(logits, v)
        torch.autograd.backward([pooled], [g_pooled])
        return alpha, pooled

    for i in range(args.warmup):
        step(1000 + i)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    timer = ops.KernelTimer()
    t0 = time.perf_counter()
    for i in range(args.steps):
        alpha, pooled = step(2000 + i)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:     # the last timed step's outputs and gradients, before the per-kernel pass reruns it
        vl, ql = sets[(2000 + args.steps - 1) % len(sets)][:2]
        write_outputs(args.dump_outputs, {name: t.detach().float().cpu().numpy() for name, t in (
            ("alpha", alpha), ("pooled", pooled), ("grad.v_low", vl.grad), ("grad.q_low", ql.grad), ("grad.filter", w.grad),
            ("grad.bias", bias.grad))})
    if args.full:
        ops.set_kernel_timer(timer)
        for i in range(min(args.steps, 10)):       # per-kernel durations from a second pass (event pairs around each launch)
            torch.cuda._sleep(24_000_000)
            step(3000 + i)
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
    t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = float(t.item())
    assert torch.isfinite(alpha).all() and torch.isfinite(w.grad).all() and all(torch.isfinite(st[0].grad).all() for st in sets if st[0].grad is not None)
    if rank == 0:
        result = {
            "metric": "ODA object-difference attention op samples/sec (fwd+bwd), batch %d, %dx%d pairwise" % (B, N, N),
            "value": round(world * B * args.steps / elapsed, 1), "unit": "samples/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
            "config": {"workload": "ODA attention op alone (BASELINE configs[2]; SURVEY 8d config 3): v_low [%d,%d,310], q_low, "
                                   "v [%d,%d,2048], filter (4, %d) -> alpha, pooled; fwd+bwd, dropout 0.5 in K2"
                                   % (B, N, B, N, N * LOW), "global_batch": world * B, "launch": "eager",
                       "parallelism": "dp%d" % world}}
        if args.full:
            entries = step_table(timer, min(args.steps, 10), B, N, False, "oda-attention")
            dominant = next(e for e in entries if e["bound"] is not None)
            result["roofline"] = {k: dominant[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel",
                                                           "mean_ms", "launches", "mfma_busy_pct", "valu_issue_pct_min")
                                  if k in dominant}
            result["roofline_all"] = entries
        emit(result, args.detail_file)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--cpu-baseline-worker":
        return cpu_baseline_worker(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]))
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    # defaults: a timed region of ~0.5 s (200 replayed steps) behind 10 warm-up steps -- long enough for a utilisation sampler
    # and for the clocks to settle (measured: 20, 200 and 1000 timed steps after 10 warm-up steps agree within 0.2 %; after
    # only 5 the first timed steps still run ~1 % slow); the whole default run with --full, sub-records and CPU baseline
    # included, takes about 75 s
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--full", action="store_true", help="after the timed region, also measure what takes runs of its own: "
                    "the per-kernel roofline pass, the resident-batch pass, the all-reduce alone (N > 1), the sub-records "
                    "and the CPU baseline (headline config at N = 1); without it a run only sets up, warms up, times the "
                    "steps, writes --dump-outputs and prints the line")
    ap.add_argument("--batch", type=int, default=BATCH, help="per-GPU batch (BASELINE config: 512)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: leave out the CPU baseline")
    ap.add_argument("--relation-mode", type=int, default=1, help="K1: 0 = pairwise, 1 = factored")
    ap.add_argument("--model", default="cor2", choices=["cor2", "oda", "oda-attention"], help="cor2 = the headline config; "
                    "oda = the ODA head (3000 answers), reported the same way; oda-attention = BASELINE configs[2] / SURVEY "
                    "8d config 3: the object-difference attention op alone (K2 logits + K3 softmax-pool, fwd+bwd)")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="f32 = the reference's arithmetic (headline); "
                    "bf16 = BASELINE configs[4]: bf16 storage + bf16 MFMA on the region side, fp32 accumulate, fp32 "
                    "master weights (use with --regions 100 --batch 128)")
    ap.add_argument("--f32-products", default=os.environ.get("VQA_F32_PRODUCTS", "split"), choices=["mfma", "split"],
                    help="how the tall fp32 projections form their products: split (default, the headline since round 5) = exact "
                         "three-way bf16 splits of both operands, six partial products on v_mfma_f32_16x16x32_bf16, fp32 "
                         "accumulation; mfma = v_mfma_f32_16x16x4_f32")
    ap.add_argument("--regions", type=int, default=REGIONS, help="regions per image (36; configs[4]: 100 dense regions)")
    ap.add_argument("--encoder", action="store_true", help="include the question encoder (SURVEY 8f row 3): SkipThoughts = "
                    "embedding(620) + 26-step BayesianGRU(2400), randomly initialised, fed int64 token ids [B,26] instead of "
                    "question vectors")
    ap.add_argument("--overlap", action="store_true", help="CoR2: backward in two halves, the second reasoning step's "
                    "gradients all-reduced under the second half (trainer overlap; at one GPU it only splits the backward)")
    ap.add_argument("--no-rotate", action="store_true", help="time the steps on ONE resident batch instead of %d rotating ones" % ROTATE)
    ap.add_argument("--copy-inputs", action="store_true", help="rotating batches are COPIED into one pair of graph input buffers "
                    "(one device-to-device copy per step inside the timed region) instead of the step being captured once per "
                    "resident batch (trainer input_slots)")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel from the host instead of replaying "
                    "the captured hipGraphs of the step")
    ap.add_argument("--detail-file", default=os.path.join(os.getcwd(), "bench_detail.json"), help="where the full record "
                    "(with --full: roofline_all, counters, step coverage, full sub-records) is written; stdout carries the "
                    "compact line only")
    ap.add_argument("--no-sub-records", action="store_true", help="--full: do not attach the other single-GPU "
                    "BASELINE configs (ODA, the ODA attention op, CoR2 pairwise, CoR2 bf16 N=100) as sub-records")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (float32; "
                    "float64 scalars): loss, grad_norm, param.<name> after the update and grad.<name> (the ODA attention op: "
                    "alpha, pooled, the input and filter gradients); at most 64 MB in all, larger tensors as a fixed seeded "
                    "sample of their elements (sample_outputs).  Same arguments, same inputs: two builds compare output for output")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1: the timed region is exactly that many steps")
    os.environ["VQA_F32_PRODUCTS"] = args.f32_products     # (read per call by ops.split_products; children inherit it)

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args)          # no launcher around us: start the ranks ourselves (never measure 1 GPU silently)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if os.environ.get("VQA_ONE_GPU_REHEARSAL") == "1":
        local = 0                                               # all ranks share GPU 0 (gloo rehearsal only)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    if world != args.gpus:
        raise SystemExit("bench.py --gpus %d but the launcher started %d rank(s): the two must agree" % (args.gpus, world))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the HIP path has no CPU fallback")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        backend = os.environ.get("VQA_DIST_BACKEND", "nccl")   # "nccl" IS RCCL on ROCm; "gloo" only to rehearse the
        if backend == "nccl":                                   # multi-rank flow on a single-GPU box
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("process group has %d rank(s), --gpus says %d" % (dist.get_world_size(), args.gpus))

    from vqa_playground_pytorch_amd import CoR2Model, ODAModel, ops
    from vqa_playground_pytorch_amd.trainer import DataParallelTrainer

    if args.model == "oda-attention":
        return bench_oda_attention(args, world, rank, dev, ops)

    answers = ANSWERS if args.model == "cor2" else 3000
    bf16 = args.dtype == "bf16"
    if bf16 and args.model != "cor2":
        raise SystemExit("--dtype bf16 is the CoR2 configuration (BASELINE configs[4])")
    B = args.batch

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def log(msg):
        if rank == 0 and os.environ.get("VQA_BENCH_VERBOSE"):
            print("[bench %.1fs] %s" % (time.perf_counter() - t_start, msg), file=sys.stderr, flush=True)

    def max_over_ranks(seconds):
        t = torch.tensor([seconds], device=dev, dtype=torch.float64)
        if world > 1:
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    t_start = time.perf_counter()
    # `value` is measured over ROTATE different resident batches, visited in turn: every step's 151 MB of regions then comes from
    # HBM and not from the 256 MB Infinity Cache (one batch re-read every step would).  The batches are the slots of a feeder's
    # ring: the trainer captures the forward + backward graph once per slot (input_slots), each reading its slot in place, so no
    # step copies its batch (--copy-inputs: one pair of graph input buffers and a device-to-device copy per step, rounds 1-4's
    # rotating pass).  The resident-batch figure is reported beside it (`config.inputs`, `resident_inputs`).  --no-rotate: the
    # resident batch only (profiling passes).
    rotate = not args.no_rotate and not args.encoder

    def run_schedule(overlap):
        """Model + trainer + the W warm-up steps + EXACTLY K timed steps between barriers (MAX over ranks) for one gradient-
        reduction schedule (overlap False: one all-reduce between backward and clip; True: backward in two halves, the second
        reasoning step's gradients reduced under the second half).  Same seeds either way: same weights, same batches."""
        torch.manual_seed(1234)
        if args.model == "cor2":
            vocab = ["PAD", "UNK"] + ["w%d" % i for i in range(14998)] if args.encoder else ["PAD", "UNK"]
            model = CoR2Model(vocab, answers, relation_mode=args.relation_mode,
                              compute_dtype=torch.bfloat16 if bf16 else None,
                              seq2vec="skipthoughts" if args.encoder else None).to(dev).train()
        else:
            model = ODAModel(["PAD", "UNK"], answers).to(dev).train()
        # adopt_inputs: the synthetic batches are resident; the first one's tensors become the replayed graphs' input buffers
        # (a real feeder goes through the trainer's private input buffers: tools/feed_bench.py)
        trainer = DataParallelTrainer(model, lr=1e-4, clip=0.25, graph=not args.no_graph, adopt_inputs=True,
                                      overlap=("force" if world == 1 else True) if overlap else False,
                                      input_slots=1 if (not rotate or args.copy_inputs) else ROTATE)
        torch.manual_seed(100 + rank)  # per-rank dropout streams and data shards differ
        v = torch.randn(B, args.regions, FEAT, device=dev)
        if bf16:
            v = v.to(torch.bfloat16)   # the feature store hands over bf16 regions: half the bytes of the dominant stream
        q = torch.randn(B, QDIM, device=dev)
        if args.encoder:      # left-aligned token ids, 0 = PAD, lengths 5..26 (datasets.py:671-672)
            lengths = torch.randint(5, 27, (B,), device=dev)
            q = torch.randint(1, 15000, (B, 26), device=dev) * (torch.arange(26, device=dev)[None, :] < lengths[:, None])
        a = torch.softmax(2.0 * torch.randn(B, answers, device=dev), dim=1)
        batches = [({"v": v, "q_idxes": q}, a)]
        if rotate:
            for _ in range(ROTATE - 1):
                batches.append(({"v": torch.randn_like(v.float()).to(v.dtype), "q_idxes": torch.randn_like(q)},
                                torch.softmax(2.0 * torch.randn(B, answers, device=dev), dim=1)))
        # 2 eager steps precede the first capture; each further input slot is captured by the first step that lands in it; and the
        # FIRST replay of a captured graph is not a steady-state step either (hipGraphLaunch uploads the executable graph then:
        # measured 2.05 ms per step over 20 steps that hold the four first replays against 2.00 without them), so the warm-up runs
        # until every slot's graph has been replayed once -- at least W steps, never fewer; the timed region is exactly K replays
        slots = 1 if (not rotate or args.copy_inputs) else ROTATE
        warm = max(args.warmup, 2 + 2 * slots) if not args.no_graph else args.warmup
        for i in range(warm):
            trainer.step(*batches[i % len(batches)])
            if i == 0:
                torch.cuda.synchronize()
                log("first step done")
        graphed = trainer._graph is not None
        log("warmup done (graph replay: %s, overlap: %s)" % (graphed, bool(trainer.overlap)))
        timer = ops.KernelTimer()
        barrier()
        if not graphed and args.no_graph:     # (with or without --full: the timed steps are the same either way)
            ops.set_kernel_timer(timer)
        t0 = time.perf_counter()
        for i in range(args.steps):
            loss, gnorm = trainer.step(*batches[i % len(batches)])
        barrier()
        elapsed = time.perf_counter() - t0
        ops.set_kernel_timer(None)
        log("timed region done: %.3f s" % elapsed)
        out = {"trainer": trainer, "model": model, "batches": batches, "graphed": graphed, "timer": timer, "warm": warm,
               "elapsed": max_over_ranks(elapsed), "elapsed_local": elapsed, "overlap": bool(trainer.overlap),
               "final_loss": float(loss.item()), "final_gnorm": float(gnorm.item()), "resident": None,
               # (taken before any further step runs on this trainer: the resident pass below updates the same weights)
               "outputs": step_outputs(trainer, model, loss, gnorm) if args.dump_outputs and rank == 0 else None}
        # --full: the same steps on ONE resident batch (no copy, inputs from the Infinity Cache), what rounds 1-4 reported
        # as `value`
        if rotate and args.full:
            for _ in range(2):
                trainer.step(*batches[0])
            barrier()
            r0 = time.perf_counter()
            for _ in range(args.steps):
                trainer.step(*batches[0])
            barrier()
            r_el = max_over_ranks(time.perf_counter() - r0)
            out["resident"] = {"batches": 1, "value": round(world * B * args.steps / r_el, 1), "unit": "samples/s",
                               "ms_per_step": round(1e3 * r_el / args.steps, 3),
                               "note": "one resident batch re-read every step (it fits the 256 MB Infinity Cache), no copy"}
        return out

    # N > 1: BOTH reduction schedules in one invocation (no scaling run has ever told them apart: VERDICT r04 item 6); `value` is
    # the faster one, `distributed.schedules` holds both.  N = 1: the single-pass step (there is nothing to overlap with).
    schedules = [bool(args.overlap)]
    if world > 1 and not args.overlap and args.model in ("cor2", "oda") and not args.no_graph and \
            os.environ.get("VQA_BENCH_BOTH_SCHEDULES", "1") == "1":
        schedules = [False, True]
    runs = []
    for ov in schedules:
        if runs:       # free the previous schedule's model, graphs and activations before building the next
            prev = runs[-1]
            for k in ("trainer", "model", "batches", "timer"):
                prev.pop(k, None)
            import gc
            gc.collect()
            torch.cuda.empty_cache()
        try:
            runs.append(run_schedule(ov))
        except Exception as e:      # noqa: BLE001 -- the second schedule must not cost the first one's record
            if not runs:
                raise
            print("bench.py: schedule overlap=%s failed (%s: %s); keeping the first" % (ov, type(e).__name__, e), file=sys.stderr)
            runs.append({"failed": "%s: %s" % (type(e).__name__, str(e)[:200]), "overlap": ov})
            break
    done = [r for r in runs if "elapsed" in r]
    best = min(done, key=lambda r: r["elapsed"])
    if args.dump_outputs and rank == 0:
        write_outputs(args.dump_outputs, best["outputs"])
    live = done[-1]                 # (the schedule whose trainer is still alive: the per-kernel pass below runs on it)
    trainer, batches, graphed, timer = live["trainer"], live["batches"], live["graphed"], live["timer"]
    (sample, a), v = batches[0], batches[0][0]["v"]
    elapsed, resident = best["elapsed"], best["resident"]
    final_loss, final_gnorm = best["final_loss"], best["final_gnorm"]
    if args.full and (graphed or not args.no_graph):
        # HIP events cannot be recorded inside hipGraph replays, so the per-kernel durations for `roofline` are taken
        # live from an identical run of the same steps launched kernel by kernel, right after the timed region.
        # Each of these steps is queued behind a ~10 ms device-side sleep, so the host has enqueued the whole step before
        # the GPU starts it: the event pairs then bracket back-to-back kernels (pure kernel time, which is what
        # rocprofv3's per-kernel average reports) instead of the host's launch gaps.
        for i in range(min(args.steps, 10) + 2):
            if i == 2:                      # two untimed eager steps first: allocator and caches as in steady state
                ops.set_kernel_timer(timer)
            torch.cuda._sleep(24_000_000)
            trainer.step_eager(*batches[i % len(batches)])
        barrier()
        ops.set_kernel_timer(None)
    headline = world == 1 and args.model == "cor2" and not bf16 and args.regions == REGIONS and not args.encoder
    want_cpu = rank == 0 and headline and args.full and not args.no_cpu_baseline
    dist_info = None
    if world > 1:
        # what a reader needs to sanity-check a scaling record: ranks seen by the process group, the all-reduce payload, the
        # per-rank rate and, with --full, the all-reduce's duration measured on its own (back to back, nothing to overlap with)
        payload = trainer.flat.g
        dist_info = {"nranks": dist.get_world_size(), "backend": dist.get_backend(), "allreduce_payload_bytes": payload.numel() * 4,
                     "per_rank_samples_per_s": round(B * args.steps / elapsed, 1), "overlap": bool(best["overlap"]),
                     # both reduction schedules, timed in this invocation (K steps each); `value` is the faster one
                     "schedules": {("overlap" if r["overlap"] else "single"):
                                   ({"value": round(world * B * args.steps / r["elapsed"], 1),
                                     "ms_per_step": round(1e3 * r["elapsed"] / args.steps, 3)} if "elapsed" in r
                                    else {"error": r["failed"]}) for r in runs}}
        if args.full:
            for _ in range(3):
                dist.all_reduce(payload, op=dist.ReduceOp.SUM)
            barrier()
            a0 = time.perf_counter()
            for _ in range(10):
                dist.all_reduce(payload, op=dist.ReduceOp.SUM)
            barrier()
            ar_ms = 1e3 * (time.perf_counter() - a0) / 10
            payload.zero_()
            dist_info["allreduce_ms_alone"] = round(ar_ms, 3)
            dist_info["allreduce_busbw_GBs"] = round(2 * (world - 1) / world * payload.numel() * 4 / (ar_ms * 1e-3) / 1e9, 1)
    # sanity of the timed steps themselves (a replayed graph that computed garbage would still be fast): the loss of
    # the last timed step is finite and positive (a KL divergence) and the gradient norm is of a trainable size
    assert final_loss == final_loss and 0.0 < final_loss < 1e6, "implausible loss %r in the timed region" % final_loss
    assert final_gnorm == final_gnorm and 0.0 < final_gnorm < 1e4, "implausible gradient norm %r" % final_gnorm

    if rank == 0:
        ms_step = 1e3 * elapsed / args.steps
        if rotate:
            inputs = "%d rotating batches (%s)" % (ROTATE, "+1 device copy/step" if args.copy_inputs else
                                                   "a step graph per batch slot, no copy")
            inputs_note = ("`value` visits %d different resident batches in turn (%.0f MB of regions each: together beyond the "
                           "256 MB Infinity Cache); %s" % (ROTATE, v.numel() * v.element_size() / 1e6,
                                                           "one device-to-device copy into the replayed graphs' input buffers "
                                                           "per step inside the timed region" if args.copy_inputs else
                                                           "the forward + backward graph is captured once per batch slot and "
                                                           "reads its slot in place (trainer input_slots), no copy"))
            if resident is not None:         # (--full)
                inputs += "; 1 resident batch: %.1f (%+.1f%%)" % (
                    resident["value"], 100.0 * (resident["value"] / (world * B * args.steps / elapsed) - 1.0))
                inputs_note += "; `resident_inputs` re-reads ONE batch (cache-resident)"
        else:
            inputs, inputs_note = "1 resident batch", "ONE resident batch re-read every step"
        result = {
            "metric": "VQA samples/sec (fwd+bwd), %s batch %d, %dx2048 regions%s"
                      % ("CoR2" if args.model == "cor2" else "ODA", B, args.regions,
                         ", incl. SkipThoughts question encoder" if args.encoder else ""),
            "value": round(world * B * args.steps / elapsed, 1),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {"workload": ("CoR2 fwd+bwd bf16 (bf16 regions + bf16 MFMA, fp32 accumulate + master weights), batch %d/GPU, "
                                    "%dx2048 regions + 2400-d question, 2-step chain, 2000 answers (BASELINE configs[4])"
                                    % (B, args.regions)) if bf16 else
                       ("CoR2 fwd+bwd fp32, batch %d/GPU, %dx2048 regions + 2400-d question, 2-step chain, 2000 answers "
                        "(BASELINE configs[1]; configs[3] at 8 GPUs)" % (B, args.regions))
                       if args.model == "cor2" else
                       ("ODA fwd+bwd fp32, batch %d/GPU, 36x2048 regions + 2400-d question, 36x36 object-difference "
                        "attention, 3000 answers (BASELINE configs[2])" % B),
                       "global_batch": world * B, "step": "forward + KLD-sum loss + backward + grad sum-all-reduce "
                       "+ clip 0.25 + Adam (dropout active)", "parallelism": "dp%d" % world,
                       "launch": ("hipGraph replay (3 graphs: backward in two halves, the first all-reduce under the second)"
                                  if best["overlap"] else "hipGraph replay (2 graphs + eager all-reduce)") if best["graphed"] else "eager",
                       "warmup_run": ("%d untimed steps (>= --warmup: 2 kernel-by-kernel, then every input slot's graph captured and "
                                      "replayed once -- a graph's first launch uploads it)" % best["warm"]) if best["graphed"] else
                                     "%d untimed steps" % best["warm"],
                       "relation_mode": "factored" if args.relation_mode == 1 else "pairwise",
                       "f32_products": ("fp32 MFMA (v_mfma_f32_16x16x4_f32)" if args.f32_products == "mfma" else
                                        "3xbf16 split, 6 partial products, fp32 accumulate"),
                       "library_gemms": __import__("vqa_playground_pytorch_amd.tuned_gemms", fromlist=["describe"]).describe(),
                       "inputs": inputs, "inputs_note": inputs_note},
            "final_loss": round(final_loss, 3), "final_grad_norm": round(final_gnorm, 3),
        }
        if args.full:
            result.update(roofline_record(timer, args, B, bf16, graphed, ms_step))
        if resident is not None:
            result["resident_inputs"] = resident
        if world > 1:
            result["distributed"] = dist_info
        if args.full and headline and B == BATCH and not args.no_sub_records and graphed:
            # the other single-GPU BASELINE configs, measured on this GPU in the same invocation (child runs of this file)
            result["sub_records"] = run_sub_records(args.steps, args.warmup, args.detail_file)
        if want_cpu:       # after the GPU sub-records: a 16-thread CPU job beside them cost the ODA record 12 % (host-bound replays)
            result["cpu_baseline"] = CpuBaseline().result()
        emit(result, args.detail_file)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
