"""The multi-rank step on hardware that has ONE GPU: two ranks (gloo, device tensors) share cuda:0 and must reproduce the
single-process step on the whole batch -- kernel by kernel and replayed from hipGraphs, with the single flat all-reduce and
with the two-half backward whose first all-reduce runs under the second half (trainer.DataParallelTrainer; train.py:517's
DataParallel replaced by one process per GPU).  backend = "nccl" puts rank r on cuda:r and the collectives on RCCL across
the devices -- BASELINE configs[3]'s transport; it needs >= 2 GPUs and is skipped on the one-GPU test box."""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "dp2_one_gpu.py")


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(world, env):
    # (VQA_DUMP_AFTER: should a run hang, every rank prints its threads' stacks after that many seconds and exits)
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VQA_DUMP_AFTER="240", **env)
    if world == 1:
        cmd = [sys.executable, TOOL]
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr",
               "127.0.0.1", "--master-port", str(_free_port()), TOOL]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=420, env=e, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[-1])


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
@pytest.mark.parametrize("model", ["cor2", "oda"])
def test_two_ranks_match_one_process(model, backend):
    if backend == "nccl" and torch.cuda.device_count() < 2:       # (counting devices does not initialise the GPU)
        pytest.skip("RCCL across devices needs >= 2 GPUs; this box has %d" % torch.cuda.device_count())
    want = _run(1, {"G": "0", "MODEL": model})
    assert want["world"] == 1 and len(want["losses"]) == 7
    for graph in ("0", "1"):
        for overlap in ("0", "1"):
            got = _run(2, {"G": graph, "VQA_DP_OVERLAP": overlap, "MODEL": model, "BACKEND": backend})
            tag = (model, backend, graph, overlap)
            assert got["world"] == 2 and got["backend"] == backend, tag
            assert got["graph"] == (graph == "1"), tag           # the step really was captured / really was not
            assert got["overlap"] == (overlap == "1"), tag
            for a, b in zip(got["losses"], want["losses"]):
                assert abs(a - b) <= 1e-4 * abs(b), (tag, got["losses"], want["losses"])
            for a, b in zip(got["norms"], want["norms"]):
                assert abs(a - b) <= 1e-3 * abs(b), (tag, got["norms"], want["norms"])
            # (a sum over a few thousand weights after 7 Adam steps: the two ranks add their gradient halves in another
            #  order than one process does, and Adam's normalisation amplifies rounding where a gradient is near zero)
            assert abs(got["weight_digest"] - want["weight_digest"]) <= 1e-4 * abs(want["weight_digest"]) + 1e-5, tag


def test_bench_two_rank_rehearsal_prints_a_valid_record(tmp_path):
    """`bench.py --gpus 2` as the driver's scaling run starts it, rehearsed on ONE GPU: VQA_ONE_GPU_REHEARSAL=1 lets both ranks
    share cuda:0, gloo carries the collectives.  The first 8-GPU run must produce a valid record without a second try
    (VERDICT r04 item 6): the compact line parses, stays under 2 KB WITH the `distributed` block, says n_gpus = 2 and a global
    batch of 2 per-rank batches, and the block holds BOTH reduction schedules (single all-reduce / two-half backward with
    the first all-reduce under the second half), `value` being the faster one.  With --full, as here, the line also carries
    the roofline of the per-kernel pass and the block the all-reduce timed on its own."""
    detail = tmp_path / "bench_detail.json"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", VQA_ONE_GPU_REHEARSAL="1", VQA_DIST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "3", "--batch", "64",
           "--full", "--detail-file", str(detail)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    assert len(lines[0]) < 2000
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["steps"] == 4 and line["warmup"] == 3 and line["scaling"] == "weak"
    assert line["config"]["global_batch"] == 128 and line["config"]["parallelism"] == "dp2"
    assert line["dtype"] == "f32" and line["config"]["f32_products"].startswith("3xbf16 split")
    d = line["distributed"]
    assert d["nranks"] == 2 and d["backend"] == "gloo" and d["allreduce_payload_bytes"] >= 4 * 11940244
    assert set(d["schedules"]) == {"single", "overlap"} and d["allreduce_ms_alone"] > 0
    rates = [s["value"] for s in d["schedules"].values()]
    assert all(v > 0 for v in rates) and abs(line["value"] - max(rates)) <= 1e-6 * max(rates)
    assert "roofline" in line and line["roofline"]["frac"] is not None and 0 < line["roofline"]["frac"] < 1
    assert "cpu_baseline" not in line and "sub_records" not in line          # N = 1 only
    full = json.load(open(detail))
    assert full["distributed"]["schedules"].keys() == d["schedules"].keys() and len(full["roofline_all"]) > 10
