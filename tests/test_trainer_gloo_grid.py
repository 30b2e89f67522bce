"""world_size-2 `gloo` test of the mean losses' global-batch scale: BCE and CE are means over the GLOBAL batch in the reference
(under DataParallel the criterion sees the gathered outputs) while the gradient all-reduce is a SUM, so every rank scales by its
local batch x the world size.  Two ranks on half batches must reproduce one process on the whole batch -- losses that add up to
the global loss, the same clipped norm, the same weights -- for BCE + sgd and CE + rms."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

from vqa_playground_pytorch_amd.trainer import DataParallelTrainer

CELLS = (("BCE", "sgd"), ("CE", "rms"))


class Tiny(nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(12, 16)
        self.b = nn.Linear(16, 9)

    def forward(self, sample):
        return self.b(torch.tanh(self.a(sample["x"])))


def make_data(loss, steps=4, batch=8):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(steps):
        x = torch.randn(batch, 12, generator=g)
        if loss == "CE":
            a = torch.randint(0, 9, (batch,), generator=g)
        else:
            a = torch.rand(batch, 9, generator=g) * (torch.rand(batch, 9, generator=g) < 0.3)
        out.append((x, a))
    return out


def run_single(loss, optim):
    torch.manual_seed(0)
    model = Tiny()
    tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, loss=loss, optim=optim)
    out = []
    for x, a in make_data(loss):
        value, norm = tr.step({"x": x}, a)
        out.append((value.item(), norm.item()))
    return out, [p.detach().clone() for p in model.parameters()], tr.lr


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    for loss, optim in CELLS:
        torch.manual_seed(100 + rank)  # different init per rank: the trainer must broadcast rank 0's weights
        model = Tiny()
        if rank == 0:
            torch.manual_seed(0)
            model = Tiny()
        tr = DataParallelTrainer(model, lr=1e-2, clip=0.25, loss=loss, optim=optim)
        losses = []
        for x, a in make_data(loss):
            value, norm = tr.step({"x": tr.shard(x)}, tr.shard(a))
            t = value.clone()
            dist.all_reduce(t)
            losses.append((t.item(), norm.item()))
        q.put((rank, loss, losses, [p.detach().numpy().copy() for p in model.parameters()], tr.lr))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_equal_one_process_under_the_mean_losses():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = [q.get(timeout=120) for _ in range(2 * len(CELLS))]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for loss, optim in CELLS:
        ref_losses, ref_params, ref_lr = run_single(loss, optim)
        cell = sorted((r for r in results if r[1] == loss), key=lambda r: r[0])
        assert [r[0] for r in cell] == [0, 1]
        for rank, _, losses, params, lr in cell:
            assert lr == pytest.approx(ref_lr, rel=1e-12)
            for (l, n), (rl, rn) in zip(losses, ref_losses):
                assert l == pytest.approx(rl, rel=1e-5)     # the ranks' shares add up to the mean over the global batch
                assert n == pytest.approx(rn, rel=1e-5)     # clip sees the global-batch gradient norm on every rank
            for p, rp in zip(params, ref_params):
                np.testing.assert_allclose(p, rp.numpy(), rtol=1e-4, atol=1e-6)
        for p0, p1 in zip(cell[0][3], cell[1][3]):
            np.testing.assert_allclose(p0, p1, rtol=0, atol=1e-7)   # replicas stay in lock-step
