"""Helpers to run a function across N processes with the gloo backend
(CPU; the same code path runs over RCCL on the MI355X node), and a
host-staged communicator that lets several rank processes share ONE GPU:
compute stays on the device, the wire is gloo on host copies."""

import datetime
import os
import pickle
import tempfile
import time

import torch
import torch.multiprocessing as mp

from cuvite_amd.parallel import Comm


class HostStagedComm(Comm):
    """Comm whose `device` is the compute device while every collective
    runs on host copies through a stock CPU `Comm` (count negotiation,
    recv_counts, self-copy and empty peers stay the production code); the
    results are copied back to `device`. No device tensor ever reaches
    torch.distributed, so rank processes need neither RCCL nor a GPU each."""

    def __init__(self, device: torch.device):
        super().__init__(device, transport="p2p")
        self._host = Comm(torch.device("cpu"), transport="p2p")

    def allreduce_sum_(self, t: torch.Tensor) -> torch.Tensor:
        h = t.cpu()
        self._host.allreduce_sum_(h)
        if h is not t:
            t.copy_(h)
        return t

    def allreduce_scalar(self, x: float, op: str = "sum") -> float:
        return self._host.allreduce_scalar(x, op)

    def allgather_counts(self, counts: torch.Tensor) -> torch.Tensor:
        return self._host.allgather_counts(counts.cpu()).to(self.device)

    def barrier(self):
        self._host.barrier()

    def all_to_all_v(self, send, recv_counts=None):
        got = self._host.all_to_all_v([s.cpu() for s in send], recv_counts)
        return [g.to(self.device) for g in got]

    def exchange_fixed(self, send, recv):
        h_recv = [torch.empty(r.shape, dtype=r.dtype) for r in recv]
        self._host.exchange_fixed([s.cpu() for s in send], h_recv)
        for r, h in zip(recv, h_recv):
            if r.numel():
                r.copy_(h)


def _worker(rank, world, fn, args, port, out_dir, init_timeout_s):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["RANK"] = str(rank)
    os.environ["WORLD_SIZE"] = str(world)
    import torch.distributed as dist
    # short collective timeout: a rank whose peer died errors out instead
    # of waiting for the 30 minute default
    dist.init_process_group(
        "gloo", rank=rank, world_size=world,
        timeout=datetime.timedelta(seconds=init_timeout_s))
    try:
        result = fn(rank, world, *args)
        with open(os.path.join(out_dir, f"out_{rank}.pkl"), "wb") as f:
            pickle.dump(result, f)
    finally:
        dist.destroy_process_group()


def _reap(procs):
    """Terminate, then kill, every process still alive; returns the ranks
    that had to be stopped. No process outlives the caller."""
    stragglers = [r for r, p in enumerate(procs) if p.is_alive()]
    for r in stragglers:
        procs[r].terminate()
    for r in stragglers:
        procs[r].join(timeout=10)
    for r in stragglers:
        if procs[r].is_alive():
            procs[r].kill()
            procs[r].join(timeout=10)
    return stragglers


def run_dist(world: int, fn, *args, port: int = None, timeout_s: float = 300,
             init_timeout_s: float = 60):
    """Run fn(rank, world, *args) in `world` processes; returns [result_rank0,
    ..., result_rankN-1]. `timeout_s` bounds the whole launch; a rank still
    running after it is stopped and fails the launch. One attempt, no
    retries: a rank that exits non-zero (a signal shows as a negative exit
    code) or runs out of time fails the caller."""
    if port is None:
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
    with tempfile.TemporaryDirectory() as out_dir:
        ctx = mp.get_context("spawn")
        procs = []
        try:
            for r in range(world):
                p = ctx.Process(target=_worker,
                                args=(r, world, fn, args, port, out_dir,
                                      init_timeout_s))
                p.start()
                procs.append(p)
            deadline = time.monotonic() + timeout_s
            for p in procs:
                p.join(timeout=max(0.0, deadline - time.monotonic()))
        finally:
            stragglers = _reap(procs)
        assert not stragglers, \
            f"rank(s) {stragglers} still running after {timeout_s} s; stopped"
        for r, p in enumerate(procs):
            assert p.exitcode == 0, f"rank {r} exited with {p.exitcode}"
        outs = []
        for r in range(world):
            with open(os.path.join(out_dir, f"out_{r}.pkl"), "rb") as f:
                outs.append(pickle.load(f))
        return outs
