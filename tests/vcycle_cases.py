"""CPU-only builders shared by the V-cycle tests (test_vcycle.py,
test_gpu_vcycle.py). Plain torch, no GPU and no `cuvite_amd.ops` import.

The graphs are the quality graphs of quality_cases.py and R-MAT
(`rmat_graph(s, 16, seed=1)`); "rmat10u" is R-MAT s10 with unit weights, so
every sum is exact and a device run can be held to the CPU oracle label for
label."""

from __future__ import annotations

import functools

import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm
from cuvite_amd.quality import partition_quality
from cuvite_amd.uncoarsen import run_uncoarsen_phase

from quality_cases import shard, whole_graph

QUALITY_GRAPHS = ("karate", "karate2", "lfr", "rgg")


@functools.lru_cache(maxsize=None)
def graph(name: str) -> Graph:
    if name == "rmat10u":
        g = rmat_graph(10, 16, seed=1)
        return Graph(g.rowptr, g.tails, torch.ones_like(g.weights))
    if name.startswith("rmat"):
        return rmat_graph(int(name[4:]), 16, seed=1)
    return whole_graph(name)


def cfg(**kw) -> LouvainConfig:
    return LouvainConfig(backend="torch", **kw)


def _key(kw: dict):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _run(name: str, key, vcycle: bool):
    return louvain(single_partition(graph(name)), Comm(),
                   cfg(vcycle=vcycle, **dict(key)))


def plain_run(name: str, **kw):
    """One-rank CPU run without the option, computed once per session."""
    return _run(name, _key(kw), False)


def vcycle_run(name: str, **kw):
    """The same run with vcycle=True."""
    return _run(name, _key(kw), True)


def exact_q(name: str, labels: torch.Tensor) -> float:
    return partition_quality(single_partition(graph(name)), labels, Comm(),
                             backend="torch").modularity


def boundary_loop(rowptr, tails, labels):
    """The boundary mask by a python loop over the edges: row v is marked iff
    some edge of it has a tail inside `labels` with another label."""
    rp, t, lab = rowptr.tolist(), tails.tolist(), labels.tolist()
    nv = len(rp) - 1
    out = [0] * nv
    for v in range(nv):
        for e in range(rp[v], rp[v + 1]):
            if 0 <= t[e] < len(lab) and lab[t[e]] != lab[v]:
                out[v] = 1
    return torch.tensor(out, dtype=torch.uint8)


class QRecorder:
    """observe hook of run_uncoarsen_phase: keeps every ("q", ...) event."""

    def __init__(self):
        self.q = []

    def __call__(self, event, **kw):
        if event == "q":
            self.q.append(kw)


@functools.lru_cache(maxsize=None)
def phase_oracle(name: str):
    """One CPU refinement phase on the input graph from the plain run's
    labels: (labels, VcycleLevel, [q events])."""
    rec = QRecorder()
    lab, _, rep = run_uncoarsen_phase(
        single_partition(graph(name)), Comm(), cfg(),
        plain_run(name).communities.clone(), observe=rec)
    return lab, rep, rec.q


def report_tuple(lv):
    """The integer part of a VcycleLevel, and its q's."""
    return ((lv.level, lv.nv_global, lv.boundary, lv.sweeps, lv.evaluated,
             lv.moved, tuple(lv.sizes_per_sweep)),
            (lv.q_before, lv.q_after) + tuple(lv.q_per_sweep))


def same_reports(got, want, tol: float = 1e-12) -> bool:
    """Two V-cycle reports agree: counts exactly, every q within `tol` (the
    sums run in another order on another rank count or device)."""
    if len(got) != len(want):
        return False
    for a, b in zip(got, want):
        (ia, qa), (ib, qb) = report_tuple(a), report_tuple(b)
        if ia != ib or len(qa) != len(qb):
            return False
        if any(abs(x - y) > tol for x, y in zip(qa, qb)):
            return False
    return True


def dist_vcycle(rank, world, comm, dev, backend, name, balanced, **kw):
    """One rank of louvain(vcycle=True) on the sharded graph. Returns CPU
    pieces the parent concatenates."""
    dg = shard(graph(name), rank, world, balanced).to(dev)
    res = louvain(dg, comm, LouvainConfig(backend=backend, vcycle=True, **kw))
    return {"labels": res.communities.cpu(), "vcycle": res.vcycle,
            "modularity": res.modularity}
