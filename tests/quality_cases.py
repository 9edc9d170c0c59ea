"""CPU-only builders shared by the partition-scoring and warm-start tests
(test_quality.py, test_warm_start.py, test_gpu_quality.py). Plain torch and
numpy, no GPU and no `cuvite_amd.ops` import.

Exactness follows kernel_cases.py: weights are small integers wherever a
test says "equal", so every sum is exact in fp32 and fp64 in any order."""

from __future__ import annotations

import functools

import numpy as np
import torch

from cuvite_amd.generators import (karate_graph, lfr_dist_graph,
                                   rgg_dist_graph)
from cuvite_amd.graph import DistGraph, Graph, Partition, single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm


def whole_graph(name: str) -> Graph:
    """The three graphs the issue pins, as single CSRs."""
    if name == "karate":
        return karate_graph()
    if name == "lfr":
        return lfr_dist_graph(2000, 0, 1, mu=0.3, seed=1)[0].g
    if name == "rgg":
        return rgg_dist_graph(4096, 0, 1, seed=1, random_edge_percent=5.0).g
    if name == "karate2":
        # two disjoint karate clubs: split in the middle, neither rank of a
        # 2-rank run has a ghost
        g = karate_graph()
        return Graph(torch.cat([g.rowptr, g.rowptr[1:] + g.ne]),
                     torch.cat([g.tails, g.tails + g.nv]),
                     torch.cat([g.weights, g.weights]))
    raise ValueError(name)


def lfr_truth() -> torch.Tensor:
    """Planted LFR communities, compacted to [0, k)."""
    truth = lfr_dist_graph(2000, 0, 1, mu=0.3, seed=1)[1]
    _, inv = np.unique(truth.numpy(), return_inverse=True)
    return torch.from_numpy(inv.astype(np.int64).reshape(-1))


def shard(g: Graph, rank: int, world: int, balanced: bool = False) -> DistGraph:
    part = Partition.edge_balanced(g.rowptr, world) if balanced \
        else Partition.contiguous(g.nv, world)
    b, e = part.base(rank), part.bound(rank)
    e0, e1 = int(g.rowptr[b]), int(g.rowptr[e])
    return DistGraph(Graph((g.rowptr[b:e + 1] - g.rowptr[b]).clone(),
                           g.tails[e0:e1].clone(),
                           g.weights[e0:e1].clone()), part, rank)


@functools.lru_cache(maxsize=None)
def cold_run(name: str):
    """Single-rank CPU Louvain from singletons, computed once per session."""
    return louvain(single_partition(whole_graph(name)), Comm(),
                   LouvainConfig(backend="torch"))


def brute_modularity(g: Graph, labels: torch.Tensor) -> float:
    """Q from the dense adjacency matrix, in numpy fp64."""
    n = g.nv
    a = np.zeros((n, n))
    src = np.repeat(np.arange(n), g.degrees().numpy())
    np.add.at(a, (src, g.tails.numpy()), g.weights.numpy().astype(np.float64))
    k = a.sum(axis=1)
    two_m = k.sum()
    lab = labels.numpy()
    same = lab[:, None] == lab[None, :]
    return float((a[same].sum() - (np.outer(k, k)[same]).sum() / two_m)
                 / two_m)


def dup_graph(seed: int = 3, nv: int = 40) -> Graph:
    """Small weighted graph with self-loops and parallel edges (the `dup`
    idea of kernel_cases.ladder_inputs): integer weights 1..4, every
    undirected edge stored in both rows, a self-loop stored once in its
    row."""
    g = torch.Generator().manual_seed(seed)
    m = 4 * nv
    u = torch.randint(0, nv, (m,), generator=g)
    v = torch.randint(0, nv, (m,), generator=g)
    keep = u != v
    u, v = u[keep], v[keep]
    # parallel edges: repeat the first quarter of the pairs
    q = u.numel() // 4
    u, v = torch.cat([u, u[:q]]), torch.cat([v, v[:q]])
    w = torch.randint(1, 5, (u.numel(),), generator=g).to(torch.float64)
    loops = torch.arange(0, nv, 3)
    wl = torch.randint(1, 5, (loops.numel(),), generator=g).to(torch.float64)
    src = torch.cat([u, v, loops, loops[:4]])
    dst = torch.cat([v, u, loops, loops[:4]])
    ww = torch.cat([w, w, wl, wl[:4]])
    return Graph.from_edge_tuples(nv, src, dst, ww)


def edge_list_intra(g: Graph, labels: torch.Tensor):
    """Per-vertex intra-community weight by a python loop over the edges."""
    out = [0.0] * g.nv
    rp, t, w = g.rowptr.tolist(), g.tails.tolist(), g.weights.tolist()
    lab = labels.tolist()
    for v in range(g.nv):
        for e in range(rp[v], rp[v + 1]):
            if lab[t[e]] == lab[v]:
                out[v] += w[e]
    return torch.tensor(out, dtype=torch.float64)


def csr_from_degrees(degs, n_ghost: int, seed: int):
    """(rowptr int64, tails int32 in [0, nv + n_ghost), integer weights fp64,
    labels int64 [nv + n_ghost] drawn from 3 communities) with exactly the
    given row degrees."""
    g = torch.Generator().manual_seed(seed)
    nv = len(degs)
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    if nv:
        rowptr[1:] = torch.cumsum(torch.tensor(degs, dtype=torch.int64), 0)
    ne = int(rowptr[-1])
    nl = nv + n_ghost
    tails = torch.randint(0, max(nl, 1), (ne,), generator=g).to(torch.int32)
    w = torch.randint(1, 5, (ne,), generator=g).to(torch.float64)
    labels = torch.randint(0, 3, (nl,), generator=g)
    return rowptr, tails, w, labels
