"""CPU-only builders shared by the resolution tests (test_resolution.py,
test_gpu_resolution.py). Plain torch and numpy, no GPU and no
`cuvite_amd.ops` import.

Q_gamma = sum_c [in_c / 2m - gamma (a_c / 2m)^2]. The move functions take
gamma through `MoveInputs.constant` = gamma / (2m): it scales the degree term
of the gain and nothing else.

Exactness of the scaled ladder (`scaled_ladder`): kernel_cases.ladder_inputs
has integer weights and a power-of-two `constant`, and the factors here are
powers of two, so the scaled constant (2^-18 times 2^-2, 2^6 or 2^10) is a
power of two as well. On these inputs vdeg is an integer below 2^15 and
(ay - ax) one below 2^18, so 2 * vdeg * (ay - ax) is an integer below 2^34
and 2 * (eiy - eix) one below 2^17: every intermediate and the gain itself
are integer multiples of 2^-20 below 2^34, which fit 53 bits. The gain is
exact in fp64 in any evaluation order, fused multiply-adds included, and a
correct kernel equals the twin bit for bit."""

from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.local_move import local_move_torch
from cuvite_amd.louvain import LouvainConfig, louvain, resolution_scan
from cuvite_amd.parallel import Comm
from cuvite_amd.quality import partition_quality

from kernel_cases import ladder_inputs
from quality_cases import dup_graph, shard, whole_graph

GAMMAS = (0.25, 0.5, 1.0, 2.0, 4.0)
SCAN_GAMMAS = (4.0, 2.0, 1.0, 0.5, 0.25)
FACTORS = (0.25, 64.0, 1024.0)      # powers of two: the gain stays exact
KARATE_COUNTS = {0.25: 1, 0.5: 2, 1.0: 4, 2.0: 6, 4.0: 13}
MODES = {"plain": {}, "vcycle": dict(vcycle=True),
         "leiden": dict(algorithm="leiden")}


def clique_ring(n_cliques: int, k: int) -> Graph:
    """Ring of `n_cliques` K_k: clique c is vertices k*c .. k*c + k - 1, unit
    weights, plus the edge (k*c + k - 1, k*((c + 1) mod n_cliques))."""
    src, dst = [], []
    for c in range(n_cliques):
        for i in range(k):
            for j in range(k):
                if i != j:
                    src.append(k * c + i)
                    dst.append(k * c + j)
        a, b = k * c + k - 1, k * ((c + 1) % n_cliques)
        src += [a, b]
        dst += [b, a]
    s, d = torch.tensor(src), torch.tensor(dst)
    return Graph.from_edge_tuples(n_cliques * k, s, d,
                                  torch.ones(s.numel(), dtype=torch.float64))


def _unit(g: Graph) -> Graph:
    return Graph(g.rowptr, g.tails, torch.ones_like(g.weights))


@functools.lru_cache(maxsize=None)
def graph(name: str) -> Graph:
    """ring32k4 / ring30k5, the quality graphs, `dup`, and the unit-weight
    graphs a device run is held to the CPU oracle on label for label: rggu
    (the quality RGG with unit weights), rmat10u, rmat12u."""
    if name == "ring32k4":
        return clique_ring(32, 4)
    if name == "ring30k5":
        return clique_ring(30, 5)
    if name == "dup":
        return dup_graph()
    if name == "rggu":
        return _unit(whole_graph("rgg"))
    if name in ("rmat10u", "rmat12u"):
        return _unit(rmat_graph(int(name[4:-1]), 16, seed=1))
    return whole_graph(name)


def brute_q_gamma(g: Graph, labels: torch.Tensor, gamma: float) -> float:
    """Q_gamma from the dense adjacency matrix, in numpy fp64 (the idea of
    quality_cases.brute_modularity with the null-model term scaled)."""
    n = g.nv
    a = np.zeros((n, n))
    src = np.repeat(np.arange(n), g.degrees().numpy())
    np.add.at(a, (src, g.tails.numpy()), g.weights.numpy().astype(np.float64))
    k = a.sum(axis=1)
    two_m = k.sum()
    lab = labels.numpy()
    same = lab[:, None] == lab[None, :]
    return float((a[same].sum()
                  - gamma * (np.outer(k, k)[same]).sum() / two_m) / two_m)


def q_gamma(name: str, labels: torch.Tensor, gamma: float) -> float:
    """partition_quality(resolution=gamma) on one CPU rank."""
    return partition_quality(single_partition(graph(name)), labels, Comm(),
                             backend="torch", resolution=gamma).modularity


def num_communities(labels: torch.Tensor) -> int:
    return int(torch.unique(labels).numel())


@functools.lru_cache(maxsize=None)
def _run(name: str, gamma: float, key):
    return louvain(single_partition(graph(name)), Comm(),
                   LouvainConfig(backend="torch", resolution=gamma,
                                 **dict(key)))


def gamma_run(name: str, gamma: float, **kw):
    """One-rank CPU run at `gamma`, computed once per session."""
    return _run(name, float(gamma), tuple(sorted(kw.items())))


@functools.lru_cache(maxsize=None)
def scan_run(name: str, gammas=SCAN_GAMMAS):
    """One-rank CPU resolution_scan, computed once per session."""
    return resolution_scan(single_partition(graph(name)), list(gammas),
                           Comm(), LouvainConfig(backend="torch"))


def connected_communities(g: Graph, labels: torch.Tensor) -> bool:
    """Every community induces a connected subgraph (union-find over the
    intra-community edges)."""
    parent = list(range(g.nv))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    lab = labels.tolist()
    src = torch.repeat_interleave(torch.arange(g.nv), g.degrees()).tolist()
    for u, v in zip(src, g.tails.tolist()):
        if lab[u] == lab[v]:
            parent[find(u)] = find(v)
    roots = {find(v) for v in range(g.nv)}
    return len(roots) == num_communities(labels)


# ---- the scaled ladder ------------------------------------------------------

LADDER_STATES = ("few", "random", "tied")


@functools.lru_cache(maxsize=None)
def base_ladder(wdtype, state: str, ghosts: bool):
    """kernel_cases.ladder_inputs(..., seed=21) (ghosts come with parallel
    edges and self-loops, as in the frontier tests) and the torch twin's
    answer at its own constant."""
    inp, L = ladder_inputs(wdtype, state, ghosts, ghosts, seed=21)
    return inp, L, local_move_torch(inp)


def scaled(inp, factor: float):
    return dataclasses.replace(inp, constant=inp.constant * factor)


@functools.lru_cache(maxsize=None)
def scaled_ladder(wdtype, state: str, ghosts: bool, factor: float):
    """(MoveInputs with constant * factor, L, (target, cw) of the torch
    twin)."""
    inp, L, _ = base_ladder(wdtype, state, ghosts)
    s = scaled(inp, factor)
    return s, L, local_move_torch(s)


# ---- ranks ------------------------------------------------------------------

def dist_run(rank, world, comm, dev, backend, name, balanced, gamma, kw,
             init=None):
    """One rank of louvain(resolution=gamma, **kw) on the sharded graph;
    `init`: the whole start partition (warm start), or None. Returns CPU
    pieces the parent concatenates."""
    dg = shard(graph(name), rank, world, balanced).to(dev)
    mine = None if init is None else init[dg.base:dg.bound].clone().to(dev)
    res = louvain(dg, comm, LouvainConfig(backend=backend, resolution=gamma,
                                          **kw), init_labels=mine)
    return {"labels": res.communities.cpu(), "iters": res.total_iters,
            "phases": res.phases, "modularity": res.modularity}


def dist_scan(rank, world, comm, dev, backend, name, gammas):
    dg = shard(graph(name), rank, world, False).to(dev)
    out = resolution_scan(dg, list(gammas), comm,
                          LouvainConfig(backend=backend))
    return [{"labels": r.communities.cpu(), "iters": r.total_iters}
            for r in out]
