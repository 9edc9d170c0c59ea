"""CPU-only builders shared by the dynamic-frontier tests (test_dynamic.py,
test_gpu_dynamic.py). Plain torch, no GPU and no `cuvite_amd.ops` import.

The batch recipe is the one the frontier prototype was measured with: list
the undirected pairs s < d of the CSR in CSR order, delete a random `frac`
of them, insert as many random pairs (self pairs dropped) with weight 1."""

from __future__ import annotations

import functools

import torch

from cuvite_amd.dynamic import (EdgeBatch, affected_vertices,
                                apply_edge_batch, ghost_reverse_csr,
                                run_frontier_phase)
from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

from quality_cases import cold_run, dup_graph, shard, whole_graph


def undirected_pairs(g: Graph):
    src = torch.repeat_interleave(torch.arange(g.nv), g.degrees())
    m = src < g.tails
    return src[m], g.tails[m]


def recipe_batch(g: Graph, frac: float) -> EdgeBatch:
    gen = torch.Generator().manual_seed(7)
    s, d = undirected_pairs(g)
    # a pair with parallel edges is listed once per copy; deleting it once
    # or several times removes all copies alike
    m = s.numel()
    k = max(1, int(frac * m))
    perm = torch.randperm(m, generator=gen)
    dele = perm[:k]
    ins_u = torch.randint(0, g.nv, (k,), generator=gen)
    ins_v = torch.randint(0, g.nv, (k,), generator=gen)
    keep = ins_u != ins_v
    ins_u, ins_v = ins_u[keep], ins_v[keep]
    return EdgeBatch(ins_u, ins_v,
                     torch.ones(ins_u.numel(), dtype=torch.float64),
                     s[dele], d[dele])


@functools.lru_cache(maxsize=None)
def base_graph(name: str) -> Graph:
    if name == "dup":
        return dup_graph()
    if name == "rmat12":
        # unit weights: every sum is exact, so the device run can be held to
        # the CPU oracle label for label
        g = rmat_graph(12, 16, seed=1)
        return Graph(g.rowptr, g.tails, torch.ones_like(g.weights))
    return whole_graph(name)


@functools.lru_cache(maxsize=None)
def prev_labels(name: str) -> torch.Tensor:
    """The cold CPU run's labels on the old graph."""
    if name in ("karate", "lfr"):
        return cold_run(name).communities
    return louvain(single_partition(base_graph(name)), Comm(),
                   LouvainConfig(backend="torch")).communities


@functools.lru_cache(maxsize=None)
def perturbed(name: str, frac: float):
    """(new graph, batch, prev, frontier0) on one CPU rank."""
    g = base_graph(name)
    batch = recipe_batch(g, frac)
    dg = apply_edge_batch(single_partition(g), Comm(), batch)
    prev = prev_labels(name)
    f0 = affected_vertices(dg, Comm(), prev, batch)
    return dg.g, batch, prev, f0


@functools.lru_cache(maxsize=None)
def oracle_run(name: str, frac: float):
    """CPU frontier phase on the perturbed graph: (estimate, labels, sweeps,
    report)."""
    g, _, prev, f0 = perturbed(name, frac)
    est, lab, it, _, rep = run_frontier_phase(
        single_partition(g), Comm(), LouvainConfig(backend="torch"),
        prev.clone(), f0.clone())
    return est, lab, it, rep


def share_of(batch: EdgeBatch, rank: int, world: int) -> EdgeBatch:
    """Every world-th entry of the batch, starting at `rank`."""
    return EdgeBatch(batch.ins_src[rank::world], batch.ins_dst[rank::world],
                     batch.ins_w[rank::world], batch.del_src[rank::world],
                     batch.del_dst[rank::world])


def dist_update(rank, world, comm, dev, backend, name, frac, balanced, prev):
    """One rank of: shard the old graph, apply this rank's share of the
    batch, mark the affected vertices, run louvain with the frontier (one
    phase). `prev`: the whole old partition, computed by the parent (a cold
    run inside a rank process would be a collective). Returns CPU pieces the
    parent concatenates."""
    g = base_graph(name)
    batch = recipe_batch(g, frac)
    old = shard(g, rank, world, balanced).to(dev)
    dg = apply_edge_batch(old, comm, share_of(batch, rank, world))
    mine = prev[dg.base:dg.bound].clone().to(dev)
    f0 = affected_vertices(dg, comm, mine, share_of(batch, rank, world))
    res = louvain(dg, comm, LouvainConfig(backend=backend, one_phase=True),
                  init_labels=mine, init_frontier=f0)
    rep = res.levels[0]["frontier"]
    # CSR rows as sorted (dst, w) keys: the device builder leaves row order
    # open
    src = torch.repeat_interleave(torch.arange(dg.nv, device=dev),
                                  dg.g.degrees()) + dg.base
    key = (src * g.nv + dg.g.tails).cpu()
    order = torch.argsort(key, stable=True)
    return {"rowptr": dg.g.rowptr.cpu(), "key": key[order],
            "w": dg.g.weights.cpu()[order].to(torch.float64),
            "f0": f0.cpu(), "labels": res.communities.cpu(),
            "sizes": list(rep.sizes_per_sweep),
            "estimates": list(rep.estimates), "sweeps": rep.sweeps}


def csr_key(g: Graph):
    """Sorted (src, dst) keys and their weights, for CSR comparison."""
    src = torch.repeat_interleave(torch.arange(g.nv), g.degrees())
    key = src * g.nv + g.tails
    order = torch.argsort(key, stable=True)
    return key[order], g.weights[order].to(torch.float64)


def expand_case(degs, n_ghost: int, ghost_heads, seed: int = 5):
    """A level graph with the given local row degrees whose tails are drawn
    from [0, nv + n_ghost), plus extra edges head -> ghost for every
    (ghost, [heads]) in `ghost_heads`. Returns (rowptr int64, tails int32,
    g_rowptr, g_heads)."""
    gen = torch.Generator().manual_seed(seed)
    nv = len(degs)
    rows = []
    for v, d in enumerate(degs):
        t = torch.randint(0, nv, (d,), generator=gen)
        extra = [nv + gh for gh, heads in ghost_heads if v in heads]
        rows.append(torch.cat([t, torch.tensor(extra, dtype=torch.int64)]))
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([r.numel() for r in rows]), 0)
    tails = torch.cat(rows).to(torch.int32) if rows else \
        torch.empty(0, dtype=torch.int32)
    g_rowptr, g_heads = ghost_reverse_csr(rowptr, tails, n_ghost)
    return rowptr, tails, g_rowptr, g_heads


def expand_loop(changed, rowptr, tails, g_rowptr, g_heads):
    """frontier_expand by a python loop."""
    nv = rowptr.numel() - 1
    rp, t = rowptr.tolist(), tails.tolist()
    grp, gh = g_rowptr.tolist(), g_heads.tolist()
    act = [False] * nv
    for x in changed.tolist():
        if x < nv:
            act[x] = True
            nb = t[rp[x]:rp[x + 1]]
        else:
            nb = gh[grp[x - nv]:grp[x - nv + 1]]
        for u in nb:
            if u < nv:
                act[u] = True
    return torch.tensor(act, dtype=torch.bool)
