"""CPU-only builders and the oracle shared by the connectivity tests
(test_connectivity.py, test_gpu_connectivity.py,
test_gpu_connectivity_multirank.py). Plain torch and python: no GPU, no
scipy and no `cuvite_amd.ops` import.

The oracle is a union-find over the edges whose endpoints carry the same
label; it returns, per node, the smallest node id of its component, which is
what `cc_components_torch`, `ops.cc_components` and `split_disconnected`
promise. Everything here is integer valued, so every comparison built on it
is torch.equal."""

from __future__ import annotations

import functools

import torch

from cuvite_amd.graph import Graph

PATH_N = 4096
PATH_ORDERS = ("natural", "reversed", "random", "zigzag")
PATH_BLOCK = 100


def uf_min_labels(rowptr: torch.Tensor, tails: torch.Tensor,
                  labels: torch.Tensor) -> torch.Tensor:
    """int64 [len(labels)]: the smallest node id of every node's component in
    the graph restricted to edges (row, tail) with labels[row] ==
    labels[tail]. Nodes past the rows (ghosts) have no row of their own."""
    rp, t, lab = rowptr.tolist(), tails.tolist(), labels.tolist()
    n = len(lab)
    parent = list(range(n))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    for v in range(len(rp) - 1):
        for e in range(rp[v], rp[v + 1]):
            u = t[e]
            if 0 <= u < n and lab[u] == lab[v]:
                a, b = find(v), find(u)
                if a != b:
                    # the smaller id stays the root
                    if a < b:
                        parent[b] = a
                    else:
                        parent[a] = b
    return torch.tensor([find(x) for x in range(n)], dtype=torch.int64)


def num_components(min_labels: torch.Tensor) -> int:
    return int(torch.unique(min_labels).numel())


def all_connected(g: Graph, labels: torch.Tensor) -> bool:
    """Whether every community of `labels` is connected on `g`."""
    comp = uf_min_labels(g.rowptr, g.tails, labels)
    return num_components(comp) == int(torch.unique(labels).numel())


# ---- paths ------------------------------------------------------------------

def path_order(order: str, n: int = PATH_N) -> torch.Tensor:
    """perm[i] = id of the vertex at position i along the path."""
    assert order in PATH_ORDERS
    if order == "natural":
        return torch.arange(n)
    if order == "reversed":
        return torch.arange(n - 1, -1, -1)
    if order == "random":
        return torch.randperm(n, generator=torch.Generator().manual_seed(7))
    lo = torch.arange((n + 1) // 2)
    hi = n - 1 - torch.arange(n // 2)
    out = torch.empty(n, dtype=torch.int64)
    out[0::2] = lo
    out[1::2] = hi
    return out


@functools.lru_cache(maxsize=None)
def path_case(order: str, labelling: str, n: int = PATH_N):
    """(rowptr int64, tails int32, labels int64 [n], expected comp int64 [n])
    of an n-vertex path whose vertices are numbered by `order`. labelling
    "one": a single label, one component; "blocks": labels alternate in
    blocks of PATH_BLOCK along the path, ceil(n / PATH_BLOCK) components."""
    perm = path_order(order, n)
    g = Graph.from_edge_tuples(
        n, torch.cat([perm[:-1], perm[1:]]), torch.cat([perm[1:], perm[:-1]]),
        torch.ones(2 * (n - 1), dtype=torch.float64))
    labels = torch.zeros(n, dtype=torch.int64)
    if labelling == "blocks":
        labels[perm] = (torch.arange(n) // PATH_BLOCK) % 2
    else:
        assert labelling == "one"
    tails = g.tails.to(torch.int32)
    return g.rowptr, tails, labels, uf_min_labels(g.rowptr, tails, labels)


# ---- hand-built graphs ----------------------------------------------------------

def hand_cases():
    """name -> (rowptr, tails int32, labels int64 [nv + ng], expected comp as
    a list). Dense node space: locals first, then ghosts."""
    i64 = dict(dtype=torch.int64)
    i32 = dict(dtype=torch.int32)
    return {
        # path a-b-c labelled 0,1,0: three components
        "aba": (torch.tensor([0, 1, 3, 4], **i64),
                torch.tensor([1, 0, 2, 1], **i32),
                torch.tensor([0, 1, 0], **i64), [0, 1, 2]),
        # two locals joined only through a same-label ghost
        "via_ghost": (torch.tensor([0, 1, 2], **i64),
                      torch.tensor([2, 2], **i32),
                      torch.tensor([5, 5, 5], **i64), [0, 0, 0]),
        # the ghost relabelled: nothing joins them
        "ghost_relabelled": (torch.tensor([0, 1, 2], **i64),
                             torch.tensor([2, 2], **i32),
                             torch.tensor([5, 5, 7], **i64), [0, 1, 2]),
        # isolated vertices around one edge, one label
        "isolated": (torch.tensor([0, 0, 1, 1, 2, 2], **i64),
                     torch.tensor([3, 1], **i32),
                     torch.tensor([4, 4, 4, 4, 4], **i64), [0, 1, 2, 1, 4]),
    }


def star_case(n_leaves: int):
    """A hub (vertex 0) with n_leaves leaves, leaves in two labels, the hub
    in the first: the first-label leaves join the hub, the others stay
    alone. Stored in both directions."""
    leaves = torch.arange(1, n_leaves + 1)
    hub = torch.zeros(n_leaves, dtype=torch.int64)
    g = Graph.from_edge_tuples(
        n_leaves + 1, torch.cat([hub, leaves]), torch.cat([leaves, hub]),
        torch.ones(2 * n_leaves, dtype=torch.float64))
    labels = torch.cat([torch.zeros(1, dtype=torch.int64), leaves % 2])
    tails = g.tails.to(torch.int32)
    return g.rowptr, tails, labels, uf_min_labels(g.rowptr, tails, labels)
