"""Are the communities connected? Find the ones that are not and split them.

Louvain can return a community that is not connected: when a bridging vertex
moves out, its old community stays behind in pieces. Splitting such a
community into its connected components never lowers modularity (the weight
inside communities is unchanged and the sum of squared community degrees
shrinks), so it is a free quality gain and the guarantee a user of community
detection expects.

`split_disconnected` computes the connected components of the graph
restricted to edges whose endpoints carry the same label and relabels every
vertex with the smallest global vertex id of its component. That label lies
in [0, nv_global), so `validate_labels`, `coarsen`, `partition_quality` and
warm start take it unchanged, and it depends on neither atomic order, rank
count nor partition.

Per rank the components are found over local vertices plus ghosts (dense
node space of `halo.tails_dense`, locals first) by hook-and-compress rounds
with a monotone min: the HIP kernels of `ops.cc_components` on a GPU,
`cc_components_torch` on the CPU. Components that span ranks are then
stitched by exchanging the component values of the ghosts until no rank
changes anything.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .graph import DistGraph
from .halo import build_halo, exchange_ghost_labels, push_remote_deltas
from .parallel import Comm
from .quality import _EDGE_CHUNK, _use_hip, validate_labels


@dataclass
class ConnectivityReport:
    labels: torch.Tensor      # int64 [nv]: smallest global vertex id of the
    #   vertex's component (this rank's slice)
    num_communities: int      # distinct labels before the split (global)
    num_components: int       # distinct labels after it (global)
    num_disconnected: int     # communities that had more than one component
    rounds: Tuple[int, int]   # (local hook + compress rounds on this rank,
    #   cross-rank exchange rounds)


def cc_components_torch(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                        labels_all: torch.Tensor,
                        chunk: int = _EDGE_CHUNK):
    """Plain-torch twin of ops.cc_components (its oracle, and the CPU path).
    Returns (comp int32 [nv + ng], rounds): comp[x] is the smallest dense id
    in x's component of the graph restricted to edges whose endpoints carry
    the same label. Same rounds as the kernels: scatter_reduce_ amin hooks
    the larger root of every such edge under the smaller one, comp =
    comp[comp] compresses, until a hook pass sees no edge between two roots.
    A tail outside the label array matches nothing."""
    nv = rowptr.numel() - 1
    ne = tails_dense.numel()
    nl = labels_all.numel()
    dev = rowptr.device
    comp = torch.arange(nl, dtype=torch.int64, device=dev)
    if nv == 0 or ne == 0:
        return comp.to(torch.int32), 0
    # the intra edges, once (chunked like intra_weight_torch)
    us, ts = [], []
    for c0 in range(0, ne, chunk):
        c1 = min(c0 + chunk, ne)
        e = torch.arange(c0, c1, device=dev)
        row = torch.searchsorted(rowptr, e, right=True) - 1
        t = tails_dense[c0:c1].to(torch.int64)
        inb = (t >= 0) & (t < nl)
        tc = t.clamp(0, nl - 1)
        same = inb & (tc != row) & (labels_all[tc] == labels_all[row])
        us.append(row[same])
        ts.append(tc[same])
    u, t = torch.cat(us), torch.cat(ts)
    rounds = 0
    while True:
        if rounds > nl:
            raise RuntimeError(f"cc_components_torch: no fixed point after "
                               f"{rounds} rounds")
        rounds += 1
        ru, rt = comp[u], comp[t]
        diff = ru != rt
        if not bool(diff.any()):
            break
        ru, rt = ru[diff], rt[diff]
        comp.scatter_reduce_(0, torch.maximum(ru, rt), torch.minimum(ru, rt),
                             reduce="amin")
        while True:
            nxt = comp[comp]
            if torch.equal(nxt, comp):
                break
            comp = nxt
    return comp.to(torch.int32), rounds


def _count_by_community(dg: DistGraph, comm: Comm, halo,
                        labs: torch.Tensor) -> torch.Tensor:
    """int64 [nv]: how often each community this rank OWNS occurs in `labs`
    (global community ids, any number of them), indexed by (id - base).
    Collective; the quality.community_aggregates pattern without degrees."""
    dev = labs.device
    base, bound, nv = dg.base, dg.bound, dg.nv
    cnt = torch.zeros(nv, dtype=torch.int64, device=dev)
    if comm.world == 1:
        cnt.index_add_(0, labs, torch.ones_like(labs))
        return cnt
    is_local = (labs >= base) & (labs < bound)
    li = labs[is_local] - base
    cnt.index_add_(0, li, torch.ones_like(li))
    rem, rcnt = torch.unique(labs[~is_local], return_counts=True)
    zero = torch.zeros(rem.numel(), dtype=torch.float64, device=dev)
    push_remote_deltas(halo, rem, rcnt, zero, cnt,
                       torch.zeros(nv, dtype=torch.float64, device=dev))
    return cnt


def split_disconnected(dg: DistGraph, labels: torch.Tensor,
                       comm: Optional[Comm] = None, halo=None,
                       backend: str = "auto") -> ConnectivityReport:
    """Split every community of `labels` (int64 [nv], this rank's slice,
    global community ids in [0, nv_global)) into its connected components on
    `dg`. Collective: every rank calls it with its own slice. `halo`: reuse
    a HaloContext already built for `dg`. On a GPU the edge pass is the HIP
    cc_components kernels (a missing extension raises); backend="torch"
    forces the torch twin.

    The new label of a vertex is the smallest global vertex id of its
    component. Splitting the result again changes nothing."""
    comm = comm or Comm(dg.g.device)
    dev = dg.g.device
    validate_labels(dg, comm, labels)
    use_hip = _use_hip(backend, dev)
    labels = labels.to(dev)
    if halo is None:
        halo = build_halo(dg, comm)
    nv, base = dg.nv, dg.base
    ghost = exchange_ghost_labels(halo, labels)
    all_labels = torch.cat([labels, ghost])
    if use_hip:
        from . import ops
        comp, local_rounds = ops.cc_components(dg.g.rowptr, halo.tails_dense,
                                               all_labels)
    else:
        comp, local_rounds = cc_components_torch(dg.g.rowptr,
                                                 halo.tails_dense, all_labels)
    comp = comp.to(torch.int64)
    # a component that holds a local vertex has a local root (locals come
    # first); a ghost that no local vertex reaches is a component of its own
    # here and takes no part below
    val = base + comp[:nv]
    cross_rounds = 0
    big = torch.iinfo(torch.int64).max
    while True:
        cross_rounds += 1
        gval = exchange_ghost_labels(halo, val)
        cmin = torch.full((comp.numel(),), big, dtype=torch.int64, device=dev)
        cmin.scatter_reduce_(0, comp, torch.cat([val, gval]), reduce="amin")
        new = cmin[comp[:nv]]
        changed = float(bool((new != val).any()))
        val = new
        if comm.allreduce_scalar(changed) == 0.0:
            break
    # one vertex per component carries its own id
    gids = torch.arange(base, dg.bound, device=dev)
    rep = val == gids
    ncomp = int(comm.allreduce_scalar(float(rep.sum())))
    ncomm = int(comm.allreduce_scalar(float(
        (_count_by_community(dg, comm, halo, labels) > 0).sum())))
    ndisc = int(comm.allreduce_scalar(float(
        (_count_by_community(dg, comm, halo, labels[rep]) > 1).sum())))
    return ConnectivityReport(labels=val, num_communities=ncomm,
                              num_components=ncomp, num_disconnected=ndisc,
                              rounds=(int(local_rounds), cross_rounds))
