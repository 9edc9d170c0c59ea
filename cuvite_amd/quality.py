"""Exact scoring of an arbitrary partition, and the helpers warm start shares.

`LouvainResult.modularity` is the reference's convergence estimate: each
sweep mixes the intra-community weight under the labels BEFORE the sweep with
the community degrees AFTER it, and the phase returns the labels of the sweep
before that. `partition_quality` computes the modularity of a given labelling
itself:

    Q = sum_v iw[v] / 2m  -  sum_c (deg[c] / 2m)^2

where iw[v] is the weight of v's edges into v's own community (self-loops and
parallel edges count, exactly the `cw` of local_move) and deg[c] the summed
weighted degree of community c's members.

Labels are global community ids in [0, nv_global); community c's aggregates
live on the rank whose vertex range contains c (the PhaseState slot
convention), whether or not that rank holds any member of c.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from .graph import DistGraph
from .halo import build_halo, exchange_ghost_labels, push_remote_deltas
from .local_move import modularity_parts
from .ops import scatter_add_
from .parallel import Comm

_EDGE_CHUNK = 1 << 24  # edges per step of the torch oracle


@dataclass
class PartitionQuality:
    modularity: float     # Q_gamma at `resolution`
    num_communities: int
    intra_weight: float   # sum of edge weight inside communities (directed)
    total_weight: float   # 2m: sum of all weighted degrees
    coverage: float       # intra_weight / total_weight
    resolution: float = 1.0  # gamma `modularity` was computed under
    degree_sq: float = 0.0   # sum over communities of deg[c]^2

    def at(self, gamma: float) -> float:
        """Q under another resolution from the stored sums: one edge pass
        scores a partition at any number of resolutions. at(self.resolution)
        is `modularity`, bit for bit."""
        # same guard as PhaseState.inv_2m: an edgeless graph scores Q = 0
        c = 1.0 / self.total_weight if self.total_weight > 0.0 else 0.0
        return self.intra_weight * c - gamma * self.degree_sq * c * c


def intra_weight_torch(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                       weights: torch.Tensor, labels: torch.Tensor,
                       chunk: int = _EDGE_CHUNK) -> torch.Tensor:
    """out[v] = sum of w[e] over row v's edges with labels[tails_dense[e]] ==
    labels[v], accumulated and returned in fp64 (plain torch; the oracle of
    ops.intra_weight and the CPU path). `labels` covers local vertices first,
    then ghosts. Chunked over the edge list so the temporaries stay bounded."""
    nv = rowptr.numel() - 1
    ne = tails_dense.numel()
    dev = rowptr.device
    out = torch.zeros(nv, dtype=torch.float64, device=dev)
    for c0 in range(0, ne, chunk):
        c1 = min(c0 + chunk, ne)
        e = torch.arange(c0, c1, device=dev)
        # largest row with rowptr[row] <= e (skips edgeless rows)
        row = torch.searchsorted(rowptr, e, right=True) - 1
        same = labels[tails_dense[c0:c1].to(torch.int64)] == labels[row]
        out.index_add_(0, row[same], weights[c0:c1][same].to(torch.float64))
    return out


def validate_labels(dg: DistGraph, comm: Comm, labels) -> None:
    """Raise ValueError on EVERY rank if any rank's label slice is not int64
    [nv] with values in [0, nv_global). The verdict is allreduced so a rank
    with a good slice does not walk into a collective its peer never joins."""
    why = ""
    if not torch.is_tensor(labels) or labels.dtype != torch.int64 \
            or labels.dim() != 1:
        why = "labels must be a 1-D int64 tensor"
    elif labels.numel() != dg.nv:
        why = f"expected {dg.nv} labels for this rank, got {labels.numel()}"
    elif labels.numel() and (int(labels.min()) < 0
                             or int(labels.max()) >= dg.nv_global):
        why = (f"label values must lie in [0, {dg.nv_global}); got "
               f"[{int(labels.min())}, {int(labels.max())}]")
    bad = comm.allreduce_scalar(1.0 if why else 0.0)
    if bad > 0.0:
        raise ValueError(
            f"invalid community labels on rank {comm.rank}: {why}" if why else
            f"invalid community labels on {int(bad)} other rank(s)")


def community_aggregates(dg: DistGraph, comm: Comm, halo,
                         labels: torch.Tensor, v_degree: torch.Tensor):
    """(size int64 [nv], degree W [nv]) of the communities this rank OWNS
    under arbitrary global `labels`, indexed by (community id - base). No
    densify and no universe: members on this rank add locally, members
    elsewhere arrive through one push_remote_deltas round (collective)."""
    dev = labels.device
    base, bound, nv = dg.base, dg.bound, dg.nv
    size = torch.zeros(nv, dtype=torch.int64, device=dev)
    degree = torch.zeros(nv, dtype=v_degree.dtype, device=dev)
    if comm.world == 1:
        if labels.is_cuda:
            from . import ops
            # recount_ zeroes its outputs before accumulating
            ops._require().recount_(labels, v_degree, base, size, degree)
        else:
            size.index_add_(0, labels, torch.ones_like(labels))
            degree.index_add_(0, labels, v_degree)
        return size, degree
    is_local = (labels >= base) & (labels < bound)
    li = labels[is_local] - base
    size.index_add_(0, li, torch.ones_like(li))
    scatter_add_(degree, li, v_degree[is_local])
    # one entry per distinct remote community, not per member
    rem, inv = torch.unique(labels[~is_local], return_inverse=True)
    rsize = torch.zeros(rem.numel(), dtype=torch.int64, device=dev)
    rsize.index_add_(0, inv, torch.ones_like(inv))
    rdeg = torch.zeros(rem.numel(), dtype=v_degree.dtype, device=dev)
    scatter_add_(rdeg, inv, v_degree[~is_local])
    push_remote_deltas(halo, rem, rsize, rdeg, size, degree)
    return size, degree


def _use_hip(backend: str, dev: torch.device) -> bool:
    if backend == "torch":
        return False
    if backend == "hip" and dev.type != "cuda":
        raise RuntimeError("backend='hip' requires a CUDA/HIP device")
    if backend not in ("auto", "hip"):
        raise ValueError(f"unknown backend {backend!r}")
    return dev.type == "cuda"


def partition_quality(dg: DistGraph, labels: torch.Tensor,
                      comm: Optional[Comm] = None, halo=None,
                      backend: str = "auto",
                      resolution: float = 1.0) -> PartitionQuality:
    """Exact modularity of `labels` (int64 [nv], this rank's slice, global
    community ids in [0, nv_global)) on `dg`, at `resolution` gamma:
    Q_gamma = sum_v iw[v] / 2m - gamma sum_c (deg[c] / 2m)^2
    (PartitionQuality.at rescores under another gamma without a second
    pass). Collective: every rank calls it
    with its own slice and gets the same result. `halo`: reuse a HaloContext
    already built for `dg`. On a GPU the per-vertex pass is the HIP
    intra_weight kernel (a missing extension raises); backend="torch" forces
    the fp64 torch oracle."""
    comm = comm or Comm(dg.g.device)
    dev = dg.g.device
    validate_labels(dg, comm, labels)
    use_hip = _use_hip(backend, dev)
    labels = labels.to(dev)
    if halo is None:
        halo = build_halo(dg, comm)
    ghost = exchange_ghost_labels(halo, labels)
    all_labels = torch.cat([labels, ghost])
    v_degree = dg.local_degree_sum()
    if use_hip:
        from . import ops
        iw = ops.intra_weight(dg.g.rowptr, halo.tails_dense, dg.g.weights,
                              all_labels)
    else:
        iw = intra_weight_torch(dg.g.rowptr, halo.tails_dense, dg.g.weights,
                                all_labels)
    size, degree = community_aggregates(dg, comm, halo, labels, v_degree)
    if use_hip:
        parts = ops.modularity_parts(iw, degree)
    else:
        parts = modularity_parts(iw, degree)
    comm.allreduce_sum_(parts)
    tw = comm.allreduce_scalar(float(v_degree.to(torch.float64).sum()))
    ncomm = int(comm.allreduce_scalar(float((size > 0).sum())))
    # same guard as PhaseState.inv_2m: an edgeless graph scores Q = 0
    c = 1.0 / tw if tw > 0.0 else 0.0
    intra = float(parts[0])
    gamma = float(resolution)
    return PartitionQuality(
        modularity=intra * c - gamma * float(parts[1]) * c * c,
        num_communities=ncomm, intra_weight=intra, total_weight=tw,
        coverage=intra * c, resolution=gamma, degree_sq=float(parts[1]))
