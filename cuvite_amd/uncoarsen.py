"""The way back up: refine the partition level by level (V-cycle).

A run coarsens until a phase stops gaining and would return the composition
of the level partitions as it stands. With `LouvainConfig(vcycle=True)` the
hierarchy is kept (`Hierarchy`), and `refine_up` walks it from the coarsest
accepted level K down to the input graph:

  - level K starts from its own phase's labels, level k < K from the refined
    labels of level k + 1 gathered through map_k (the next-level vertex of
    every level-k vertex);
  - every level runs one refinement phase, `run_uncoarsen_phase`: the sweeps
    of the dynamic-frontier phase (dynamic.FrontierSweeps) from a first
    frontier built on the device, the boundary vertices: a vertex whose
    neighbours all carry its own label has no candidate and cannot move;
  - the phase stops on the EXACT modularity. The move of sweep j returns cw
    under the labels the sweep started from for every vertex (dynamic.py's
    invariant), and the aggregates it read belong to the same labels, so
    q_j = sum(cw) c - gamma sum(deg^2) c^2 (c = 1/2m, gamma =
    cfg.resolution) costs one reduction and one allreduce.
    The labels with the largest known q are returned; the targets of the last
    sweep have no known Q and are dropped.

q_after >= q_before at every level by construction, and coarsening preserves
modularity, so the run never returns a lower exact Q than it would have
without the option.
"""

from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from .coarsen import number_survivors, remap_labels
from .dynamic import FrontierSweeps
from .graph import DistGraph
from .parallel import Comm
from .quality import _EDGE_CHUNK


def intra_boundary_torch(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                         weights: torch.Tensor, labels: torch.Tensor,
                         chunk: int = _EDGE_CHUNK):
    """Twin of ops.intra_boundary: (cw fp64 [nv], mask uint8 [nv]). cw is
    quality.intra_weight_torch's sum, edge for edge in the same order;
    mask[v] = 1 iff row v holds an edge whose tail lies inside `labels`
    (locals first, then ghosts) and carries another label than v. A tail
    outside the label array matches nothing and marks nothing."""
    nv = rowptr.numel() - 1
    ne = tails_dense.numel()
    nl = labels.numel()
    dev = rowptr.device
    out = torch.zeros(nv, dtype=torch.float64, device=dev)
    mask = torch.zeros(nv, dtype=torch.uint8, device=dev)
    for c0 in range(0, ne, chunk):
        c1 = min(c0 + chunk, ne)
        e = torch.arange(c0, c1, device=dev)
        row = torch.searchsorted(rowptr, e, right=True) - 1
        t = tails_dense[c0:c1].to(torch.int64)
        inb = (t >= 0) & (t < nl)
        same = inb.clone()
        same[inb] = labels[t[inb]] == labels[row[inb]]
        out.index_add_(0, row[same], weights[c0:c1][same].to(torch.float64))
        mask[row[inb & ~same]] = 1
    return out, mask


@dataclass
class VcycleLevel:
    """What the refinement phase of one level did (global counts)."""

    level: int
    nv_global: int
    boundary: int       # size of the first frontier
    sweeps: int
    evaluated: int      # sum of the frontier sizes
    moved: int          # vertices whose final label differs from the
    #                     projected one
    q_before: float     # exact Q of the projected labels on the level graph
    q_after: float      # exact Q of the returned labels
    sizes_per_sweep: List[int] = field(default_factory=list)
    q_per_sweep: List[float] = field(default_factory=list)  # q_1 .. q_j: the
    #   exact Q of the labels sweep j started from
    setup_s: float = 0.0    # host clock: state, the cw + boundary edge pass
    #   and q_1 (ends in the host read of the boundary size)
    sweeps_s: float = 0.0   # host clock over the sweeps (each ends in the
    #   host read of its moved count)


def run_uncoarsen_phase(dg: DistGraph, comm: Comm, cfg, start: torch.Tensor,
                        halo=None, *, level: int = 0, full: bool = False,
                        observe: Optional[Callable] = None, timers=None):
    """One refinement phase on a level graph from the labels `start` (int64
    [nv], this rank's slice, global ids). Collective. Returns (labels int64
    [nv], halo, VcycleLevel).

    Sweep 1 evaluates the boundary vertices of `start`, every later sweep the
    moved vertices and their neighbours. q_1 is the exact Q of `start`; in
    sweep j >= 2 q_j, the exact Q of the labels that sweep started from, is
    known after its move and before its aggregate update. The phase stops
    when q_j - max(q_1 .. q_{j-1}) < cfg.threshold, when a sweep moved
    nothing on any rank, when the frontier is empty (then before the first
    sweep), or after cfg.max_iters_per_phase sweeps, and returns the labels
    with the largest known q.

    `full=True` (test hook): the first frontier is all vertices and is never
    replaced, i.e. every sweep is a full sweep. `observe` / `timers` as in
    run_frontier_phase; `observe` also gets ("q", sweep=j, q=q_j,
    labels=...)."""
    from .louvain import _modularity

    t0 = time.perf_counter()
    frontier0 = None
    if full:
        frontier0 = torch.ones(dg.nv, dtype=torch.bool, device=dg.g.device)
    sw = FrontierSweeps(dg, comm, cfg, start, frontier0, halo,
                        boundary=not full, expand=not full, observe=observe,
                        timers=timers)
    state = sw.state
    first = state.curr_comm          # validated copy of `start`

    def count(x) -> int:
        n = int(x)
        return int(comm.allreduce_scalar(float(n))) if comm.world > 1 else n

    def exact_q(sweep: int) -> float:
        with sw.span("modularity"):
            q = _modularity(state)
        if observe is not None:
            observe("q", sweep=sweep, q=q, labels=state.curr_comm.clone())
        return q

    boundary = count(sw.active.sum())
    qs = [exact_q(1)]
    best_q, best = qs[0], first
    sizes: List[int] = []
    sweeps = 0
    t1 = time.perf_counter()
    while boundary > 0 and sweeps < cfg.max_iters_per_phase:
        sweeps += 1
        target, n_act = sw.move(sweeps)
        sizes.append(n_act)
        if sweeps >= 2:
            q = exact_q(sweeps)
            gain = q - best_q
            qs.append(q)
            if q > best_q:
                best_q, best = q, state.curr_comm
            if cfg.verbose and comm.rank == 0:
                print(f"  uncoarsen sweep {sweeps}: |A|={n_act} Q={q:.6f}")
            if gain < cfg.threshold:
                break
        if count((target != state.curr_comm).sum()) == 0:
            break
        sw.apply(target)
        sw.adopt(target)

    report = VcycleLevel(
        level=level, nv_global=dg.nv_global, boundary=boundary,
        sweeps=sweeps, evaluated=sum(sizes),
        moved=count((best != first).sum()), q_before=qs[0], q_after=best_q,
        sizes_per_sweep=sizes, q_per_sweep=qs, setup_s=t1 - t0,
        sweeps_s=time.perf_counter() - t1)
    return best, state.halo, report


@dataclass
class Hierarchy:
    """The levels a V-cycle run keeps on the way down, finest first: for
    every accepted phase its level graph, its HaloContext and map_k, the
    next-level vertex (global id) of every vertex of the level; the last
    entry's map is None. `labels` are the last accepted phase's."""

    graphs: list = field(default_factory=list)
    halos: list = field(default_factory=list)
    maps: list = field(default_factory=list)
    labels: Optional[torch.Tensor] = None

    def push(self, dg: DistGraph, halo, labels: torch.Tensor) -> None:
        self.graphs.append(dg)
        self.halos.append(halo)
        self.maps.append(None)
        self.labels = labels

    def __len__(self) -> int:
        return len(self.graphs)


def dense_renumber(dg: DistGraph, comm: Comm,
                   labels: torch.Tensor) -> torch.Tensor:
    """`labels` with the ids that occur renumbered to [0, k), ascending in the
    old id (collective)."""
    renum, _, _ = number_survivors(dg, comm, labels)
    return renum(labels)


def refine_up(hier: Hierarchy, comm: Comm, cfg, *, full: bool = False):
    """Walk the hierarchy from its coarsest level to level 0 (module
    docstring). Collective; consumes `hier`: a level's graph, halo and map
    are dropped as soon as the labels of the level below are projected.
    Returns (level-0 labels renumbered densely, [VcycleLevel] coarsest
    first)."""
    reports: List[VcycleLevel] = []
    labels = hier.labels
    hier.labels = None
    dg0 = hier.graphs[0]
    dev = dg0.g.device
    for k in range(len(hier) - 1, -1, -1):
        dg, halo = hier.graphs[k], hier.halos[k]
        if dev.type == "cuda":
            from . import ops
            ops.clear_phase_caches()  # keyed by the level graph
        labels, _, rep = run_uncoarsen_phase(dg, comm, cfg, labels, halo,
                                             level=k, full=full)
        reports.append(rep)
        if k > 0:
            # project: level k-1 vertex v sits in level-k vertex map[v]
            labels = remap_labels(dg, comm, hier.maps[k - 1], labels)
            hier.maps[k - 1] = None
        hier.graphs[k] = hier.halos[k] = None
        del dg, halo
    if dev.type == "cuda":
        from . import ops
        ops.clear_phase_caches()
    return dense_renumber(dg0, comm, labels), reports
