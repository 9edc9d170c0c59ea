"""Updating a partition after a batch of edge changes: the dynamic-frontier
phase.

Warm start (`louvain(..., init_labels=prev)`) continues from a saved
partition but every sweep it keeps still evaluates every vertex. Here a sweep
evaluates a marked subset only:

  - `affected_vertices` marks the endpoints of the changed edges that can
    matter: both endpoints of a deleted edge inside a community of `prev`,
    both endpoints of an inserted edge between two communities;
  - every sweep of `run_frontier_phase` evaluates the marked vertices only;
  - the next frontier is moved ∪ N(moved): every vertex whose label changed in
    the sweep, every ghost whose exchanged label differs from the previous
    sweep's, and their neighbours in the level graph's dense space.

The sweeps stay synchronous, so the phase is stated exactly and held to the
torch twins below like everything else: the same gain, tie-break, singleton
guard, self-loop and parallel-edge handling as `local_move`, the stop test,
rotation and returned labels of `run_phase`. The invariant that makes the
convergence estimate the one a full sweep would give: before every sweep
cw[v] is the intra-community weight of v under the current labels for every
v, because a vertex whose own or whose neighbours' label changed is in the
frontier and gets its cw from the move.

The frontier phase replaces phase 0 only (`louvain(..., init_frontier=mask)`);
later phases are ordinary phases on the coarsened graph.

Edge batches (`EdgeBatch`, `apply_edge_batch`) hold global ids, each
undirected edge once. In a multi-rank run every rank passes its own share of
the batch; the batch is the union of the shares, and a rank's share may name
any vertices. A batch is routed to the owners of its sources and then applied
to every rank's CSR on its own: on the GPU by ops.apply_batch, whose result,
row order included, is the one of its twin apply_routed_batch_torch; on the
CPU by a rebuild of the CSR. `update_stream` follows a sequence of batches,
carrying graph and partition from one to the next.
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import torch

from .graph import DistGraph, Graph
from .halo import exchange_ghost_labels
from .local_move import MoveInputs, local_move_torch
from .parallel import Comm
from .quality import _use_hip, intra_weight_torch, validate_labels


# ---------------------------------------------------------------------------
# torch twins of the HIP frontier ops (CPU path and oracle)
# ---------------------------------------------------------------------------

def ghost_reverse_csr(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                      ng: int):
    """Ghost -> local reverse adjacency of a level graph: (g_rowptr int64
    [ng + 1], g_heads int32) where g_heads[g_rowptr[g]:g_rowptr[g + 1]] are
    the local rows that hold an edge to ghost g (dense id nv + g), one entry
    per stored edge. Built once per phase with torch ops from the edges whose
    tail is a ghost."""
    nv = rowptr.numel() - 1
    dev = rowptr.device
    g_rowptr = torch.zeros(ng + 1, dtype=torch.int64, device=dev)
    if ng == 0:
        return g_rowptr, torch.empty(0, dtype=torch.int32, device=dev)
    e = (tails_dense >= nv).nonzero(as_tuple=True)[0]
    g = tails_dense[e].to(torch.int64) - nv
    row = torch.searchsorted(rowptr, e, right=True) - 1
    order = torch.argsort(g, stable=True)
    g_rowptr[1:] = torch.cumsum(torch.bincount(g, minlength=ng), dim=0)
    return g_rowptr, row[order].to(torch.int32)


def _rows_neighbours(ids: torch.Tensor, rp: torch.Tensor,
                     adj: torch.Tensor) -> torch.Tensor:
    """Concatenated adjacency of the rows `ids` of the CSR (rp, adj)."""
    dev = rp.device
    deg = rp[ids + 1] - rp[ids]
    tot = int(deg.sum())
    if tot == 0:
        return torch.empty(0, dtype=torch.int64, device=dev)
    offs = torch.cumsum(deg, dim=0) - deg
    seg = torch.repeat_interleave(torch.arange(ids.numel(), device=dev), deg)
    eidx = rp[ids][seg] + (torch.arange(tot, device=dev) - offs[seg])
    return adj[eidx].to(torch.int64)


def frontier_expand_torch(changed: torch.Tensor, rowptr: torch.Tensor,
                          tails_dense: torch.Tensor, g_rowptr: torch.Tensor,
                          g_heads: torch.Tensor,
                          active: torch.Tensor) -> torch.Tensor:
    """Twin of ops.frontier_expand: marks (in place, returns `active`) every
    changed local id and every local neighbour of a changed dense id.
    `changed` holds dense ids in [0, nv + ng); neighbours >= nv (ghost tails
    in a local row) are skipped."""
    nv = rowptr.numel() - 1
    ch = changed.to(torch.int64)
    loc = ch[ch < nv]
    gh = ch[ch >= nv] - nv
    active[loc] = 1
    for ids, rp, adj in ((loc, rowptr, tails_dense), (gh, g_rowptr, g_heads)):
        if ids.numel() == 0:
            continue
        u = _rows_neighbours(ids, rp, adj)
        active[u[u < nv]] = 1
    return active


def frontier_move_torch(inp: MoveInputs, active: torch.Tensor,
                        cw_prev: torch.Tensor):
    """Twin of ops.frontier_move: the plain local move for the vertices
    marked in `active`, label and `cw_prev` entry kept for everyone else.
    Evaluates local_move_torch over all vertices and masks."""
    t, cw = local_move_torch(inp)
    act = active.to(torch.bool)
    nv = inp.nv
    return (torch.where(act, t, inp.curr_comm[:nv]),
            torch.where(act, cw, cw_prev.to(cw.dtype)))


# ---------------------------------------------------------------------------
# the frontier phase
# ---------------------------------------------------------------------------

@dataclass
class FrontierReport:
    sizes_per_sweep: List[int]   # global frontier size of every sweep run
    evaluated: int               # their sum: vertices evaluated in the phase
    sweeps: int
    estimates: List[float] = field(default_factory=list)  # the convergence
    #   estimate after every sweep


def _check_frontier(dg: DistGraph, comm: Comm, mask) -> None:
    """ValueError on every rank if any rank's mask is not bool [nv]."""
    bad = not (torch.is_tensor(mask) and mask.dtype == torch.bool
               and mask.dim() == 1 and mask.numel() == dg.nv)
    if comm.allreduce_scalar(1.0 if bad else 0.0) > 0.0:
        raise ValueError("init_frontier must be a bool mask with one entry "
                         "per local vertex on every rank")


class FrontierSweeps:
    """The sweep both frontier phases run, in steps the caller orders:
    run_frontier_phase below (stop test on the convergence estimate, after
    the aggregate update) and uncoarsen.run_uncoarsen_phase (stop test on the
    exact Q, before it).

    Construction sets up PhaseState(init_labels=prev) and one edge pass under
    `prev`: cw for ALL vertices and the ghost -> local adjacency. The first
    frontier is the mask `frontier0` (bool [nv]) or, with `boundary=True`,
    the boundary of `prev`: every vertex with a neighbour of another label,
    from the same edge pass (ops.intra_boundary)."""

    def __init__(self, dg: DistGraph, comm: Comm, cfg, prev: torch.Tensor,
                 frontier0: Optional[torch.Tensor] = None, halo=None, *,
                 boundary: bool = False, expand: bool = True,
                 observe: Optional[Callable] = None, timers=None):
        from .louvain import PhaseState
        dev = dg.g.device
        self.dg, self.comm, self.cfg = dg, comm, cfg
        self.use_hip = _use_hip(cfg.backend, dev)
        self.state = state = PhaseState(dg, comm, halo=halo, init_labels=prev,
                                        resolution=cfg.resolution)
        state.use_hip = self.use_hip
        if not boundary:
            _check_frontier(dg, comm, frontier0)
        self.expand, self.observe, self.timers = expand, observe, timers
        if self.use_hip:
            from . import ops
            self.ops = ops
        hl = state.halo
        rowptr, tails, weights = dg.g.rowptr, hl.tails_dense, dg.g.weights

        self.ghost = exchange_ghost_labels(hl, state.curr_comm)
        all_labels = torch.cat([state.curr_comm, self.ghost])
        if not boundary:
            if self.use_hip:
                self.cw = ops.intra_weight(rowptr, tails, weights, all_labels)
            else:
                self.cw = intra_weight_torch(rowptr, tails, weights,
                                             all_labels).to(weights.dtype)
            self.active = frontier0.to(dev).clone()
        else:
            if self.use_hip:
                self.cw, mask = ops.intra_boundary(rowptr, tails, weights,
                                                   all_labels)
            else:
                from .uncoarsen import intra_boundary_torch
                self.cw, mask = intra_boundary_torch(rowptr, tails, weights,
                                                     all_labels)
                self.cw = self.cw.to(weights.dtype)
            self.active = mask.to(torch.bool)
        del all_labels
        state.cluster_weight = self.cw
        self.g_rowptr, self.g_heads = ghost_reverse_csr(rowptr, tails, hl.ng)
        self.moved = None           # local vertices whose label changed in
        #                             the last sweep adopted
        self._ghost_prev = self.ghost  # ghost labels as of the previous
        #                                sweep's exchange
        self._remote_gids = None

    def span(self, name):
        import contextlib
        return self.timers(name) if self.timers is not None \
            else contextlib.nullcontext()

    def move(self, sweep: int):
        """Sweep `sweep` (1-based) up to and including the move: ghost
        exchange, the next frontier (moved + N(moved), changed ghosts
        included) from sweep 2 on, densify, frontier_move. Returns (target
        global labels [nv], global frontier size). Afterwards self.cw /
        state.cluster_weight hold cw under state.curr_comm for every vertex;
        the aggregates are still the ones the sweep read."""
        state, dg, comm = self.state, self.dg, self.comm
        from .louvain import _dense_to_gid
        dev = dg.g.device
        nv = dg.nv
        hl = state.halo
        rowptr, tails, weights = dg.g.rowptr, hl.tails_dense, dg.g.weights
        with self.span("exchange"):
            if sweep > 1:
                self.ghost = exchange_ghost_labels(hl, state.curr_comm)
        ghost = self.ghost
        if sweep > 1 and self.expand:
            with self.span("expand"):
                ch = [self.moved.nonzero(as_tuple=True)[0]]
                if hl.ng:
                    ch.append(nv + (ghost != self._ghost_prev).nonzero(
                        as_tuple=True)[0])
                changed = torch.cat(ch).to(torch.int32)
                self.active = torch.zeros(nv, dtype=torch.bool, device=dev)
                if self.use_hip:
                    self.ops.frontier_expand(changed, rowptr, tails,
                                             self.g_rowptr, self.g_heads,
                                             self.active)
                else:
                    frontier_expand_torch(changed, rowptr, tails,
                                          self.g_rowptr, self.g_heads,
                                          self.active)
        self._ghost_prev = ghost
        active = self.active
        if self.observe is not None:
            self.observe("begin", sweep=sweep, active=active.clone(),
                         curr=state.curr_comm.clone(), ghost=ghost.clone(),
                         cw=self.cw.clone())
        with self.span("densify"):
            dense, remote_gids, c_size, c_degree, c_gid = state.densify(ghost)
            inp = MoveInputs(rowptr, tails, weights, dense, state.v_degree,
                             c_size, c_degree, c_gid, state.constant,
                             local_gid_base=dg.base)
        if self.use_hip:
            with self.span("compact"):
                lists = self.ops.frontier_lists(rowptr, active)
                n_act = sum(int(v.numel()) for v in lists)
            with self.span("move"):
                tgt_dense, self.cw = self.ops.frontier_move(
                    inp, active, self.cw, lists=lists)
        else:
            n_act = int(active.sum())
            tgt_dense, self.cw = frontier_move_torch(inp, active, self.cw)
        state.cluster_weight = self.cw
        self._remote_gids = remote_gids
        target = _dense_to_gid(state, tgt_dense, remote_gids)
        if comm.world > 1:
            n_act = int(comm.allreduce_scalar(float(n_act)))
        return target, n_act

    def apply(self, target: torch.Tensor) -> None:
        """The aggregate update for `target` (what move returned), on the
        delta path: the fused next_size / next_degree accounting counts
        visited vertices only."""
        with self.span("aggregates"):
            self.state.apply_moves(target, self._remote_gids, recount=False)

    def adopt(self, target: torch.Tensor) -> None:
        """Make `target` the current labels (run_phase's rotation)."""
        state = self.state
        self.moved = target != state.curr_comm
        state.past_comm, state.curr_comm = state.curr_comm, target


def run_frontier_phase(dg: DistGraph, comm: Comm, cfg, prev: torch.Tensor,
                       frontier0: torch.Tensor, halo=None, *,
                       lower: float = -1.0,
                       threshold: Optional[float] = None,
                       expand: bool = True,
                       observe: Optional[Callable] = None,
                       timers=None):
    """Local moving from the labels `prev` (int64 [nv], this rank's slice,
    global ids, validated like init_labels) in which sweep 1 evaluates the
    vertices of the bool mask `frontier0` and every later sweep the moved
    vertices and their neighbours (module docstring). Collective. Returns
    run_phase's tuple plus a FrontierReport:
    (estimate, labels int64 [nv], sweeps, halo, report).

    `lower` / `threshold` as in run_phase (default cfg.threshold).
    `expand=False` keeps the first frontier for every sweep; with an all-true
    mask the phase is then run_phase's warm start, label for label.
    `observe(event, **state)`: test hook, called with "begin" once the
    sweep's frontier is known and with "end" after its move. `timers`: a
    utils.timers.Timers that accumulates the parts of a sweep."""
    from .louvain import _modularity

    sw = FrontierSweeps(dg, comm, cfg, prev, frontier0, halo, expand=expand,
                        observe=observe, timers=timers)
    state = sw.state
    if threshold is None:
        threshold = cfg.threshold
    prev_mod = lower
    iters = 0
    sizes: List[int] = []
    estimates: List[float] = []

    while iters < cfg.max_iters_per_phase:
        iters += 1
        target, n_act = sw.move(iters)
        sw.apply(target)
        with sw.span("modularity"):
            curr_mod = _modularity(state)
        sizes.append(n_act)
        estimates.append(curr_mod)
        if observe is not None:
            observe("end", sweep=iters, target=target.clone(),
                    cw=sw.cw.clone(), estimate=curr_mod)
        if cfg.verbose and comm.rank == 0:
            print(f"  frontier sweep {iters}: |A|={sizes[-1]} "
                  f"Q={curr_mod:.6f}")

        # stop test and rotation exactly as run_phase
        if (curr_mod - prev_mod) < threshold:
            break
        prev_mod = max(curr_mod, lower)
        sw.adopt(target)

    report = FrontierReport(sizes, sum(sizes), iters, estimates)
    return prev_mod, state.past_comm, iters, state.halo, report


# ---------------------------------------------------------------------------
# edge batches
# ---------------------------------------------------------------------------

@dataclass
class EdgeBatch:
    """Edge changes in global vertex ids, each undirected edge once (either
    orientation). One rank's share of the batch in a multi-rank run."""

    ins_src: torch.Tensor   # int64 [ni]
    ins_dst: torch.Tensor   # int64 [ni]
    ins_w: torch.Tensor     # float [ni]
    del_src: torch.Tensor   # int64 [nd]
    del_dst: torch.Tensor   # int64 [nd]

    @staticmethod
    def empty() -> "EdgeBatch":
        z = torch.empty(0, dtype=torch.int64)
        return EdgeBatch(z, z.clone(), torch.empty(0, dtype=torch.float64),
                         z.clone(), z.clone())

    def to(self, device) -> "EdgeBatch":
        return EdgeBatch(*[t.to(device) for t in (
            self.ins_src, self.ins_dst, self.ins_w, self.del_src,
            self.del_dst)])


def _check_batch(dg: DistGraph, comm: Comm, batch: EdgeBatch) -> None:
    """ValueError on every rank if any share is malformed."""
    why = ""
    ids = (batch.ins_src, batch.ins_dst, batch.del_src, batch.del_dst)
    if any(t.dtype != torch.int64 or t.dim() != 1 for t in ids):
        why = "vertex ids must be 1-D int64 tensors"
    elif batch.ins_src.numel() != batch.ins_dst.numel() \
            or batch.ins_src.numel() != batch.ins_w.numel() \
            or batch.del_src.numel() != batch.del_dst.numel():
        why = "source / destination / weight lengths differ"
    else:
        for t in ids:
            if t.numel() and (int(t.min()) < 0
                              or int(t.max()) >= dg.nv_global):
                why = f"vertex ids must lie in [0, {dg.nv_global})"
    if comm.allreduce_scalar(1.0 if why else 0.0) > 0.0:
        raise ValueError(f"invalid edge batch: {why}" if why else
                         "invalid edge batch on another rank")


def _directed(src: torch.Tensor, dst: torch.Tensor, *payload):
    """Both directions of every undirected pair; a self-loop once."""
    rev = src != dst
    out = [torch.cat([src, dst[rev]]), torch.cat([dst, src[rev]])]
    for p in payload:
        out.append(torch.cat([p, p[rev]]))
    return out


def _route_by_owner(dg: DistGraph, comm: Comm, key: torch.Tensor, *cols):
    """Send every entry to the owner of global vertex key[i]; returns the
    received (key, *cols), concatenated in rank order."""
    if comm.world == 1:
        return (key,) + cols
    owner = dg.partition.owner(key)
    order = torch.argsort(owner, stable=True)
    offs = torch.searchsorted(
        owner[order], torch.arange(comm.world + 1, device=key.device))
    out = []
    counts = None
    for col in (key,) + cols:
        c = col[order]
        got = comm.all_to_all_v(
            [c[offs[p]:offs[p + 1]] for p in range(comm.world)], counts)
        if counts is None:
            counts = [int(g.numel()) for g in got]
        out.append(torch.cat(got))
    return tuple(out)


def _route_batch(dg: DistGraph, comm: Comm, batch: EdgeBatch):
    """Both directions of every change, each at the owner of its source:
    (d_src, d_dst, i_src, i_dst, i_w), global ids, i_w in fp64."""
    d_src, d_dst = _directed(batch.del_src, batch.del_dst)
    d_src, d_dst = _route_by_owner(dg, comm, d_src, d_dst)
    i_src, i_dst, i_w = _directed(batch.ins_src, batch.ins_dst,
                                  batch.ins_w.to(torch.float64))
    i_src, i_dst, i_w = _route_by_owner(dg, comm, i_src, i_dst, i_w)
    return d_src, d_dst, i_src, i_dst, i_w


def _stable_rows(g: Graph, base: int, nv_global: int, d_src, d_dst, i_src,
                 i_dst, i_w):
    """apply_routed_batch_torch without the raise: (Graph or None, absent)."""
    nv, dev = g.nv, g.device
    src = torch.repeat_interleave(torch.arange(nv, device=dev), g.degrees())
    key = src * nv_global + g.tails
    dkey = torch.unique((d_src - base) * nv_global + d_dst)
    if dkey.numel() > 0 and not bool(torch.isin(dkey, key).all()):
        return None, True
    keep = ~torch.isin(key, dkey)
    # old entries first, then the insertions: a stable sort by source leaves
    # both in their order inside every row
    rows = torch.cat([src[keep], i_src - base])
    order = torch.argsort(rows, stable=True)
    rowptr = torch.zeros(nv + 1, dtype=torch.int64, device=dev)
    if rows.numel():
        rowptr[1:] = torch.cumsum(torch.bincount(rows, minlength=nv), dim=0)
    tails = torch.cat([g.tails[keep], i_dst])[order]
    weights = torch.cat([g.weights[keep], i_w.to(g.weights.dtype)])[order]
    return Graph(rowptr, tails, weights), False


def apply_routed_batch_torch(g: Graph, base: int, nv_global: int,
                             d_src: torch.Tensor, d_dst: torch.Tensor,
                             i_src: torch.Tensor, i_dst: torch.Tensor,
                             i_w: torch.Tensor) -> Graph:
    """Twin of ops.apply_batch: the routed lists of one rank (directed,
    global ids, every source owned by this rank) applied to its CSR `g`, with
    the order inside a row fixed ("stable rows"):

      - row v keeps its old entries whose (v, dst) is not in the deletion
        set, in their old order;
      - after them come the insertions with source v, in the order of the
        routed list;
      - weights are copied (cast to the graph's dtype), never added.

    A deletion that matches no stored entry raises ValueError; `g` is never
    modified. Works on any device; runs over all `ne` entries."""
    out, absent = _stable_rows(g, base, nv_global, d_src, d_dst, i_src,
                               i_dst, i_w)
    if absent:
        raise ValueError("edge batch deletes an edge the graph does not hold")
    return out


def _rebuild(g: Graph, base: int, nv_global: int, d_src, d_dst, i_src, i_dst,
             i_w):
    """The whole-graph rebuild through Graph.from_edge_tuples: (Graph or
    None, absent). Row order is the builder's: sorted by dst on the CPU, open
    on the device."""
    nv, dev = g.nv, g.device
    src = base + torch.repeat_interleave(
        torch.arange(nv, device=dev), g.degrees())
    key = src * nv_global + g.tails
    dkey = torch.unique(d_src * nv_global + d_dst)
    if dkey.numel() > 0 and not bool(torch.isin(dkey, key).all()):
        return None, True
    keep = ~torch.isin(key, dkey)
    return Graph.from_edge_tuples(
        nv, torch.cat([src[keep], i_src]),
        torch.cat([g.tails[keep], i_dst]),
        torch.cat([g.weights[keep], i_w.to(g.weights.dtype)]),
        base=base), False


def _batch_on_device(dev) -> bool:
    """Whether apply_edge_batch takes the HIP path (ops.apply_batch): the
    graph is on the GPU, the extension is built and CUVITE_BATCH_DEVICE is
    not 0 (read per call)."""
    if dev.type != "cuda":
        return False
    if os.environ.get("CUVITE_BATCH_DEVICE", "1") in ("0", "off"):
        return False
    from . import ops
    return ops.available()


def apply_edge_batch(dg: DistGraph, comm: Comm,
                     batch: EdgeBatch) -> DistGraph:
    """The graph after the batch: same vertex set and partition. Collective;
    every rank passes its share. Each direction of an edge goes to the owner
    of its source. A deletion removes every stored copy of u-v from both
    rows; a deletion that matches nothing raises ValueError on every rank. An
    insertion adds (u, v, w) and (v, u, w), or a self-loop once; a pair that
    is already present becomes a parallel edge. Deletions apply to the old
    graph, insertions come after. The input graph is not modified.

    On the GPU the routed lists are applied by ops.apply_batch: work on the
    touched rows plus one copy of the CSR, rows in the stable order of
    apply_routed_batch_torch. On the CPU, and with CUVITE_BATCH_DEVICE=0, the
    CSR is rebuilt through Graph.from_edge_tuples."""
    if dg.g._ne_released >= 0:
        raise RuntimeError("tails released: apply edge batches before "
                           "Graph.release_tails()")
    _check_batch(dg, comm, batch)
    dev = dg.g.device
    batch = batch.to(dev)
    routed = _route_batch(dg, comm, batch)
    if _batch_on_device(dev):
        from . import ops
        out = ops.apply_batch(dg.g.rowptr, dg.g.tails, dg.g.weights, dg.base,
                              dg.nv_global, *routed)
        g, absent = (None, True) if out is None else (Graph(*out), False)
    else:
        g, absent = _rebuild(dg.g, dg.base, dg.nv_global, *routed)
    if comm.allreduce_scalar(1.0 if absent else 0.0) > 0.0:
        raise ValueError("edge batch deletes an edge the graph does not hold")
    return DistGraph(g, dg.partition, dg.rank)


def affected_vertices(dg_new: DistGraph, comm: Comm, prev: torch.Tensor,
                      batch: EdgeBatch) -> torch.Tensor:
    """Initial frontier of a batch under the labels `prev` (the
    dynamic-frontier rule): both endpoints of a deleted edge whose endpoints
    share a label, both endpoints of an inserted edge whose endpoints do
    not. Returns a bool mask over this rank's vertices. Collective; labels of
    remote endpoints come from their owners. The union over ranks depends on
    neither rank count nor partition."""
    from .coarsen import _owner_lookup
    validate_labels(dg_new, comm, prev)
    _check_batch(dg_new, comm, batch)
    dev = dg_new.g.device
    batch = batch.to(dev)
    prev = prev.to(dev)
    base, nv = dg_new.base, dg_new.nv
    ends = torch.cat([batch.del_src, batch.del_dst, batch.ins_src,
                      batch.ins_dst])
    query = torch.unique(ends)  # sorted
    lab = _owner_lookup(comm, dg_new.partition, query,
                        lambda g: prev[g - base])

    def label_of(v):
        return lab[torch.searchsorted(query, v.contiguous())]

    dmark = label_of(batch.del_src) == label_of(batch.del_dst)
    imark = label_of(batch.ins_src) != label_of(batch.ins_dst)
    marked = torch.cat([batch.del_src[dmark], batch.del_dst[dmark],
                        batch.ins_src[imark], batch.ins_dst[imark]])
    (mine,) = _route_by_owner(dg_new, comm, marked)
    mask = torch.zeros(nv, dtype=torch.bool, device=dev)
    mask[mine - base] = True
    return mask


# ---------------------------------------------------------------------------
# a stream of batches
# ---------------------------------------------------------------------------

@dataclass
class StreamStep:
    """One batch of update_stream."""

    inserted: int       # undirected insertions of the batch, all ranks
    deleted: int        # undirected deletions listed in the batch, all ranks
    affected: int       # size of the first frontier, all ranks
    result: object      # the LouvainResult of the run after the batch


class StreamError(ValueError):
    """A batch of update_stream was refused. `steps`: the StreamSteps
    finished before it, still valid; `dg`: the graph they reached."""

    def __init__(self, message: str, steps: List[StreamStep], dg: DistGraph):
        super().__init__(message)
        self.steps = steps
        self.dg = dg


_STREAM_REJECTS = ("coloring", "ordering", "early_term", "threshold_scaling")


def update_stream(dg: DistGraph, comm: Comm, cfg, prev: torch.Tensor,
                  batches: Sequence[EdgeBatch]):
    """Follow a stream of edge batches: for every batch in order apply it
    (apply_edge_batch), mark the affected vertices under the current labels
    (affected_vertices) and run louvain from those labels with that frontier;
    the run's communities are the labels the next batch starts from.
    Collective: every rank passes its own share of each batch and its slice
    `prev` of the partition of `dg`. Returns (graph after the last batch,
    [StreamStep per batch]).

    Coloring, ordering, early termination and threshold scaling are rejected
    on every rank before any collective, as louvain(init_frontier=...) does.
    A bad batch raises StreamError (a ValueError) at its step, on every
    rank; it carries the finished steps and the graph they reached."""
    for flag in _STREAM_REJECTS:
        if getattr(cfg, flag):
            raise ValueError(f"update_stream cannot be combined with {flag}")
    from .louvain import louvain
    labels = prev
    steps: List[StreamStep] = []
    for batch in batches:
        try:
            new = apply_edge_batch(dg, comm, batch)
            mask = affected_vertices(new, comm, labels, batch)
        except ValueError as e:
            raise StreamError(str(e), steps, dg) from e
        dg = new
        counts = [float(batch.ins_src.numel()), float(batch.del_src.numel()),
                  float(mask.sum())]
        if comm.world > 1:
            counts = [comm.allreduce_scalar(c) for c in counts]
        res = louvain(dg, comm, cfg, init_labels=labels, init_frontier=mask)
        steps.append(StreamStep(int(counts[0]), int(counts[1]),
                                int(counts[2]), res))
        labels = res.communities
    return dg, steps
