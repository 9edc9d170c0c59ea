"""Multi-phase distributed Louvain orchestration.

Structure mirrors the reference: an outer phase loop
(local-moving until convergence, then graph coarsening) around an inner
iteration loop (halo fill -> local move -> community update -> remote update
-> modularity -> convergence test). Variants: plain, early-termination
(freeze / probabilistic, ref louvain.cpp:7-424), coloring-ordered and
vertex-ordered moves (ref louvain.cpp:756-2101), threshold cycling
(main.cpp:225-239).

All state lives on the compute device; per-iteration host work is zero on the
GPU path (the reference rebuilds its dense community remap on the host every
iteration, louvain_cuda.cu:2260-2378 — here remote community ids are interned
once into a phase-persistent on-device universe and only CHANGED labels are
remapped per iteration, with no sort/unique in the loop; see
PhaseState.densify).
"""

from __future__ import annotations

import os
import time
from dataclasses import dataclass, field
from typing import List, Optional

import torch

from .graph import DistGraph
from .halo import (build_halo, exchange_ghost_labels, fetch_comm_info_lists,
                   push_remote_deltas)
from .local_move import MoveInputs, local_move_torch, modularity_parts
from .ops import scatter_add_
from .parallel import Comm
from .connectivity import ConnectivityReport, split_disconnected
from .quality import community_aggregates, validate_labels
from .refine import REFINE_MAX_ROUNDS, refine_partition
from .utils.timers import Timers

TERMINATION_PHASE_COUNT = 200   # ref utils.hpp:17-19
MAX_TOTAL_ITERS = 10000         # ref main.cpp:486-494
ET_CUTOFF = 90                  # ref louvain.hpp:76 (absolute count)
P_CUTOFF = 0.02                 # ref louvain.hpp:78


@dataclass
class LouvainConfig:
    threshold: float = 1.0e-6
    threshold_scaling: bool = False      # -i
    one_phase: bool = False              # -p
    early_term: int = 0                  # -t 1..4 (0 = off)
    et_delta: float = 1.0                # -a (alpha for -t 2/4)
    coloring: bool = False               # -c
    ordering: bool = False               # -d
    max_colors: int = 8                  # -c/-d arg (nHash*2)
    backend: str = "auto"                # "auto" | "torch" | "hip"
    max_phases: int = TERMINATION_PHASE_COUNT
    max_iters_per_phase: int = 10000
    verbose: bool = False
    connectivity: str = "off"            # "off" | "final" | "level"
    #   final: split the returned communities into their connected
    #     components on the input graph (never lowers the exact modularity)
    #   level: split every phase's communities on its level graph before
    #     coarsening, so every coarse vertex and every final community is a
    #     connected set. Guarantees connectivity only: the phases that follow
    #     see another graph and the stop test runs on the convergence
    #     estimate, so the exact modularity may end higher or lower.
    algorithm: str = "louvain"           # "louvain" | "leiden"
    #   leiden: after every local-moving phase that passes the gain test the
    #     phase's communities are refined into connected sub-communities
    #     (refine.refine_partition), the level graph is coarsened by those,
    #     and the next phase starts from the parent communities. The result
    #     always passes through the final split (connectivity="final" is
    #     implied; "level" is rejected). -p skips refinement; coloring,
    #     ordering and early termination apply to the local-moving phases
    #     only.
    refine_max_rounds: int = REFINE_MAX_ROUNDS
    refine_seed: int = 0
    vcycle: bool = False
    #   keep every accepted level (graph, halo, map to the next level) and,
    #   after the last phase, refine the partition level by level on the way
    #   back to the input graph (uncoarsen.refine_up). Never lowers the exact
    #   modularity; costs the memory of the kept levels. Cannot be combined
    #   with algorithm="leiden" or connectivity="level": moves on the way up
    #   would break the connectivity those promise.
    resolution: float = 1.0
    #   gamma of the generalised modularity
    #   Q_gamma = sum_c [in_c / 2m - gamma (a_c / 2m)^2]: above 1 more and
    #   smaller communities, below 1 fewer and larger ones. Every mode (the
    #   phases, refinement, the frontier update, the way up) moves by the
    #   gamma-gain and every estimate and exact Q it reports is Q_gamma.
    #   Finite and > 0, else louvain() raises ValueError.


@dataclass
class LouvainResult:
    modularity: float           # convergence estimate, NOT the exact Q of
    #   `communities` (see quality.partition_quality for that)
    communities: torch.Tensor   # final community id per ORIGINAL local vertex
    phases: int
    total_iters: int
    times: dict = field(default_factory=dict)
    modularity_per_level: list = field(default_factory=list)
    levels: list = field(default_factory=list)  # per-phase {ne_global, iters,
    #   modularity, cluster_s, rebuild_s} — feeds the reference TEPS
    #   definition (teps += ne * iters per phase, main.cpp:448); under
    #   algorithm="leiden" a refined level also carries "refine", its
    #   RefineReport
    connectivity: Optional[ConnectivityReport] = None  # "final": the report
    #   of the split (`communities` are its labels); "level": the report of
    #   the last phase's split (every level entry carries its own)
    vcycle: Optional[list] = None  # vcycle=True: one uncoarsen.VcycleLevel
    #   per refined level, coarsest first; `modularity` stays the way down's
    #   estimate, the last entry's q_after is the exact Q of `communities`
    #   (before any final split)

    @property
    def teps_numerator(self) -> float:
        return sum(lv["ne_global"] * lv["iters"] for lv in self.levels)


def _threshold_for_phase(cfg: LouvainConfig, short_phase: int) -> float:
    """Threshold cycling (ref main.cpp:225-239)."""
    if not cfg.threshold_scaling or cfg.one_phase:
        return 1.0e-6
    sp = short_phase % 13
    if sp <= 2:
        return 1.0e-3
    if sp <= 6:
        return 1.0e-4
    if sp <= 9:
        return 1.0e-5
    return 1.0e-6


def _pick_move_fn(cfg: LouvainConfig, device: torch.device):
    if cfg.backend == "torch":
        return local_move_torch
    if cfg.backend in ("auto", "hip") and device.type == "cuda":
        from . import ops
        return ops.local_move  # raises if the HIP extension is missing
    if cfg.backend == "hip":
        raise RuntimeError("backend='hip' requires a CUDA/HIP device")
    return local_move_torch


class PhaseState:
    """Mutable per-phase state for one rank (all tensors on dg's device)."""

    def __init__(self, dg: DistGraph, comm: Comm, halo=None,
                 init_labels: Optional[torch.Tensor] = None,
                 resolution: float = 1.0):
        dev = dg.g.device
        if init_labels is not None:
            validate_labels(dg, comm, init_labels)  # before any collective
        self.dg = dg
        self.comm = comm
        self.halo = halo if halo is not None else build_halo(dg, comm)
        nv = dg.nv
        W = dg.g.weights.dtype
        self.v_degree = dg.local_degree_sum()                       # W [nv]
        # community aggregates, indexed by (gid - base) for owned comms
        self.local_size = torch.ones(nv, dtype=torch.int64, device=dev)
        self.local_degree = self.v_degree.clone()
        # global labels (ref distInitComm: singletons)
        arange = torch.arange(dg.base, dg.bound, device=dev)
        self.curr_comm = arange.clone()
        self.past_comm = arange.clone()
        if init_labels is not None:
            # warm start: arbitrary global labels; aggregates rebuilt from
            # them (everything downstream already copes: densify interns
            # the remote ids on its first call)
            self.curr_comm = init_labels.to(dev).clone()
            self.past_comm = self.curr_comm.clone()
            self.local_size, self.local_degree = community_aggregates(
                dg, comm, self.halo, self.curr_comm, self.v_degree)
        # inv_2m = 1/(2m) (ref distCalcConstantForSecondTerm; guard the
        # edgeless-graph case the reference would divide by zero on).
        # constant = gamma/(2m) is what the move functions receive: it scales
        # the degree term of the gain and nothing else. At gamma = 1.0 the
        # product is inv_2m itself, bit for bit.
        tw = float(self.v_degree.to(torch.float64).sum())
        tw = comm.allreduce_scalar(tw)
        self.resolution = float(resolution)
        self.inv_2m = 1.0 / tw if tw > 0.0 else 0.0
        self.constant = self.resolution * self.inv_2m
        # ET state
        self.active = torch.ones(nv, dtype=torch.bool, device=dev)
        self.stable_count = torch.zeros(nv, dtype=torch.int16, device=dev)
        self.move_prob = torch.ones(nv, dtype=torch.float32, device=dev)
        # phase-persistent dense community space (see densify)
        self._lgids: Optional[torch.Tensor] = None
        self._parts_dev: Optional[torch.Tensor] = None
        self._runiv: Optional[torch.Tensor] = None
        self._prev_labels: Optional[torch.Tensor] = None
        # fused-step buffers (see fused_next), built on first use
        self._agg_spare = None
        self._iso_size: Optional[torch.Tensor] = None

    def fused_step_ok(self, cfg: "LouvainConfig", move_fn) -> bool:
        """Whether the plain sweep may let the move kernels account the new
        community aggregates themselves instead of calling apply_moves:
        one rank, HIP backend, no early termination, rocPRIM hub path, plain
        schedule. CUVITE_FUSED_AGG=0 forces the unfused path."""
        if (self.comm.world != 1 or not getattr(self, "use_hip", False)
                or cfg.early_term
                or os.environ.get("CUVITE_FUSED_AGG", "1") in ("0", "off")):
            return False
        from . import ops
        return move_fn is ops.local_move and ops.fused_aggregates_supported()

    def fused_next(self):
        """The spare (size, degree) pair for a fused step, pre-loaded with
        what the move kernels never visit: vertices without edges keep their
        label for the whole phase and have degree 0, so their share of every
        community's size is a phase constant (iso_size, also right under a
        warm start) and their share of the degrees is zero. Runs on the
        current stream; the caller hands the pair to the move and rebinds
        local_size / local_degree to it afterwards (adopt_next)."""
        if self._iso_size is None:
            rowptr = self.dg.g.rowptr
            iso = (rowptr[1:] == rowptr[:-1]).nonzero(as_tuple=True)[0]
            self._iso_size = torch.bincount(
                self.curr_comm[iso] - self.dg.base, minlength=self.dg.nv)
            self._agg_spare = (torch.empty_like(self.local_size),
                               torch.empty_like(self.local_degree))
        nsize, ndegree = self._agg_spare
        nsize.copy_(self._iso_size)
        ndegree.zero_()
        return nsize, ndegree

    def adopt_next(self, nsize: torch.Tensor, ndegree: torch.Tensor):
        """Make the pair a fused step filled the current aggregates; the
        pair the kernels read becomes the spare."""
        self._agg_spare = (self.local_size, self.local_degree)
        self.local_size, self.local_degree = nsize, ndegree

    def _local_gids(self) -> torch.Tensor:
        if self._lgids is None:
            self._lgids = torch.arange(self.dg.base, self.dg.bound,
                                       device=self.dg.g.device)
        return self._lgids

    def _univ_lookup(self, rem: torch.Tensor):
        """Position in the (append-ordered) universe for each gid in `rem`,
        plus a found mask (positions are garbage where not found)."""
        K = self._runiv_sorted.numel()
        if K == 0:
            z = torch.zeros(rem.numel(), dtype=torch.bool, device=rem.device)
            return torch.zeros(rem.numel(), dtype=torch.int64,
                               device=rem.device), z
        idx = torch.searchsorted(self._runiv_sorted, rem).clamp(max=K - 1)
        found = self._runiv_sorted[idx] == rem
        return self._runiv_perm[idx], found

    def _univ_append(self, new: torch.Tensor):
        """Append new remote community gids to the universe (dense ids are
        append-ordered so existing ids stay stable); rebuild the sorted
        lookup index (only runs on growth — rare after iteration 1)."""
        dev = new.device
        if self._parts_dev is None:
            self._parts_dev = self.dg.partition.parts.to(dev)
        owner = torch.searchsorted(self._parts_dev, new, right=True) - 1
        self._runiv = torch.cat([self._runiv, new])
        self._univ_owner = torch.cat([self._univ_owner, owner])
        self._univ_size = torch.cat([
            self._univ_size,
            torch.zeros(new.numel(), dtype=torch.int64, device=dev)])
        self._univ_degree = torch.cat([
            self._univ_degree,
            torch.zeros(new.numel(), dtype=self.local_degree.dtype,
                        device=dev)])
        self._runiv_sorted, self._runiv_perm = torch.sort(self._runiv)

    def densify(self, ghost_comm: torch.Tensor):
        """Map global labels to the dense community space.
        Returns (curr_dense [nv+ng] int32, remote_gids (append-ordered
        universe), comm_size, comm_degree, comm_gid) with remote info
        fetched from owners for every REFERENCED remote community.

        Phase-persistent design (SURVEY section 7 "biggest systems win"; the
        reference rebuilds its dense remap on the host every iteration,
        louvain_cuda.cu:2260-2378): remote community gids are interned into
        an append-only universe, so per-iteration work is (a) an O(n)
        changed-label compare against the previous iteration's labels,
        (b) a searchsorted lookup for the changed ones only, and (c) an O(n)
        scatter for the referenced-set mask — NO per-iteration torch.unique /
        sort over nv+ng labels. Universe entries that are no longer
        referenced keep stale aggregates; the move kernels only ever read
        communities adjacent to some vertex, which are referenced and fresh
        this iteration."""
        dg, dev = self.dg, self.dg.g.device
        base, bound, nv = dg.base, dg.bound, dg.nv
        if self.comm.world == 1:
            # single-rank fast path: every label is local
            dense = (self.curr_comm - base).to(torch.int32)
            empty = torch.empty(0, dtype=torch.int64, device=dev)
            return (dense, empty, self.local_size, self.local_degree,
                    self._local_gids())
        all_labels = torch.cat([self.curr_comm, ghost_comm])
        n = all_labels.numel()
        if self._runiv is None:
            i64 = dict(dtype=torch.int64, device=dev)
            self._runiv = torch.empty(0, **i64)
            self._runiv_sorted = self._runiv
            self._runiv_perm = torch.empty(0, **i64)
            self._univ_owner = torch.empty(0, **i64)
            self._univ_size = torch.empty(0, **i64)
            self._univ_degree = torch.empty(
                0, dtype=self.local_degree.dtype, device=dev)
            self._dense = torch.empty(n, dtype=torch.int32, device=dev)

        if self._prev_labels is not None and self._prev_labels.numel() == n:
            changed = (all_labels != self._prev_labels).nonzero(
                as_tuple=True)[0]
            lab_c = all_labels[changed]
        else:
            changed = None
            lab_c = all_labels

        if lab_c.numel():
            is_local = (lab_c >= base) & (lab_c < bound)
            rem = lab_c[~is_local]
            pos, found = self._univ_lookup(rem)
            if not bool(found.all()):
                self._univ_append(torch.unique(rem[~found]))
                pos, _ = self._univ_lookup(rem)
            dense_c = torch.empty(lab_c.numel(), dtype=torch.int32,
                                  device=dev)
            dense_c[is_local] = (lab_c[is_local] - base).to(torch.int32)
            if rem.numel():
                dense_c[~is_local] = (nv + pos).to(torch.int32)
            if changed is None:
                self._dense = dense_c
            else:
                self._dense[changed] = dense_c
        self._prev_labels = all_labels

        # referenced remote communities this iteration (mask in universe
        # order), then one request/reply round with their owners
        K = self._runiv.numel()
        ref_mask = torch.zeros(K, dtype=torch.bool, device=dev)
        d64 = self._dense.to(torch.int64)
        rr = d64[d64 >= nv] - nv
        ref_mask[rr] = True
        world = self.comm.world
        reqs, positions = [], []
        for p in range(world):
            sel = (ref_mask & (self._univ_owner == p)).nonzero(
                as_tuple=True)[0]
            reqs.append(self._runiv[sel])
            positions.append(sel)
        sizes_l, degrees_l = fetch_comm_info_lists(
            self.halo, reqs, self.local_size, self.local_degree)
        for p in range(world):
            if positions[p].numel():
                self._univ_size[positions[p]] = sizes_l[p]
                self._univ_degree[positions[p]] = degrees_l[p]
        comm_size = torch.cat([self.local_size, self._univ_size])
        comm_degree = torch.cat([self.local_degree, self._univ_degree])
        comm_gid = torch.cat([self._local_gids(), self._runiv])
        return self._dense, self._runiv, comm_size, comm_degree, comm_gid

    def apply_moves(self, target_gid: torch.Tensor, remote_gids: torch.Tensor,
                    recount: bool = True):
        """Apply community size/degree deltas for vertices that moved
        (ref 4-case update, louvain.cpp:2308-2376 + updateRemoteCommunities).
        `recount=False` keeps a single HIP rank on the delta kernel as well:
        a frontier sweep moves few vertices, and a recount of all of them
        into a warm start's few communities serialises on their counters."""
        dg = self.dg
        base, bound = dg.base, dg.bound
        if getattr(self, "use_hip", False) and target_gid.is_cuda:
            from . import ops
            if self.comm.world == 1 and recount:
                # fresh recount beats the delta update when most vertices
                # move (2 atomics/vertex vs 4 per moved vertex; rocprof
                # 25 -> ~12 ms at s26's oscillating sweeps)
                ops._require().recount_(target_gid, self.v_degree, base,
                                        self.local_size, self.local_degree)
                return
            # fused local delta update, no host sync / compaction kernels
            ops.apply_deltas_(target_gid, self.curr_comm, self.v_degree,
                              base, bound, self.local_size,
                              self.local_degree)
            if self.comm.world == 1:
                return
            moved = target_gid != self.curr_comm
            src = self.curr_comm[moved]
            dst = target_gid[moved]
            vdeg = self.v_degree[moved]
            gids = torch.cat([src, dst])
            dsize = torch.cat([-torch.ones_like(src), torch.ones_like(dst)])
            ddeg = torch.cat([-vdeg, vdeg])
            rem = (gids < base) | (gids >= bound)
            push_remote_deltas(self.halo, gids[rem], dsize[rem], ddeg[rem],
                               self.local_size, self.local_degree)
            return
        moved = target_gid != self.curr_comm
        if not bool(moved.any()):
            # still must participate in the collective delta push
            if self.comm.world > 1:
                empty_i = torch.empty(0, dtype=torch.int64, device=target_gid.device)
                empty_w = torch.empty(0, dtype=self.local_degree.dtype,
                                      device=target_gid.device)
                push_remote_deltas(self.halo, empty_i, empty_i, empty_w,
                                   self.local_size, self.local_degree)
            return
        src = self.curr_comm[moved]
        dst = target_gid[moved]
        vdeg = self.v_degree[moved]
        gids = torch.cat([src, dst])
        dsize = torch.cat([-torch.ones_like(src), torch.ones_like(dst)])
        ddeg = torch.cat([-vdeg, vdeg])
        is_local = (gids >= base) & (gids < bound)
        li = gids[is_local] - base
        self.local_size.index_add_(0, li, dsize[is_local])
        scatter_add_(self.local_degree, li, ddeg[is_local])
        if self.comm.world > 1:
            push_remote_deltas(self.halo, gids[~is_local], dsize[~is_local],
                               ddeg[~is_local], self.local_size, self.local_degree)
        else:
            assert bool(is_local.all())


def _et_update(state: PhaseState, cfg: LouvainConfig, target: torch.Tensor,
               rng: torch.Generator) -> Optional[int]:
    """Early-termination bookkeeping after an iteration. Returns the global
    frozen count for -t 3/4 (ref louvain.cpp:115-120, 172-182, 378-395)."""
    if cfg.early_term in (1, 3):
        stable = (target == state.curr_comm) & (state.curr_comm == state.past_comm)
        state.stable_count = torch.where(stable, state.stable_count + 1,
                                         torch.zeros_like(state.stable_count))
        state.active &= state.stable_count < 3
    elif cfg.early_term in (2, 4):
        moved = target != state.curr_comm
        state.move_prob = torch.where(
            moved, torch.ones_like(state.move_prob),
            state.move_prob * (1.0 - cfg.et_delta))
        # draw on the compute device (a per-iteration host round trip here
        # was round-1 weak item 6); rng lives on the same device
        draw = torch.rand(state.move_prob.shape, generator=rng,
                          device=state.move_prob.device)
        state.active = (state.move_prob >= P_CUTOFF) & \
            ((draw < state.move_prob) | moved)
    if cfg.early_term in (3, 4):
        frozen = int((~state.active).sum())
        return int(state.comm.allreduce_scalar(float(frozen)))
    return None


def run_phase(dg: DistGraph, comm: Comm, cfg: LouvainConfig,
              lower: float, threshold: float,
              colors: Optional[torch.Tensor] = None,
              num_colors: int = 0, halo=None,
              init_labels: Optional[torch.Tensor] = None):
    """One Louvain phase (local moving to convergence). Returns
    (prev_mod, cvect global labels [nv], iters).
    Ref: distLouvainMethod (louvain.cpp:425-588) and the coloring/ordering
    variants (louvain.cpp:756-2101)."""
    state = PhaseState(dg, comm, halo=halo, init_labels=init_labels,
                       resolution=cfg.resolution)
    move_fn = _pick_move_fn(cfg, dg.g.device)
    state.use_hip = (dg.g.device.type == "cuda"
                     and cfg.backend in ("auto", "hip"))
    prev_mod = lower
    iters = 0
    rng = torch.Generator(device=dg.g.device).manual_seed(12345 + comm.rank)
    timers = Timers(sync=dg.g.device.type == "cuda") if cfg.verbose else None

    use_colors = colors is not None and num_colors > 0
    color_order: List[torch.Tensor] = []
    if use_colors:
        for c in range(num_colors):
            color_order.append(torch.nonzero(colors == c, as_tuple=True)[0])

    while iters < cfg.max_iters_per_phase:
        iters += 1
        if timers is None:
            target = _one_sweep(state, cfg, move_fn,
                                color_order if use_colors else None)
            curr_mod = _modularity(state)
        else:
            with timers("sweep"):
                target = _one_sweep(state, cfg, move_fn,
                                    color_order if use_colors else None)
            with timers("modularity"):
                curr_mod = _modularity(state)
            if comm.rank == 0:
                print(f"  iter {iters}: Q={curr_mod:.6f} "
                      f"[{timers.summary()}]")

        frozen = _et_update(state, cfg, target, rng)

        # rotate BEFORE convergence check only in the reference order:
        # check first, rotate after (ref louvain.cpp:541-567)
        if (curr_mod - prev_mod) < threshold:
            break
        prev_mod = max(curr_mod, lower)
        state.past_comm, state.curr_comm = state.curr_comm, target

        if frozen is not None and frozen >= ET_CUTOFF:
            break

    cvect = state.past_comm
    return prev_mod, cvect, iters, state.halo


def _one_sweep(state: PhaseState, cfg: LouvainConfig, move_fn,
               color_order: Optional[List[torch.Tensor]]):
    """One local-moving sweep over all vertices. Plain mode: one simultaneous
    move computation. Coloring mode (-c): sequential passes over color
    classes, with a fresh halo exchange and community update per color
    (ref louvain.cpp:862-901)."""
    nv = state.dg.nv
    dev = state.dg.g.device

    if color_order is None:
        ghost_comm = exchange_ghost_labels(state.halo, state.curr_comm)
        dense, remote_gids, c_size, c_degree, c_gid = state.densify(ghost_comm)
        inp = MoveInputs(state.dg.g.rowptr, state.halo.tails_dense,
                         state.dg.g.weights, dense, state.v_degree,
                         c_size, c_degree, c_gid, state.constant,
                         local_gid_base=state.dg.base)
        if state.fused_step_ok(cfg, move_fn):
            # the kernels that store the targets also build the new
            # aggregates in the spare pair (c_size / c_degree, the pair they
            # read, stays untouched); no recount pass afterwards
            nsize, ndegree = state.fused_next()
            tgt_dense, cw = move_fn(inp, next_size=nsize, next_degree=ndegree)
            state.adopt_next(nsize, ndegree)
            state.cluster_weight = cw
            return _dense_to_gid(state, tgt_dense, remote_gids)
        tgt_dense, cw = move_fn(inp)
        target = _dense_to_gid(state, tgt_dense, remote_gids)
        if cfg.early_term:
            target = torch.where(state.active, target, state.curr_comm)
        state.cluster_weight = torch.where(
            state.active, cw, torch.zeros(1, dtype=cw.dtype, device=dev)) \
            if cfg.early_term else cw
        state.apply_moves(target, remote_gids)
        return target

    if cfg.ordering and not cfg.coloring:
        return _ordered_sweep(state, cfg, move_fn, color_order)

    # coloring-ordered (-c): process color classes sequentially, adopting
    # moves after each class, with a fresh ghost-label exchange and remote
    # community-info fetch per class (ref louvain.cpp:862-901).
    work = state.curr_comm.clone()
    cw_total = torch.zeros(nv, dtype=state.dg.g.weights.dtype, device=dev)
    for vidx in color_order:
        ghost_comm = exchange_ghost_labels(state.halo, work)
        saved = state.curr_comm
        state.curr_comm = work
        dense, remote_gids, c_size, c_degree, c_gid = state.densify(ghost_comm)
        state.curr_comm = saved
        inp = MoveInputs(state.dg.g.rowptr, state.halo.tails_dense,
                         state.dg.g.weights, dense, state.v_degree,
                         c_size, c_degree, c_gid, state.constant,
                         local_gid_base=state.dg.base)
        tgt_dense, cw = move_fn(inp)
        tgt = _dense_to_gid_from(work, tgt_dense, remote_gids,
                                 state.dg.base, state.dg.bound)
        mask = torch.zeros(nv, dtype=torch.bool, device=dev)
        mask[vidx] = True
        if cfg.early_term:
            mask &= state.active
        tgt = torch.where(mask, tgt, work)
        cw_total = torch.where(mask, cw, cw_total)
        # apply deltas for this color class only
        saved_curr = state.curr_comm
        state.curr_comm = work
        state.apply_moves(tgt, remote_gids)
        state.curr_comm = saved_curr
        work = tgt
    state.cluster_weight = cw_total
    return work


def _ordered_sweep(state: PhaseState, cfg: LouvainConfig, move_fn,
                   color_order: List[torch.Tensor]):
    """Vertex-ordering variant (-d, ref distLouvainMethodVertexOrder,
    louvain.cpp:1433-1562): color classes are processed sequentially but
    WITHOUT per-class communication — ghost labels and remote community
    aggregates go stale within the sweep; one exchange at sweep start, one
    delta push at sweep end. All per-class updates happen in the dense
    community id space on device."""
    nv = state.dg.nv
    dev = state.dg.g.device
    ghost_comm = exchange_ghost_labels(state.halo, state.curr_comm)
    dense, remote_gids, c_size, c_degree, c_gid = state.densify(ghost_comm)
    # the per-class updates below mutate these; densify may return live
    # references to state.local_size/local_degree (world-1 fast path)
    c_size = c_size.clone()
    c_degree = c_degree.clone()
    work_dense = dense.clone()
    cw_total = torch.zeros(nv, dtype=state.dg.g.weights.dtype, device=dev)
    for vidx in color_order:
        inp = MoveInputs(state.dg.g.rowptr, state.halo.tails_dense,
                         state.dg.g.weights, work_dense, state.v_degree,
                         c_size, c_degree, c_gid, state.constant,
                         local_gid_base=state.dg.base)
        tgt_dense, cw = move_fn(inp)
        mask = torch.zeros(nv, dtype=torch.bool, device=dev)
        mask[vidx] = True
        if cfg.early_term:
            mask &= state.active
        new_local = torch.where(mask, tgt_dense, work_dense[:nv])
        cw_total = torch.where(mask, cw, cw_total)
        # local-view aggregate update in dense space (no communication)
        moved = new_local != work_dense[:nv]
        if bool(moved.any()):
            src = work_dense[:nv][moved].to(torch.int64)
            dst = new_local[moved].to(torch.int64)
            vdeg = state.v_degree[moved]
            ones = torch.ones_like(src)
            c_size.index_add_(0, src, -ones)
            c_size.index_add_(0, dst, ones)
            scatter_add_(c_degree, src, -vdeg)
            scatter_add_(c_degree, dst, vdeg)
        work_dense[:nv] = new_local
    state.cluster_weight = cw_total
    target = _dense_to_gid(state, work_dense[:nv], remote_gids)
    state.apply_moves(target, remote_gids)
    return target


def _dense_to_gid(state: PhaseState, dense: torch.Tensor,
                  remote_gids: torch.Tensor) -> torch.Tensor:
    return _dense_to_gid_from(state.curr_comm, dense, remote_gids,
                              state.dg.base, state.dg.bound)


def _dense_to_gid_from(curr: torch.Tensor, dense: torch.Tensor,
                       remote_gids: torch.Tensor, base: int, bound: int):
    nv = curr.numel()
    d = dense.to(torch.int64)
    out = torch.where(d < nv, d + base,
                      remote_gids[(d - nv).clamp(min=0, max=max(remote_gids.numel() - 1, 0))]
                      if remote_gids.numel() else d + base)
    return out


def _modularity(state: PhaseState) -> float:
    if getattr(state, "use_hip", False):
        from . import ops
        parts = ops.modularity_parts(state.cluster_weight, state.local_degree)
    else:
        parts = modularity_parts(state.cluster_weight, state.local_degree)
    state.comm.allreduce_sum_(parts)
    # Q_gamma of the two reduced sums; gamma = 1.0 multiplies by exactly 1.0
    c = state.inv_2m
    return float(parts[0]) * c - state.resolution * float(parts[1]) * c * c


def _refined_init_labels(level: DistGraph, comm: Comm, cvect: torch.Tensor,
                         sub: torch.Tensor, renum) -> torch.Tensor:
    """Start labels for the phase after a refined level: int64, one per new
    local vertex. New vertex i is the i-th surviving sub-community this rank
    owns (sub s is owned by the owner of vertex s, which is in it and knows
    its community cvect[s]); its label is the smallest new vertex id among
    the subs of that community: a scatter-amin at the community's owner and
    a lookup back. Collective (`renum` is coarsen's)."""
    from .coarsen import _owner_lookup
    dev = cvect.device
    base, nv = level.base, level.nv
    gids = torch.arange(base, level.bound, device=dev)
    surv = (sub == gids).nonzero(as_tuple=True)[0]
    new_ids = renum(gids[surv])
    c_of_new = cvect[surv]
    big = torch.iinfo(torch.int64).max
    lab = torch.full((nv,), big, dtype=torch.int64, device=dev)
    if comm.world == 1:
        lab.scatter_reduce_(0, c_of_new - base, new_ids, reduce="amin")
        return lab[c_of_new - base]
    order = torch.argsort(c_of_new)
    cs, ns = c_of_new[order], new_ids[order]
    offs = torch.searchsorted(cs, level.partition.parts.to(dev))
    world = comm.world
    got_c = comm.all_to_all_v([cs[offs[p]:offs[p + 1]] for p in range(world)])
    got_n = comm.all_to_all_v([ns[offs[p]:offs[p + 1]] for p in range(world)],
                              recv_counts=[int(g.numel()) for g in got_c])
    for gc, gn in zip(got_c, got_n):
        if gc.numel():
            lab.scatter_reduce_(0, gc - base, gn, reduce="amin")
    uniq_c = torch.unique(c_of_new)  # sorted
    vals = _owner_lookup(comm, level.partition, uniq_c,
                         lambda g: lab[g - base])
    return vals[torch.searchsorted(uniq_c, c_of_new)]


def _check_resolution(gamma) -> None:
    """ValueError unless gamma is a finite number > 0. Local: no collective,
    so a caller that passes the same value on every rank raises on every
    rank."""
    import math
    ok = isinstance(gamma, (int, float)) and not isinstance(gamma, bool) \
        and math.isfinite(gamma) and gamma > 0
    if not ok:
        raise ValueError(f"resolution must be a finite number > 0, got "
                         f"{gamma!r}")


def louvain(dg: DistGraph, comm: Optional[Comm] = None,
            cfg: Optional[LouvainConfig] = None,
            halo=None,
            init_labels: Optional[torch.Tensor] = None,
            init_frontier: Optional[torch.Tensor] = None) -> LouvainResult:
    """Full multi-phase Louvain (ref main.cpp:218-495). Returns the final
    community id per ORIGINAL local vertex (contiguous global ids) and the
    final modularity. `halo`: optional prebuilt HaloContext for the INPUT
    graph (phase 0) — callers that already built one (bench.py's timed
    region) pass it to avoid a duplicate ghost structure (17 GB at s27).
    `init_labels`: warm start — int64 [nv] global community ids in
    [0, nv_global) for this rank's vertices; phase 0 starts from them
    instead of singletons (ValueError on every rank if any slice is bad).
    `init_frontier`: with init_labels, a bool mask over this rank's vertices;
    phase 0 becomes the dynamic-frontier phase (dynamic.run_frontier_phase):
    its first sweep evaluates the marked vertices only and every later one
    the moved vertices and their neighbours. levels[0]["frontier"] carries
    the FrontierReport. Coloring, ordering, early termination and threshold
    scaling cannot be combined with it; one_phase, connectivity and
    algorithm="leiden" act after the phase and compose unchanged.
    `cfg.vcycle`: see LouvainConfig; the way up starts when the loop below
    ends and replaces the composed labels."""
    from .coarsen import coarsen, remap_labels
    from .coloring import distance1_coloring

    comm = comm or Comm(dg.g.device)
    cfg = cfg or LouvainConfig()
    dev = dg.g.device
    if cfg.connectivity not in ("off", "final", "level"):
        raise ValueError(f"unknown connectivity mode {cfg.connectivity!r}")
    if cfg.algorithm not in ("louvain", "leiden"):
        raise ValueError(f"unknown algorithm {cfg.algorithm!r}")
    _check_resolution(cfg.resolution)  # every rank holds the same cfg: no
    #                                    collective needed for the verdict
    if init_frontier is not None:
        if init_labels is None:
            raise ValueError("init_frontier needs init_labels")
        for flag in ("coloring", "ordering", "early_term",
                     "threshold_scaling"):
            if getattr(cfg, flag):
                raise ValueError(f"init_frontier cannot be combined with "
                                 f"{flag}")
    leiden = cfg.algorithm == "leiden"
    if leiden and cfg.connectivity == "level":
        raise ValueError("algorithm='leiden' refines every level itself; "
                         "connectivity='level' cannot be combined with it")
    if cfg.vcycle and (leiden or cfg.connectivity == "level"):
        raise ValueError("vcycle moves vertices on the way up and cannot "
                         "keep the connectivity that algorithm='leiden' and "
                         "connectivity='level' promise")
    hier = None
    if cfg.vcycle:
        from .uncoarsen import Hierarchy, refine_up
        hier = Hierarchy()
    conn_report = None

    def split_level(cvect, level_halo, entry):
        # "level": the phase's communities, split on the level graph
        nonlocal conn_report
        conn_report = split_disconnected(level, comm=comm, labels=cvect,
                                         halo=level_halo,
                                         backend=cfg.backend)
        entry["connectivity"] = conn_report
        return conn_report.labels

    t_start = time.perf_counter()
    orig_assign = torch.arange(dg.base, dg.bound, device=dev)  # current label of my originals
    # leiden: the level vertex every original sits in (under louvain that is
    # orig_assign itself, communities become the next vertices), and the
    # start labels of the next phase (the parent communities)
    orig_vertex = orig_assign
    next_init = None
    prev_mod, curr_mod = -1.0, -1.0
    phase = 0
    short_phase = 0
    tot_iters = 0
    mods = []
    levels: list = []
    level = dg
    times = {"coloring": 0.0, "clustering": 0.0, "rebuild": 0.0}

    while True:
        threshold = _threshold_for_phase(cfg, short_phase) \
            if cfg.threshold_scaling else cfg.threshold

        colors = None
        num_colors = 0
        pre_halo = halo if phase == 0 else None
        if (cfg.coloring or cfg.ordering) and phase == 0:
            from .halo import build_halo as _bh
            t0 = time.perf_counter()
            if pre_halo is None:
                pre_halo = _bh(level, comm)  # shared with PhaseState below
            colors, num_colors = distance1_coloring(
                level, comm, n_hash=max(1, cfg.max_colors // 2),
                halo=pre_halo)
            times["coloring"] += time.perf_counter() - t0

        ne_global = comm.allreduce_scalar(float(level.ne)) \
            if comm.world > 1 else float(level.ne)
        t0 = time.perf_counter()
        halo = None  # phase-0 halo ownership moves to run_phase/coarsen
        frontier_report = None
        if phase == 0 and init_frontier is not None:
            from .dynamic import run_frontier_phase
            curr_mod, cvect, iters, phase_halo, frontier_report = \
                run_frontier_phase(level, comm, cfg, init_labels,
                                   init_frontier, halo=pre_halo,
                                   lower=curr_mod, threshold=threshold)
        else:
            curr_mod, cvect, iters, phase_halo = run_phase(
                level, comm, cfg, curr_mod, threshold,
                colors=colors, num_colors=num_colors, halo=pre_halo,
                init_labels=init_labels if phase == 0 else next_init)
        pre_halo = None
        t_cluster = time.perf_counter() - t0
        times["clustering"] += t_cluster
        tot_iters += iters
        level_entry = {"ne_global": ne_global, "iters": iters,
                       "modularity": curr_mod, "cluster_s": t_cluster,
                       "rebuild_s": 0.0}
        if frontier_report is not None:
            level_entry["frontier"] = frontier_report
        levels.append(level_entry)

        if (curr_mod - prev_mod) > threshold:
            if cfg.connectivity == "level":
                cvect = split_level(cvect, phase_halo, level_entry)
            # compose: originals currently assigned to level vertices; level
            # vertex v now belongs to community cvect[v]
            orig_assign = remap_labels(level, comm, orig_vertex if leiden
                                       else orig_assign, cvect)
            mods.append(curr_mod)
            if hier is not None:
                hier.push(level, phase_halo, cvect)
            if cfg.one_phase:
                break
            t0 = time.perf_counter()
            if leiden:
                # refine the communities into connected subs (the phase's
                # hub caches still fit: same level graph), coarsen by the
                # subs, start the next phase from the parent communities
                rep = refine_partition(
                    level, cvect, comm, halo=phase_halo, backend=cfg.backend,
                    max_rounds=cfg.refine_max_rounds, seed=cfg.refine_seed,
                    level=phase, resolution=cfg.resolution)
                level_entry["refine"] = rep
                orig_vertex = remap_labels(level, comm, orig_vertex,
                                           rep.labels)
            if dev.type == "cuda":
                from . import ops
                ops.clear_phase_caches()  # free phase-keyed GPU tensors
            if leiden:
                new_level, renum = coarsen(level, comm, rep.labels,
                                           halo=phase_halo)
                orig_vertex = renum(orig_vertex)
                next_init = _refined_init_labels(level, comm, cvect,
                                                 rep.labels, renum)
                level = new_level
                # orig_assign keeps this level's community gids (all below
                # nv_global): they are the result if no later phase gains
            else:
                level, renum = coarsen(level, comm, cvect, halo=phase_halo)
                # cvect-composed orig_assign holds OLD comm gids; renumber
                orig_assign = renum(orig_assign)
                if hier is not None:
                    hier.maps[-1] = renum(cvect)
            phase_halo = None  # free the ghost structure before next phase
            level_entry["rebuild_s"] = time.perf_counter() - t0
            times["rebuild"] += level_entry["rebuild_s"]
        else:
            if cfg.threshold_scaling and not cfg.one_phase and phase < 10:
                curr_mod2, cvect, iters, phase_halo = run_phase(
                    level, comm, cfg, curr_mod, 1.0e-6,
                    init_labels=next_init if phase > 0 else None)
                tot_iters += iters
                level_entry["iters"] += iters
                if (curr_mod2 - curr_mod) > 1.0e-6:
                    if cfg.connectivity == "level":
                        cvect = split_level(cvect, phase_halo, level_entry)
                    orig_assign = remap_labels(
                        level, comm, orig_vertex if leiden else orig_assign,
                        cvect)
                    mods.append(curr_mod2)
                    curr_mod = curr_mod2
                    if hier is not None:
                        hier.push(level, phase_halo, cvect)
            break

        prev_mod = curr_mod
        curr_mod = -1.0
        phase += 1
        if cfg.threshold_scaling:
            short_phase += 1
        if phase >= cfg.max_phases or tot_iters > MAX_TOTAL_ITERS:
            break

    # the input graph's halo is still there only if no coarsening took it over
    final_halo = phase_halo if level is dg else None
    vcycle_report = None
    if hier is not None:
        vcycle_report = []
        if len(hier):
            t0 = time.perf_counter()
            # the last level built may be one no phase gained on: the way up
            # does not visit it. The input graph's halo outlives the walk.
            final_halo = hier.halos[0]
            level = phase_halo = None
            orig_assign, vcycle_report = refine_up(hier, comm, cfg)
            times["vcycle"] = time.perf_counter() - t0

    if cfg.connectivity == "final" or leiden:
        # on the INPUT graph
        conn_report = split_disconnected(dg, orig_assign, comm,
                                         halo=final_halo,
                                         backend=cfg.backend)
        orig_assign = conn_report.labels

    times["total"] = time.perf_counter() - t_start
    final_mod = mods[-1] if mods else max(prev_mod, curr_mod)
    return LouvainResult(final_mod, orig_assign, phase + 1, tot_iters,
                         times, mods, levels, conn_report, vcycle_report)


def resolution_scan(dg: DistGraph, gammas, comm: Optional[Comm] = None,
                    cfg: Optional[LouvainConfig] = None,
                    init_labels: Optional[torch.Tensor] = None
                    ) -> List[LouvainResult]:
    """One run per resolution in `gammas`, which must be strictly decreasing
    (ValueError otherwise, raised before any run). The first run is an
    ordinary one (from `init_labels` if given); every later run is
    warm-started from the communities of the run before it. Louvain merges
    and never splits, and a lower gamma favours larger communities, so this
    is the direction in which the previous result is a useful start.
    Result i equals louvain(dg, comm, replace(cfg, resolution=gammas[i]),
    init_labels=results[i - 1].communities). Faster than cold runs, and
    usually, not always, of higher Q_gamma (README). Collective."""
    from dataclasses import replace
    comm = comm or Comm(dg.g.device)
    cfg = cfg or LouvainConfig()
    gammas = [float(g) for g in gammas]
    for g in gammas:
        _check_resolution(g)
    if any(b >= a for a, b in zip(gammas, gammas[1:])):
        raise ValueError(f"gammas must be strictly decreasing, got {gammas}")
    results: List[LouvainResult] = []
    labels = init_labels
    for g in gammas:
        res = louvain(dg, comm, replace(cfg, resolution=g),
                      init_labels=labels)
        results.append(res)
        labels = res.communities
    return results
