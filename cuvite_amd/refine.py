"""Leiden refinement: rebuild every community from singletons into connected
sub-communities, on the level graph, synchronously and deterministically.

Louvain's local moving can leave a community in pieces (a bridge vertex moves
out). The Leiden refinement step prevents that during clustering: after a
local-moving phase with community labels C (the *bound*, fixed here), every
vertex starts again as a singleton sub-community and singletons merge into
neighbouring sub-communities of their own community by gain-positive moves.
The level graph is then coarsened by the sub-communities, each of which is
connected and lies inside one community.

The project's sweeps are synchronous and equal the CPU oracle on any rank
count, so this is not the CAS-racing refinement of GVE-Leiden. Rounds come
in pairs p = 0, 1, ...; `refine_coin(gid, p, level, seed)` is one bit per
vertex and pair. In the first round of a pair the *movers* are the singleton
sub-communities whose vertex has coin 1, in the second those with coin 0;
everything else is an *anchor* that round. A mover evaluates the usual gain
(`local_move.refine_move_torch`) over the neighbouring sub-communities that
lie in its own community and are not singleton movers of this round, and
takes the largest strictly positive one, ties to the smaller global id.
Every proposal is applied: a target never moves in the round it is joined,
so a sub-community's label stays the global id of a vertex still in it, and
by induction every sub-community is connected. Refinement stops after the
first pair in which no vertex moved anywhere (one allreduce per round), or
at `max_rounds`. Leftover singletons are legal.

This is the greedy variant: Leiden's randomised choice among the positive
gains and its well-connectedness pre-tests are not implemented. The gain is
the gamma-gain of the run (`resolution`).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

from .graph import DistGraph
from .halo import exchange_ghost_labels
from .local_move import MoveInputs, refine_move_torch
from .parallel import Comm
from .quality import _use_hip, validate_labels

# Largest round count seen on any level of the quality graphs and R-MAT s14
# is 18 (R-MAT s14, level 0; profiles/leiden.md); the default is that,
# doubled.
REFINE_MAX_ROUNDS = 36

_M32 = 0xFFFFFFFF
_MUL = 0x45D9F3B   # < 2^27: (32-bit value) * _MUL stays below 2^63


def refine_coin(gids: torch.Tensor, pair: int, level: int = 0,
                seed: int = 0) -> torch.Tensor:
    """One bit per global vertex id: bool tensor like `gids` (int64). A pure
    integer hash in torch int64 ops whose intermediates stay below 2^63, so
    it gives the same bits on the CPU, on a GPU and on any rank count."""
    salt = (0x27D4EB2F + 0x9E3779B1 * (int(pair) + 1)
            + 0x85EBCA6B * (int(level) + 1)
            + 0xC2B2AE35 * (int(seed) + 1)) & _M32
    x = gids.to(torch.int64)
    x = (x ^ (x >> 32)) & _M32
    x = x ^ salt
    x = ((x ^ (x >> 16)) * _MUL) & _M32
    x = ((x ^ (x >> 16)) * _MUL) & _M32
    x = x ^ (x >> 16)
    return ((x >> 7) & 1).to(torch.bool)


@dataclass
class RefineReport:
    labels: torch.Tensor        # int64 [nv]: sub-community of every local
    #   vertex, the global id of a vertex that is in it
    num_communities: int        # distinct bound labels (global)
    num_subcommunities: int     # distinct sub-community labels (global)
    rounds: int                 # refine rounds run (two per pair)
    moved_per_round: List[int] = field(default_factory=list)  # global counts


def refine_partition(dg: DistGraph, labels: torch.Tensor,
                     comm: Optional[Comm] = None, halo=None,
                     backend: str = "auto",
                     max_rounds: int = REFINE_MAX_ROUNDS, seed: int = 0,
                     level: int = 0,
                     trace: Optional[Callable[[dict], None]] = None,
                     resolution: float = 1.0) -> RefineReport:
    """Refine the communities `labels` (int64 [nv], this rank's slice, global
    ids in [0, nv_global)) of `dg` into connected sub-communities.
    Collective: every rank calls it with its own slice. `halo`: reuse a
    HaloContext already built for `dg`. On a GPU the move is the HIP refine
    kernels (a missing extension raises); backend="torch" forces the torch
    twin. `trace`, if given, is called after every round with
    {"round", "curr", "target"} (this rank's sub labels before and after).
    `resolution`: gamma of the gain the movers evaluate (LouvainConfig).

    The result depends on neither rank count nor partition."""
    from .connectivity import _count_by_community
    from .louvain import PhaseState, _dense_to_gid

    comm = comm or Comm(dg.g.device)
    dev = dg.g.device
    validate_labels(dg, comm, labels)
    labels = labels.to(dev)
    use_hip = _use_hip(backend, dev)
    if use_hip:
        from . import ops
        move_fn = ops.refine_move   # raises if the extension is missing
    else:
        move_fn = refine_move_torch

    # singleton sub labels; sizes and degrees are the sub aggregates
    state = PhaseState(dg, comm, halo=halo, resolution=resolution)
    state.use_hip = use_hip
    halo = state.halo
    nv = dg.nv
    gids = state._local_gids()

    # bound ids: a rank-local int32 numbering of C over locals and ghosts
    all_c = torch.cat([labels, exchange_ghost_labels(halo, labels)])
    bid_all = torch.unique(all_c, return_inverse=True)[1].to(torch.int32)
    minus1 = torch.full((1,), -1, dtype=torch.int32, device=dev)

    moved_per_round: List[int] = []
    rounds = 0
    while rounds < max_rounds:
        pair, want = rounds // 2, rounds % 2 == 0
        ghost_s = exchange_ghost_labels(halo, state.curr_comm)
        dense, remote_gids, c_size, c_degree, c_gid = state.densify(ghost_s)
        # singleton movers of this round, as sub-communities: size 1 and the
        # coin of the sub's gid (its one member) shows this round's face
        sub_moves = (c_size == 1) & (refine_coin(c_gid, pair, level, seed)
                                     == want)
        d64 = dense.to(torch.int64)
        mover = (state.curr_comm == gids) & sub_moves[d64[:nv]]
        mover_bound = torch.where(mover, bid_all[:nv], minus1)
        # bound of every referenced sub: all its members agree on C
        cand_bound = torch.full((c_size.numel(),), -1, dtype=torch.int32,
                                device=dev)
        cand_bound[d64] = bid_all
        cand_bound = torch.where(sub_moves, minus1, cand_bound)

        inp = MoveInputs(dg.g.rowptr, halo.tails_dense, dg.g.weights, dense,
                         state.v_degree, c_size, c_degree, c_gid,
                         state.constant, local_gid_base=dg.base)
        tgt_dense, _ = move_fn(inp, mover_bound, cand_bound)
        target = _dense_to_gid(state, tgt_dense, remote_gids)
        moved = comm.allreduce_scalar(
            float((target != state.curr_comm).sum()))
        if trace is not None:
            trace({"round": rounds, "curr": state.curr_comm.clone(),
                   "target": target.clone()})
        state.apply_moves(target, remote_gids)
        state.curr_comm = target
        moved_per_round.append(int(moved))
        rounds += 1
        if rounds % 2 == 0 and moved_per_round[-1] == 0 \
                and moved_per_round[-2] == 0:
            break

    sub = state.curr_comm
    nsub = int(comm.allreduce_scalar(float((sub == gids).sum())))
    ncomm = int(comm.allreduce_scalar(float(
        (_count_by_community(dg, comm, halo, labels) > 0).sum())))
    return RefineReport(labels=sub, num_communities=ncomm,
                        num_subcommunities=nsub, rounds=rounds,
                        moved_per_round=moved_per_round)
