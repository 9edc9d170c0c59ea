"""CPU-only input builders for the refine-move tests (one Leiden refinement
round: `local_move.refine_move_*`, `ops.refine_move`).

Everything here is plain torch on the CPU: no GPU, no `cuvite_amd.ops`
import. `tests/test_refine_cases.py` checks on the oracle alone that these
inputs have the properties the GPU test relies on; `tests/
test_gpu_refine.py` feeds them to the HIP kernels.

The inputs are `kernel_cases.ladder_inputs` (one vertex at every degree
where the routing changes, integer weights, power-of-two `constant`, so
every gain is exact and every comparison is torch.equal) plus the two bound
arrays of a refine round:

  mover_bound int32 [nv]  bound of a vertex that moves, -1: it does not
  cand_bound  int32 [nc]  bound of a community that may be joined, -1: not

Cases, each with and without ghosts (ghosts come with `dup` parallel edges
and self-loops, the `ghostdup` shape of the kernel edge tests):

  foreign     `tied` state, the pool communities (and the remote ones)
              spread over three bounds. Without a filter every ladder
              vertex takes the lowest-gid neighbour among its tied best
              (`unfiltered`); the even ladder vertices are given a bound
              other than that neighbour's, so a kernel that drops the
              filter is wrong on them, on every route. Pool vertices move
              with their own community's bound, except two of every four.
  ineligible  the same, and for the odd ladder vertices (whose unfiltered
              winner has their bound) that winner is made ineligible
              (cand_bound = -1).
  none        the same as `foreign`, but every third ladder vertex has
              bound 3, which no community has: it stays.
  nonmovers   the same as `foreign`, but every second ladder vertex does not
              move (mover_bound = -1), next to the class-0 pool groups in
              which two of four do not move.
  random      `random` state (communities with several members, many
              candidates per vertex), random bounds, a random half moves.
"""

from __future__ import annotations

import torch

from cuvite_amd.local_move import local_move_torch

from kernel_cases import ladder_inputs

CASES = ("foreign", "ineligible", "none", "nonmovers", "random")
N_BOUNDS = 3
SEED = 20


def refine_case(name: str, wdtype, ghostdup: bool):
    """Returns (MoveInputs on CPU, L, mover_bound int32 [nv], cand_bound
    int32 [nc], unfiltered int64 [nv]): `unfiltered` is the plain local
    move's target on the same inputs."""
    assert name in CASES
    state = "random" if name == "random" else "tied"
    inp, L = ladder_inputs(wdtype, state, ghostdup, ghostdup, SEED)
    nv, nc = inp.nv, inp.comm_size.numel()
    g = torch.Generator().manual_seed(77)
    unfiltered = local_move_torch(inp)[0].to(torch.int64)
    cand = torch.randint(0, N_BOUNDS, (nc,), generator=g).to(torch.int32)
    own = inp.curr_comm[:nv].to(torch.int64)
    if name == "random":
        mover = cand[own].clone()
        mover[torch.rand(nv, generator=g) < 0.5] = -1
        return inp, L, mover, cand, unfiltered

    # pool vertices: their own community's bound, two of every four stay
    mover = cand[own].clone()
    pool = torch.arange(L, nv)
    mover[pool[((pool - L) % 4 == 1) | ((pool - L) % 4 == 2)]] = -1
    lad = torch.arange(L)
    win = cand[unfiltered[:L]]
    # even ladder vertices: a bound other than their unfiltered winner's
    mover[:L] = torch.where(lad % 2 == 0, (win + 1) % N_BOUNDS, win)
    if name == "ineligible":
        odd = lad[lad % 2 == 1]
        cand[unfiltered[odd]] = -1
    elif name == "none":
        mover[lad[lad % 3 == 0]] = N_BOUNDS
    elif name == "nonmovers":
        mover[lad[lad % 2 == 1]] = -1
    return inp, L, mover, cand, unfiltered
