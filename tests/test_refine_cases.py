"""Conditions the GPU refine test (test_gpu_refine.py) relies on, shown on
the CPU oracle alone: the refine cases of refine_cases.py make the bound
filter, the ineligible candidates, the vertices without a candidate and the
non-movers decide the answer on every route, and the torch twin equals the
dict golden model bit for bit."""

import functools

import pytest
import torch

from cuvite_amd.local_move import refine_move_pydict, refine_move_torch

from kernel_cases import LADDER
from refine_cases import CASES, N_BOUNDS, refine_case

SHAPES = [False, True]
_sh = {False: "plain", True: "ghostdup"}.get
# upper ends of the routes at the default hub cut: the seven LDS classes
# and the hub pipeline (at cut 2049, which the GPU test also runs, the last
# two are both hub vertices, all but the deg-2049 one)
ROUTES = (16, 64, 256, 512, 1024, 2048, 6144, 8001)


@functools.lru_cache(maxsize=None)
def _case(name, ghostdup, wdtype=torch.float64):
    inp, L, mover, cand, unfiltered = refine_case(name, wdtype, ghostdup)
    return inp, L, mover, cand, unfiltered, refine_move_torch(inp, mover,
                                                              cand)


def _routes_hit(vertices):
    """Which degree routes the given ladder vertices cover."""
    degs = [LADDER[v] for v in vertices]
    hit, lo = [], 0
    for hi in ROUTES:
        hit.append(any(lo < d <= hi for d in degs))
        lo = hi
    return hit


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
def test_torch_matches_pydict_exact(name, ghostdup):
    inp, _, mover, cand, _, (t, cw) = _case(name, ghostdup)
    t_ref, cw_ref = refine_move_pydict(inp, mover, cand)
    assert t.dtype == t_ref.dtype and cw.dtype == cw_ref.dtype
    assert torch.equal(t, t_ref)
    assert torch.equal(cw, cw_ref)


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
def test_fp32_build_matches_fp64(name, ghostdup):
    _, _, _, _, _, (t64, cw64) = _case(name, ghostdup)
    inp32, _, _, _, _, (t32, cw32) = _case(name, ghostdup, torch.float32)
    assert inp32.weights.dtype == torch.float32 and cw32.dtype == torch.float32
    assert torch.equal(t32, t64)
    assert torch.equal(cw32.to(torch.float64), cw64)


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
def test_every_move_respects_the_bounds(name, ghostdup):
    """A vertex that changed its label was a mover and joined an eligible
    community of its own bound; everyone else kept (label, 0)."""
    inp, _, mover, cand, _, (t, cw) = _case(name, ghostdup)
    nv = inp.nv
    own = inp.curr_comm[:nv]
    moved = t != own
    assert int(moved.sum()) > 100
    assert bool((mover[moved] >= 0).all())
    assert torch.equal(cand[t[moved].to(torch.int64)], mover[moved])
    still = mover < 0
    assert int(still.sum()) > 100
    assert torch.equal(t[still], own[still])
    assert not bool(cw[still].any())
    assert bool((cw[~still] >= 0).all())


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
def test_foreign_bound_changes_the_answer_on_every_route(ghostdup):
    """Even ladder vertices: the unfiltered winner lies in a foreign bound,
    so a kernel without the filter returns it; with the filter they still
    move, elsewhere. Every route has such a vertex."""
    inp, L, mover, cand, unf, (t, _) = _case("foreign", ghostdup)
    t = t.to(torch.int64)
    own = inp.curr_comm[:L].to(torch.int64)
    lad = torch.arange(L)
    hinge = (lad % 2 == 0) & (unf[:L] != own) & (t[:L] != unf[:L])
    assert bool((cand[unf[:L]][hinge] != mover[:L][hinge]).all())
    assert all(_routes_hit(hinge.nonzero(as_tuple=True)[0].tolist()))
    # and they do not simply stay: most find another tied neighbour
    went = hinge & (t[:L] != own)
    assert sum(_routes_hit(went.nonzero(as_tuple=True)[0].tolist())) >= 7
    # odd ladder vertices keep the unfiltered winner
    odd = lad % 2 == 1
    assert torch.equal(t[:L][odd], unf[:L][odd])


def test_ineligible_winner_changes_the_answer_on_every_route():
    inp, L, mover, cand, unf, (t, _) = _case("ineligible", False)
    t = t.to(torch.int64)
    lad = torch.arange(L)
    odd = lad % 2 == 1
    assert bool((cand[unf[:L]][odd] == -1).all())
    hinge = odd & (t[:L] != unf[:L])
    assert torch.equal(hinge, odd)
    assert all(_routes_hit(hinge.nonzero(as_tuple=True)[0].tolist()))
    # the same vertices took that winner while it was eligible
    t_for = _case("foreign", False)[5][0].to(torch.int64)
    assert torch.equal(t_for[:L][odd], unf[:L][odd])


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
def test_vertex_without_candidate_stays(ghostdup):
    inp, L, mover, cand, unf, (t, cw) = _case("none", ghostdup)
    lad = torch.arange(L)
    lone = lad % 3 == 0
    assert bool((mover[:L][lone] == N_BOUNDS).all())
    assert not bool((cand == N_BOUNDS).any())
    assert torch.equal(t[:L][lone], inp.curr_comm[:L][lone])
    # they were movers: their own-community weight is reported
    assert all(_routes_hit(lone.nonzero(as_tuple=True)[0].tolist()))
    # without the filter they would have moved
    assert bool((unf[:L][lone] != inp.curr_comm[:L][lone].to(torch.int64))
                .any())


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
def test_non_movers_sit_beside_movers(ghostdup):
    """Every second ladder vertex stays while its neighbours in the class
    lists move, and the class-0 pool groups of four hold two movers and two
    non-movers each (positions in the class-0 list, which is ascending in
    the vertex id: pool vertices are consecutive)."""
    inp, L, mover, cand, unf, (t, _) = _case("nonmovers", ghostdup)
    nv = inp.nv
    own = inp.curr_comm[:nv]
    lad = torch.arange(L)
    assert bool((mover[:L][lad % 2 == 1] == -1).all())
    assert bool((mover[:L][lad % 2 == 0] >= 0).all())
    moved = t != own
    assert int(moved[:L][lad % 2 == 0].sum()) >= L // 2 - 2
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    cls0 = ((deg > 0) & (deg <= 16)).nonzero(as_tuple=True)[0]
    pool0 = cls0[cls0 >= L]
    assert pool0.numel() > 4000
    pos = torch.searchsorted(cls0, pool0)
    pat = (mover[pool0] >= 0).to(torch.int64)
    # groups of four positions that are four consecutive pool vertices
    full = ((pos % 4 == 0)[:-3] & (pool0[3:] - pool0[:-3] == 3)) \
        .nonzero(as_tuple=True)[0]
    assert full.numel() > 500
    per_group = pat[full] + pat[full + 1] + pat[full + 2] + pat[full + 3]
    assert bool((per_group == 2).all())
    # and movers in such groups do move
    assert int(moved[pool0].sum()) > 500


@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
def test_hub_sort_fallback_matches_twin(name, ghostdup):
    """ops._hub_moves_sorted on CPU tensors is the torch-sort fallback; with
    the bound pair it is the refine round's hub path behind
    CUVITE_HUB_SEGSORT=0."""
    from cuvite_amd import ops
    inp, _, mover, cand, _, (t_ref, cw_ref) = _case(name, ghostdup)
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    hubs = (deg > 2049).nonzero(as_tuple=True)[0]
    assert hubs.numel() == 8
    ops.clear_phase_caches()
    try:
        tgt, cw = ops._hub_moves_sorted(inp, hubs, deg[hubs], None,
                                        (mover, cand))
    finally:
        ops.clear_phase_caches()
    assert torch.equal(tgt, t_ref[hubs])
    assert torch.equal(cw, cw_ref[hubs])
