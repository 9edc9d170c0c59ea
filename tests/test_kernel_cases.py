"""Conditions the GPU edge tests (test_gpu_kernel_edges.py) rely on, shown
on the CPU oracle alone: the ladder inputs of kernel_cases.py give exact,
dtype-independent oracle answers, populate every degree class and both
sides of the hub cut, and make the global-id tie-break matter."""

import functools

import pytest
import torch

from cuvite_amd.local_move import local_move_pydict, local_move_torch

from kernel_cases import (LADDER, STATES, ladder_inputs, move_inputs_to,
                          with_arange_gid)

SEED = 20
CASES = [(state, ghosts, unit)
         for state in STATES
         for ghosts in (False, True)     # (ghosts, dup) in {(F,F), (T,T)}
         for unit in (False, True)]
_ids = [f"{s}-{'ghostdup' if g else 'plain'}-{'unit' if u else 'w1to4'}"
        for s, g, u in CASES]


@functools.lru_cache(maxsize=None)
def _case(state, ghosts, unit, wdtype=torch.float64):
    inp, L = ladder_inputs(wdtype, state, ghosts, ghosts, SEED, unit=unit)
    return inp, L, local_move_torch(inp)


@pytest.mark.parametrize("state,ghosts,unit", CASES, ids=_ids)
def test_torch_matches_pydict_exact(state, ghosts, unit):
    inp, _, (t_vec, cw_vec) = _case(state, ghosts, unit)
    t_ref, cw_ref = local_move_pydict(inp)
    assert torch.equal(t_ref, t_vec)
    assert torch.equal(cw_ref, cw_vec)


@pytest.mark.parametrize("state,ghosts,unit", CASES, ids=_ids)
def test_fp32_build_matches_fp64(state, ghosts, unit):
    _, _, (t64, cw64) = _case(state, ghosts, unit)
    inp32, _, (t32, cw32) = _case(state, ghosts, unit, torch.float32)
    assert inp32.weights.dtype == torch.float32
    assert cw32.dtype == torch.float32
    assert torch.equal(t32, t64)
    assert torch.equal(cw32.to(torch.float64), cw64)


@pytest.mark.parametrize("state,ghosts,unit", CASES, ids=_ids)
def test_ladder_degrees_and_shapes(state, ghosts, unit):
    inp, L, _ = _case(state, ghosts, unit)
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    assert deg[:L].tolist() == list(LADDER)
    nv = inp.nv
    assert int((deg > 6144).sum()) == 4 and int((deg > 8000).sum()) == 1
    assert int(deg[L:].min()) >= 1
    assert int(inp.comm_gid.min()) > 1 << 32
    assert inp.comm_gid.unique().numel() == inp.comm_gid.numel()
    if ghosts:
        # distributed shape: ghost tails, labels longer than nv, nc > nv
        assert int(inp.tails.max()) >= nv
        assert inp.curr_comm.numel() > nv
        assert inp.comm_size.numel() > nv
        assert int(inp.curr_comm[nv:].min()) >= nv
        assert bool((inp.comm_size[nv:] == 1).any())
        # duplicate neighbours and a self-loop on every ladder row >= 8
        for v in (3, L - 1):
            row = inp.tails[inp.rowptr[v]:inp.rowptr[v + 1]].to(torch.int64)
            assert int((row == v).sum()) == 1
            assert row.unique().numel() == \
                LADDER[v] - max(LADDER[v] // 8 - 1, 0)
    else:
        assert int(inp.tails.max()) < nv
        assert inp.curr_comm.numel() == nv
        row = inp.tails[inp.rowptr[L - 1]:inp.rowptr[L]]
        assert row.unique().numel() == LADDER[-1]


@pytest.mark.parametrize("state,ghosts,unit",
                         [c for c in CASES if c[0] in ("singleton", "random")],
                         ids=[i for c, i in zip(CASES, _ids)
                              if c[0] in ("singleton", "random")])
def test_gid_permutation_changes_answer(state, ghosts, unit):
    """A kernel that compared dense ids where it must compare global ids
    (or truncated the gid) would compute the arange-gid answer; it must
    differ from the real one often enough to be seen. In these two states
    nearly all of the difference comes from the singleton guard."""
    inp, L, (t, _) = _case(state, ghosts, unit)
    t_id, _ = local_move_torch(with_arange_gid(inp))
    diff = t != t_id
    n, n_lad = int(diff.sum()), int(diff[:L].sum())
    print(f"targets changed by arange gid: {n} (ladder: {n_lad})")
    if state == "singleton":
        assert n >= 1000
        assert n_lad >= 10
    else:
        assert n >= 100


@pytest.mark.parametrize("unit", [False, True], ids=["w1to4", "unit"])
def test_tied_state_hinges_on_tie_break(unit):
    """In the `tied` state (plain shape) the guard is off for every ladder
    vertex, all of them move, and with the dense-id order in place of the
    global-id order the chosen target changes in every degree class, on
    both sides of the default cut and on the hub path of every cut."""
    inp, L, (t, _) = _case("tied", False, unit)
    assert bool((t[:L].to(torch.int64) != torch.arange(L)).all())
    assert bool((inp.comm_size[t[:L].to(torch.int64)] == 2).all())
    t_id, _ = local_move_torch(with_arange_gid(inp))
    changed = {LADDER[v] for v in
               (t != t_id)[:L].nonzero(as_tuple=True)[0].tolist()}
    print(f"ladder degrees whose target hinges on the tie-break: "
          f"{sorted(changed)}")
    lo = 16
    for hi in (64, 256, 512, 1024, 2048, 6144, 8000, 8001):
        assert any(lo < d <= hi for d in changed), (lo, hi)
        lo = hi


@pytest.mark.parametrize("state,ghosts,unit", CASES, ids=_ids)
def test_hub_sort_fallback_matches_oracle(state, ghosts, unit):
    """ops._hub_moves_sorted on CPU tensors is the torch-sort fallback."""
    from cuvite_amd import ops
    inp, _, (t_ref, cw_ref) = _case(state, ghosts, unit)
    inp = move_inputs_to(inp, torch.device("cpu"))
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    hubs = (deg > 6144).nonzero(as_tuple=True)[0]
    assert [LADDER[int(h)] for h in hubs] == [6145, 7999, 8000, 8001]
    ops.clear_phase_caches()
    try:
        tgt, cw = ops._hub_moves_sorted(inp, hubs, deg[hubs])
    finally:
        ops.clear_phase_caches()
    assert torch.equal(tgt, t_ref[hubs])
    assert torch.equal(cw, cw_ref[hubs])
