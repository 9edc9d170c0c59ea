"""Conditions the class-schedule GPU tests (test_gpu_class_schedule.py) rely
on, shown on the CPU oracle alone: the pipeline ladder holds every listed
degree once and populates every class and the hub path, its answers are
exact and dtype-independent, its `tied` state hinges on the tie-break, and
the crowded graph fills the block classes."""

import dataclasses
import functools

import pytest
import torch

from cuvite_amd.local_move import local_move_pydict, local_move_torch

from fused_cases import aggregates_of, isolated_sizes, with_isolated
from schedule_cases import (BLOCK_WIDTHS, CLASS_BOUNDS, CROWDED_GROUPS,
                            CROWDED_HUBS, CUT, LADDER, N_POOL, STATES,
                            class_counts, crowded, pipeline_ladder)


@functools.lru_cache(maxsize=None)
def _ladder(state, dup, wdtype=torch.float64):
    inp, L = pipeline_ladder(wdtype, state, dup)
    return inp, L, local_move_torch(inp)


@functools.lru_cache(maxsize=None)
def _crowded(state, wdtype=torch.float64):
    inp, L = crowded(wdtype, state)
    return inp, L, local_move_torch(inp)


def test_ladder_lists_every_live_slot_change():
    assert len(set(LADDER)) == len(LADDER)
    for stride, lo, hi in ((16, 1, 16), (64, 17, 512)) + tuple(
            (b, 513, CUT) for b in BLOCK_WIDTHS):
        for k in range(1, 6):
            for d in (k * stride - 1, k * stride, k * stride + 1):
                if lo <= d <= hi:
                    assert d in LADDER, (stride, k, d)
    for b in CLASS_BOUNDS + (CUT,):
        assert b in LADDER and b + 1 in LADDER


@pytest.mark.parametrize("dup", [False, True], ids=["plain", "dup"])
@pytest.mark.parametrize("state", STATES)
def test_ladder_degrees_once_and_all_routes(state, dup):
    inp, L, _ = _ladder(state, dup)
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    assert deg[:L].tolist() == list(LADDER)         # each exactly once
    assert int(deg[L:].max()) <= CLASS_BOUNDS[1]    # pool: low classes
    assert int(deg[L:].min()) >= 1
    counts = class_counts(inp)
    assert all(c > 0 for c in counts), counts
    assert counts[-1] == 1                          # the deg CUT + 1 row
    if dup:
        for v in (LADDER.index(15), L - 1):
            row = inp.tails[inp.rowptr[v]:inp.rowptr[v + 1]].to(torch.int64)
            assert int((row == v).sum()) == 1
            assert row.unique().numel() == \
                LADDER[v] - max(LADDER[v] // 8 - 1, 0)


@pytest.mark.parametrize("dup", [False, True], ids=["plain", "dup"])
@pytest.mark.parametrize("state", STATES)
def test_ladder_oracle_exact_and_dtype_independent(state, dup):
    inp, _, (t64, cw64) = _ladder(state, dup)
    t_ref, cw_ref = local_move_pydict(inp)
    assert torch.equal(t_ref, t64) and torch.equal(cw_ref, cw64)
    _, _, (t32, cw32) = _ladder(state, dup, torch.float32)
    assert cw32.dtype == torch.float32
    assert torch.equal(t32, t64)
    assert torch.equal(cw32.to(torch.float64), cw64)


def test_ladder_tied_state_hinges_on_tie_break():
    """Every ladder vertex moves into a size-2 pool community, and with the
    dense-id order in place of the global-id order the target changes in
    every degree class and on the hub path."""
    inp, L, (t, _) = _ladder("tied", False)
    assert bool((t[:L].to(torch.int64) != torch.arange(L)).all())
    assert bool((inp.comm_size[t[:L].to(torch.int64)] == 2).all())
    by_dense = dataclasses.replace(
        inp, comm_gid=torch.arange(inp.comm_gid.numel(), dtype=torch.int64))
    t_id, _ = local_move_torch(by_dense)
    changed = {LADDER[v] for v in
               (t != t_id)[:L].nonzero(as_tuple=True)[0].tolist()}
    lo = 1
    for hi in CLASS_BOUNDS + (CUT, CUT + 1):
        assert any(lo < d <= hi for d in changed), (lo, hi)
        lo = hi


@pytest.mark.parametrize("state", STATES)
def test_crowded_fills_the_block_classes(state):
    inp, L, (t64, cw64) = _crowded(state)
    counts = class_counts(inp)
    want = {6: CROWDED_GROUPS[0][0], 5: CROWDED_GROUPS[1][0],
            4: CROWDED_GROUPS[2][0], 2: CROWDED_GROUPS[3][0],
            0: CROWDED_GROUPS[4][0], 7: len(CROWDED_HUBS)}
    for c, n in want.items():
        assert counts[c] == n, (c, counts)
    assert 3_500_000 <= inp.tails.numel() <= 4_500_000
    tails = inp.tails.to(torch.int64)
    seg = torch.repeat_interleave(torch.arange(inp.nv),
                                  inp.rowptr[1:] - inp.rowptr[:-1])
    other = tails != seg
    assert int(tails[other].min()) >= L
    assert int(tails[other].max()) < L + N_POOL
    assert int((~other).sum()) >= 1000              # self-loops
    # something moves on every route
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    moved = t64.to(torch.int64) != inp.curr_comm.to(torch.int64)
    for lo, hi in ((0, 16), (64, 256), (512, 1024), (1024, 2048),
                   (2048, CUT), (CUT, 1 << 20)):
        assert bool(moved[(deg > lo) & (deg <= hi)].any()), (state, lo, hi)


def test_crowded_oracle_dtype_independent():
    _, _, (t64, cw64) = _crowded("random")
    _, _, (t32, cw32) = _crowded("random", torch.float32)
    assert torch.equal(t32, t64)
    assert torch.equal(cw32.to(torch.float64), cw64)


def test_crowded_with_isolated_aggregates():
    """The fused-aggregate GPU test appends the isolated vertices of
    fused_cases.with_isolated: the aggregates then count every vertex once
    and stay exact integers in fp32."""
    inp0, L, (t0, _) = _crowded("random")
    inp, mover = with_isolated(inp0, L, t0)
    assert mover < L
    t, _ = local_move_torch(inp)
    size, degree = aggregates_of(inp, t)
    assert int(size.sum()) == inp.nv
    assert int(isolated_sizes(inp).sum()) == inp.nv - inp0.nv
    assert float(degree.max()) < float(1 << 24)
    assert torch.equal(degree, degree.round())
