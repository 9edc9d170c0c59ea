"""Conditions the GPU tests of test_gpu_fused_step.py rely on, shown on the
CPU oracle alone: the computed-gid inputs make every wrong reading of a
global id visible on every kernel route, the fused-aggregate inputs move
vertices on every route and let a vertex without edges decide a community's
size, the R-MAT step inputs reach the hub path and class 6 at the smallest
hub cut, and the hand-built hub segments do what their names say."""

import dataclasses
import functools

import pytest
import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.local_move import local_move_torch

from fused_cases import (GID_BASES, N_ISO, N_TIE, RMAT_STEP_CASES, SEED,
                         SLICES, aggregates_of, computed_gid_inputs, hub_case,
                         hub_lengths, isolated_sizes, routes, span_run,
                         with_isolated, wrong_gid_readings)
from kernel_cases import LADDER, STATES, ladder_inputs

CUTS = (6144, 2049)


# ------------------------------ computed gids ------------------------------

@functools.lru_cache(maxsize=None)
def _gid_case(base):
    inp, L = computed_gid_inputs(torch.float64, base)
    return inp, L, local_move_torch(inp)[0]


@pytest.mark.parametrize("base", GID_BASES)
def test_computed_gid_inputs_keep_the_promise(base):
    inp, L, t = _gid_case(base)
    nv = inp.nv
    assert inp.local_gid_base == base
    assert torch.equal(inp.comm_gid[:nv], base + torch.arange(nv))
    assert inp.comm_gid.unique().numel() == inp.comm_gid.numel()
    remote = inp.comm_gid[nv:]
    assert remote.numel() == 512
    assert bool((inp.comm_size[nv:] == 2).all())
    assert bool((inp.comm_degree[nv:] == 8.0).all())
    # every ghost alone in its remote community
    assert torch.equal(inp.curr_comm[nv:].to(torch.int64),
                       nv + torch.arange(512))
    if base > 0:
        assert int((remote < base).sum()) == 256
        assert int((remote >= base + nv).sum()) == 256
        assert int(inp.comm_gid.argmin()) == nv
        # below the base, yet above every dense id (and above 2^32 where
        # the base is): dropping or truncating the base reorders them
        assert int(remote.min()) > inp.comm_gid.numel()
        if base > 1 << 33:
            assert int(remote.min()) >= 1 << 32
    else:
        assert int(remote.min()) > nv
    # every ladder vertex moves: the tie-break alone picks its target
    assert bool((t[:L].to(torch.int64) != torch.arange(L)).all())


@pytest.mark.parametrize("base", GID_BASES)
def test_wrong_gid_readings_show_on_every_route(base):
    """Each wrong reading of a global id changes at least one ladder target
    in every LDS class (class 0 included), in class 6 at cut 2049 (the
    single degree-2049 row) and on the hub path of both cuts.

    Which readings can show depends on the base. At base 0 a dropped or
    truncated base is the right value, and no id fits below the base, so no
    reading is distinguishable there (that case checks gid_base = 0 itself).
    At 1 << 20 truncation to 32 bits is still the identity. At
    (3 << 32) + 7 all four readings differ from the truth."""
    inp, L, t = _gid_case(base)
    deg = (inp.rowptr[1:] - inp.rowptr[:-1])[:L]
    expect = {0: (),
              1 << 20: ("dense_order", "base_dropped", "nv_as_local"),
              (3 << 32) + 7: ("dense_order", "base_dropped", "truncated",
                              "nv_as_local")}[base]
    for name, gid in wrong_gid_readings(inp, base).items():
        t_w = local_move_torch(dataclasses.replace(inp, comm_gid=gid))[0]
        changed = (t_w != t)[:L]
        for cut in CUTS:
            hit = {r: int((changed & m).sum())
                   for r, m in routes(deg, cut).items()}
            print(f"base={base} {name} cut={cut}: {hit}")
            if name in expect:
                assert all(n >= 1 for n in hit.values()), (name, cut, hit)
        if name not in expect and name != "dense_order":
            assert not bool(changed.any()), name
    if base == 0:
        return
    # the single class-6 row at cut 2049 hinges on comm_gid[nv] itself
    v = LADDER.index(2049)
    assert int(t[v]) == inp.nv


# ---------------------------- fused aggregates -----------------------------

@functools.lru_cache(maxsize=None)
def _iso_case(state):
    base_inp, L = ladder_inputs(torch.float64, state, False, False, SEED)
    t0, _ = local_move_torch(base_inp)
    inp, mover = with_isolated(base_inp, L, t0)
    t, cw = local_move_torch(inp)
    return base_inp, inp, L, mover, t0, t, cw


@pytest.mark.parametrize("state", STATES)
def test_isolated_vertices_shape(state):
    base_inp, inp, L, mover, t0, t, cw = _iso_case(state)
    nv0, nv = base_inp.nv, inp.nv
    assert nv == nv0 + N_ISO
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    assert int((deg == 0).sum()) == N_ISO and bool((deg[nv0:] == 0).all())
    assert bool((inp.v_degree[nv0:] == 0).all())
    # vertices without edges keep their label and a zero cluster weight
    assert torch.equal(t[nv0:], inp.curr_comm[nv0:])
    assert not bool(cw[nv0:].any())
    # the three kinds of label
    lab = inp.curr_comm[nv0:].to(torch.int64)
    assert lab[:3].tolist() == [nv0, nv0 + 1, nv0 + 2]
    assert bool((lab[3:6] < nv0).all())
    assert int(lab[6]) == int(inp.curr_comm[mover]) and mover < L
    assert int(t[mover]) != int(inp.curr_comm[mover])


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("cut", [2049, 6144, 8000])
def test_fused_inputs_move_on_every_route(state, cut):
    """At least one vertex moves in every LDS class and on the hub path
    (singleton state: see below), and vertices without edges decide
    community sizes: every community they belong to would come out smaller
    without the pre-loaded count, and where the labels are singletons at
    least one community loses every other member in the step and keeps its
    new size through such a vertex alone."""
    base_inp, inp, L, mover, t0, t, cw = _iso_case(state)
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    moved = t.to(torch.int64) != inp.curr_comm[:inp.nv].to(torch.int64)
    hit = {r: int((moved & m).sum()) for r, m in routes(deg, cut).items()}
    print(f"{state} cut={cut}: movers per route {hit}")
    if state == "singleton":
        # the singleton guard keeps every class-1 and class-4 vertex of
        # this seed in place (they are accounted all the same: a vertex
        # that stays is added to its own community)
        assert all(n >= 1 for r, n in hit.items()
                   if r not in ("class1", "class4")), hit
    else:
        assert all(n >= 1 for n in hit.values()), hit
    size, degree = aggregates_of(inp, t)
    iso = isolated_sizes(inp)
    assert int(iso.sum()) == N_ISO
    assert int((iso > 0).sum()) >= 5
    assert bool((size >= iso).all())
    alone = (iso > 0) & (size == iso) & (inp.comm_size != size)
    print(f"{state}: communities left to vertices without edges alone: "
          f"{int(alone.sum())}")
    if state in ("singleton", "tied"):
        assert int(alone.sum()) >= 1
    # sizes and degrees do change in the step
    assert not torch.equal(size, inp.comm_size)
    assert int(size.sum()) == inp.nv
    assert float(degree.sum()) == float(inp.v_degree.to(torch.float64).sum())


# ------------------------------ fused R-MAT step ---------------------------

@pytest.mark.parametrize("scale,cut", RMAT_STEP_CASES)
def test_rmat_step_inputs_reach_hub_and_class6(scale, cut):
    """The unit-weight R-MAT graphs of the fused-step test have at least one
    hub at hub cut 2049 and vertices without edges. Class 6 holds the
    degrees in (2048, cut], at cut 2049 the single degree 2049, which no
    vertex of these graphs has (nor of seeds 1-5): that cut checks the hub
    path with the most hubs, and scale 14 at cut 3600 is the case with a
    non-empty class 6 next to a non-empty hub list."""
    g = rmat_graph(scale, 16, seed=3)
    deg = g.rowptr[1:] - g.rowptr[:-1]
    n_hub = int((deg > cut).sum())
    n_c6 = int(((deg > 2048) & (deg <= cut)).sum())
    print(f"s{scale} cut {cut}: max degree {int(deg.max())}, hubs {n_hub}, "
          f"class 6 {n_c6}, isolated {int((deg == 0).sum())}")
    assert int((deg == 0).sum()) >= 1
    assert n_hub >= 1
    if cut == 2049:
        assert n_c6 == 0
    else:
        assert n_c6 >= 1


# ------------------------------- hub slices --------------------------------

@functools.lru_cache(maxsize=None)
def _hub(computed):
    case = hub_case(torch.float64, SLICES, computed)
    t, cw = local_move_torch(case.inp)
    return case, t, cw


@pytest.mark.parametrize("computed", [False, True], ids=["table", "computed"])
def test_hub_segments_do_what_they_say(computed):
    case, t, cw = _hub(computed)
    inp = case.inp
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    lab = inp.curr_comm.to(torch.int64)
    assert sorted({n for _, n in case.specs}) == sorted(set(hub_lengths(SLICES)))
    assert bool((deg[case.nhub:] == 0).all())
    kinds = set()
    for h, (kind, n) in enumerate(case.specs):
        kinds.add(kind)
        assert int(deg[h]) == n and int(lab[h]) == h
        row = inp.tails[inp.rowptr[h]:inp.rowptr[h + 1]].to(torch.int64)
        assert row.unique().numel() == n          # duplicate-free segment
        keys = lab[row]
        w = inp.weights[inp.rowptr[h]:inp.rowptr[h + 1]]
        if kind == "own":
            assert bool((keys == h).all())
            assert int(t[h]) == h and float(cw[h]) == float(w.sum())
        else:
            assert not bool((keys == h).any()) and float(cw[h]) == 0.0
        if kind == "single":
            assert keys.unique().numel() == n
        if kind == "span":
            off, k = span_run(n, SLICES)
            skeys = keys.sort().values
            run = skeys[off]
            assert int((skeys == run).sum()) == k
            pos = (skeys == run).nonzero(as_tuple=True)[0]
            sl = {int(s) for s in range(SLICES)
                  if any(s * n // SLICES <= int(p) < (s + 1) * n // SLICES
                         for p in pos)}
            assert len(sl) >= 3, (n, sl)
            assert int(t[h]) == int(run)
        if kind == "tie":
            skeys = keys.sort().values
            pos_l = (skeys == case.tie_local).nonzero(as_tuple=True)[0]
            pos_r = (skeys == case.tie_remote).nonzero(as_tuple=True)[0]
            assert pos_l.numel() == N_TIE and pos_r.numel() == N_TIE
            sl_l = {s for s in range(SLICES) for p in pos_l.tolist()
                    if s * n // SLICES <= p < (s + 1) * n // SLICES}
            sl_r = {s for s in range(SLICES) for p in pos_r.tolist()
                    if s * n // SLICES <= p < (s + 1) * n // SLICES}
            assert len(sl_l) == 2 and len(sl_r) == 1     # stitched, interior
            assert case.tie_remote > case.tie_local
            assert int(inp.comm_gid[case.tie_remote]) < \
                int(inp.comm_gid[case.tie_local])
            assert int(t[h]) == case.tie_remote
            t_dense = local_move_torch(dataclasses.replace(
                inp, comm_gid=torch.arange(inp.comm_gid.numel())))[0]
            assert int(t_dense[h]) == case.tie_local
    assert kinds == {"own", "absent", "single", "span", "tie"}
    if computed:
        assert torch.equal(inp.comm_gid[:inp.nv],
                           inp.local_gid_base + torch.arange(inp.nv))
    else:
        assert inp.local_gid_base is None
    # some hubs move and some stay: both stores of the final kernel
    moved = t[:case.nhub].to(torch.int64) != torch.arange(case.nhub)
    assert 0 < int(moved.sum()) < case.nhub
