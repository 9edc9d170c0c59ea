"""The HIP local-move kernels with computed global ids, with the community
aggregates accounted where the targets are stored, and with the hub argmax
read straight from the sorted pairs.

All data is integer-valued (kernel_cases.py, fused_cases.py), so every
comparison is torch.equal against the CPU oracle, no tolerance.
tests/test_fused_cases.py shows on the CPU that the inputs have the
properties relied on here."""

import functools

import pytest
import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import single_partition
from cuvite_amd.local_move import local_move_torch
from cuvite_amd.louvain import (LouvainConfig, PhaseState, _modularity,
                                _one_sweep, _pick_move_fn)
from cuvite_amd.parallel import Comm

from fused_cases import (GID_BASES, RMAT_STEP_CASES, SEED, SLICES,
                         aggregates_of, computed_gid_inputs, hub_case,
                         isolated_sizes, with_isolated)
from kernel_cases import STATES, ladder_inputs, move_inputs_to

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
SENTINEL, PAD = -7, 64


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _assert_same(got, ref, what=""):
    t, cw = got[0].cpu(), got[1].cpu()
    assert t.dtype == ref[0].dtype and cw.dtype == ref[1].dtype
    bad = ((t != ref[0]) | (cw != ref[1])).nonzero(as_tuple=True)[0]
    assert bad.numel() == 0, (f"{what}: {bad.numel()} vertices differ from "
                              f"the oracle, first {bad[:20].tolist()}")


# ------------------------------ computed gids ------------------------------

@functools.lru_cache(maxsize=None)
def _gid_case(wdtype, base):
    inp, L = computed_gid_inputs(wdtype, base)
    return inp, local_move_torch(inp)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("cut", [6144, 2049])
@pytest.mark.parametrize("base", GID_BASES)
def test_computed_gids_match_oracle(ops, dev, monkeypatch, base, cut, wdtype):
    """ops.local_move with local_gid_base: the kernels compute base + y for
    the local communities and read comm_gid for the remote ones. Every
    ladder target hinges on the global-id tie-break, on every route."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    inp_cpu, ref = _gid_case(wdtype, base)
    inp = move_inputs_to(inp_cpu, dev)
    assert inp.local_gid_base == base
    _assert_same(ops.local_move(inp), ref, f"base {base} cut {cut}")


# ---------------------------- fused aggregates -----------------------------

@functools.lru_cache(maxsize=None)
def _iso_case(wdtype, state):
    base_inp, L = ladder_inputs(wdtype, state, False, False, SEED)
    t0, _ = local_move_torch(base_inp)
    inp, _ = with_isolated(base_inp, L, t0)
    t, cw = local_move_torch(inp)
    size, degree = aggregates_of(inp, t)
    return inp, (t, cw), size, degree, isolated_sizes(inp)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("variant", ["cut2049", "cut6144", "cut8000",
                                     "four_hub_groups"])
def test_fused_aggregates_kernel_level(ops, dev, monkeypatch, variant, state,
                                       wdtype):
    """The next_* buffers end up as bincount / index_add_ of the oracle's
    targets over ALL vertices (the vertices without edges come from the
    pre-loaded count), targets and cw equal the unfused call's, and the
    sentinels around the buffer slices stay intact."""
    if variant == "four_hub_groups":
        monkeypatch.setattr(ops, "_HUB_SORT_CHUNK", 9000)
    else:
        monkeypatch.setenv("CUVITE_HUB_CUT", variant[3:])
    inp_cpu, ref, size_ref, degree_ref, iso = _iso_case(wdtype, state)
    inp = move_inputs_to(inp_cpu, dev)
    nc = inp.comm_size.numel()
    t0, cw0 = ops.local_move(inp)
    _assert_same((t0, cw0), ref, "unfused")
    size_buf = torch.full((nc + 2 * PAD,), SENTINEL, dtype=torch.int64,
                          device=dev)
    deg_buf = torch.full((nc + 2 * PAD,), SENTINEL, dtype=wdtype, device=dev)
    nsize, ndegree = size_buf[PAD:PAD + nc], deg_buf[PAD:PAD + nc]
    assert nsize.is_contiguous() and ndegree.is_contiguous()
    nsize.copy_(iso.to(dev))
    ndegree.zero_()
    size_in, degree_in = inp.comm_size.clone(), inp.comm_degree.clone()
    t1, cw1 = ops.local_move(inp, next_size=nsize, next_degree=ndegree)
    if variant == "four_hub_groups":
        _, hubs, hdeg = ops._buckets_for(inp.rowptr)
        assert len(ops._hub_groups(inp, hubs, hdeg)) == 4
    assert torch.equal(t0, t1) and torch.equal(cw0, cw1)
    assert torch.equal(nsize.cpu(), size_ref)
    assert ndegree.dtype == wdtype
    assert torch.equal(ndegree.cpu(), degree_ref.to(wdtype))
    for buf in (size_buf, deg_buf):
        assert bool((buf[:PAD] == SENTINEL).all())
        assert bool((buf[-PAD:] == SENTINEL).all())
    # the pair the kernels read is not written
    assert torch.equal(inp.comm_size, size_in)
    assert torch.equal(inp.comm_degree, degree_in)


# --------------------------- fused step vs unfused -------------------------

def _unit_rmat(scale):
    g = rmat_graph(scale, 16, seed=3)
    g.weights.fill_(1.0)
    return g


def _run_steps(g, dev, backend, n_steps):
    """Drive PhaseState / _one_sweep / _modularity the way bench.py does."""
    dg = single_partition(g.to(dev))
    cfg = LouvainConfig(backend=backend)
    state = PhaseState(dg, Comm(dev))
    state.use_hip = dev.type == "cuda" and backend in ("auto", "hip")
    move_fn = _pick_move_fn(cfg, dev)
    out = []
    for _ in range(n_steps):
        target = _one_sweep(state, cfg, move_fn, None)
        q = _modularity(state)
        state.past_comm, state.curr_comm = state.curr_comm, target
        out.append((state.curr_comm.cpu().clone(),
                    state.local_size.cpu().clone(),
                    state.local_degree.cpu().clone(),
                    state.cluster_weight.cpu().clone(), q))
    return out, state


@functools.lru_cache(maxsize=None)
def _cpu_steps(scale):
    out, _ = _run_steps(_unit_rmat(scale), torch.device("cpu"), "torch", 4)
    return out[-1]


@pytest.mark.parametrize("scale,cut", RMAT_STEP_CASES)
def test_fused_step_matches_unfused_step(ops, dev, monkeypatch, scale, cut):
    """Four consecutive steps, default (fused) against CUVITE_FUSED_AGG=0:
    labels, aggregates, cluster weights and Q bit-identical after every
    step (unit weights: every sum is an exact integer in any order), and
    equal to the torch backend on the CPU after the last one."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    g = _unit_rmat(scale)
    monkeypatch.delenv("CUVITE_FUSED_AGG", raising=False)
    fused, st = _run_steps(g, dev, "hip", 4)
    assert st._agg_spare is not None          # the fused path did run
    assert int(st._iso_size.sum()) >= 1
    ops.clear_phase_caches()
    monkeypatch.setenv("CUVITE_FUSED_AGG", "0")
    unfused, st0 = _run_steps(g, dev, "hip", 4)
    assert st0._agg_spare is None
    for i, (a, b) in enumerate(zip(fused, unfused)):
        for x, y, name in zip(a[:4], b[:4], ("curr_comm", "local_size",
                                             "local_degree",
                                             "cluster_weight")):
            assert torch.equal(x, y), (i, name)
        assert a[4] == b[4], (i, a[4], b[4])
    ref = _cpu_steps(scale)
    for x, y, name in zip(fused[-1][:4], ref[:4],
                          ("curr_comm", "local_size", "local_degree",
                           "cluster_weight")):
        assert torch.equal(x, y), name
    assert fused[-1][4] == ref[4]
    assert torch.equal(fused[-1][1],
                       torch.bincount(fused[-1][0], minlength=g.nv))


# ------------------------------- hub slices --------------------------------

@functools.lru_cache(maxsize=None)
def _hub(wdtype, computed):
    case = hub_case(wdtype, SLICES, computed)
    return case, local_move_torch(case.inp)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("computed", [False, True], ids=["table", "computed"])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "accounted"])
def test_hub_moves_binding_on_hand_built_segments(ops, dev, fused, computed,
                                                  wdtype):
    """hub_moves called directly on flat segments of lengths 1, 2, 63, 64,
    65, slices - 1, slices, slices + 1 and 64 * slices + 1 (own-community
    run, own community absent, all singletons, a winning run over three
    slices, a tie between a stitched and an interior run): targets and cw
    per hub equal local_move_torch on the MoveInputs the arrays describe,
    with an arbitrary comm_gid table (n_local = 0) and with computed gids."""
    ext = ops._require()
    assert ext.hub_slices() == SLICES
    case, (t_ref, cw_ref) = _hub(wdtype, computed)
    inp = move_inputs_to(case.inp, dev)
    nhub, nv = case.nhub, inp.nv
    eoffs = inp.rowptr[:nhub + 1].contiguous()
    ne = int(eoffs[-1])
    kw = {}
    if computed:
        kw.update(gid_base=inp.local_gid_base, n_local=nv)
    nc = inp.comm_size.numel()
    if fused:
        nsize = torch.zeros(nc, dtype=torch.int64, device=dev)
        ndegree = torch.zeros(nc, dtype=wdtype, device=dev)
        kw.update(next_size=nsize, next_degree=ndegree)
    tgt, cw = ext.hub_moves(
        inp.tails[:ne].contiguous(), inp.weights[:ne].contiguous(), eoffs,
        torch.arange(nhub, dtype=torch.int32, device=dev),
        torch.zeros(nhub, dtype=torch.float64, device=dev), inp.curr_comm,
        inp.v_degree, inp.comm_size, inp.comm_degree, inp.comm_gid,
        float(inp.constant), **kw)
    tgt, cw = tgt.cpu(), cw.cpu()
    assert cw.dtype == wdtype
    bad = [(case.specs[h], int(tgt[h]), int(t_ref[h]), float(cw[h]),
            float(cw_ref[h]))
           for h in range(nhub)
           if int(tgt[h]) != int(t_ref[h]) or float(cw[h]) != float(cw_ref[h])]
    assert not bad, bad[:10]
    if fused:
        t64 = t_ref[:nhub].to(torch.int64)
        assert torch.equal(nsize.cpu(), torch.bincount(t64, minlength=nc))
        deg_ref = torch.zeros(nc, dtype=torch.float64).index_add_(
            0, t64, case.inp.v_degree[:nhub].to(torch.float64))
        assert torch.equal(ndegree.cpu(), deg_ref.to(wdtype))
