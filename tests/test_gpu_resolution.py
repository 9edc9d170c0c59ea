"""The HIP kernels at a resolution other than 1: gamma reaches them through
`constant` = gamma / (2m), an argument they have only ever seen near 1/(2m),
where the degree term of the gain decides few argmaxes. Here it is scaled by
0.25, 64 and 1024 on the ladder inputs, where it decides thousands
(tests/test_resolution.py shows that on the CPU, for every route), and the
kernels are held to their torch twins bit for bit. Then exact scoring and
whole runs at gamma = 0.5 and 2 against the CPU oracle, on one rank and on
two ranks sharing the GPU.

All data is integer-valued and every scaled constant is a power of two
(resolution_cases.py), so every kernel comparison is torch.equal; the whole
runs use unit weights, so labels and sweep counts are compared exactly."""

import functools

import pytest
import torch

from cuvite_amd import (affected_vertices, apply_edge_batch,
                        partition_quality, resolution_scan)
from cuvite_amd.graph import single_partition
from cuvite_amd.local_move import refine_move_torch
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

from tests.dist_utils import run_dist

import dynamic_cases as dyc
import resolution_cases as rc
import vcycle_cases as vc
from fused_cases import aggregates_of
from kernel_cases import move_inputs_to
from quality_cases import shard
from refine_cases import CASES, refine_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
SHAPES = [False, True]
_sh = {False: "plain", True: "ghostdup"}.get
CUTS = [2049, 6144]
RUN_GAMMAS = [0.5, 2.0]
RUN_GRAPHS = ["karate", "rggu", "rmat10u"]


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _assert_same(got, ref, inp_cpu, what):
    t, cw = got[0].cpu(), got[1].cpu()
    t_ref, cw_ref = ref
    assert t.dtype == t_ref.dtype and cw.dtype == cw_ref.dtype
    if torch.equal(t, t_ref) and torch.equal(cw, cw_ref):
        return
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    bad = ((t != t_ref) | (cw != cw_ref)).nonzero(as_tuple=True)[0]
    pytest.fail(f"{what}: {bad.numel()} vertices differ from the twin; "
                f"degrees of the first 40: {deg[bad][:40].tolist()}")


# ---- the move kernels against the twins ------------------------------------

def _local_move_at_factors(ops, dev, wdtype, state, ghosts):
    for factor in rc.FACTORS:
        ops.clear_phase_caches()
        inp_cpu, L, ref = rc.scaled_ladder(wdtype, state, ghosts, factor)
        _, _, (t_base, _) = rc.base_ladder(wdtype, state, ghosts)
        inp = move_inputs_to(inp_cpu, dev)
        got = ops.local_move(inp)
        _assert_same(got, ref, inp_cpu, f"factor {factor}")
        if not ghosts:
            # one rank: the kernels that store the targets also account the
            # new aggregates (no vertex of the ladder is without edges)
            nc = inp.comm_size.numel()
            nsize = torch.zeros(nc, dtype=torch.int64, device=dev)
            ndegree = torch.zeros(nc, dtype=wdtype, device=dev)
            fused = ops.local_move(inp, next_size=nsize, next_degree=ndegree)
            _assert_same(fused, ref, inp_cpu, f"fused, factor {factor}")
            size_ref, degree_ref = aggregates_of(inp_cpu, ref[0])
            assert torch.equal(nsize.cpu(), size_ref)
            assert torch.equal(ndegree.cpu(), degree_ref.to(wdtype))
        print(f"factor {factor}: {int((ref[0] != t_base).sum())} targets "
              f"differ from the unscaled constant's")


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghosts", SHAPES, ids=_sh)
@pytest.mark.parametrize("state", rc.LADDER_STATES)
@pytest.mark.parametrize("cut", CUTS)
def test_local_move_matches_twin_at_scaled_constants(ops, dev, monkeypatch,
                                                     cut, state, ghosts,
                                                     wdtype):
    """All seven classes and the hub pipeline (cut 2049: eight hubs, cut
    6144: four), targets and cw, plus the fused next_size / next_degree on
    the ghost-free shape."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    _local_move_at_factors(ops, dev, wdtype, state, ghosts)


@pytest.mark.parametrize("cut", CUTS)
def test_local_move_torch_sort_hub_fallback(ops, dev, monkeypatch, cut):
    """CUVITE_HUB_SEGSORT=0: the hubs go through the torch-sort fallback,
    which evaluates the gain itself. The state on which most ladder
    vertices, hubs included, change their target."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    monkeypatch.setenv("CUVITE_HUB_SEGSORT", "0")
    for factor in rc.FACTORS:
        ops.clear_phase_caches()
        inp_cpu, L, ref = rc.scaled_ladder(torch.float64, "few", True, factor)
        got = ops.local_move(move_inputs_to(inp_cpu, dev))
        _assert_same(got, ref, inp_cpu, f"factor {factor}")


@functools.lru_cache(maxsize=None)
def _refine_ref(name, wdtype, ghostdup, factor):
    inp, L, mover, cand, _ = refine_case(name, wdtype, ghostdup)
    inp = rc.scaled(inp, factor)
    return inp, mover, cand, refine_move_torch(inp, mover, cand)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("cut", CUTS)
def test_refine_move_matches_twin_at_scaled_constants(ops, dev, monkeypatch,
                                                      cut, name, ghostdup,
                                                      wdtype):
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    base = _refine_ref(name, wdtype, ghostdup, 1.0)[3][0]
    for factor in rc.FACTORS:
        ops.clear_phase_caches()
        inp_cpu, mover, cand, ref = _refine_ref(name, wdtype, ghostdup,
                                                factor)
        inp = move_inputs_to(inp_cpu, dev)
        got = ops.refine_move(inp, mover.to(dev), cand.to(dev))
        _assert_same(got, ref, inp_cpu, f"factor {factor}")
        print(f"{name} factor {factor}: {int((ref[0] != base).sum())} "
              f"targets differ from the unscaled constant's")


def _active(kind, inp, L, cut):
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    a = torch.zeros(inp.nv, dtype=torch.bool)
    if kind == "ladder":
        a[:L] = True
    else:                                   # one_hub
        a[int((deg > cut).nonzero()[0, 0])] = True
    return a


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghosts", SHAPES, ids=_sh)
@pytest.mark.parametrize("state", rc.LADDER_STATES)
@pytest.mark.parametrize("cut", CUTS)
def test_frontier_move_matches_twin_at_scaled_constants(ops, dev, monkeypatch,
                                                        cut, state, ghosts,
                                                        wdtype):
    """Active vertices get the scaled plain move's answer, everyone else
    keeps label and cw_prev entry."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    g = torch.Generator().manual_seed(3)
    for factor in rc.FACTORS:
        inp_cpu, L, (t_full, cw_full) = rc.scaled_ladder(wdtype, state,
                                                         ghosts, factor)
        nv = inp_cpu.nv
        cw_prev = -torch.randint(1, 100, (nv,), generator=g).to(wdtype)
        curr = inp_cpu.curr_comm[:nv]
        inp = move_inputs_to(inp_cpu, dev)
        for kind in ("ladder", "one_hub"):
            ops.clear_phase_caches()
            a = _active(kind, inp_cpu, L, cut)
            ref = (torch.where(a, t_full, curr),
                   torch.where(a, cw_full, cw_prev))
            got = ops.frontier_move(inp, a.to(dev), cw_prev.to(dev))
            _assert_same(got, ref, inp_cpu, f"{kind}, factor {factor}")


# ---- scoring ----------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.25, 2.0, 3.5])
@pytest.mark.parametrize("name", ["dup", "rggu", "rmat10u"])
def test_partition_quality_hip_equals_torch(ops, dev, name, gamma):
    g = rc.graph(name)
    lab = rc.gamma_run(name, 2.0).communities
    want = partition_quality(single_partition(g), lab, Comm(),
                             backend="torch", resolution=gamma)
    got = partition_quality(single_partition(g).to(dev), lab.to(dev),
                            Comm(dev), backend="hip", resolution=gamma)
    print(f"{name} gamma {gamma}: Q {got.modularity:.15g}")
    assert got == want                    # every field, bit for bit
    assert got.resolution == gamma and got.at(1.0) == want.at(1.0)


# ---- whole runs -------------------------------------------------------------

@pytest.mark.parametrize("mode", list(rc.MODES))
@pytest.mark.parametrize("name", RUN_GRAPHS)
@pytest.mark.parametrize("gamma", RUN_GAMMAS)
def test_whole_run_matches_cpu_oracle(ops, dev, gamma, name, mode):
    kw = rc.MODES[mode]
    want = rc.gamma_run(name, gamma, **kw)
    dg = single_partition(rc.graph(name)).to(dev)
    res = louvain(dg, Comm(dev), LouvainConfig(backend="hip",
                                               resolution=gamma, **kw))
    print(f"{name} gamma {gamma} {mode}: "
          f"{rc.num_communities(res.communities.cpu())} communities, "
          f"{res.total_iters} sweeps, {res.phases} phases")
    assert torch.equal(res.communities.cpu(), want.communities)
    assert res.total_iters == want.total_iters and res.phases == want.phases
    assert [lv["iters"] for lv in res.levels] == \
        [lv["iters"] for lv in want.levels]
    assert abs(res.modularity - want.modularity) < 1e-12
    if mode == "vcycle":
        assert vc.same_reports(res.vcycle, want.vcycle)


def test_whole_run_without_the_fused_step(ops, dev, monkeypatch):
    """CUVITE_FUSED_AGG=0: the sweeps recount the aggregates in a pass of
    their own; same labels and sweeps at gamma = 2."""
    monkeypatch.setenv("CUVITE_FUSED_AGG", "0")
    want = rc.gamma_run("rmat10u", 2.0)
    dg = single_partition(rc.graph("rmat10u")).to(dev)
    res = louvain(dg, Comm(dev), LouvainConfig(backend="hip", resolution=2.0))
    assert torch.equal(res.communities.cpu(), want.communities)
    assert res.total_iters == want.total_iters


def _update_case(name, gamma, frac=0.01):
    """(new graph, batch, prev = the CPU cold run at gamma on the old graph,
    first frontier), one CPU rank."""
    g = rc.graph(name)
    batch = dyc.recipe_batch(g, frac)
    dg = apply_edge_batch(single_partition(g), Comm(), batch)
    prev = rc.gamma_run(name, gamma).communities
    return dg, batch, prev, affected_vertices(dg, Comm(), prev, batch)


@functools.lru_cache(maxsize=None)
def _update_oracle(name, gamma):
    dg, _, prev, f0 = _update_case(name, gamma)
    res = louvain(dg, Comm(), LouvainConfig(backend="torch",
                                            resolution=gamma),
                  init_labels=prev.clone(), init_frontier=f0.clone())
    return dg, prev, f0, res


@pytest.mark.parametrize("gamma", RUN_GAMMAS)
def test_frontier_update_matches_cpu_oracle(ops, dev, gamma):
    dg, prev, f0, want = _update_oracle("rmat12u", gamma)
    res = louvain(dg.to(dev), Comm(dev),
                  LouvainConfig(backend="hip", resolution=gamma),
                  init_labels=prev.to(dev), init_frontier=f0.to(dev))
    rep, rep_w = res.levels[0]["frontier"], want.levels[0]["frontier"]
    print(f"rmat12u gamma {gamma}: frontier sizes {rep.sizes_per_sweep}")
    assert rep.sizes_per_sweep == rep_w.sizes_per_sweep
    assert torch.equal(res.communities.cpu(), want.communities)
    assert res.total_iters == want.total_iters


# ---- two ranks on one GPU ---------------------------------------------------

def _w_two_ranks(rank, world, name, gamma, mode, prev):
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(8)
    dev = torch.device("cuda:0")
    comm = HostStagedComm(dev)
    g = rc.graph(name)
    if mode != "update":
        res = louvain(shard(g, rank, world).to(dev), comm,
                      LouvainConfig(backend="hip", resolution=gamma,
                                    **rc.MODES[mode]))
        return {"labels": res.communities.cpu(), "iters": res.total_iters,
                "vcycle": res.vcycle}
    # the frontier update: this rank's share of the batch
    share = dyc.share_of(dyc.recipe_batch(g, 0.01), rank, world)
    dg = apply_edge_batch(shard(g, rank, world).to(dev), comm, share)
    mine = prev[dg.base:dg.bound].clone().to(dev)
    f0 = affected_vertices(dg, comm, mine, share)
    res = louvain(dg, comm, LouvainConfig(backend="hip", resolution=gamma),
                  init_labels=mine, init_frontier=f0)
    return {"labels": res.communities.cpu(), "iters": res.total_iters,
            "sizes": list(res.levels[0]["frontier"].sizes_per_sweep)}


@pytest.mark.parametrize("mode", list(rc.MODES) + ["update"])
@pytest.mark.parametrize("gamma", RUN_GAMMAS)
def test_two_ranks_on_one_gpu_match_cpu_oracle(gamma, mode):
    """Both rank processes compute on cuda:0, the wire is gloo on host
    copies: labels and sweep counts equal the one-rank CPU oracle's."""
    name = "rggu"
    prev = None
    if mode == "update":
        _, prev, _, want = _update_oracle(name, gamma)
    else:
        want = rc.gamma_run(name, gamma, **rc.MODES[mode])
    parts = run_dist(2, _w_two_ranks, name, gamma, mode, prev, timeout_s=60)
    assert torch.equal(torch.cat([p["labels"] for p in parts]),
                       want.communities)
    for p in parts:
        assert p["iters"] == want.total_iters
        if mode == "vcycle":
            assert vc.same_reports(p["vcycle"], want.vcycle)
        if mode == "update":
            assert p["sizes"] == \
                want.levels[0]["frontier"].sizes_per_sweep


# ---- scan -------------------------------------------------------------------

def test_scan_matches_cpu_scan(ops, dev):
    gammas = (2.0, 1.0, 0.5)
    want = rc.scan_run("rggu", gammas)
    dg = single_partition(rc.graph("rggu")).to(dev)
    got = resolution_scan(dg, list(gammas), Comm(dev),
                          LouvainConfig(backend="hip"))
    for g, a, b in zip(gammas, got, want):
        print(f"rggu scan gamma {g}: "
              f"{rc.num_communities(b.communities)} communities, "
              f"{b.total_iters} sweeps")
        assert torch.equal(a.communities.cpu(), b.communities)
        assert a.total_iters == b.total_iters
