"""Leiden mode on the GPU against the CPU oracle: refinement alone on a graph
with hub vertices, and whole `louvain(algorithm="leiden")` runs, on one rank
and on two rank processes that share `cuda:0` over
`dist_utils.HostStagedComm` (compute on the device with backend "hip", the
wire gloo on host copies), as test_gpu_multirank.py does for Louvain.

All graphs carry unit weights (dist_cases.py), so every sum is exact and
every comparison is torch.equal and ==.

Launch wall time measured on an MI355X (process start and imports
included): 3.4 s. LAUNCH_TIMEOUT_S is about four times that."""

import functools
import os
import time

import pytest
import torch

from cuvite_amd.graph import single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm
from cuvite_amd.refine import refine_partition

from tests.dist_utils import run_dist

import connectivity_cases as cc
import dist_cases as dc

pytestmark = pytest.mark.gpu

LAUNCH_TIMEOUT_S = 15
BOUND_STATES = ("few", "random")


def _summary(res):
    return {"communities": res.communities, "modularity": res.modularity,
            "total_iters": res.total_iters, "phases": res.phases,
            "refine": [(lv["refine"].labels, lv["refine"].moved_per_round,
                        lv["refine"].num_subcommunities)
                       for lv in res.levels if "refine" in lv],
            "split": (res.connectivity.num_communities,
                      res.connectivity.num_disconnected,
                      res.connectivity.num_components)}


def _refine_summary(rep):
    return {"labels": rep.labels, "moved": rep.moved_per_round,
            "nsub": rep.num_subcommunities, "ncomm": rep.num_communities}


@functools.lru_cache(maxsize=None)
def _cpu_leiden(**kw):
    return dc._cpu(_summary(louvain(
        single_partition(dc.converging_graph()), Comm(),
        LouvainConfig(backend="torch", algorithm="leiden", **kw))))


@functools.lru_cache(maxsize=None)
def _cpu_refine(state):
    g = dc.hub_graph()
    return dc._cpu(_refine_summary(refine_partition(
        single_partition(g), dc.label_state(state, g.nv), Comm(),
        backend="torch")))


@pytest.fixture
def hub_cut(monkeypatch):
    from cuvite_amd import ops
    monkeypatch.setenv("CUVITE_HUB_CUT", str(dc.HUB_CUT))
    ops.clear_phase_caches()
    yield
    ops.clear_phase_caches()


@pytest.mark.parametrize("state", BOUND_STATES)
def test_refine_partition_with_hubs_matches_cpu(hub_cut, state):
    """hub_graph: planted vertices above the (lowered) hub cut and in the
    two widest LDS classes; `few` puts most of the graph into five bounds,
    `random` into nv/8."""
    dev = torch.device("cuda:0")
    g = dc.hub_graph()
    assert int((g.degrees() > dc.HUB_CUT).sum()) >= 4
    ref = _cpu_refine(state)
    rep = refine_partition(single_partition(g.to(dev)),
                           dc.label_state(state, g.nv).to(dev), Comm(dev),
                           backend="hip")
    dc.assert_same(dc._cpu(_refine_summary(rep)), ref)
    # the oracle's answer has what the test is about
    sub = ref["labels"]
    comp = cc.uf_min_labels(g.rowptr, g.tails, sub)
    assert cc.num_components(comp) == ref["nsub"] < g.nv
    hubs = (g.degrees() > dc.HUB_CUT).nonzero(as_tuple=True)[0]
    print(f"{state}: {ref['ncomm']} bounds -> {ref['nsub']} subs, moved "
          f"{ref['moved']}; hubs moved: "
          f"{int((sub[hubs] != hubs).sum())} of {hubs.numel()}")


@pytest.mark.parametrize("kw", [{}, {"threshold_scaling": True}],
                         ids=["plain", "cycling"])
def test_leiden_matches_cpu(kw):
    dev = torch.device("cuda:0")
    g = dc.converging_graph()
    ref = _cpu_leiden(**kw)
    assert len(ref["refine"]) >= 2
    res = louvain(single_partition(g.to(dev)), Comm(dev),
                  LouvainConfig(backend="hip", algorithm="leiden", **kw))
    dc.assert_same(dc._cpu(_summary(res)), ref)
    assert cc.all_connected(g, ref["communities"])


def _rank_worker(rank, world, devname):
    """Both scenarios, oracle first (plain Comm, CPU, torch), then on the
    device through HostStagedComm with the HIP backend."""
    from cuvite_amd import ops
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(max(1, 16 // world))
    os.environ["CUVITE_HUB_CUT"] = str(dc.HUB_CUT)
    dc._forbid_device_tensors_on_the_wire()
    out = {}
    for side, comm, dev, backend in (
            ("oracle", Comm(), torch.device("cpu"), "torch"),
            ("staged", HostStagedComm(torch.device(devname)),
             torch.device(devname), "hip")):
        g = dc.hub_graph()
        dg = dc.shard(g, rank, world).to(dev)
        lab = dc.label_state("few", g.nv)[dg.base:dg.bound].clone().to(dev)
        rep = refine_partition(dg, lab, comm, backend=backend)
        ops.clear_phase_caches()
        dg = dc.shard(dc.converging_graph(), rank, world).to(dev)
        res = louvain(dg, comm, LouvainConfig(backend=backend,
                                              algorithm="leiden"))
        ops.clear_phase_caches()
        out[side] = dc._cpu({"refine": _refine_summary(rep),
                             "leiden": _summary(res)})
    return out


@functools.lru_cache(maxsize=None)
def _launch():
    """One attempt per session; a failed launch is cached as its exception."""
    assert torch.cuda.is_available()
    t0 = time.perf_counter()
    try:
        outs = run_dist(2, _rank_worker, "cuda:0",
                        timeout_s=LAUNCH_TIMEOUT_S)
    except Exception as e:
        outs = e
    print(f"two-rank launch: {time.perf_counter() - t0:.1f} s "
          f"(limit {LAUNCH_TIMEOUT_S} s)")
    return outs


def _cat(parts, key):
    return torch.cat([p[key] for p in parts])


def test_two_ranks_on_one_gpu_match_the_cpu_oracle():
    import multiprocessing
    outs = _launch()
    if isinstance(outs, Exception):
        raise AssertionError(f"two-rank launch failed: {outs!r}")
    assert multiprocessing.active_children() == []
    for r, o in enumerate(outs):
        dc.assert_same(o["oracle"], o["staged"], f"rank {r}")
    # and the two-rank answers are the single-rank ones
    ref = _cpu_refine("few")
    got = [o["staged"]["refine"] for o in outs]
    assert torch.equal(_cat(got, "labels"), ref["labels"])
    assert all(x["moved"] == ref["moved"] and x["nsub"] == ref["nsub"]
               for x in got)
    ref = _cpu_leiden()
    got = [o["staged"]["leiden"] for o in outs]
    assert torch.equal(_cat(got, "communities"), ref["communities"])
    for x in got:
        assert x["modularity"] == ref["modularity"]
        assert (x["total_iters"], x["phases"]) == (ref["total_iters"],
                                                   ref["phases"])
        assert x["split"] == ref["split"]
        assert [m for _, m, _ in x["refine"]] == \
            [m for _, m, _ in ref["refine"]]
