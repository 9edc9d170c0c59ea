"""CPU-only checks of the multi-rank case builders (dist_cases.py): the
inputs have the properties the GPU tests rely on, and the host-staged
communicator changes nothing.

The staged launches below run every scenario of test_gpu_multirank.py with
`HostStagedComm(cpu)` and backend "torch" against plain `Comm()`, through
the same worker and the same parent-side checks: the conditions on the
inputs (universe growth, hub moves) are asserted on the oracle side there,
and a defect in the multi-rank state handling shows here without a GPU."""

import functools

import pytest
import torch

from tests.dist_utils import run_dist

import dist_cases as dc
from cuvite_amd.graph import single_partition

WORLDS = (2, 3)


# ---- graphs -----------------------------------------------------------------

@pytest.mark.parametrize("world", WORLDS)
def test_hub_graph_degree_classes_and_ghosts_per_rank(world):
    g = dc.hub_graph()
    assert g.nv == 4096
    assert bool((g.weights == 1.0).all())
    # below the collision-safe load of the widest LDS class (default cut)
    assert int(g.degrees().max()) < 6144
    for r, p in enumerate(dc.slice_profile(g, world)):
        assert p["hub"] >= 1, (r, p)
        assert p["c2048"] >= 2, (r, p)
        assert p["c1024"] >= 3, (r, p)
        assert p["ghosts"] >= 1500, (r, p)


def test_hub_graph_is_symmetric_and_int_weights_are_small_integers():
    for kind in ("unit", "int"):
        g = dc.hub_graph(kind)
        src = torch.repeat_interleave(torch.arange(g.nv), g.degrees())
        fwd = torch.sort(src * g.nv + g.tails)
        rev = torch.sort(g.tails * g.nv + src)
        assert torch.equal(fwd.values, rev.values)
        assert torch.equal(g.weights[fwd.indices], g.weights[rev.indices])
    w = dc.hub_graph("int").weights
    assert w.unique().tolist() == [1.0, 2.0, 3.0, 4.0]
    # fp32 sums of these weights stay exact
    assert float(dc.hub_graph().weights.sum()) < 2 ** 24
    assert float(w.sum()) < 2 ** 24


def test_converging_graph_runs_many_sweeps_and_phases():
    g = dc.converging_graph()
    assert bool((g.weights == 1.0).all())
    res = dc.single_rank_louvain("louvain_plain")
    assert res.total_iters >= 8
    assert res.phases >= 3
    for world in WORLDS:
        for r in range(world):
            assert dc.shard(g, r, world).ghost_vertices().numel() >= 1
    # the small graph of the coloring / ordering variants
    for name in ("louvain_coloring", "louvain_ordering"):
        res = dc.single_rank_louvain(name)
        assert res.total_iters >= 8 and res.phases >= 3


@pytest.mark.parametrize("nv", [1024, 4096])
def test_label_states(nv):
    assert torch.equal(dc.label_state("singletons", nv), torch.arange(nv))
    rnd = dc.label_state("random", nv)
    few = dc.label_state("few", nv)
    for lab in (rnd, few):
        assert lab.dtype == torch.int64 and lab.shape == (nv,)
        assert int(lab.min()) >= 0 and int(lab.max()) < nv
    assert few.unique().numel() == 5
    assert 0.8 * nv / 8 <= rnd.unique().numel() <= nv // 8
    for world in WORLDS:
        for r in range(world):
            b, e = r * nv // world, (r + 1) * nv // world
            mine = rnd[b:e]
            remote = (mine < b) | (mine >= e)
            assert float(remote.float().mean()) > 0.4


# ---- the staging layer, and the scenarios on the oracle alone ------------------

# on the CPU the fp32 and default-cut sweeps take the same torch path as the
# fp64 ones; their input conditions are asserted on the oracle side of the
# GPU launch
CPU_SCENARIOS = tuple(n for n in dc.SCENARIOS
                      if "fp32" not in n and "default_cut" not in n)


@functools.lru_cache(maxsize=None)
def _staged_launch(world):
    try:
        return run_dist(world, dc.launch_worker, CPU_SCENARIOS, "cpu")
    except Exception as e:   # cached: one launch per world, no retry
        return e


@pytest.mark.parametrize("name", CPU_SCENARIOS)
@pytest.mark.parametrize("world", WORLDS)
def test_staged_on_cpu_equals_plain_comm(world, name):
    outs = _staged_launch(world)
    if isinstance(outs, Exception):
        raise AssertionError(f"world-{world} launch failed: {outs!r}")
    dc.check_scenario(name, world, [o[name] for o in outs], "cpu")


# ---- run_dist: stragglers and dead ranks ----------------------------------------

def _w_misbehave(rank, world, how):
    if rank == 1 and how == "hang":
        import time
        time.sleep(600)
    if rank == 1 and how == "die":
        import os
        os._exit(3)
    return rank


def test_run_dist_stops_and_names_a_straggler():
    import multiprocessing
    import time
    t0 = time.monotonic()
    # (a slow machine may not have finished rank 0 within the limit either)
    with pytest.raises(AssertionError,
                       match=r"rank\(s\) \[(0, )?1\] still running"):
        run_dist(2, _w_misbehave, "hang", timeout_s=5)
    assert time.monotonic() - t0 < 60
    assert multiprocessing.active_children() == []


def test_run_dist_reports_a_dead_rank_once():
    import multiprocessing
    with pytest.raises(AssertionError, match="rank 1 exited with 3"):
        run_dist(2, _w_misbehave, "die")
    assert multiprocessing.active_children() == []
    assert run_dist(2, _w_misbehave, "fine") == [0, 1]


def test_single_rank_references_are_on_the_oracle_path():
    g, renum = dc.single_rank_coarsen()
    assert g.nv == (dc.hub_graph().nv + 6) // 7
    assert torch.equal(renum, dc.coarsen_labels(0, dc.hub_graph().nv))
    colors, nc = dc.single_rank_coloring()
    from cuvite_amd.coloring import check_coloring
    from cuvite_amd.parallel import Comm
    assert check_coloring(single_partition(dc.hub_graph()), Comm(), colors,
                          exclude_color=nc - 1) == 0
