"""Warm start (louvain(init_labels=...)) on the CPU: identity with the cold
run from singleton labels, improvement and faster convergence from a run's
own output, and rank invariance."""

import pytest
import torch

from tests.dist_utils import run_dist

from cuvite_amd import partition_quality
from cuvite_amd.graph import single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

from quality_cases import cold_run, lfr_truth, shard, whole_graph


def _warm(name, init):
    return louvain(single_partition(whole_graph(name)), Comm(),
                   LouvainConfig(backend="torch"), init_labels=init)


def _exact(name, labels):
    return partition_quality(single_partition(whole_graph(name)), labels,
                             Comm(), backend="torch").modularity


# ---- 4. init_labels=arange is the cold run ----------------------------------

@pytest.mark.parametrize("name", ["karate", "lfr", "rgg"])
def test_arange_init_equals_cold_run(name):
    cold = cold_run(name)
    warm = _warm(name, torch.arange(whole_graph(name).nv))
    assert torch.equal(warm.communities, cold.communities)
    assert warm.modularity == cold.modularity
    assert warm.modularity_per_level == cold.modularity_per_level
    assert warm.total_iters == cold.total_iters
    assert warm.phases == cold.phases


# ---- 5. restart from a partition --------------------------------------------

@pytest.mark.parametrize("name,start", [("karate", "own"), ("lfr", "own"),
                                        ("rgg", "own"), ("lfr", "truth")])
def test_warm_start_improves_and_converges_faster(name, start):
    """Not a theorem for synchronous Louvain: holds on these pinned inputs
    (karate 4 vs 11 sweeps, lfr 4 vs 33, rgg 11 vs 37 from the own output)."""
    cold = cold_run(name)
    init = cold.communities if start == "own" else lfr_truth()
    q_start = _exact(name, init)
    warm = _warm(name, init.clone())
    q_end = _exact(name, warm.communities)
    print(f"{name}/{start}: start Q={q_start:.12f} end Q={q_end:.12f} "
          f"sweeps warm={warm.total_iters} cold={cold.total_iters}")
    assert q_end >= q_start - 1e-9
    assert warm.total_iters < cold.total_iters


def test_init_labels_are_not_modified():
    init = cold_run("karate").communities.clone()
    keep = init.clone()
    _warm("karate", init)
    assert torch.equal(init, keep)


# ---- 6. ranks 1, 2, 4 -------------------------------------------------------

def _w_warm(rank, world, init_by_name):
    out = {}
    for name, init in init_by_name.items():
        dg = shard(whole_graph(name), rank, world)
        res = louvain(dg, Comm(), LouvainConfig(backend="torch"),
                      init_labels=init[dg.base:dg.bound].clone())
        out[name] = (res.modularity, res.modularity_per_level,
                     res.communities.cpu(), res.total_iters)
    return out


@pytest.mark.parametrize("world", [2, 4])
def test_warm_start_rank_invariant(world):
    """Same comparison as the cold-run rank-invariance tests: modularity to
    1e-9 at every level, identical communities and sweep counts."""
    inits = {n: cold_run(n).communities for n in ("karate", "rgg")}
    inits["lfr"] = lfr_truth()
    single = {n: _warm(n, init.clone()) for n, init in inits.items()}
    outs = run_dist(world, _w_warm, inits)
    for name, ref in single.items():
        for o in outs:
            mod, per_level, _, iters = o[name]
            assert abs(mod - ref.modularity) < 1e-9
            assert len(per_level) == len(ref.modularity_per_level)
            assert all(abs(a - b) < 1e-9 for a, b in
                       zip(per_level, ref.modularity_per_level))
            assert iters == ref.total_iters
        comms = torch.cat([o[name][2] for o in outs])
        assert torch.equal(comms, ref.communities)
