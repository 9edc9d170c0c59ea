"""Leiden refinement (cuvite_amd/refine.py) on the CPU: every sub-community
lies in one community and is connected, a round never moves a vertex that is
joined in it, the result is reproducible and the same on 1, 2 and 3 ranks
for both partitioners, the round limit is not reached, and the coin is fair.

Inputs are the cold-run communities of the four quality graphs. Labels are
compared with torch.equal: karate carries unit weights (every sum exact);
lfr and rgg carry real weights, where a label could in principle hinge on
the last bit of a degree sum taken in another order, which these seeds do
not do (tests/test_connectivity.py relies on the same)."""

import functools

import pytest
import torch

from cuvite_amd import RefineReport, refine_coin, refine_partition
from cuvite_amd.graph import single_partition
from cuvite_amd.parallel import Comm
from cuvite_amd.refine import REFINE_MAX_ROUNDS

from tests.dist_utils import run_dist

import connectivity_cases as cc
from quality_cases import cold_run, shard, whole_graph

NAMES = ("karate", "lfr", "rgg", "karate2")


@functools.lru_cache(maxsize=None)
def _refined(name):
    """(RefineReport, trace) of the single-rank run, once per session."""
    trace = []
    rep = refine_partition(single_partition(whole_graph(name)),
                           cold_run(name).communities, Comm(),
                           backend="torch", trace=trace.append)
    return rep, trace


@pytest.mark.parametrize("name", NAMES)
def test_subs_are_connected_parts_of_one_community(name):
    g = whole_graph(name)
    comm_labels = cold_run(name).communities
    rep, _ = _refined(name)
    sub = rep.labels
    assert isinstance(rep, RefineReport)
    assert sub.dtype == torch.int64 and sub.numel() == g.nv
    # a sub's label is a vertex that is in it
    assert torch.equal(sub[sub], sub)
    # every sub lies in one community
    assert torch.equal(comm_labels[sub], comm_labels)
    # every sub is connected: splitting the subs changes nothing
    comp = cc.uf_min_labels(g.rowptr, g.tails, sub)
    nsub = int(torch.unique(sub).numel())
    assert cc.num_components(comp) == nsub
    assert rep.num_subcommunities == nsub
    assert rep.num_communities == int(torch.unique(comm_labels).numel())
    # refinement did something: fewer subs than vertices, and no fewer subs
    # than the communities have components
    ncomp = cc.num_components(cc.uf_min_labels(g.rowptr, g.tails,
                                               comm_labels))
    assert ncomp <= nsub < g.nv
    print(f"{name}: {rep.num_communities} communities ({ncomp} components) "
          f"-> {nsub} subs in {rep.rounds} rounds, moved "
          f"{rep.moved_per_round}")


@pytest.mark.parametrize("name", NAMES)
def test_no_vertex_moves_and_is_joined_in_one_round(name):
    rep, trace = _refined(name)
    assert len(trace) == rep.rounds == len(rep.moved_per_round)
    total = 0
    for r, t in enumerate(trace):
        assert t["round"] == r
        curr, target = t["curr"], t["target"]
        moved = target != curr
        assert int(moved.sum()) == rep.moved_per_round[r]
        total += int(moved.sum())
        # movers were singletons carrying their own id ...
        ids = moved.nonzero(as_tuple=True)[0]
        assert torch.equal(curr[ids], ids)
        assert int((curr == ids[:, None]).sum()) == ids.numel()
        # ... and no joined sub holds a vertex that moved this round
        joined = torch.zeros(curr.numel(), dtype=torch.bool)
        joined[target[moved]] = True
        assert not bool(joined[curr[moved]].any())
    assert total == int((rep.labels != torch.arange(rep.labels.numel()))
                        .sum())
    assert torch.equal(trace[-1]["target"], rep.labels)


@pytest.mark.parametrize("name", NAMES)
def test_two_runs_agree_and_the_round_limit_is_not_reached(name):
    rep, _ = _refined(name)
    again = refine_partition(single_partition(whole_graph(name)),
                             cold_run(name).communities, Comm(),
                             backend="torch")
    assert torch.equal(again.labels, rep.labels)
    assert again.moved_per_round == rep.moved_per_round
    # stopped by the first pair without a move, not by the limit (the
    # default is twice the largest count seen, profiles/leiden.md)
    assert rep.rounds % 2 == 0
    assert rep.moved_per_round[-2:] == [0, 0]
    assert rep.rounds < REFINE_MAX_ROUNDS
    assert all(a or b for a, b in zip(rep.moved_per_round[:-2:2],
                                      rep.moved_per_round[1:-2:2]))


def test_max_rounds_cuts_the_run_short():
    rep, _ = _refined("lfr")
    cut = refine_partition(single_partition(whole_graph("lfr")),
                           cold_run("lfr").communities, Comm(),
                           backend="torch", max_rounds=2)
    assert cut.rounds == 2
    assert cut.moved_per_round == rep.moved_per_round[:2]
    g = whole_graph("lfr")
    comp = cc.uf_min_labels(g.rowptr, g.tails, cut.labels)
    assert cc.num_components(comp) == cut.num_subcommunities


def test_seed_and_level_change_the_coin_not_the_guarantees():
    g = whole_graph("rgg")
    base, _ = _refined("rgg")
    other = refine_partition(single_partition(g),
                             cold_run("rgg").communities, Comm(),
                             backend="torch", seed=5, level=2)
    assert not torch.equal(other.labels, base.labels)
    comp = cc.uf_min_labels(g.rowptr, g.tails, other.labels)
    assert cc.num_components(comp) == other.num_subcommunities


def _rank_worker(rank, world, labels_by_name):
    comm = Comm()
    out = {}
    for name, lab in labels_by_name.items():
        g = whole_graph(name)
        for balanced in (False, True):
            dg = shard(g, rank, world, balanced)
            out[name, balanced] = refine_partition(
                dg, lab[dg.base:dg.bound].clone(), comm, backend="torch")
    return out


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_invariance(world):
    outs = run_dist(world, _rank_worker,
                    {n: cold_run(n).communities for n in NAMES},
                    timeout_s=300)
    for name in NAMES:
        ref, _ = _refined(name)
        for balanced in (False, True):
            reps = [o[name, balanced] for o in outs]
            got = torch.cat([r.labels for r in reps])
            assert torch.equal(got, ref.labels), (name, world, balanced)
            for r in reps:
                assert r.moved_per_round == ref.moved_per_round
                assert r.num_subcommunities == ref.num_subcommunities
                assert r.num_communities == ref.num_communities


def test_bad_labels_raise():
    dg = single_partition(whole_graph("karate"))
    with pytest.raises(ValueError):
        refine_partition(dg, torch.zeros(3, dtype=torch.int64), Comm(),
                         backend="torch")
    with pytest.raises(RuntimeError):
        refine_partition(dg, torch.zeros(34, dtype=torch.int64), Comm(),
                         backend="hip")


@pytest.mark.parametrize("pair", range(8))
def test_coin_is_fair(pair):
    """4096 fair bits have standard deviation 32: [40%, 60%] is 12 sigma."""
    ids = torch.arange(4096)
    for gids, kw in ((ids, {}), (ids + (5 << 32), {"level": 3, "seed": 9})):
        n = int(refine_coin(gids, pair, **kw).sum())
        print(f"pair {pair} {kw}: {n} of 4096")
        assert 0.4 * 4096 <= n <= 0.6 * 4096


def test_coin_is_a_pure_function_of_its_arguments():
    ids = torch.arange(4096) * 7919
    a = refine_coin(ids, 3, level=1, seed=2)
    assert a.dtype == torch.bool
    assert torch.equal(a, refine_coin(ids.clone(), 3, level=1, seed=2))
    assert torch.equal(a[1000:2000], refine_coin(ids[1000:2000], 3, 1, 2))
    for other in (refine_coin(ids, 4, level=1, seed=2),
                  refine_coin(ids, 3, level=2, seed=2),
                  refine_coin(ids, 3, level=1, seed=3)):
        # another pair, level or seed is another coin: about half differ
        assert 0.4 * 4096 <= int((a != other).sum()) <= 0.6 * 4096
