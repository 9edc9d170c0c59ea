"""Connected components inside communities on the CPU: the torch rounds
against the union-find oracle, split_disconnected, rank invariance,
LouvainConfig.connectivity and the CLI flags. All comparisons of labels are
torch.equal: everything is integer valued."""

import functools
import os
import subprocess
import sys

import pytest
import torch

from cuvite_amd import (ConnectivityReport, cc_components_torch,
                        partition_quality, split_disconnected)
from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm
from cuvite_amd.quality import validate_labels

from tests.dist_utils import run_dist

import connectivity_cases as cc
from quality_cases import cold_run, dup_graph, shard, whole_graph

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPHS = ("karate", "lfr", "rgg", "rmat10")


@functools.lru_cache(maxsize=None)
def _graph(name):
    return rmat_graph(10, 8, seed=2) if name == "rmat10" else whole_graph(name)


@functools.lru_cache(maxsize=None)
def _cold(name, **kw):
    """Cold single-rank CPU run, once per session and configuration."""
    if name != "rmat10" and not kw:
        return cold_run(name)
    return louvain(single_partition(_graph(name)), Comm(),
                   LouvainConfig(backend="torch", **kw))


@functools.lru_cache(maxsize=None)
def _split(name) -> ConnectivityReport:
    return split_disconnected(single_partition(_graph(name)),
                              _cold(name).communities, Comm(),
                              backend="torch")


def _exact(name, labels):
    return partition_quality(single_partition(_graph(name)), labels, Comm(),
                             backend="torch")


# ---- 1. the torch rounds against the union-find oracle -----------------------

@pytest.mark.parametrize("case", list(cc.hand_cases()))
def test_hand_built(case):
    rowptr, tails, labels, want = cc.hand_cases()[case]
    assert cc.uf_min_labels(rowptr, tails, labels).tolist() == want
    comp, rounds = cc_components_torch(rowptr, tails, labels)
    print(f"{case}: rounds={rounds}")
    assert comp.dtype == torch.int32
    assert comp.tolist() == want


def test_no_edges_and_no_vertices():
    comp, rounds = cc_components_torch(
        torch.zeros(6, dtype=torch.int64), torch.empty(0, dtype=torch.int32),
        torch.zeros(8, dtype=torch.int64))
    assert comp.tolist() == list(range(8)) and rounds == 0
    comp, rounds = cc_components_torch(
        torch.zeros(1, dtype=torch.int64), torch.empty(0, dtype=torch.int32),
        torch.empty(0, dtype=torch.int64))
    assert comp.numel() == 0 and rounds == 0


def test_dup_graph_three_random_labels():
    g = dup_graph()
    labels = torch.randint(0, 3, (g.nv,),
                           generator=torch.Generator().manual_seed(5))
    tails = g.tails.to(torch.int32)
    want = cc.uf_min_labels(g.rowptr, tails, labels)
    assert 3 < cc.num_components(want) < g.nv
    comp, rounds = cc_components_torch(g.rowptr, tails, labels)
    print(f"dup_graph: rounds={rounds}")
    assert torch.equal(comp.to(torch.int64), want)


@pytest.mark.parametrize("labelling", ["one", "blocks"])
@pytest.mark.parametrize("order", cc.PATH_ORDERS)
def test_path_orders(order, labelling):
    rowptr, tails, labels, want = cc.path_case(order, labelling)
    assert cc.num_components(want) == (1 if labelling == "one" else 41)
    comp, rounds = cc_components_torch(rowptr, tails, labels)
    print(f"path {order}/{labelling}: rounds={rounds}")
    assert torch.equal(comp.to(torch.int64), want)


# ---- 2. split_disconnected on cold-run labels ------------------------------------

@pytest.mark.parametrize("name", GRAPHS)
def test_split_cold_run_labels(name):
    g = _graph(name)
    lab = _cold(name).communities
    rep = _split(name)
    want = cc.uf_min_labels(g.rowptr, g.tails, lab)
    print(f"{name}: communities={rep.num_communities} "
          f"components={rep.num_components} "
          f"disconnected={rep.num_disconnected} rounds={rep.rounds}")
    assert torch.equal(rep.labels, want)
    assert rep.num_communities == int(torch.unique(lab).numel())
    assert rep.num_components == cc.num_components(want)
    # communities that fell apart, counted from the oracle
    pairs = torch.unique(torch.stack([lab, want]), dim=1)
    per_comm = torch.unique(pairs[0], return_counts=True)[1]
    assert rep.num_disconnected == int((per_comm > 1).sum())
    validate_labels(single_partition(g), Comm(), rep.labels)
    before, after = _exact(name, lab), _exact(name, rep.labels)
    print(f"{name}: exact Q {before.modularity:.9f} -> "
          f"{after.modularity:.9f}")
    if name == "karate":
        assert rep.num_components == rep.num_communities
        assert rep.num_disconnected == 0
    else:
        # plain Louvain output really needs the feature
        assert rep.num_components > rep.num_communities
        assert rep.num_disconnected > 0
        assert after.modularity > before.modularity
    assert after.coverage == pytest.approx(before.coverage, rel=1e-12)
    assert after.num_communities == rep.num_components
    # splitting the split labels changes nothing
    again = split_disconnected(single_partition(g), rep.labels, Comm(),
                               backend="torch")
    assert torch.equal(again.labels, rep.labels)
    assert again.num_disconnected == 0
    assert again.num_components == again.num_communities == rep.num_components


def test_bad_labels_and_backend_raise():
    dg = single_partition(_graph("karate"))
    with pytest.raises(ValueError):
        split_disconnected(dg, torch.zeros(3, dtype=torch.int64), Comm())
    with pytest.raises(RuntimeError):
        split_disconnected(dg, torch.zeros(dg.nv, dtype=torch.int64), Comm(),
                           backend="hip")
    with pytest.raises(ValueError):
        louvain(dg, Comm(), LouvainConfig(backend="torch",
                                          connectivity="sometimes"))


# ---- 3. rank invariance ---------------------------------------------------------------

def _rank_worker(rank, world, labels_by_name):
    comm = Comm()
    out = {}
    for name, lab in labels_by_name.items():
        g = _graph(name)
        for balanced in (False, True):
            dg = shard(g, rank, world, balanced)
            rep = split_disconnected(dg, lab[dg.base:dg.bound].clone(), comm,
                                     backend="torch")
            out[name, balanced] = rep
    return out


@pytest.mark.parametrize("world", [1, 2, 3])
def test_rank_invariance(world):
    names = ("lfr", "rgg")
    outs = run_dist(world, _rank_worker,
                    {n: _cold(n).communities for n in names}, timeout_s=300)
    for name in names:
        ref = _split(name)
        for balanced in (False, True):
            reps = [o[name, balanced] for o in outs]
            got = torch.cat([r.labels for r in reps])
            print(f"{name} world {world} balanced={balanced}: rounds "
                  f"{[r.rounds for r in reps]}")
            assert torch.equal(got, ref.labels)
            for r in reps:
                assert r.num_communities == ref.num_communities
                assert r.num_components == ref.num_components
                assert r.num_disconnected == ref.num_disconnected


# ---- 4. LouvainConfig.connectivity --------------------------------------------------------

@pytest.mark.parametrize("name", ["lfr", "rgg"])
def test_final_equals_split_of_plain_run(name):
    plain = _cold(name)
    res = _cold(name, connectivity="final")
    assert torch.equal(res.communities, _split(name).labels)
    assert cc.all_connected(_graph(name), res.communities)
    assert res.connectivity.num_components == _split(name).num_components
    assert res.connectivity.num_disconnected > 0
    # the convergence estimate and the trajectory are the plain run's
    assert res.modularity == plain.modularity
    assert res.total_iters == plain.total_iters
    assert plain.connectivity is None


@pytest.mark.parametrize("name", ["lfr", "rgg", "rmat10"])
def test_level_leaves_every_community_connected(name):
    g = _graph(name)
    res = _cold(name, connectivity="level")
    validate_labels(single_partition(g), Comm(), res.communities)
    assert cc.all_connected(g, res.communities)
    assert isinstance(res.connectivity, ConnectivityReport)
    # connectivity is the guarantee; the exact Q may go either way
    print(f"{name}: exact Q plain "
          f"{_exact(name, _cold(name).communities).modularity:.9f} level "
          f"{_exact(name, res.communities).modularity:.9f}")


def test_level_with_threshold_cycling():
    """-i ends with a re-run of the last level at the finest threshold; its
    communities are split as well."""
    g = _graph("lfr")
    res = _cold("lfr", connectivity="level", threshold_scaling=True)
    assert cc.all_connected(g, res.communities)
    assert all("connectivity" in lv for lv in res.levels[:-1])


@pytest.mark.parametrize("name", ["karate", "lfr"])
def test_off_is_the_default_run(name):
    off = _cold(name, connectivity="off")
    plain = _cold(name)
    assert torch.equal(off.communities, plain.communities)
    assert off.modularity == plain.modularity
    assert off.total_iters == plain.total_iters
    assert off.connectivity is None


# ---- 5. CLI -----------------------------------------------------------------------------

def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run(
        [sys.executable, "-m", "cuvite_amd", "--device", "cpu", "--backend",
         "torch"] + args, capture_output=True, text=True, cwd=cwd, env=env,
        timeout=300)


def _connectivity_line(stdout):
    lines = [ln for ln in stdout.splitlines()
             if ln.startswith("Connectivity:")]
    assert len(lines) == 1, stdout
    return {k: int(v) for k, v in
            (field.split("=") for field in lines[0].split()[1:])}


@pytest.mark.parametrize("source,name", [(["--karate"], "karate"),
                                         (["--lfr", "2000", "--mu", "0.3"],
                                          "lfr")])
def test_cli_flags(tmp_path, source, name):
    ref = _split(name)
    r = _cli(source + ["--check-connected"], tmp_path)
    assert r.returncode == 0, r.stderr
    plain = _connectivity_line(r.stdout)
    assert plain == {"communities": ref.num_communities,
                     "disconnected": ref.num_disconnected,
                     "components": ref.num_components}
    # without the flags not one line is added
    r0 = _cli(source, tmp_path)
    assert r0.returncode == 0, r0.stderr
    assert "Connectivity" not in r0.stdout
    assert len(r0.stdout.splitlines()) == len(r.stdout.splitlines()) - 1

    r = _cli(source + ["--connectivity", "final", "-o", "--check-connected"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    final = _connectivity_line(r.stdout)
    assert final["disconnected"] == 0
    assert final["communities"] == final["components"] == ref.num_components
    dump = str(tmp_path / "graph.communities")
    assert os.path.exists(dump)
    r = _cli(source + ["--score-communities", dump, "--check-connected"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.startswith("Partition ")]
    assert len(at) == 1 and lines[at[0] + 1].startswith("Connectivity:")
    assert _connectivity_line(r.stdout) == final

    r = _cli(source + ["--connectivity", "level", "--check-connected"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    assert _connectivity_line(r.stdout)["disconnected"] == 0
