"""Exact partition scoring on the CPU: the torch oracle against brute-force
formulas, partition_quality across ranks and partitions, label validation,
and the CLI flags built on them."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.dist_utils import run_dist

from cuvite_amd import (PartitionQuality, intra_weight_torch,
                        partition_quality)
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.parallel import Comm

from quality_cases import (brute_modularity, cold_run, dup_graph,
                           edge_list_intra, shard, whole_graph)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pq(g, labels):
    return partition_quality(single_partition(g), labels, Comm(),
                             backend="torch")


# ---- 1. oracle vs the dense formula on karate ------------------------------

def test_karate_singletons_one_community_and_random():
    g = whole_graph("karate")
    k = np.zeros(g.nv)
    np.add.at(k, np.repeat(np.arange(g.nv), g.degrees().numpy()),
              g.weights.numpy())
    single = _pq(g, torch.arange(g.nv))
    assert isinstance(single, PartitionQuality)
    assert abs(single.modularity + float(((k / k.sum()) ** 2).sum())) <= 1e-12
    assert single.num_communities == g.nv
    assert single.total_weight == float(k.sum())
    one = _pq(g, torch.zeros(g.nv, dtype=torch.int64))
    assert abs(one.modularity) <= 1e-15
    assert one.num_communities == 1
    assert one.coverage == pytest.approx(1.0, abs=1e-15)
    lab = torch.randint(0, 5, (g.nv,),
                        generator=torch.Generator().manual_seed(4))
    rnd = _pq(g, lab)
    assert abs(rnd.modularity - brute_modularity(g, lab)) <= 1e-12
    assert rnd.num_communities == lab.unique().numel()
    assert rnd.coverage == pytest.approx(
        rnd.intra_weight / rnd.total_weight, abs=1e-15)
    for lb in (torch.arange(g.nv), lab):
        assert abs(_pq(g, lb).modularity - brute_modularity(g, lb)) <= 1e-12


# ---- 2. self-loops and parallel edges, exact -------------------------------

@pytest.mark.parametrize("wdtype", [torch.float32, torch.float64])
def test_self_loops_and_parallel_edges_exact(wdtype):
    g = dup_graph()
    src = torch.repeat_interleave(torch.arange(g.nv), g.degrees())
    assert int((g.tails == src).sum()) > 0          # self-loops present
    key = src * g.nv + g.tails
    assert key.unique().numel() < key.numel()       # parallel edges present
    g = Graph(g.rowptr, g.tails, g.weights.to(wdtype))
    gen = torch.Generator().manual_seed(9)
    for ncomm in (1, 3, g.nv):
        lab = torch.randint(0, ncomm, (g.nv,), generator=gen)
        ref = edge_list_intra(g, lab)
        # a tiny chunk forces many chunk boundaries inside rows
        for chunk in (7, 1 << 24):
            got = intra_weight_torch(g.rowptr, g.tails.to(torch.int32),
                                     g.weights, lab, chunk=chunk)
            assert got.dtype == torch.float64
            assert torch.equal(got, ref)
        q = _pq(g, lab)
        assert q.intra_weight == float(ref.sum())
        assert q.total_weight == float(g.weights.double().sum())
        assert abs(q.modularity - brute_modularity(g, lab)) <= 1e-12


def test_edgeless_graph_scores_zero():
    g = Graph(torch.zeros(6, dtype=torch.int64),
              torch.empty(0, dtype=torch.int64),
              torch.empty(0, dtype=torch.float64))
    q = _pq(g, torch.tensor([0, 0, 1, 4, 4]))
    assert q.modularity == 0.0 and q.total_weight == 0.0
    assert q.coverage == 0.0 and q.num_communities == 3


# ---- 3. ranks 1, 2, 4; contiguous and edge-balanced ------------------------

def _labelings(name):
    """Labelings scored on every rank count: the cold-run partition, and the
    same partition with ids mirrored to the top of the id range, which moves
    every community's owner to the last rank(s)."""
    g = whole_graph(name)
    if name == "karate2":
        return {"fold": torch.arange(g.nv) % (g.nv // 2)}
    lab = cold_run(name).communities
    return {"cold": lab, "mirrored": g.nv - 1 - lab}


def _w_quality(rank, world, balanced, labelings):
    # the labelings come from the parent: a cold run needs a single-rank Comm
    out = {}
    for name in ("rgg", "lfr", "karate2"):
        g = whole_graph(name)
        dg = shard(g, rank, world, balanced)
        comm = Comm()
        from cuvite_amd.halo import build_halo
        halo = build_halo(dg, comm)
        for lname, lab in labelings[name].items():
            q = partition_quality(dg, lab[dg.base:dg.bound].clone(), comm,
                                  halo=halo, backend="torch")
            # owner-without-members: communities this rank owns (size > 0
            # after the push) that none of its own vertices carries
            mine = lab[dg.base:dg.bound]
            owned = lab[(lab >= dg.base) & (lab < dg.bound)].unique()
            orphan = int((~torch.isin(owned, mine)).sum())
            out[(name, lname)] = (q.modularity, q.num_communities,
                                  q.intra_weight, q.total_weight,
                                  int(halo.ng), orphan)
    return out


@pytest.mark.parametrize("balanced", [False, True], ids=["contig", "balanced"])
@pytest.mark.parametrize("world", [2, 4])
def test_partition_quality_rank_invariant(world, balanced):
    ref = {}
    labelings = {n: _labelings(n) for n in ("rgg", "lfr", "karate2")}
    for name in labelings:
        g = whole_graph(name)
        for lname, lab in labelings[name].items():
            q = _pq(g, lab)
            assert abs(q.modularity - brute_modularity(g, lab)) <= 1e-12
            ref[(name, lname)] = q
    outs = run_dist(world, _w_quality, balanced, labelings)
    for key, q in ref.items():
        for o in outs:
            mod, ncomm, intra, tw, ng, orphan = o[key]
            assert abs(mod - q.modularity) <= 1e-12, (key, mod, q.modularity)
            assert ncomm == q.num_communities
            assert tw == pytest.approx(q.total_weight, rel=1e-12)
        assert all(o[key][:2] == outs[0][key][:2] for o in outs)
    # the mirrored labeling puts communities on an owner without members
    # (rgg communities are local in vertex id; the last rank owns them all)
    assert sum(o[("rgg", "mirrored")][5] for o in outs) > 0
    assert sum(o[("karate2", "fold")][5] for o in outs) == 0
    if world == 2 and not balanced:
        # two disjoint halves: no rank has a ghost, yet rank 1's vertices
        # all belong to communities that rank 0 owns
        assert [o[("karate2", "fold")][4] for o in outs] == [0, 0]
    assert all(o[("rgg", "cold")][4] > 0 for o in outs)


# ---- 7. bad labels ----------------------------------------------------------

def _bad(kind, n, nv_global):
    lab = torch.zeros(n, dtype=torch.int64)
    if kind == "length":
        return lab[:-1]
    if kind == "negative":
        lab[0] = -1
    elif kind == "too_big":
        lab[-1] = nv_global
    elif kind == "dtype":
        return lab.to(torch.int32)
    return lab


@pytest.mark.parametrize("kind", ["length", "negative", "too_big", "dtype"])
def test_bad_labels_raise(kind):
    from cuvite_amd.louvain import PhaseState, louvain
    g = whole_graph("karate")
    dg = single_partition(g)
    with pytest.raises(ValueError):
        partition_quality(dg, _bad(kind, g.nv, g.nv), Comm(), backend="torch")
    with pytest.raises(ValueError):
        louvain(dg, Comm(), init_labels=_bad(kind, g.nv, g.nv))
    with pytest.raises(ValueError):
        PhaseState(dg, Comm(), init_labels=_bad(kind, g.nv, g.nv))


def _w_bad(rank, world):
    from cuvite_amd.louvain import LouvainConfig, louvain
    g = whole_graph("karate")
    dg = shard(g, rank, world)
    comm = Comm()
    raised = []
    for kind in ("length", "negative", "too_big"):
        # only rank 1's slice is bad
        lab = _bad(kind if rank == 1 else "ok", dg.nv, g.nv)
        for fn in (lambda: partition_quality(dg, lab, comm, backend="torch"),
                   lambda: louvain(dg, comm, LouvainConfig(backend="torch"),
                                   init_labels=lab)):
            try:
                fn()
                raised.append(False)
            except ValueError:
                raised.append(True)
    # still in step with the peer after six rejected calls
    ok = partition_quality(dg, _bad("ok", dg.nv, g.nv), comm, backend="torch")
    return raised, ok.num_communities


def test_bad_labels_raise_on_every_rank():
    outs = run_dist(2, _w_bad)
    for raised, ncomm in outs:
        assert raised == [True] * 6
        assert ncomm == 1


# ---- 8. CLI ------------------------------------------------------------------

def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run(
        [sys.executable, "-m", "cuvite_amd", "--device", "cpu", "--backend",
         "torch"] + args, capture_output=True, text=True, cwd=cwd, env=env,
        timeout=300)


def _field(stdout, prefix, key):
    line = [ln for ln in stdout.splitlines() if ln.startswith(prefix)]
    assert len(line) == 1, stdout
    return line[0].split(key)[1].split()[0].strip("()")


def test_cli_score_init_and_exact(tmp_path):
    gfile = str(tmp_path / "g.bin")
    r = _cli(["-n", "512", "-e", "3", "-s", gfile, "-o",
              "--exact-modularity"], tmp_path)
    assert r.returncode == 0, r.stderr
    exact = float(_field(r.stdout, "Exact modularity:", "Exact modularity:"))
    ncomm = int(r.stdout.split("Exact modularity:")[1].split("(")[1].split()[0])
    dump = gfile + ".communities"
    assert os.path.exists(dump)

    # scoring the dump reproduces the run's exact value
    r2 = _cli(["-f", gfile, "--score-communities", dump], tmp_path)
    assert r2.returncode == 0, r2.stderr
    assert "Final modularity" not in r2.stdout      # no clustering
    q = float(_field(r2.stdout, f"Partition {dump}:", "modularity="))
    assert abs(q - exact) <= 1e-12
    assert int(_field(r2.stdout, "Partition ", "communities=")) == ncomm
    cov = float(_field(r2.stdout, "Partition ", "coverage="))
    assert q < cov <= 1.0

    # the value is independent of the file's id space: 1-based ids with gaps
    lab = np.loadtxt(dump, dtype=np.int64)
    gappy = str(tmp_path / "gappy.txt")
    np.savetxt(gappy, lab * 7 + 1 + 10 * len(lab), fmt="%d")
    r3 = _cli(["-f", gfile, "--score-communities", gappy, "-z"], tmp_path)
    assert r3.returncode == 0, r3.stderr
    assert abs(float(_field(r3.stdout, "Partition ", "modularity=")) - q) \
        <= 1e-12

    # warm start prints the same initial score with and without the
    # per-rank degree relabelling (pins the direction of the permutation)
    init = []
    for extra in ([], ["--vertex-order", "degree"]):
        r4 = _cli(["-f", gfile, "--init-communities", dump,
                   "--exact-modularity"] + extra, tmp_path)
        assert r4.returncode == 0, r4.stderr
        init.append(float(_field(r4.stdout, "Initial partition:",
                                 "modularity=")))
        assert int(_field(r4.stdout, "Initial partition:",
                          "communities=")) == ncomm
        after = float(_field(r4.stdout, "Exact modularity:",
                             "Exact modularity:"))
        assert after >= init[-1] - 1e-9
    assert abs(init[0] - q) <= 1e-12
    assert abs(init[1] - q) <= 1e-12


def test_cli_wrong_line_count_and_no_new_lines(tmp_path):
    short = tmp_path / "short.txt"
    short.write_text("0\n1\n2\n")
    for flag in ("--score-communities", "--init-communities"):
        r = _cli(["--karate", flag, str(short)], tmp_path)
        assert r.returncode != 0
        assert "3 entries" in r.stderr and "34 vertices" in r.stderr
    r = _cli(["--karate", "--score-communities", str(tmp_path / "nope")],
             tmp_path)
    assert r.returncode != 0 and "nope" in r.stderr
    plain = _cli(["--karate"], tmp_path)
    assert plain.returncode == 0, plain.stderr
    for new in ("Exact modularity", "Initial partition", "Partition "):
        assert new not in plain.stdout
