"""The dynamic-frontier phase on the CPU oracle: the frontier rule and its
invariant, the edge-batch graph layer, rank invariance and the CLI."""

import os
import subprocess
import sys

import pytest
import torch

from tests.dist_utils import run_dist

from cuvite_amd import (EdgeBatch, affected_vertices, apply_edge_batch,
                        frontier_expand_torch, partition_quality,
                        run_frontier_phase)
from cuvite_amd.dynamic import ghost_reverse_csr
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.io import write_communities, write_dist_graph
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm
from cuvite_amd.quality import intra_weight_torch

import dynamic_cases as dyc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = LouvainConfig(backend="torch")


def _q(g, labels):
    return partition_quality(single_partition(g), labels, Comm(),
                             backend="torch").modularity


# ---- the frontier phase -----------------------------------------------------

@pytest.mark.parametrize("name", ["karate", "lfr", "dup"])
def test_full_frontier_without_expansion_is_warm_start(name):
    g, _, prev, _ = dyc.perturbed(name, 0.05)
    dg = single_partition(g)
    ref = louvain(dg, Comm(), LouvainConfig(backend="torch", one_phase=True),
                  init_labels=prev.clone())
    est, lab, it, _, rep = run_frontier_phase(
        dg, Comm(), CFG, prev.clone(), torch.ones(g.nv, dtype=torch.bool),
        expand=False)
    assert it == ref.total_iters and rep.sweeps == it
    assert rep.sizes_per_sweep == [g.nv] * it
    if ref.modularity_per_level:        # the phase gained: labels returned
        assert torch.equal(lab, ref.communities)
        assert est == ref.modularity


class _Recorder:
    def __init__(self):
        self.begin, self.end = [], []

    def __call__(self, event, **kw):
        getattr(self, event).append(kw)


@pytest.mark.parametrize("frac", [0.05, 0.3])
def test_cw_invariant_and_estimate_with_integer_weights(frac):
    g, _, prev, f0 = dyc.perturbed("dup", frac)
    dg = single_partition(g)
    rec = _Recorder()
    _, _, it, _, rep = run_frontier_phase(dg, Comm(), CFG, prev.clone(),
                                          f0.clone(), observe=rec)
    assert len(rec.begin) == len(rec.end) == it >= 2
    tails32 = g.tails.to(torch.int32)
    vdeg = dg.local_degree_sum()
    c = 1.0 / float(vdeg.sum())
    moved_any = False
    for k, (b, e) in enumerate(zip(rec.begin, rec.end)):
        iw = intra_weight_torch(g.rowptr, tails32, g.weights, b["curr"])
        outside = ~b["active"]
        # cw is current for every vertex the sweep will not evaluate (in the
        # first sweep: for all of them)
        assert torch.equal(b["cw"][outside], iw[outside])
        if k == 0:
            assert torch.equal(b["cw"], iw)
        # a vertex outside the frontier keeps its label
        assert torch.equal(e["target"][outside], b["curr"][outside])
        moved_any |= bool((e["target"] != b["curr"]).any())
        # after the sweep cw is the full recomputation under the labels the
        # sweep started from, and so is the estimate
        assert torch.equal(e["cw"], iw)
        deg = torch.zeros(g.nv, dtype=torch.float64).index_add_(
            0, e["target"], vdeg)
        full = float(iw.sum()) * c - float((deg ** 2).sum()) * c * c
        assert abs(e["estimate"] - full) < 1e-12
        assert rep.sizes_per_sweep[k] == int(b["active"].sum())
    assert moved_any
    assert rep.evaluated == sum(rep.sizes_per_sweep)


def test_next_frontier_is_moved_and_neighbours():
    g, _, prev, f0 = dyc.perturbed("lfr", 0.01)
    rec = _Recorder()
    run_frontier_phase(single_partition(g), Comm(), CFG, prev.clone(),
                       f0.clone(), observe=rec)
    assert torch.equal(rec.begin[0]["active"], f0)
    g_rowptr, g_heads = ghost_reverse_csr(g.rowptr, g.tails.to(torch.int32),
                                          0)
    for b, e, nxt in zip(rec.begin, rec.end, rec.begin[1:]):
        moved = (e["target"] != b["curr"]).nonzero(as_tuple=True)[0]
        want = dyc.expand_loop(moved, g.rowptr, g.tails, g_rowptr, g_heads)
        assert torch.equal(nxt["active"], want)


def _hand_graph(rows, n_ghost):
    rowptr = torch.zeros(len(rows) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    tails = torch.tensor([t for r in rows for t in r], dtype=torch.int32)
    return (rowptr, tails) + ghost_reverse_csr(rowptr, tails, n_ghost)


@pytest.mark.parametrize("changed", [[], [0], [1], [2], [3], [4], [5, 6],
                                     [5], [6], [0, 1, 2, 3, 4, 5, 6],
                                     [2, 2, 5]])
def test_frontier_expand_torch_against_a_loop(changed):
    """Vertex 0 is isolated, 1 has only a self-loop, 2-3-4 is a path with a
    parallel edge, 3 and 4 see ghost 5, nobody sees ghost 6."""
    case = _hand_graph([[], [1], [3, 3], [2, 2, 4, 5], [3, 5]], 2)
    ch = torch.tensor(changed, dtype=torch.int32)
    got = frontier_expand_torch(ch, *case, torch.zeros(5, dtype=torch.bool))
    assert torch.equal(got, dyc.expand_loop(ch, *case))
    expect = {(): [], (0,): [0], (1,): [1], (5,): [3, 4], (6,): [],
              (2,): [2, 3]}.get(tuple(changed))
    if expect is not None:
        assert got.nonzero(as_tuple=True)[0].tolist() == expect


@pytest.mark.parametrize("frac,n0", [(0.001, 42), (0.01, 353), (0.05, 1234)])
def test_lfr_batches_keep_quality_and_touch_few(frac, n0):
    g, _, prev, f0 = dyc.perturbed("lfr", frac)
    assert int(f0.sum()) == n0          # the recipe's recorded frontier
    _, lab, _, rep = dyc.oracle_run("lfr", frac)
    q_new, q_prev = _q(g, lab), _q(g, prev)
    print(f"lfr {frac}: sizes {rep.sizes_per_sweep} Q {q_new:.6f} "
          f"(prev on new graph {q_prev:.6f})")
    assert q_new >= q_prev
    if frac < 0.05:
        assert rep.evaluated < g.nv


def test_louvain_init_frontier_report_and_checks():
    g, _, prev, f0 = dyc.perturbed("lfr", 0.01)
    dg = single_partition(g)
    res = louvain(dg, Comm(), CFG, init_labels=prev.clone(),
                  init_frontier=f0.clone())
    rep = res.levels[0]["frontier"]
    assert rep.sizes_per_sweep == dyc.oracle_run("lfr", 0.01)[3].sizes_per_sweep
    assert res.levels[0]["iters"] == rep.sweeps
    assert all("frontier" not in lv for lv in res.levels[1:])
    assert _q(g, res.communities) >= _q(g, prev)
    with pytest.raises(ValueError):
        louvain(dg, Comm(), CFG, init_frontier=f0)
    for kw in (dict(coloring=True), dict(ordering=True), dict(early_term=1),
               dict(threshold_scaling=True)):
        with pytest.raises(ValueError):
            louvain(dg, Comm(), LouvainConfig(backend="torch", **kw),
                    init_labels=prev, init_frontier=f0)
    with pytest.raises(ValueError):
        louvain(dg, Comm(), CFG, init_labels=prev,
                init_frontier=f0.to(torch.int64))
    with pytest.raises(ValueError):
        louvain(dg, Comm(), CFG, init_labels=prev, init_frontier=f0[:-1])


@pytest.mark.parametrize("kw", [dict(algorithm="leiden"),
                                dict(connectivity="final"),
                                dict(one_phase=True)])
def test_init_frontier_composes(kw):
    g, _, prev, f0 = dyc.perturbed("lfr", 0.01)
    res = louvain(single_partition(g), Comm(),
                  LouvainConfig(backend="torch", **kw),
                  init_labels=prev.clone(), init_frontier=f0.clone())
    assert "frontier" in res.levels[0]
    assert _q(g, res.communities) >= _q(g, prev)


# ---- edge batches -----------------------------------------------------------

def _same_csr(a: Graph, b: Graph):
    ka, wa = dyc.csr_key(a)
    kb, wb = dyc.csr_key(b)
    return torch.equal(a.rowptr, b.rowptr) and torch.equal(ka, kb) \
        and torch.equal(wa, wb)


def _batch(ins=(), dels=()):
    i64 = torch.int64
    return EdgeBatch(torch.tensor([e[0] for e in ins], dtype=i64),
                     torch.tensor([e[1] for e in ins], dtype=i64),
                     torch.tensor([e[2] for e in ins], dtype=torch.float64),
                     torch.tensor([e[0] for e in dels], dtype=i64),
                     torch.tensor([e[1] for e in dels], dtype=i64))


def test_apply_edge_batch_round_trip():
    g = dyc.base_graph("karate")
    dg = single_partition(g)
    assert int(((g.tails == 20) & (torch.repeat_interleave(
        torch.arange(g.nv), g.degrees()) == 9)).sum()) == 0
    up = apply_edge_batch(dg, Comm(), _batch(ins=[(9, 20, 2.0), (4, 4, 3.0)]))
    assert up.ne == g.ne + 3                    # two directions + one loop
    back = apply_edge_batch(up, Comm(), _batch(dels=[(20, 9), (4, 4)]))
    assert _same_csr(back.g, g)
    assert _same_csr(apply_edge_batch(dg, Comm(), EdgeBatch.empty()).g, g)


def test_apply_edge_batch_parallel_edges_and_self_loops():
    g = dyc.base_graph("karate")
    dg = single_partition(g)
    # 0-1 exists: inserting it again stores a parallel edge in both rows
    up = apply_edge_batch(dg, Comm(), _batch(ins=[(0, 1, 5.0), (1, 0, 7.0)]))
    row0 = up.g.tails[up.g.rowptr[0]:up.g.rowptr[1]]
    row1 = up.g.tails[up.g.rowptr[1]:up.g.rowptr[2]]
    assert int((row0 == 1).sum()) == 3 and int((row1 == 0).sum()) == 3
    assert float(up.g.weights.sum()) == float(g.weights.sum()) + 24.0
    # one deletion removes every copy from both rows
    down = apply_edge_batch(up, Comm(), _batch(dels=[(1, 0)]))
    assert down.ne == g.ne - 2
    row0 = down.g.tails[down.g.rowptr[0]:down.g.rowptr[1]]
    assert int((row0 == 1).sum()) == 0
    # a self-loop is stored once; deleted and inserted in one batch
    loop = apply_edge_batch(dg, Comm(), _batch(ins=[(3, 3, 1.0)]))
    assert loop.ne == g.ne + 1
    swap = apply_edge_batch(loop, Comm(), _batch(ins=[(3, 3, 2.0)],
                                                 dels=[(3, 3)]))
    r3 = slice(int(swap.g.rowptr[3]), int(swap.g.rowptr[4]))
    assert swap.g.weights[r3][swap.g.tails[r3] == 3].tolist() == [2.0]


def test_apply_edge_batch_rejects():
    dg = single_partition(dyc.base_graph("karate"))
    with pytest.raises(ValueError):
        apply_edge_batch(dg, Comm(), _batch(dels=[(9, 20)]))
    with pytest.raises(ValueError):
        apply_edge_batch(dg, Comm(), _batch(ins=[(0, 34, 1.0)]))


def test_affected_vertices_rule():
    g = dyc.base_graph("karate")
    prev = dyc.prev_labels("karate")
    s, d = dyc.undirected_pairs(g)
    same = prev[s] == prev[d]
    a, b = int(same.nonzero()[0, 0]), int((~same).nonzero()[0, 0])
    dels = [(int(s[a]), int(d[a])), (int(s[b]), int(d[b]))]
    u = 0
    v_same = int(((prev == prev[u]) & (torch.arange(g.nv) != u)).nonzero()[0, 0])
    v_diff = int((prev != prev[u]).nonzero()[0, 0])
    batch = _batch(ins=[(u, v_same, 1.0), (v_diff, u, 1.0), (7, 7, 1.0)],
                   dels=dels)
    dg = apply_edge_batch(single_partition(g), Comm(), batch)
    mask = affected_vertices(dg, Comm(), prev, batch)
    want = sorted({dels[0][0], dels[0][1], u, v_diff})
    assert mask.nonzero(as_tuple=True)[0].tolist() == want


# ---- ranks ------------------------------------------------------------------

def _w_update(rank, world, name, frac, balanced, prev):
    return dyc.dist_update(rank, world, Comm(), torch.device("cpu"), "torch",
                           name, frac, balanced, prev)


@pytest.mark.parametrize("balanced", [False, True],
                         ids=["contiguous", "balanced"])
@pytest.mark.parametrize("world", [2, 3])
def test_update_is_rank_invariant(world, balanced):
    name, frac = "lfr", 0.01
    g, _, prev, f0 = dyc.perturbed(name, frac)
    _, lab, it, rep = dyc.oracle_run(name, frac)
    one = dyc.dist_update(0, 1, Comm(), torch.device("cpu"), "torch", name,
                          frac, balanced, prev)
    assert torch.equal(one["labels"], lab) and one["sizes"] == \
        rep.sizes_per_sweep
    parts = run_dist(world, _w_update, name, frac, balanced, prev)
    key, w = dyc.csr_key(g)
    assert torch.equal(torch.cat([p["key"] for p in parts]), key)
    assert torch.equal(torch.cat([p["w"] for p in parts]), w)
    assert torch.equal(torch.cat([p["f0"] for p in parts]), f0)
    assert torch.equal(torch.cat([p["labels"] for p in parts]), lab)
    for p in parts:
        assert p["sizes"] == rep.sizes_per_sweep and p["sweeps"] == it
        assert all(abs(a - b) < 1e-12
                   for a, b in zip(p["estimates"], rep.estimates))


def _w_absent(rank, world):
    from quality_cases import shard
    dg = shard(dyc.base_graph("karate"), rank, world)
    # only rank 1's share is bad, and the missing edge lives on rank 0
    share = _batch(dels=[(0, 9)]) if rank == 1 else EdgeBatch.empty()
    try:
        apply_edge_batch(dg, Comm(), share)
    except ValueError:
        return True
    return False


def test_absent_deletion_raises_on_every_rank():
    assert run_dist(2, _w_absent) == [True, True]


# ---- CLI --------------------------------------------------------------------

def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run(
        [sys.executable, "-m", "cuvite_amd", "--device", "cpu"] + args,
        capture_output=True, text=True, cwd=cwd, env=env, timeout=300)


def test_cli_update_edges_round_trip(tmp_path):
    g = dyc.base_graph("lfr")
    batch = dyc.recipe_batch(g, 0.01)
    _, _, prev, f0 = dyc.perturbed("lfr", 0.01)
    rep = dyc.oracle_run("lfr", 0.01)[3]
    gfile, cfile, ufile = (str(tmp_path / n) for n in
                           ("old.bin", "old.communities", "update.txt"))
    write_dist_graph(gfile, [single_partition(g)])
    write_communities(cfile, prev)
    with open(ufile, "w") as f:
        f.write("# one percent of the edges\n")
        for u, v in zip(batch.del_src.tolist(), batch.del_dst.tolist()):
            f.write(f"d {u} {v}\n")
        for i, (u, v) in enumerate(zip(batch.ins_src.tolist(),
                                       batch.ins_dst.tolist())):
            f.write(f"a {u} {v}\n" if i % 2 else f"a {u} {v} 1.0  # w\n")
    r = _cli(["-f", gfile, "--init-communities", cfile, "--update-edges",
              ufile, "-p", "--exact-modularity"], tmp_path)
    assert r.returncode == 0, r.stderr
    out = r.stdout
    assert (f"Edge batch: inserted={batch.ins_src.numel()} "
            f"deleted={batch.del_src.numel()} affected={int(f0.sum())}") in out
    assert (f"Frontier phase: sweeps={rep.sweeps} evaluated={rep.evaluated} "
            f"of {rep.sweeps * g.nv}") in out
    assert "Final modularity" in out and "Exact modularity" in out


def test_cli_update_edges_option_checks(tmp_path):
    ufile = str(tmp_path / "u.txt")
    with open(ufile, "w") as f:
        f.write("a 0 9\n")
    from cuvite_amd.cli import build_parser, validate
    cfile = str(tmp_path / "c.communities")
    write_communities(cfile, dyc.prev_labels("karate"))
    with pytest.raises(SystemExit, match="--init-communities"):
        validate(build_parser().parse_args(
            ["--karate", "--update-edges", ufile]), 1)
    for extra in (["-c", "4"], ["-d", "4"], ["-t", "1"], ["-i"]):
        with pytest.raises(SystemExit, match="cannot be combined"):
            validate(build_parser().parse_args(
                ["--karate", "--init-communities", cfile, "--update-edges",
                 ufile] + extra), 1)
    validate(build_parser().parse_args(
        ["--karate", "--init-communities", cfile, "--update-edges", ufile,
         "-p", "--leiden"]), 1)
    with open(ufile, "w") as f:
        f.write("d 9 20\n")                 # not an edge of the karate club
    r = _cli(["--karate", "--init-communities", cfile, "--update-edges",
              ufile], tmp_path)
    assert r.returncode != 0 and "does not hold" in r.stderr
    with open(ufile, "w") as f:
        f.write("x 1 2\n")
    r = _cli(["--karate", "--init-communities", cfile, "--update-edges",
              ufile], tmp_path)
    assert r.returncode != 0 and "expected" in r.stderr
