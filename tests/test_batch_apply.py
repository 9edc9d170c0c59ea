"""Edge batches on the CPU: the stable-rows twin against a python loop and
against apply_edge_batch's rebuild, on one and on several ranks; a stream of
batches (update_stream) against the explicit loop; the CLI with several
--update-edges files.

Every weight is an integer or is copied, so every comparison is exact."""

import os
import re
import subprocess
import sys

import pytest
import torch

from tests.dist_utils import run_dist

from cuvite_amd import (EdgeBatch, StreamError, StreamStep, affected_vertices,
                        apply_edge_batch, apply_routed_batch_torch,
                        update_stream)
from cuvite_amd.dynamic import _route_batch
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.io import (load_ground_truth, write_communities,
                           write_dist_graph)
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

import batch_cases as bc
import dynamic_cases as dyc
from quality_cases import shard

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = LouvainConfig(backend="torch")
SPAN = 1024   # the edge-batch kernels' span; the CPU tests need no extension
GRAPHS = ("karate", "lfr", "rmat12", "dup")
FRACS = (0.001, 0.01, 0.05, 0.5)


# ---- the twin ---------------------------------------------------------------

@pytest.mark.parametrize("name", bc.NAMED)
def test_twin_matches_python_loop(name):
    g = bc.span_graph(SPAN)
    lists = bc.routed(bc.named_batches(SPAN)[name])
    before = (g.rowptr.clone(), g.tails.clone(), g.weights.clone())
    got = apply_routed_batch_torch(g, 0, g.nv, *lists)
    rowptr, tails, weights = bc.loop_apply(g, 0, *lists)
    assert got.rowptr.tolist() == rowptr
    assert got.tails.tolist() == tails
    assert got.weights.tolist() == weights
    assert got.weights.dtype == g.weights.dtype
    assert bc.same_graph(g, Graph(*before))
    if name == "empty":
        assert bc.same_graph(got, g)


def test_twin_copies_weights_in_fp32():
    g64 = bc.span_graph(SPAN)
    g = Graph(g64.rowptr, g64.tails, g64.weights.to(torch.float32))
    lists = bc.routed(bc.named_batches(SPAN)["mixed"])
    got = apply_routed_batch_torch(g, 0, g.nv, *lists)
    ref = apply_routed_batch_torch(g64, 0, g.nv, *lists)
    assert got.weights.dtype == torch.float32
    assert torch.equal(got.tails, ref.tails)
    assert torch.equal(got.weights.to(torch.float64), ref.weights)


def _twin_vs_rebuild(rank, world, balanced):
    """Every graph and fraction on this rank: the twin of the routed lists
    and apply_edge_batch's graph, rows sorted by (dst, weight). Returns the
    cases that differ."""
    if world > 1:
        torch.set_num_threads(4)   # several rank processes share the host
    bad = []
    for name in GRAPHS:
        g = dyc.base_graph(name)
        old = shard(g, rank, world, balanced)
        for frac in FRACS:
            share = dyc.share_of(dyc.recipe_batch(g, frac), rank, world)
            comm = Comm()
            new = apply_edge_batch(old, comm, share)
            lists = _route_batch(old, comm, share)
            twin = apply_routed_batch_torch(old.g, old.base, g.nv, *lists)
            same = all(torch.equal(a, b) for a, b in zip(
                bc.sorted_rows(twin), bc.sorted_rows(new.g)))
            if not same or twin.weights.dtype != new.g.weights.dtype:
                bad.append((name, frac))
    return bad


def test_twin_matches_rebuild_one_rank():
    assert _twin_vs_rebuild(0, 1, False) == []
    # rmat12 and dup hold parallel edges: the comparison covers them
    for name in ("rmat12", "dup"):
        g = dyc.base_graph(name)
        src = torch.repeat_interleave(torch.arange(g.nv), g.degrees())
        key = src * g.nv + g.tails
        assert torch.unique(key).numel() < key.numel()


@pytest.mark.parametrize("balanced", [False, True],
                         ids=["contiguous", "balanced"])
@pytest.mark.parametrize("world", [2, 3])
def test_twin_matches_rebuild_on_ranks(world, balanced):
    assert run_dist(world, _twin_vs_rebuild, balanced) == [[]] * world


def _w_absent(rank, world):
    g = bc.span_graph(SPAN)
    old = shard(g, rank, world)
    before = (old.g.rowptr.clone(), old.g.tails.clone(),
              old.g.weights.clone())
    # only rank 1's share is bad
    share = bc.named_batches(SPAN)["absent"] if rank == world - 1 \
        else EdgeBatch.empty()
    try:
        apply_edge_batch(old, Comm(), share)
        raised = False
    except ValueError:
        raised = True
    return raised and bc.same_graph(old.g, Graph(*before))


def test_absent_raises_everywhere_and_leaves_the_graph():
    g = bc.span_graph(SPAN)
    lists = bc.routed(bc.named_batches(SPAN)["absent"])
    before = (g.rowptr.clone(), g.tails.clone(), g.weights.clone())
    assert bc.loop_apply(g, 0, *lists) is None
    with pytest.raises(ValueError, match="does not hold"):
        apply_routed_batch_torch(g, 0, g.nv, *lists)
    assert bc.same_graph(g, Graph(*before))
    assert _w_absent(0, 1)
    assert run_dist(2, _w_absent) == [True, True]


# ---- a stream of batches ----------------------------------------------------

def _step_facts(step: StreamStep):
    res = step.result
    return {"inserted": step.inserted, "deleted": step.deleted,
            "affected": step.affected, "labels": res.communities.cpu(),
            "sweeps": res.levels[0]["frontier"].sweeps,
            "sizes": list(res.levels[0]["frontier"].sizes_per_sweep),
            "iters": res.total_iters, "phases": res.phases}


def _w_stream(rank, world, prev):
    g = dyc.base_graph("lfr")
    old = shard(g, rank, world)
    shares = [dyc.share_of(b, rank, world) for b in bc.stream_batches()]
    dg, steps = update_stream(old, Comm(), CFG, prev[old.base:old.bound],
                              shares)
    return [_step_facts(s) for s in steps], bc.sorted_rows(dg.g)


def test_update_stream_equals_explicit_loop():
    g = dyc.base_graph("lfr")
    prev = dyc.prev_labels("lfr")
    batches = bc.stream_batches()
    dg_end, steps = update_stream(single_partition(g), Comm(), CFG, prev,
                                  batches)
    assert len(steps) == 3
    dg, labels = single_partition(g), prev
    for batch, step in zip(batches, steps):
        dg = apply_edge_batch(dg, Comm(), batch)
        mask = affected_vertices(dg, Comm(), labels, batch)
        res = louvain(dg, Comm(), CFG, init_labels=labels,
                      init_frontier=mask)
        assert step.inserted == batch.ins_src.numel()
        assert step.deleted == batch.del_src.numel()
        assert step.affected == int(mask.sum()) > 0
        assert torch.equal(step.result.communities, res.communities)
        assert step.result.total_iters == res.total_iters
        assert step.result.levels[0]["frontier"].sweeps == \
            res.levels[0]["frontier"].sweeps
        assert step.result.modularity == res.modularity
        labels = res.communities
    assert bc.same_graph(dg_end.g, dg.g)
    # the stream's graph is the old one after all changes at once
    once = apply_edge_batch(single_partition(g), Comm(),
                            bc.concat_batches(batches))
    assert all(torch.equal(a, b) for a, b in zip(bc.sorted_rows(dg_end.g),
                                                 bc.sorted_rows(once.g)))
    assert bc.same_graph(g, dyc.base_graph("lfr"))


def test_update_stream_is_rank_invariant():
    prev = dyc.prev_labels("lfr")
    one_steps, one_rows = _w_stream(0, 1, prev)
    outs = run_dist(2, _w_stream, prev)
    for k, ref in enumerate(one_steps):
        parts = [o[0][k] for o in outs]
        assert torch.equal(torch.cat([p["labels"] for p in parts]),
                           ref["labels"])
        for p in parts:
            for key in ("inserted", "deleted", "affected", "sweeps", "sizes",
                        "iters", "phases"):
                assert p[key] == ref[key], (k, key)
    # rowptr restarts on every rank; tails and weights concatenate
    for i in (1, 2):
        assert torch.equal(torch.cat([o[1][i] for o in outs]), one_rows[i])


def test_update_stream_rejects_and_bad_batch():
    dg = single_partition(dyc.base_graph("karate"))
    prev = dyc.prev_labels("karate")
    for kw in (dict(coloring=True), dict(ordering=True), dict(early_term=1),
               dict(threshold_scaling=True)):
        with pytest.raises(ValueError, match="cannot be combined"):
            update_stream(dg, Comm(), LouvainConfig(backend="torch", **kw),
                          prev, [EdgeBatch.empty()])
    i64 = torch.int64
    good = EdgeBatch(torch.tensor([0]), torch.tensor([9]),
                     torch.ones(1, dtype=torch.float64),
                     torch.empty(0, dtype=i64), torch.empty(0, dtype=i64))
    bad = EdgeBatch(torch.empty(0, dtype=i64), torch.empty(0, dtype=i64),
                    torch.empty(0, dtype=torch.float64), torch.tensor([9]),
                    torch.tensor([20]))   # not an edge of the karate club
    with pytest.raises(StreamError, match="does not hold") as info:
        update_stream(dg, Comm(), CFG, prev, [good, bad, good])
    assert isinstance(info.value, ValueError)
    # the first step stands
    steps = info.value.steps
    assert len(steps) == 1 and steps[0].inserted == 1
    ref = update_stream(dg, Comm(), CFG, prev, [good])[1][0]
    assert torch.equal(steps[0].result.communities, ref.result.communities)
    assert info.value.dg.ne == dg.ne + 2


# ---- CLI --------------------------------------------------------------------

def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run(
        [sys.executable, "-m", "cuvite_amd", "--device", "cpu"] + args,
        capture_output=True, text=True, cwd=cwd, env=env, timeout=300)


def _write_batch(path, batch):
    with open(path, "w") as f:
        for u, v in zip(batch.del_src.tolist(), batch.del_dst.tolist()):
            f.write(f"d {u} {v}\n")
        for u, v, w in zip(batch.ins_src.tolist(), batch.ins_dst.tolist(),
                           batch.ins_w.tolist()):
            f.write(f"a {u} {v} {w}\n")


def _masked(out):
    """CLI output with its run-to-run figures (times, TEPS, memory) masked."""
    out = re.sub(r"(ingest=|time: )[0-9.]+s", r"\1<s>", out)
    out = re.sub(r"TEPS: \S+", "TEPS: <n>", out)
    return re.sub(r"rss \d+ MB", "rss <n> MB", out)


ONE_FILE_OUTPUT = """\
Graph: nv=2000 ne(directed)=24144 ranks=1 device=cpu ingest=<s>
Edge batch: inserted=120 deleted=121 affected=356
Initial partition: modularity=0.612594375787237 communities=28
Frontier phase: sweeps=4 evaluated=488 of 8000
Level 0: modularity = 0.613953
Final modularity: 0.613953
Phases: 2  Iterations: 6
Coloring time: <s>
Clustering time: <s>
Rebuild time: <s>
Total time: <s>  TEPS: <n>
Peak memory: host rss <n> MB
Exact modularity: 0.613952578360683 (28 communities)
"""


def test_cli_several_update_files(tmp_path):
    g = dyc.base_graph("lfr")
    prev = dyc.prev_labels("lfr")
    batches = bc.stream_batches()[:2]
    gfile, cfile = str(tmp_path / "old.bin"), str(tmp_path / "old.communities")
    ufiles = [str(tmp_path / f"u{k}.txt") for k in (1, 2)]
    write_dist_graph(gfile, [single_partition(g)])
    write_communities(cfile, prev)
    for path, batch in zip(ufiles, batches):
        _write_batch(path, batch)
    _, steps = update_stream(single_partition(g), Comm(), CFG, prev, batches)

    r = _cli(["-f", gfile, "--init-communities", cfile, "--update-edges",
              ufiles[0], "--update-edges", ufiles[1], "-o",
              "--exact-modularity"], tmp_path)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    heads = [i for i, ln in enumerate(lines) if ln.startswith("Batch ")]
    assert [lines[i] for i in heads] == [f"Batch 1/2: {ufiles[0]}",
                                         f"Batch 2/2: {ufiles[1]}"]
    for k, (i, step) in enumerate(zip(heads, steps)):
        block = lines[i + 1:heads[k + 1] if k == 0 else len(lines)]
        assert block[0] == (f"Edge batch: inserted={step.inserted} "
                            f"deleted={step.deleted} "
                            f"affected={step.affected}")
        fr = step.result.levels[0]["frontier"]
        assert (f"Frontier phase: sweeps={fr.sweeps} "
                f"evaluated={fr.evaluated} of {fr.sweeps * g.nv}") in block
        assert sum(ln.startswith("Final modularity") for ln in block) == 1
    # -o and --exact-modularity act on the last result, once
    assert sum(ln.startswith("Exact modularity") for ln in lines) == 1
    assert lines.index(f"Wrote communities to {gfile}.communities") > heads[1]
    dump = load_ground_truth(gfile + ".communities")
    assert torch.equal(dump, steps[-1].result.communities)

    # one file: the output is the one the CLI gave before several files were
    # allowed (recorded below from that version on these inputs), verbatim
    # but for the figures that change from run to run
    one = _cli(["-f", gfile, "--init-communities", cfile, "--update-edges",
                ufiles[0], "--exact-modularity"], tmp_path)
    assert one.returncode == 0, one.stderr
    assert _masked(one.stdout) == ONE_FILE_OUTPUT
    # and it is the first block of the two-file run
    first = lines[heads[0] + 1:heads[1]]
    assert [_masked(ln) for ln in first] == \
        ONE_FILE_OUTPUT.splitlines()[1:len(first) + 1]
