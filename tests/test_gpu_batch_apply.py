"""ops.apply_batch (mark / copy / compact / insert kernels) against its torch
twin, dynamic.apply_routed_batch_torch: bit for bit in rowptr, tails and
weights, the order inside every row included. Shapes are built around the
kernels' span (batch_cases.span_graph). Then the rebuild path behind
CUVITE_BATCH_DEVICE=0, two ranks on one GPU, and a stream of batches against
the CPU oracle.

Weights are small integers (span graph, dup) or 1 (rmat12, lfr): exact in
fp32 and fp64."""

import functools

import pytest
import torch

from cuvite_amd import (apply_edge_batch, apply_routed_batch_torch,
                        update_stream)
from cuvite_amd.dynamic import _route_batch
from cuvite_amd.graph import DistGraph, Graph, single_partition
from cuvite_amd.louvain import LouvainConfig
from cuvite_amd.parallel import Comm

from tests.dist_utils import run_dist

import batch_cases as bc
import dynamic_cases as dyc
from quality_cases import shard

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    return _ops


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _cast(g: Graph, wdtype) -> Graph:
    return Graph(g.rowptr, g.tails, g.weights.to(wdtype))


def _device_apply(ops, g: Graph, base, nvg, lists, dev):
    """ops.apply_batch on device copies; checks that the inputs come back
    unchanged. Returns a CPU Graph or None."""
    gd = g.to(dev)
    out = ops.apply_batch(gd.rowptr, gd.tails, gd.weights, base, nvg,
                          *[t.to(dev) for t in lists])
    assert bc.same_graph(gd, g)
    if out is None:
        return None
    return Graph(*[t.cpu() for t in out])


@functools.lru_cache(maxsize=None)
def _twin(span, name, wdtype):
    g = _cast(bc.span_graph(span), wdtype)
    return apply_routed_batch_torch(
        g, 0, g.nv, *bc.routed(bc.named_batches(span)[name]))


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("name", bc.NAMED)
def test_span_graph_batches_match_twin(ops, dev, monkeypatch, name, wdtype):
    span = ops.batch_span()
    g = _cast(bc.span_graph(span), wdtype)
    batch = bc.named_batches(span)[name]
    ref = _twin(span, name, wdtype)
    got = _device_apply(ops, g, 0, g.nv, bc.routed(batch), dev)
    assert got.weights.dtype == wdtype
    assert torch.equal(got.rowptr, ref.rowptr)
    bad = (got.tails != ref.tails) | (got.weights != ref.weights)
    assert not bool(bad.any()), bad.nonzero(as_tuple=True)[0][:20].tolist()
    if name == "empty":
        assert bc.same_graph(got, g)
    # apply_edge_batch takes the same path ...
    dg = single_partition(g).to(dev)
    new = apply_edge_batch(dg, Comm(dev), batch)
    assert bc.same_graph(new.g, ref)
    # ... and CUVITE_BATCH_DEVICE=0 the rebuild: same rows in another order
    monkeypatch.setenv("CUVITE_BATCH_DEVICE", "0")
    old = apply_edge_batch(dg, Comm(dev), batch)
    for a, b in zip(bc.sorted_rows(old.g), bc.sorted_rows(ref)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_absent_deletion_raises(ops, dev, monkeypatch, wdtype):
    span = ops.batch_span()
    g = _cast(bc.span_graph(span), wdtype)
    batch = bc.named_batches(span)["absent"]
    assert _device_apply(ops, g, 0, g.nv, bc.routed(batch), dev) is None
    dg = single_partition(g).to(dev)
    for knob in ("1", "0"):
        monkeypatch.setenv("CUVITE_BATCH_DEVICE", knob)
        with pytest.raises(ValueError, match="does not hold"):
            apply_edge_batch(dg, Comm(dev), batch)
        assert bc.same_graph(dg.g, g)


@pytest.mark.parametrize("frac", [0.01, 0.5])
def test_rmat12_matches_twin(ops, dev, frac):
    g = dyc.base_graph("rmat12")
    lists = bc.routed(dyc.recipe_batch(g, frac))
    ref = apply_routed_batch_torch(g, 0, g.nv, *lists)
    got = _device_apply(ops, g, 0, g.nv, lists, dev)
    assert bc.same_graph(got, ref)


def _w_two_ranks(rank, world, name, frac):
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(8)
    dev = torch.device("cuda:0")
    g = dyc.base_graph(name)
    share = dyc.share_of(dyc.recipe_batch(g, frac), rank, world)
    old = shard(g, rank, world)
    cpu = apply_edge_batch(old, Comm(), share)
    lists = _route_batch(old, Comm(), share)
    twin = apply_routed_batch_torch(old.g, old.base, g.nv, *lists)
    comm = HostStagedComm(dev)
    new = apply_edge_batch(old.to(dev), comm, share)
    ghosts = int(((new.g.tails < old.base) | (new.g.tails >= old.bound)).sum())
    return {"twin": bc.same_graph(new.g, twin),
            "cpu": all(torch.equal(a, b) for a, b in zip(
                bc.sorted_rows(new.g), bc.sorted_rows(cpu.g))),
            "ghosts": ghosts, "rows": bc.sorted_rows(new.g)}


def test_two_ranks_on_one_gpu():
    """Both rank processes compute on cuda:0, the wire is gloo on host
    copies: each rank's graph is its routed lists' twin bit for bit, equals
    the CPU rank's as sorted rows, holds ghost tails, and the two together
    are the single-rank graph."""
    name, frac = "lfr", 0.05
    outs = run_dist(2, _w_two_ranks, name, frac, timeout_s=60)
    for o in outs:
        assert o["twin"] and o["cpu"] and o["ghosts"] > 0
    g = dyc.base_graph(name)
    whole = apply_edge_batch(single_partition(g), Comm(),
                             dyc.recipe_batch(g, frac))
    ref = bc.sorted_rows(whole.g)
    for i in (1, 2):
        assert torch.equal(torch.cat([o["rows"][i] for o in outs]), ref[i])


def test_update_stream_matches_cpu_oracle(dev):
    g = dyc.base_graph("lfr")
    prev = dyc.prev_labels("lfr")
    batches = bc.stream_batches()
    end, steps = update_stream(single_partition(g), Comm(),
                               LouvainConfig(backend="torch"), prev, batches)
    end_d, steps_d = update_stream(single_partition(g).to(dev), Comm(dev),
                                   LouvainConfig(backend="hip"),
                                   prev.to(dev), batches)
    assert len(steps_d) == len(steps) == 3
    for a, b in zip(steps_d, steps):
        assert (a.inserted, a.deleted, a.affected) == \
            (b.inserted, b.deleted, b.affected)
        assert torch.equal(a.result.communities.cpu(), b.result.communities)
        assert a.result.levels[0]["frontier"].sweeps == \
            b.result.levels[0]["frontier"].sweeps
    assert isinstance(end_d, DistGraph)
    for a, b in zip(bc.sorted_rows(end_d.g), bc.sorted_rows(end.g)):
        assert torch.equal(a, b)
