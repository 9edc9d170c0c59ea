"""The edge-balanced intra_weight HIP kernel, partition_quality and warm
start on the GPU.

Kernel inputs carry small integer weights (kernel_cases.py, quality_cases.
py), so every sum is exact in fp32 and fp64 in any order, through the
atomic path included: comparisons with the CPU oracle are torch.equal."""

import functools

import pytest
import torch

from cuvite_amd import intra_weight_torch, partition_quality
from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

from kernel_cases import ladder_inputs, move_inputs_to
from quality_cases import (cold_run, csr_from_degrees, lfr_truth,
                           whole_graph)

pytestmark = pytest.mark.gpu

SEED = 20
DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


# ---- 1. ladder: against local_move's cw and against the oracle -------------

@functools.lru_cache(maxsize=None)
def _ladder(wdtype, state, ghosts):
    inp, _ = ladder_inputs(wdtype, state, ghosts, True, SEED)
    ref = intra_weight_torch(inp.rowptr, inp.tails, inp.weights,
                             inp.curr_comm.to(torch.int64))
    return inp, ref.to(wdtype)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ltype", ["int32_dense", "int64_gid"])
@pytest.mark.parametrize("ghosts", [False, True], ids=["plain", "ghosts"])
@pytest.mark.parametrize("state", ["singleton", "few", "random"])
def test_ladder_matches_local_move_and_oracle(ops, dev, state, ghosts, ltype,
                                              wdtype):
    """Degrees 1..8001: rows far shorter and longer than a span."""
    inp_cpu, ref = _ladder(wdtype, state, ghosts)
    span = ops.intra_weight_span()
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    assert int(deg.max()) > span > int(deg.min())
    inp = move_inputs_to(inp_cpu, dev)
    labels = inp.curr_comm if ltype == "int32_dense" \
        else inp.comm_gid[inp.curr_comm.to(torch.int64)]
    got = ops.intra_weight(inp.rowptr, inp.tails, inp.weights, labels)
    assert got.dtype == wdtype and got.shape == (inp.nv,)
    cw = ops.local_move(inp)[1]
    bad = (got.cpu() != ref).nonzero(as_tuple=True)[0]
    assert bad.numel() == 0, \
        f"rows differ from the oracle; degrees {deg[bad][:40].tolist()}"
    assert torch.equal(got, cw)


# ---- 2. span boundaries ------------------------------------------------------

def _span_cases(S):
    return {
        "mixed": ([0, 1, S - 1, S, S + 1, 0, 0, 3 * S + 1, 1], 16),
        "row_on_boundary": ([S, S, 2 * S, 5, S - 5, 7], 16),
        "one_long_row": ([3 * S + 1], 16),
        "no_edges": ([0] * 5, 3),
        "no_vertices": ([], 0),
        "partial_last_span": ([S // 2] * 3, 16),
    }


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ltype", [torch.int32, torch.int64],
                         ids=["int32", "int64"])
@pytest.mark.parametrize("case", ["mixed", "row_on_boundary", "one_long_row",
                                  "no_edges", "no_vertices",
                                  "partial_last_span"])
def test_span_boundaries(ops, dev, case, ltype, wdtype):
    S = ops.intra_weight_span()
    degs, n_ghost = _span_cases(S)[case]
    rowptr, tails, w, labels = csr_from_degrees(degs, n_ghost, seed=32)
    ne = tails.numel()
    if case == "row_on_boundary":
        assert S in rowptr.tolist() and 2 * S in rowptr.tolist()
    if case in ("mixed", "partial_last_span"):
        assert ne % S != 0
    ref = intra_weight_torch(rowptr, tails, w, labels)
    # equal and unequal edges in every span (a one-edge span has one kind)
    row = torch.searchsorted(rowptr, torch.arange(ne), right=True) - 1
    same = labels[tails.to(torch.int64)] == labels[row]
    for s0 in range(0, ne, S):
        n_same, n = int(same[s0:s0 + S].sum()), same[s0:s0 + S].numel()
        assert n == 1 or 0 < n_same < n
    if ltype == torch.int64:
        labels = labels + (5 << 32)      # ids that do not fit int32
    got = ops.intra_weight(rowptr.to(dev), tails.to(dev),
                           w.to(wdtype).to(dev), labels.to(ltype).to(dev))
    assert got.dtype == wdtype and got.shape == (len(degs),)
    assert torch.equal(got.cpu(), ref.to(wdtype))


# ---- 3. partition_quality ------------------------------------------------------

@pytest.mark.parametrize("name", ["rgg", "lfr"])
def test_partition_quality_matches_cpu_oracle(dev, name):
    g = whole_graph(name)
    lab = cold_run(name).communities
    cpu = partition_quality(single_partition(g), lab, Comm(),
                            backend="torch")
    gpu = partition_quality(single_partition(g.to(dev)), lab.to(dev),
                            Comm(dev), backend="hip")
    print(f"{name}: cpu Q={cpu.modularity:.15f} gpu Q={gpu.modularity:.15f}")
    assert abs(gpu.modularity - cpu.modularity) <= 1e-12
    assert gpu.num_communities == cpu.num_communities
    assert gpu.total_weight == pytest.approx(cpu.total_weight, rel=1e-12)


# ---- 4. warm start ---------------------------------------------------------------

def _hip(g, dev, init=None):
    return louvain(single_partition(g.to(dev)), Comm(dev),
                   LouvainConfig(backend="hip"),
                   init_labels=None if init is None else init.to(dev))


@pytest.mark.parametrize("name", ["karate", "rmat_unit"])
def test_arange_init_equals_cold_run_hip(dev, name):
    """Unit weights: the community aggregates are exact in any atomic order,
    so two GPU runs agree bit for bit (with fractional weights a cold run
    does not even reproduce itself to the last bit on the GPU)."""
    if name == "karate":
        g = whole_graph("karate")
    else:
        g = rmat_graph(10, 8, seed=2)
        g = Graph(g.rowptr, g.tails, torch.ones_like(g.weights))
    cold = _hip(g, dev)
    warm = _hip(g, dev, torch.arange(g.nv))
    assert torch.equal(warm.communities, cold.communities)
    assert warm.modularity == cold.modularity
    assert warm.total_iters == cold.total_iters


@pytest.mark.parametrize("name,start", [("karate", "own"), ("lfr", "own"),
                                        ("rgg", "own"), ("lfr", "truth")])
def test_warm_start_improves_and_converges_faster_hip(dev, name, start):
    g = whole_graph(name)
    cold = _hip(g, dev)
    init = cold.communities if start == "own" else lfr_truth().to(dev)
    dg = single_partition(g.to(dev))

    def exact(labels):
        return partition_quality(dg, labels, Comm(dev),
                                 backend="hip").modularity
    q_start = exact(init)
    warm = _hip(g, dev, init.clone())
    q_end = exact(warm.communities)
    print(f"{name}/{start}: start Q={q_start:.12f} end Q={q_end:.12f} "
          f"sweeps warm={warm.total_iters} cold={cold.total_iters}")
    assert q_end >= q_start - 1e-9
    assert warm.total_iters < cold.total_iters
