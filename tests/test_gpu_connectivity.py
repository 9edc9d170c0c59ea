"""The cc_hook / cc_compress HIP kernels, split_disconnected and
LouvainConfig.connectivity on the GPU.

comp is integer valued and defined without reference to any order (the
smallest dense id of the component), so every comparison with the CPU twin
`cc_components_torch` is torch.equal. The round counts differ by design (a
hook pass on the device sees what other waves already merged) and are only
printed."""

import functools

import pytest
import torch

from cuvite_amd import cc_components_torch, split_disconnected
from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm

import connectivity_cases as cc
from kernel_cases import ladder_inputs
from quality_cases import cold_run, csr_from_degrees, whole_graph
from test_gpu_quality import _span_cases

pytestmark = pytest.mark.gpu

SEED = 20
LTYPES = [torch.int32, torch.int64]
_lt = {torch.int32: "int32", torch.int64: "int64"}.get


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    return _ops


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _check(ops, dev, tag, rowptr, tails, labels, ltype):
    ref, ref_rounds = cc_components_torch(rowptr, tails, labels)
    if ltype == torch.int64:
        labels = labels + (5 << 32)      # ids that do not fit int32
    got, rounds = ops.cc_components(rowptr.to(dev), tails.to(dev),
                                    labels.to(ltype).to(dev))
    print(f"{tag}: rounds device={rounds} torch={ref_rounds} "
          f"components={int(torch.unique(ref).numel())}")
    assert got.dtype == torch.int32 and got.shape == (labels.numel(),)
    assert torch.equal(got.cpu(), ref)
    return ref


# ---- 1. span boundaries ------------------------------------------------------

@pytest.mark.parametrize("ltype", LTYPES, ids=_lt)
@pytest.mark.parametrize("case", ["mixed", "row_on_boundary", "one_long_row",
                                  "no_edges", "no_vertices",
                                  "partial_last_span"])
def test_span_boundaries(ops, dev, case, ltype):
    S = ops.intra_weight_span()
    degs, n_ghost = _span_cases(S)[case]
    rowptr, tails, _, labels = csr_from_degrees(degs, n_ghost, seed=32)
    ref = _check(ops, dev, case, rowptr, tails, labels, ltype)
    nl = len(degs) + n_ghost
    if tails.numel() == 0:
        assert ref.tolist() == list(range(nl))
    else:
        # something merged and something did not, ghosts included
        assert 1 < int(torch.unique(ref).numel()) < nl
        assert bool((ref[len(degs):] < len(degs)).any())


@pytest.mark.parametrize("ltype", LTYPES, ids=_lt)
def test_star_hub_in_two_labels(ops, dev, ltype):
    S = ops.intra_weight_span()
    rowptr, tails, labels, want = cc.star_case(3 * S + 1)
    ref = _check(ops, dev, "star", rowptr, tails, labels, ltype)
    assert torch.equal(ref.to(torch.int64), want)
    assert int((want == 0).sum()) == 1 + (3 * S + 1) // 2


# ---- 2. ladder and paths -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _ladder(state, ghosts):
    return ladder_inputs(torch.float64, state, ghosts, True, SEED)[0]


@pytest.mark.parametrize("ltype", ["int32_dense", "int64_gid"])
@pytest.mark.parametrize("ghosts", [False, True], ids=["plain", "ghosts"])
@pytest.mark.parametrize("state", ["few", "random"])
def test_ladder(ops, dev, state, ghosts, ltype):
    """Degrees 1..8001: rows far shorter and longer than a span."""
    inp = _ladder(state, ghosts)
    labels = inp.curr_comm.to(torch.int64)
    if ltype == "int64_gid":
        labels = inp.comm_gid[labels]
    ref, ref_rounds = cc_components_torch(inp.rowptr, inp.tails, labels)
    dl = labels.to(dev) if ltype == "int64_gid" else inp.curr_comm.to(dev)
    got, rounds = ops.cc_components(inp.rowptr.to(dev), inp.tails.to(dev), dl)
    print(f"ladder {state}: rounds device={rounds} torch={ref_rounds} "
          f"components={int(torch.unique(ref).numel())}")
    assert int(torch.unique(ref).numel()) < labels.numel()
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("labelling", ["one", "blocks"])
@pytest.mark.parametrize("order", cc.PATH_ORDERS)
def test_path_orders(ops, dev, order, labelling):
    """Natural order: one hook pass leaves a chain as deep as the path for
    the compress kernel; random order: the most rounds."""
    rowptr, tails, labels, want = cc.path_case(order, labelling)
    got, rounds = ops.cc_components(rowptr.to(dev), tails.to(dev),
                                    labels.to(dev))
    print(f"path {order}/{labelling}: rounds device={rounds}")
    assert torch.equal(got.cpu().to(torch.int64), want)


def test_bad_inputs_raise(ops, dev):
    rowptr, tails, labels, _ = cc.hand_cases()["aba"]
    with pytest.raises(RuntimeError):
        ops.cc_components(rowptr.to(dev), tails.to(dev),
                          labels[:2].to(dev))        # fewer labels than rows
    with pytest.raises(RuntimeError):
        ops.cc_components(rowptr.to(dev), tails.to(dev),
                          labels.to(torch.float32).to(dev))


# ---- 3. split_disconnected and louvain ----------------------------------------

def _graph(name):
    return rmat_graph(10, 8, seed=2) if name == "rmat10" else whole_graph(name)


@functools.lru_cache(maxsize=None)
def _cpu_labels(name):
    if name == "rmat10":
        return louvain(single_partition(_graph(name)), Comm(),
                       LouvainConfig(backend="torch")).communities
    return cold_run(name).communities


@pytest.mark.parametrize("name", ["lfr", "rgg", "rmat10"])
def test_split_matches_cpu(dev, name):
    g, lab = _graph(name), _cpu_labels(name)
    cpu = split_disconnected(single_partition(g), lab, Comm(),
                             backend="torch")
    gpu = split_disconnected(single_partition(g.to(dev)), lab.to(dev),
                             Comm(dev), backend="hip")
    print(f"{name}: communities={gpu.num_communities} "
          f"components={gpu.num_components} rounds device={gpu.rounds} "
          f"torch={cpu.rounds}")
    assert gpu.labels.is_cuda
    assert torch.equal(gpu.labels.cpu(), cpu.labels)
    assert gpu.num_components > gpu.num_communities
    assert (gpu.num_communities, gpu.num_components, gpu.num_disconnected) \
        == (cpu.num_communities, cpu.num_components, cpu.num_disconnected)


@pytest.mark.parametrize("name", ["karate", "rmat_unit"])
def test_louvain_final_hip(dev, name):
    """Unit weights: two GPU runs agree bit for bit (see
    test_arange_init_equals_cold_run_hip)."""
    if name == "karate":
        g = whole_graph("karate")
    else:
        g = rmat_graph(10, 8, seed=2)
        g = Graph(g.rowptr, g.tails, torch.ones_like(g.weights))
    dg = single_partition(g.to(dev))
    plain = louvain(dg, Comm(dev), LouvainConfig(backend="hip"))
    final = louvain(dg, Comm(dev),
                    LouvainConfig(backend="hip", connectivity="final"))
    want = split_disconnected(dg, plain.communities, Comm(dev),
                              backend="hip")
    print(f"{name}: communities={want.num_communities} "
          f"components={want.num_components} rounds={want.rounds}")
    assert torch.equal(final.communities, want.labels)
    assert final.connectivity.num_components == want.num_components
    assert final.modularity == plain.modularity
    assert cc.all_connected(g, final.communities.cpu())
