"""HIP kernel numerics tests (run on the MI355X box): each kernel is compared
against the plain PyTorch fp32/fp64 reference of the same op
(cuvite_amd.local_move.local_move_torch)."""

import os

import pytest
import torch

from cuvite_amd.generators import karate_graph, rmat_graph
from cuvite_amd.graph import Graph, single_partition
from cuvite_amd.local_move import (MoveInputs, local_move_torch,
                                   modularity_parts)

pytestmark = pytest.mark.gpu


def _inputs(g, dev, comm_state="singleton", seed=0, wdtype=None):
    if wdtype is not None:
        g = type(g)(g.rowptr, g.tails, g.weights.to(wdtype))
    g = g.to(dev)
    dg = single_partition(g)
    vdeg = dg.local_degree_sum()
    nv = g.nv
    if comm_state == "singleton":
        curr = torch.arange(nv, device=dev)
        size = torch.ones(nv, dtype=torch.int64, device=dev)
        cdeg = vdeg.clone()
    else:
        rng = torch.Generator().manual_seed(seed)
        curr = torch.randint(0, nv, (nv,), generator=rng).to(dev)
        size = torch.zeros(nv, dtype=torch.int64, device=dev)
        size.index_add_(0, curr, torch.ones(nv, dtype=torch.int64, device=dev))
        cdeg = torch.zeros(nv, dtype=vdeg.dtype, device=dev)
        cdeg.index_add_(0, curr, vdeg)
    return MoveInputs(g.rowptr, g.tails.to(torch.int32), g.weights,
                      curr.to(torch.int32), vdeg, size, cdeg,
                      torch.arange(nv, dtype=torch.int64, device=dev),
                      1.0 / float(vdeg.to(torch.float64).sum()))


def _unit_rmat(scale, ef=16, seed=3):
    g = rmat_graph(scale, ef, seed=seed)
    g.weights.fill_(1.0)
    return g


@pytest.mark.parametrize("comm_state", ["singleton", "random"])
def test_local_move_karate_exact(comm_state):
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(karate_graph(), dev, comm_state, seed=5)
    t_hip, cw_hip = ops.local_move(inp)
    t_ref, cw_ref = local_move_torch(inp)
    assert torch.equal(t_hip.to(torch.int64), t_ref.to(torch.int64))
    assert torch.allclose(cw_hip, cw_ref)


@pytest.mark.parametrize("scale", [10, 14])
@pytest.mark.parametrize("comm_state", ["singleton", "random"])
def test_local_move_rmat_unit_exact(scale, comm_state):
    """Unit weights: fp64 sums are exact in any order, so the HIP kernel must
    match the torch reference bit-for-bit including tie-breaks."""
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(_unit_rmat(scale), dev, comm_state, seed=scale)
    t_hip, cw_hip = ops.local_move(inp)
    t_ref, cw_ref = local_move_torch(inp)
    assert torch.equal(t_hip.to(torch.int64), t_ref.to(torch.int64))
    assert torch.equal(cw_hip, cw_ref)


def test_local_move_rmat_random_weights_fp64():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(rmat_graph(12, 16, seed=9), dev, "random", seed=1)
    t_hip, cw_hip = ops.local_move(inp)
    t_ref, cw_ref = local_move_torch(inp)
    assert torch.allclose(cw_hip, cw_ref, rtol=1e-12, atol=1e-12)
    # fp rounding of different accumulation orders can flip near-ties
    match = (t_hip == t_ref).float().mean().item()
    assert match > 0.999, f"target match fraction {match}"


def test_local_move_fp32():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    inp = _inputs(rmat_graph(10, 16, seed=4), dev, "random", seed=2,
                  wdtype=torch.float32)
    t_hip, cw_hip = ops.local_move(inp)
    t_ref, cw_ref = local_move_torch(inp)
    assert torch.allclose(cw_hip, cw_ref, rtol=1e-4, atol=1e-5)
    match = (t_hip == t_ref).float().mean().item()
    assert match > 0.99, f"target match fraction {match}"


def test_degree_class_coverage():
    """Graph with vertices in every degree class including hubs (deg above
    the hub cut, 6144 by default)."""
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    # star graph: hub 0 with 7000 spokes + chain among low vertices
    n_sp = 7000
    nv = n_sp + 1
    src = [0] * n_sp + list(range(1, nv))
    dst = list(range(1, nv)) + [0] * n_sp
    # add a few mid-degree vertices
    for v in range(1, 200):
        for u in range(1, 80):
            if u != v:
                src.append(v); dst.append(u)
    s = torch.tensor(src, dtype=torch.int64)
    d = torch.tensor(dst, dtype=torch.int64)
    w = torch.ones(s.numel(), dtype=torch.float64)
    from cuvite_amd.graph import Graph
    g = Graph.from_edge_tuples(nv, s, d, w)
    inp = _inputs(g, dev, "random", seed=3)
    t_hip, cw_hip = ops.local_move(inp)
    t_ref, cw_ref = local_move_torch(inp)
    assert torch.equal(t_hip.to(torch.int64), t_ref.to(torch.int64))
    assert torch.equal(cw_hip, cw_ref)


def test_modularity_kernel():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    for dtype in (torch.float64, torch.float32):
        cw = torch.rand(1 << 20, dtype=dtype, device=dev)
        cd = torch.rand(1 << 20, dtype=dtype, device=dev)
        ref = modularity_parts(cw, cd)
        hip = ops.modularity_parts(cw, cd)
        assert torch.allclose(hip, ref, rtol=1e-10)


def test_full_louvain_gpu_matches_cpu():
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    g = karate_graph()
    cpu = louvain(single_partition(g), Comm(),
                  LouvainConfig(backend="torch"))
    dev = torch.device("cuda:0")
    gpu = louvain(single_partition(g.to(dev)), Comm(dev),
                  LouvainConfig(backend="hip"))
    assert abs(cpu.modularity - gpu.modularity) < 1e-9
    assert torch.equal(cpu.communities, gpu.communities.cpu())


def test_full_louvain_gpu_rmat():
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    g = _unit_rmat(12)
    cpu = louvain(single_partition(g), Comm(), LouvainConfig(backend="torch"))
    dev = torch.device("cuda:0")
    gpu = louvain(single_partition(g.to(dev)), Comm(dev),
                  LouvainConfig(backend="hip"))
    # unit weights: trajectories must agree exactly
    assert abs(cpu.modularity - gpu.modularity) < 1e-9
    assert torch.equal(cpu.communities, gpu.communities.cpu())


def test_native_extension_is_loaded():
    """Guard against silent eager fallback: the HIP extension must be loaded
    from the in-tree .so on GPU boxes."""
    from cuvite_amd import ops
    assert ops.available()
    import cuvite_amd.ops._hip_ops as ext
    assert "cuvite_amd/ops" in ext.__file__


def test_scatter_add_fp64_matches_index_add():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    for dtype in (torch.float64, torch.float32):
        out = torch.zeros(1000, dtype=dtype, device=dev)
        ref = out.clone()
        idx = torch.randint(0, 1000, (1 << 20,), device=dev)
        val = torch.rand(1 << 20, dtype=dtype, device=dev)
        ops.scatter_add_(out, idx, val)
        ref.index_add_(0, idx, val)
        tol = 1e-9 if dtype == torch.float64 else 1e-2
        assert torch.allclose(out, ref, rtol=tol, atol=tol)


def test_csr_from_edges_matches_cpu_build():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    nv, ne, base = 500, 20000, 100
    src = torch.randint(base, base + nv, (ne,), device=dev)
    dst = torch.randint(0, 5000, (ne,), device=dev)
    w = torch.rand(ne, dtype=torch.float64, device=dev)
    g_gpu = Graph.from_edge_tuples(nv, src, dst, w, base=base)
    g_cpu = Graph.from_edge_tuples(nv, src.cpu(), dst.cpu(), w.cpu(), base=base)
    assert torch.equal(g_gpu.rowptr.cpu(), g_cpu.rowptr)
    # same multiset of (tail, weight) per row
    for v in range(0, nv, 37):
        e0, e1 = int(g_cpu.rowptr[v]), int(g_cpu.rowptr[v + 1])
        a = sorted(zip(g_gpu.tails[e0:e1].cpu().tolist(),
                       g_gpu.weights[e0:e1].cpu().tolist()))
        b = sorted(zip(g_cpu.tails[e0:e1].tolist(),
                       g_cpu.weights[e0:e1].tolist()))
        assert a == b


def test_row_sum_matches_degree():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    g = _unit_rmat(10).to(dev)
    out = ops.row_sum(g.rowptr, g.weights)
    seg = torch.repeat_interleave(
        torch.arange(g.nv, device=dev), g.degrees())
    ref = torch.zeros(g.nv, dtype=g.weights.dtype, device=dev)
    ref.index_add_(0, seg, g.weights)
    assert torch.allclose(out, ref, rtol=1e-12, atol=1e-12)


def test_hub_class_matches_torch_oracle():
    """deg > 4096 routes to the edge-parallel hub pipeline; compare against
    the torch fp64 oracle on a graph with a synthetic mega-hub."""
    torch.manual_seed(11)
    nv = 8192
    hub_deg = 40000
    src = torch.cat([torch.zeros(hub_deg, dtype=torch.int64),
                     torch.randint(1, nv, (nv * 8,))])
    dst = torch.cat([torch.randint(0, nv, (hub_deg,)),
                     torch.randint(0, nv, (nv * 8,))])
    w = torch.ones(src.numel(), dtype=torch.float64)
    g = Graph.from_edge_tuples(nv, src, dst, w)
    dev = torch.device("cuda:0")
    inp_gpu = _inputs(g, dev, "random", seed=5)
    inp_cpu = _inputs(g, torch.device("cpu"), "random", seed=5)
    from cuvite_amd import ops
    tgt_gpu, cw_gpu = ops.local_move(inp_gpu)
    tgt_cpu, cw_cpu = local_move_torch(inp_cpu)
    assert torch.equal(tgt_gpu.cpu().to(torch.int64),
                       tgt_cpu.to(torch.int64))
    assert torch.allclose(cw_gpu.cpu(), cw_cpu)


def test_gpu_louvain_variants_match_cpu():
    """Coloring (-c), ordering (-d) and ET variants on GPU (HIP backend)
    match the CPU torch-oracle runs on karate exactly (fp64)."""
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    dev = torch.device("cuda:0")
    g = karate_graph()
    for kwargs in ({"coloring": True, "max_colors": 6},
                   {"ordering": True, "max_colors": 6},
                   {"early_term": 1},
                   {"threshold_scaling": True}):
        cpu = louvain(single_partition(g), Comm(torch.device("cpu")),
                      LouvainConfig(backend="torch", **kwargs))
        gpu = louvain(single_partition(g.to(dev)), Comm(dev),
                      LouvainConfig(backend="hip", **kwargs))
        assert abs(cpu.modularity - gpu.modularity) < 1e-9, kwargs
        assert torch.equal(cpu.communities, gpu.communities.cpu()), kwargs


def test_gpu_lfr_recovery():
    """LFR acceptance config on GPU: planted communities recovered."""
    from cuvite_amd.generators import lfr_graph
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    from cuvite_amd.compare import compare_communities
    dev = torch.device("cuda:0")
    g, truth = lfr_graph(5000, mu=0.4, seed=2)
    res = louvain(single_partition(g.to(dev)), Comm(dev),
                  LouvainConfig(backend="hip"))
    m = compare_communities(truth, res.communities.cpu())
    assert m["recall"] > 0.75
    assert m["f_score"] > 0.6


def test_hub_segsort_matches_torch_sort_fallback():
    """The default rocPRIM segsort hub path (hub_moves binding, incl. the
    split-block argmax) must match the torch global-sort fallback
    (CUVITE_HUB_SEGSORT=0) exactly on unit weights."""
    from cuvite_amd import ops
    torch.manual_seed(11)
    nv = 8192
    src = torch.cat([torch.zeros(40000, dtype=torch.int64),
                     torch.randint(1, nv, (nv * 8,))])
    dst = torch.cat([torch.randint(0, nv, (40000,)),
                     torch.randint(0, nv, (nv * 8,))])
    w = torch.ones(src.numel(), dtype=torch.float64)
    g = Graph.from_edge_tuples(nv, src, dst, w)
    dev = torch.device("cuda:0")
    inp = _inputs(g, dev, "random", seed=5)
    os.environ["CUVITE_HUB_SEGSORT"] = "0"
    try:
        ops._bucket_cache.clear()
        ops._hub_static_cache.clear()
        t_ref, cw_ref = ops.local_move(inp)
    finally:
        del os.environ["CUVITE_HUB_SEGSORT"]
    ops._bucket_cache.clear()
    ops._hub_static_cache.clear()
    t_new, cw_new = ops.local_move(inp)
    ops._hub_static_cache.clear()
    assert torch.equal(t_ref, t_new)
    assert torch.allclose(cw_ref, cw_new)


def test_apply_deltas_matches_torch():
    """Fused apply_deltas_ kernel vs the plain torch index_add/scatter_add
    reference, including remote (out-of-range) labels that must be ignored."""
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    nv, base, bound = 5000, 1000, 6000
    curr = torch.randint(0, 8000, (nv,), dtype=torch.int64, device=dev)
    target = curr.clone()
    m = torch.rand(nv, device=dev) < 0.4
    target[m] = torch.randint(0, 8000, (int(m.sum()),), dtype=torch.int64,
                              device=dev)
    vdeg = torch.rand(nv, dtype=torch.float64, device=dev) * 3
    size = torch.randint(1, 5, (bound - base,), dtype=torch.int64, device=dev)
    degree = torch.rand(bound - base, dtype=torch.float64, device=dev)
    size_ref, degree_ref = size.clone(), degree.clone()
    # torch reference
    moved = target != curr
    gids = torch.cat([curr[moved], target[moved]])
    ds = torch.cat([-torch.ones_like(curr[moved]),
                    torch.ones_like(target[moved])])
    dd = torch.cat([-vdeg[moved], vdeg[moved]])
    loc = (gids >= base) & (gids < bound)
    size_ref.index_add_(0, gids[loc] - base, ds[loc])
    degree_ref.index_add_(0, gids[loc] - base, dd[loc])
    ops.apply_deltas_(target, curr, vdeg, base, bound, size, degree)
    assert torch.equal(size, size_ref)
    assert torch.allclose(degree, degree_ref)


def test_coarsen_aggregate_rocprim_matches_cpu():
    """GPU _aggregate (rocPRIM narrow-bit sort_reduce_pairs) vs the CPU
    sort/cumsum reference on random duplicate-heavy coarse edges."""
    from cuvite_amd.coarsen import _aggregate
    torch.manual_seed(3)
    n, gnc = 200000, 997
    s = torch.randint(0, gnc, (n,), dtype=torch.int64)
    t = torch.randint(0, gnc, (n,), dtype=torch.int64)
    w = torch.rand(n, dtype=torch.float64)
    cs, ct, cw = _aggregate(s, t, w, gnc)
    dev = torch.device("cuda:0")
    gs, gt, gw = _aggregate(s.to(dev), t.to(dev), w.to(dev), gnc)
    assert torch.equal(gs.cpu(), cs)
    assert torch.equal(gt.cpu(), ct)
    assert torch.allclose(gw.cpu(), cw, atol=1e-12)


def test_release_tails_louvain_still_runs():
    """bench.py's converged-run memory handoff: after build_halo +
    release_tails, louvain(halo=...) must produce the same result."""
    from cuvite_amd.halo import build_halo
    dev = torch.device("cuda:0")
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    # unit weights: fp64 sums are exact in any (atomic) order, so the two
    # runs must agree bit-for-bit
    g = _unit_rmat(10, seed=2).to(dev)
    dg = single_partition(g)
    ref = louvain(dg, Comm(dev), LouvainConfig(backend="hip"))
    h = build_halo(dg, Comm(dev))
    dg.g.release_tails()
    assert dg.g.ne == int(dg.g.rowptr[-1])
    got = louvain(dg, Comm(dev), LouvainConfig(backend="hip"), halo=h)
    assert got.modularity == ref.modularity
    assert torch.equal(got.communities, ref.communities)


def test_hub_cut_parity():
    """CUVITE_HUB_CUT moves vertices between the LDS block class and the
    segsort hub pipeline; results must be identical for any cut."""
    from cuvite_amd import ops
    torch.manual_seed(13)
    nv = 4096
    # several vertices with degrees straddling the 4096..8000 band
    src, dst = [], []
    for hub, d in ((0, 7000), (1, 5000), (2, 4500), (3, 9000)):
        src += [hub] * d
        dst += torch.randint(4, nv, (d,)).tolist()
    src += torch.randint(4, nv, (nv * 4,)).tolist()
    dst += torch.randint(4, nv, (nv * 4,)).tolist()
    s = torch.tensor(src, dtype=torch.int64)
    d = torch.tensor(dst, dtype=torch.int64)
    w = torch.ones(s.numel(), dtype=torch.float64)
    g = Graph.from_edge_tuples(nv, s, d, w)
    inp = _inputs(g, torch.device("cuda:0"), "random", seed=6)
    outs = []
    for cut in ("4096", "6144", "8000"):
        os.environ["CUVITE_HUB_CUT"] = cut
        try:
            ops._bucket_cache.clear()
            ops._hub_static_cache.clear()
            ops._hub_groups_cache.clear()
            outs.append(ops.local_move(inp))
        finally:
            del os.environ["CUVITE_HUB_CUT"]
    ops._bucket_cache.clear()
    ops._hub_static_cache.clear()
    for t2, cw2 in outs[1:]:
        assert torch.equal(outs[0][0], t2)
        assert torch.equal(outs[0][1], cw2)


def test_coloring_gpu_matches_cpu_exact():
    """The fused coloring_minmax kernel path must produce EXACTLY the CPU
    coloring (integer min/max, no fp, no atomics)."""
    from cuvite_amd.coloring import distance1_coloring, check_coloring
    from cuvite_amd.parallel import Comm
    g = rmat_graph(11, 16, seed=6)
    c_cpu, n_cpu = distance1_coloring(single_partition(g), Comm(), n_hash=4)
    dev = torch.device("cuda:0")
    dgg = single_partition(g.to(dev))
    c_gpu, n_gpu = distance1_coloring(dgg, Comm(dev), n_hash=4)
    assert n_cpu == n_gpu
    assert torch.equal(c_cpu, c_gpu.cpu())
    assert check_coloring(dgg, Comm(dev), c_gpu, exclude_color=n_gpu - 1) == 0


def test_recount_matches_torch():
    from cuvite_amd import ops
    dev = torch.device("cuda:0")
    torch.manual_seed(9)
    nv, base = 40000, 500
    labels = torch.randint(base, base + nv, (nv,), dtype=torch.int64,
                           device=dev)
    vdeg = torch.rand(nv, dtype=torch.float64, device=dev)
    size = torch.randint(0, 9, (nv,), dtype=torch.int64, device=dev)
    degree = torch.rand(nv, dtype=torch.float64, device=dev)
    ops._require().recount_(labels, vdeg, base, size, degree)
    size_ref = torch.bincount(labels - base, minlength=nv)
    degree_ref = torch.zeros(nv, dtype=torch.float64, device=dev)
    degree_ref.index_add_(0, labels - base, vdeg)
    assert torch.equal(size, size_ref)
    assert torch.allclose(degree, degree_ref)


def test_degree_sort_dist_gpu_louvain():
    """bench.py's default preprocessing on GPU: relabeled graph runs the
    full HIP louvain and reaches the same converged quality band."""
    from cuvite_amd.generators import degree_sort_dist
    from cuvite_amd.graph import single_partition
    from cuvite_amd.louvain import louvain, LouvainConfig
    from cuvite_amd.parallel import Comm
    dev = torch.device("cuda:0")
    g = rmat_graph(11, 16, seed=8).to(dev)
    dg = single_partition(g)
    ref = louvain(dg, Comm(dev), LouvainConfig(backend="hip"))
    dg2 = degree_sort_dist(single_partition(g), Comm(dev))
    d = dg2.g.degrees()
    assert bool((d[:-1] >= d[1:]).all())
    got = louvain(dg2, Comm(dev), LouvainConfig(backend="hip"))
    assert abs(got.modularity - ref.modularity) < 0.03
