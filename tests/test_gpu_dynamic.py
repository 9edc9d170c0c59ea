"""The HIP side of the dynamic-frontier phase against its torch twins:
frontier_move (the degree-class kernels over compacted lists, the hub
pipeline with masked scatter), frontier_expand at its span boundaries,
frontier_compact, and whole frontier phases on one and on two ranks.

All weights are integers (kernel_cases.py, unit weights in the whole runs),
so every comparison is bit for bit."""

import functools

import pytest
import torch

from cuvite_amd.dynamic import frontier_expand_torch, run_frontier_phase
from cuvite_amd.graph import single_partition
from cuvite_amd.local_move import local_move_torch
from cuvite_amd.louvain import LouvainConfig
from cuvite_amd.parallel import Comm

from tests.dist_utils import run_dist

import dynamic_cases as dyc
from kernel_cases import LADDER, ladder_inputs, move_inputs_to

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
CUTS = [2049, 6144]
ACTIVE_SETS = ("none", "all", "ladder", "alternate", "one_hub", "no_hubs")


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _ladder(wdtype, state, ghosts):
    """CPU inputs, the full local move on them and a cw_prev of sentinels."""
    inp, L = ladder_inputs(wdtype, state, ghosts, dup=ghosts, seed=21)
    t, cw = local_move_torch(inp)
    g = torch.Generator().manual_seed(3)
    cw_prev = -torch.randint(1, 100, (inp.nv,), generator=g).to(wdtype)
    return inp, L, t, cw, cw_prev


def _active(kind, inp, L, cut):
    nv = inp.nv
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    a = torch.zeros(nv, dtype=torch.bool)
    if kind == "all":
        a[:] = True
    elif kind == "ladder":
        a[:L] = True
    elif kind == "alternate":
        a[::2] = True
    elif kind == "one_hub":
        a[int((deg > cut).nonzero()[0, 0])] = True
    elif kind == "no_hubs":
        a[deg <= cut] = True
    return a


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghosts", [False, True], ids=["plain", "ghostdup"])
@pytest.mark.parametrize("state", ["singleton", "tied", "random"])
@pytest.mark.parametrize("cut", CUTS)
def test_frontier_move_matches_twin(ops, dev, monkeypatch, cut, state, ghosts,
                                    wdtype):
    """Active vertices get the plain move's answer, everyone else keeps
    label and cw_prev entry, on every route: all seven classes and the hub
    pipeline (cut 2049: eight hubs, cut 6144: four)."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    inp_cpu, L, t_full, cw_full, cw_prev = _ladder(wdtype, state, ghosts)
    inp = move_inputs_to(inp_cpu, dev)
    nv = inp.nv
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    curr = inp_cpu.curr_comm[:nv]
    for kind in ACTIVE_SETS:
        ops.clear_phase_caches()
        a = _active(kind, inp_cpu, L, cut)
        t_ref = torch.where(a, t_full, curr)
        cw_ref = torch.where(a, cw_full, cw_prev)
        prev_dev = cw_prev.to(dev)
        t, cw = ops.frontier_move(inp, a.to(dev), prev_dev)
        t, cw = t.cpu(), cw.cpu()
        assert torch.equal(prev_dev.cpu(), cw_prev), kind
        assert t.dtype == t_ref.dtype and cw.dtype == cw_ref.dtype
        bad = ((t != t_ref) | (cw != cw_ref)).nonzero(as_tuple=True)[0]
        assert bad.numel() == 0, \
            (kind, bad.numel(), deg[bad][:20].tolist(), a[bad][:20].tolist())
        if kind in ("none", "no_hubs"):
            assert len(ops._hub_static_cache) == 0  # hub pipeline skipped


@functools.lru_cache(maxsize=None)
def _expand_graph(span):
    degs = [span - 1, 0, span, 0, 0, span + 1, 3 * span + 5, 1, 0, 7, 64, 65]
    # ghost 0 touches two rows, ghost 1 nothing, ghost 2 one row
    return dyc.expand_case(degs, 3, [(0, (0, 6)), (2, (9,))]), len(degs)


@pytest.mark.parametrize("which", ["empty", "all", "span-1", "span", "span+1",
                                   "three_spans", "rows", "ghost_with",
                                   "ghost_without", "ghosts", "dups"])
def test_frontier_expand_matches_twin(ops, dev, which):
    span = ops.frontier_span()
    (rowptr, tails, g_rowptr, g_heads), nv = _expand_graph(span)
    changed = {
        "empty": [], "all": list(range(nv + 3)), "span-1": [0], "span": [2],
        "span+1": [5], "three_spans": [6], "rows": [6, 1, 0, 8, 5, 2, 11],
        "ghost_with": [nv], "ghost_without": [nv + 1],
        "ghosts": [nv + 2, nv + 1, nv], "dups": [6, 6, nv, 6, nv],
    }[which]
    ch = torch.tensor(changed, dtype=torch.int32)
    ref = frontier_expand_torch(ch, rowptr, tails, g_rowptr, g_heads,
                                torch.zeros(nv, dtype=torch.bool))
    assert torch.equal(ref, dyc.expand_loop(ch, rowptr, tails, g_rowptr,
                                            g_heads))
    act = torch.zeros(nv + 128, dtype=torch.uint8, device=dev)
    got = ops.frontier_expand(ch.to(dev), rowptr.to(dev), tails.to(dev),
                              g_rowptr.to(dev), g_heads.to(dev),
                              act[64:64 + nv])
    assert torch.equal(got.cpu().to(torch.bool), ref)
    assert int(act[:64].sum()) == 0 and int(act[64 + nv:].sum()) == 0
    # bool masks are marked in place as well
    actb = torch.zeros(nv, dtype=torch.bool, device=dev)
    ops.frontier_expand(ch.to(dev), rowptr.to(dev), tails.to(dev),
                        g_rowptr.to(dev), g_heads.to(dev), actb)
    assert torch.equal(actb.cpu(), ref)


@pytest.mark.parametrize("cut", CUTS)
def test_frontier_compact_lists(ops, dev, monkeypatch, cut):
    """Exact counts and ascending lists per class, empty classes included,
    over more than one compaction unit."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    g = torch.Generator().manual_seed(9)
    degs = torch.cat([torch.tensor(LADDER), torch.zeros(5, dtype=torch.int64),
                      torch.randint(0, 40, (3000,), generator=g),
                      torch.tensor(LADDER)])
    nv = degs.numel()
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(degs, 0)
    cls = torch.full((nv,), 7, dtype=torch.int64)   # hubs unless placed
    lo = 0
    for c, hi in enumerate((16, 64, 256, 512, 1024, 2048, cut)):
        cls[(degs > lo) & (degs <= hi)] = c
        lo = hi
    cls[degs == 0] = 8
    rp = rowptr.to(dev)
    masks = {"none": torch.zeros(nv, dtype=torch.bool),
             "all": torch.ones(nv, dtype=torch.bool),
             "alternate": torch.arange(nv) % 2 == 0,
             "random": torch.rand(nv, generator=g) < 0.3,
             "low_only": degs <= 16}
    for name, a in masks.items():
        lists = ops.frontier_lists(rp, a.to(dev))
        assert len(lists) == 9
        for c in range(9):
            ref = (a & (cls == c)).nonzero(as_tuple=True)[0].to(torch.int32)
            assert lists[c].dtype == torch.int32
            assert torch.equal(lists[c].cpu(), ref), (name, c)
    assert any(int(((cls == c) & masks["low_only"]).sum()) == 0
               for c in range(9))
    # a uint8 mask gives the same lists
    u8 = masks["random"].to(torch.uint8).to(dev)
    for x, y in zip(ops.frontier_lists(rp, u8),
                    ops.frontier_lists(rp, masks["random"].to(dev))):
        assert torch.equal(x, y)


@pytest.mark.parametrize("name", ["karate", "lfr", "rmat12"])
def test_frontier_phase_matches_cpu_oracle(ops, dev, name):
    """A 1 % batch: device labels, frontier sizes per sweep and sweep count
    equal the CPU oracle's."""
    g, _, prev, f0 = dyc.perturbed(name, 0.01)
    est, lab, it, rep = dyc.oracle_run(name, 0.01)
    dg = single_partition(g).to(dev)
    est_d, lab_d, it_d, _, rep_d = run_frontier_phase(
        dg, Comm(dev), LouvainConfig(backend="hip"), prev.to(dev),
        f0.to(dev))
    print(f"{name}: sizes {rep_d.sizes_per_sweep} of {g.nv}")
    assert rep_d.sizes_per_sweep == rep.sizes_per_sweep
    assert it_d == it
    assert torch.equal(lab_d.cpu(), lab)
    assert abs(est_d - est) < 1e-12


def _w_two_ranks(rank, world, name, frac, prev):
    from cuvite_amd.parallel import Comm as _Comm
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(8)
    dev = torch.device("cuda:0")
    cpu = torch.device("cpu")
    oracle = dyc.dist_update(rank, world, _Comm(), cpu, "torch", name, frac,
                             False, prev)
    staged = dyc.dist_update(rank, world, HostStagedComm(dev), dev, "hip",
                             name, frac, False, prev)
    return oracle, staged


def test_two_ranks_on_one_gpu_match_cpu_oracle():
    """Both rank processes compute on cuda:0, the wire is gloo on host
    copies: graph update, affected vertices and the frontier phase (changed
    ghosts, the ghost -> local adjacency) equal the CPU ranks' and the
    single-rank oracle's."""
    name, frac = "lfr", 0.01
    g, _, prev, f0 = dyc.perturbed(name, frac)
    outs = run_dist(2, _w_two_ranks, name, frac, prev, timeout_s=60)
    _, lab, it, rep = dyc.oracle_run(name, frac)
    for side in (0, 1):
        parts = [o[side] for o in outs]
        assert torch.equal(torch.cat([p["f0"] for p in parts]), f0)
        assert torch.equal(torch.cat([p["labels"] for p in parts]), lab)
        for p in parts:
            assert p["sizes"] == rep.sizes_per_sweep and p["sweeps"] == it
            assert all(abs(a - b) < 1e-12
                       for a, b in zip(p["estimates"], rep.estimates))
        key, w = dyc.csr_key(g)
        assert torch.equal(torch.cat([p["key"] for p in parts]), key)
        assert torch.equal(torch.cat([p["w"] for p in parts]), w)
