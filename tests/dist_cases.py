"""CPU-only input builders and scenario runners for the multi-rank tests.

The builders are plain torch on the CPU: no GPU, no `cuvite_amd.ops` import.
`tests/test_dist_cases.py` checks on the oracle alone that these inputs have
the properties the GPU tests rely on; `tests/test_gpu_multirank.py` runs the
scenarios with every rank computing on ONE device (`cuda:0`) while the wire
is gloo on host copies (`dist_utils.HostStagedComm`).

Exactness follows kernel_cases.py: all weights are 1 (or integers 1..4
where a builder says so), so every weight sum, degree and sum of squared
degrees is an exact integer in fp64, and in fp32 below 2^24, in any atomic
or reduction order. The gain 2*(eiy - eix) - 2*vdeg*(ay - ax)*constant is
evaluated in fp64 from those exact inputs by the oracle and the kernels
alike. Every comparison built on these inputs is therefore torch.equal on
tensors and == on modularity.

A scenario is a function of (rank, world, comm, dev, backend) that returns
plain CPU data. `launch_worker` runs each scenario twice in every rank
process, in the same order on every rank: first the oracle (plain `Comm()`,
CPU tensors, backend "torch"), then the side under test (`HostStagedComm`
on `dev`; backend "hip" on a GPU, "torch" when `dev` is the CPU, which is
how the staging layer itself is checked without a GPU).
"""

from __future__ import annotations

import functools
import os
import time

import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import DistGraph, Graph, Partition

HUB_CUT = 2049                        # smallest CUVITE_HUB_CUT the ops accept
PLANTED_DEGREES = (2100, 600, 1100)   # hub pipeline, (512,1024], (1024,2048]
N_SWEEPS = 4


# ---- graphs -----------------------------------------------------------------

def _unit(g: Graph) -> Graph:
    return Graph(g.rowptr, g.tails, torch.ones_like(g.weights))


@functools.lru_cache(maxsize=None)
def hub_graph(weights: str = "unit") -> Graph:
    """R-MAT s12 (edge factor 16), renumbered by a seeded permutation (R-MAT
    itself puts every high-degree vertex into rank 0's slice), plus four
    groups of three planted vertices at ids (2k+1)*nv/8 + {0, 1, 2} with
    about PLANTED_DEGREES extra neighbours each, distinct and drawn over the
    whole id range, symmetrised. Every slice of a 2- or 3-rank split then
    holds vertices of the hub pipeline and of the two widest LDS classes,
    with most of their neighbours remote. For per-sweep checks only: Louvain
    from singletons does not improve Q on it.

    weights: "unit", or "int" for symmetric integer weights 1..4."""
    base = rmat_graph(12, 16, seed=6)
    nv = base.nv
    gen = torch.Generator().manual_seed(61)
    perm = torch.randperm(nv, generator=gen)
    src = perm[torch.repeat_interleave(torch.arange(nv), base.degrees())]
    dst = perm[base.tails]
    ps, pd = [], []
    for k in range(4):
        for j, d in enumerate(PLANTED_DEGREES):
            v = (2 * k + 1) * nv // 8 + j
            nb = torch.randperm(nv, generator=gen)[:d + 1]
            nb = nb[nb != v][:d]
            ps.append(torch.full((d,), v, dtype=torch.int64))
            pd.append(nb)
    ps, pd = torch.cat(ps), torch.cat(pd)
    s = torch.cat([src, ps, pd])
    t = torch.cat([dst, pd, ps])
    if weights == "unit":
        w = torch.ones(s.numel(), dtype=torch.float64)
    else:
        assert weights == "int"
        lo, hi = torch.minimum(s, t), torch.maximum(s, t)
        w = (1 + (lo * 31 + hi * 17) % 4).to(torch.float64)
    return Graph.from_edge_tuples(nv, s, t, w)


@functools.lru_cache(maxsize=None)
def converging_graph() -> Graph:
    """R-MAT s10 with unit weights: full Louvain runs several phases on it
    and is exactly P-invariant."""
    return _unit(rmat_graph(10, 16, seed=3))


@functools.lru_cache(maxsize=None)
def small_graph() -> Graph:
    """R-MAT s8 with unit weights, for the coloring / ordering variants
    (sequential passes over the colour classes make them slow per sweep)."""
    return _unit(rmat_graph(8, 8, seed=3))


def with_dtype(g: Graph, wdtype) -> Graph:
    return Graph(g.rowptr, g.tails, g.weights.to(wdtype))


def shard(g: Graph, rank: int, world: int) -> DistGraph:
    part = Partition.contiguous(g.nv, world)
    b, e = part.base(rank), part.bound(rank)
    e0, e1 = int(g.rowptr[b]), int(g.rowptr[e])
    return DistGraph(Graph((g.rowptr[b:e + 1] - g.rowptr[b]).clone(),
                           g.tails[e0:e1].clone(),
                           g.weights[e0:e1].clone()), part, rank)


def slice_profile(g: Graph, world: int):
    """Per rank: number of vertices above the hub cut, in (1024, 2048] and
    in (512, 1024], and the number of ghosts."""
    out = []
    for r in range(world):
        dg = shard(g, r, world)
        deg = dg.g.degrees()
        out.append({
            "hub": int((deg > HUB_CUT).sum()),
            "c2048": int(((deg > 1024) & (deg <= 2048)).sum()),
            "c1024": int(((deg > 512) & (deg <= 1024)).sum()),
            "ghosts": int(dg.ghost_vertices().numel()),
        })
    return out


# ---- label states -------------------------------------------------------------

LABEL_STATES = ("singletons", "random", "few")


def label_state(name: str, nv: int, seed: int = 11) -> torch.Tensor:
    """Global labels int64 [nv]: `singletons`; `random`, about nv/8
    communities whose ids are drawn over the whole id range (so most are
    remote to any rank); `few`, five communities."""
    assert name in LABEL_STATES
    if name == "singletons":
        return torch.arange(nv)
    gen = torch.Generator().manual_seed(seed)
    k = nv // 8 if name == "random" else 5
    ids = torch.randperm(nv, generator=gen)[:k]
    return ids[torch.randint(0, k, (nv,), generator=gen)]


# ---- scenarios ------------------------------------------------------------------

def _cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def _sc_halo(rank, world, comm, dev, backend):
    from cuvite_amd.halo import build_halo, exchange_ghost_labels
    dg = shard(hub_graph(), rank, world).to(dev)
    ctx = build_halo(dg, comm)
    labels = torch.arange(dg.base, dg.bound, dtype=torch.int64,
                          device=dev) * 10
    got = exchange_ghost_labels(ctx, labels)
    return {"ghosts": ctx.ghosts, "tails_dense": ctx.tails_dense,
            "recv_offsets": ctx.recv_offsets, "send_idx": ctx.send_idx,
            "exchanged": got, "wire_dtype": str(ctx.wire_dtype),
            "buffers_on": sorted({b.device.type
                                  for b in ctx.send_buf + ctx.recv_buf})}


def _sweeps(rank, world, comm, dev, backend, wdtype, start, cut):
    """N_SWEEPS forced sweeps on a hub_graph shard; the labels rotate after
    every sweep whatever the modularity does."""
    from cuvite_amd.louvain import (LouvainConfig, PhaseState, _modularity,
                                    _one_sweep, _pick_move_fn)
    old = os.environ.get("CUVITE_HUB_CUT")
    if cut is None:
        os.environ.pop("CUVITE_HUB_CUT", None)
    else:
        os.environ["CUVITE_HUB_CUT"] = str(cut)
    try:
        g = with_dtype(hub_graph(), wdtype)
        dg = shard(g, rank, world).to(dev)
        init = None
        if start != "singletons":
            init = label_state(start, g.nv)[dg.base:dg.bound].clone().to(dev)
        cfg = LouvainConfig(backend=backend)
        state = PhaseState(dg, comm, init_labels=init)
        move_fn = _pick_move_fn(cfg, dev)
        state.use_hip = dev.type == "cuda" and backend in ("auto", "hip")
        hubs = (dg.g.degrees() > HUB_CUT).nonzero(as_tuple=True)[0]
        sweeps = []
        for _ in range(N_SWEEPS):
            target = _one_sweep(state, cfg, move_fn, None)
            q = _modularity(state)
            sweeps.append({
                "target": target.clone(),
                "cluster_weight": state.cluster_weight.clone(),
                "local_size": state.local_size.clone(),
                "local_degree": state.local_degree.clone(),
                "modularity": q,
                "comm_gid": torch.cat([state._local_gids(), state._runiv]),
                "universe": int(state._runiv.numel()),
                "hubs_moved": int((target[hubs]
                                   != state.curr_comm[hubs]).sum()),
            })
            state.past_comm, state.curr_comm = state.curr_comm, target
        return {"sweeps": sweeps, "n_hubs": int(hubs.numel())}
    finally:
        if old is None:
            os.environ.pop("CUVITE_HUB_CUT", None)
        else:
            os.environ["CUVITE_HUB_CUT"] = old


def _louvain(rank, world, comm, dev, backend, graph_fn, init, **kw):
    from cuvite_amd.louvain import LouvainConfig, louvain
    g = graph_fn()
    dg = shard(g, rank, world).to(dev)
    lab = None
    if init is not None:
        lab = label_state(init, g.nv)[dg.base:dg.bound].clone().to(dev)
    res = louvain(dg, comm, LouvainConfig(backend=backend, **kw),
                  init_labels=lab)
    return {"modularity": res.modularity, "communities": res.communities,
            "total_iters": res.total_iters, "phases": res.phases}


LOUVAIN_VARIANTS = {
    # name: (graph builder, init label state, LouvainConfig arguments)
    "louvain_plain": (converging_graph, None, {}),
    "louvain_et1": (converging_graph, None, {"early_term": 1}),
    "louvain_et3": (converging_graph, None, {"early_term": 3}),
    "louvain_warm": (converging_graph, "random", {}),
    "louvain_coloring": (small_graph, None,
                         {"coloring": True, "max_colors": 8}),
    "louvain_ordering": (small_graph, None,
                         {"ordering": True, "max_colors": 8}),
}


def coarsen_labels(lo: int, hi: int, dev=None) -> torch.Tensor:
    return torch.arange(lo, hi, dtype=torch.int64, device=dev) // 7


def _sc_coarsen(rank, world, comm, dev, backend):
    from cuvite_amd.coarsen import coarsen
    dg = shard(hub_graph("int"), rank, world).to(dev)
    cvect = coarsen_labels(dg.base, dg.bound, dev)
    new_dg, renum = coarsen(dg, comm, cvect)
    return {"rowptr": new_dg.g.rowptr, "tails": new_dg.g.tails,
            "weights": new_dg.g.weights, "parts": new_dg.partition.parts,
            "renum": renum(cvect.clone()),
            "on": new_dg.g.weights.device.type}


def _sc_coloring(rank, world, comm, dev, backend):
    from cuvite_amd.coloring import check_coloring, distance1_coloring
    dg = shard(hub_graph(), rank, world).to(dev)
    colors, nc = distance1_coloring(dg, comm, n_hash=4)
    conflicts = check_coloring(dg, comm, colors, exclude_color=nc - 1)
    return {"colors": colors, "num_colors": nc, "conflicts": conflicts}


def _sc_scoring(rank, world, comm, dev, backend):
    import dataclasses
    from cuvite_amd.halo import build_halo
    from cuvite_amd.quality import partition_quality
    g = converging_graph()
    dg = shard(g, rank, world).to(dev)
    halo = build_halo(dg, comm)
    out = {}
    for name in LABEL_STATES:
        lab = label_state(name, g.nv)[dg.base:dg.bound].clone().to(dev)
        q = partition_quality(dg, lab, comm, halo=halo, backend=backend)
        out[name] = dataclasses.asdict(q)
    return out


def _sweep_scenario(wdtype, start, cut):
    return lambda *a: _sweeps(*a, wdtype, start, cut)


def _louvain_scenario(name):
    graph_fn, init, kw = LOUVAIN_VARIANTS[name]
    return lambda *a: _louvain(*a, graph_fn, init, **kw)


SCENARIOS = {
    "halo": _sc_halo,
    "sweep_fp64_singletons": _sweep_scenario(torch.float64, "singletons",
                                             HUB_CUT),
    "sweep_fp64_random": _sweep_scenario(torch.float64, "random", HUB_CUT),
    "sweep_fp32_singletons": _sweep_scenario(torch.float32, "singletons",
                                             HUB_CUT),
    "sweep_fp32_random": _sweep_scenario(torch.float32, "random", HUB_CUT),
    # default hub cut: the planted hubs run in the 8192-slot LDS class
    "sweep_fp64_singletons_default_cut": _sweep_scenario(
        torch.float64, "singletons", None),
    **{name: _louvain_scenario(name) for name in LOUVAIN_VARIANTS},
    "coarsen": _sc_coarsen,
    "coloring": _sc_coloring,
    "scoring": _sc_scoring,
}
SWEEP_SCENARIOS = tuple(n for n in SCENARIOS if n.startswith("sweep_"))


def _forbid_device_tensors_on_the_wire():
    """Make torch.distributed raise on a non-CPU tensor for the rest of this
    process (the rank processes of a launch share one device; only host
    copies may travel)."""
    import torch.distributed as dist

    def check(t):
        assert t.device.type == "cpu", \
            f"{t.device} tensor handed to torch.distributed"

    def guard(fn, tensors_of):
        @functools.wraps(fn)
        def inner(*a, **k):
            for t in tensors_of(a):
                check(t)
            return fn(*a, **k)
        return inner

    dist.all_reduce = guard(dist.all_reduce, lambda a: [a[0]])
    dist.all_gather = guard(dist.all_gather, lambda a: list(a[0]) + [a[1]])
    dist.batch_isend_irecv = guard(dist.batch_isend_irecv,
                                   lambda a: [o.tensor for o in a[0]])


def launch_worker(rank, world, names, devname):
    """run_dist target: every scenario in `names`, oracle first and the
    host-staged side second, unconditionally and in the same order on every
    rank (the parent compares). Nothing is caught: a scenario that raises
    ends its rank, its peers run into the collective timeout, and the
    launch fails as a whole. Returns {name: {"oracle": ..., "staged": ...}}."""
    from cuvite_amd.parallel import Comm
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(max(1, 16 // world))
    dev = torch.device(devname)
    backend = "hip" if dev.type == "cuda" else "torch"
    _forbid_device_tensors_on_the_wire()
    cpu = torch.device("cpu")
    out = {}
    for name in names:
        fn = SCENARIOS[name]
        t0 = time.perf_counter()
        oracle = _cpu(fn(rank, world, Comm(), cpu, "torch"))
        t1 = time.perf_counter()
        staged = _cpu(fn(rank, world, HostStagedComm(dev), dev, backend))
        if dev.type == "cuda":
            from cuvite_amd import ops
            ops.clear_phase_caches()
        out[name] = {"oracle": oracle, "staged": staged,
                     "seconds": (t1 - t0, time.perf_counter() - t1)}
    return out


def assert_same(a, b, path="result"):
    """Exact, structural equality: torch.equal on tensors (dtype included),
    == on everything else."""
    assert type(a) is type(b), f"{path}: {type(a)} vs {type(b)}"
    if torch.is_tensor(a):
        assert a.dtype == b.dtype and a.shape == b.shape, \
            f"{path}: {a.dtype}{tuple(a.shape)} vs {b.dtype}{tuple(b.shape)}"
        if not torch.equal(a, b):
            bad = (a != b).nonzero(as_tuple=True)[0]
            raise AssertionError(
                f"{path}: {bad.numel()} of {a.numel()} entries differ, "
                f"first at {bad[:8].tolist()}: {a[bad[:8]].tolist()} vs "
                f"{b[bad[:8]].tolist()}")
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), f"{path}: keys differ"
        for k in a:
            assert_same(a[k], b[k], f"{path}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), f"{path}: length {len(a)} vs {len(b)}"
        for i, (x, y) in enumerate(zip(a, b)):
            assert_same(x, y, f"{path}[{i}]")
    else:
        assert a == b, f"{path}: {a!r} vs {b!r}"


# ---- single-rank CPU references and the parent-side checks ---------------------

@functools.lru_cache(maxsize=None)
def single_rank_louvain(name: str):
    from cuvite_amd.graph import single_partition
    from cuvite_amd.louvain import LouvainConfig, louvain
    from cuvite_amd.parallel import Comm
    graph_fn, init, kw = LOUVAIN_VARIANTS[name]
    g = graph_fn()
    lab = None if init is None else label_state(init, g.nv)
    return louvain(single_partition(g), Comm(),
                   LouvainConfig(backend="torch", **kw), init_labels=lab)


@functools.lru_cache(maxsize=None)
def single_rank_coarsen():
    from cuvite_amd.coarsen import coarsen
    from cuvite_amd.graph import single_partition
    from cuvite_amd.parallel import Comm
    g = hub_graph("int")
    new, renum = coarsen(single_partition(g), Comm(),
                         coarsen_labels(0, g.nv))
    return new.g, renum(coarsen_labels(0, g.nv))


@functools.lru_cache(maxsize=None)
def single_rank_coloring():
    from cuvite_amd.coloring import distance1_coloring
    from cuvite_amd.graph import single_partition
    from cuvite_amd.parallel import Comm
    return distance1_coloring(single_partition(hub_graph()), Comm(), n_hash=4)


def _check_sweeps(name, world, outs):
    for r, o in enumerate(outs):
        sw = o["oracle"]["sweeps"]
        # conditions on the inputs, on the oracle side: the universe (and
        # with it C, the packed hub keys and end_bit) changes inside the
        # phase, after the hub adjacency was cached by the first sweep
        sizes = [0] + [s["universe"] for s in sw]
        grew = [i for i in range(N_SWEEPS) if sizes[i + 1] > sizes[i]]
        if "singletons" in name:
            assert len(grew) >= 2 and grew[-1] > 0, \
                f"{name} rank {r}: universe sizes {sizes[1:]}"
        else:
            # the `random` start references all of its nv/8 communities
            # from the first sweep on and no label can appear later that
            # was not there at the start: the universe is complete at once,
            # what changes per sweep is which entries are referenced
            assert sizes[1] >= 100, f"{name} rank {r}: {sizes[1:]}"
        assert o["oracle"]["n_hubs"] >= 1
        assert max(s["hubs_moved"] for s in sw) >= 1, \
            f"{name} rank {r}: no hub vertex ever changed community"
        # every sweep moved somebody, so the delta push was not idle
        for a, b in zip(sw, sw[1:]):
            assert not torch.equal(a["target"], b["target"])
    for i in range(N_SWEEPS):
        qs = {o["staged"]["sweeps"][i]["modularity"] for o in outs}
        assert len(qs) == 1, f"{name} sweep {i}: ranks disagree on Q: {qs}"


def _check_louvain(name, world, outs):
    for side in ("oracle", "staged"):
        for key in ("modularity", "total_iters", "phases"):
            assert len({o[side][key] for o in outs}) == 1
    if name == "louvain_ordering":
        # stale ghosts inside a sweep: not P-invariant by design, the
        # same-world oracle (compared by the caller) is the reference
        return
    ref = single_rank_louvain(name)
    got = outs[0]["staged"]
    comms = torch.cat([o["staged"]["communities"] for o in outs])
    assert torch.equal(comms, ref.communities), \
        f"{name} world {world}: communities differ from the single-rank run"
    assert got["modularity"] == ref.modularity
    assert got["total_iters"] == ref.total_iters
    assert got["phases"] == ref.phases


def _check_coarsen(name, world, outs):
    ref_g, ref_renum = single_rank_coarsen()
    st = [o["staged"] for o in outs]
    rowptr = st[0]["rowptr"]
    for s in st[1:]:
        rowptr = torch.cat([rowptr, s["rowptr"][1:] + rowptr[-1]])
    tails = torch.cat([s["tails"] for s in st])
    weights = torch.cat([s["weights"] for s in st])
    assert torch.equal(rowptr, ref_g.rowptr)
    assert torch.equal(tails, ref_g.tails)
    assert torch.equal(weights, ref_g.weights)
    assert torch.equal(torch.cat([s["renum"] for s in st]), ref_renum)
    for s in st:
        assert torch.equal(s["parts"], st[0]["parts"])
        assert int(s["parts"][-1]) == ref_g.nv
    # total weight conserved exactly (integer weights)
    assert float(weights.sum()) == float(hub_graph("int").weights.sum())


def _check_coloring(name, world, outs):
    ref_colors, ref_nc = single_rank_coloring()
    colors = torch.cat([o["staged"]["colors"] for o in outs])
    assert torch.equal(colors, ref_colors), "coloring must be P-independent"
    for o in outs:
        assert o["staged"]["num_colors"] == ref_nc
        assert o["staged"]["conflicts"] == 0


def _check_scoring(name, world, outs):
    from quality_cases import brute_modularity
    g = converging_graph()
    for state in LABEL_STATES:
        want = brute_modularity(g, label_state(state, g.nv))
        for o in outs:
            got = o["staged"][state]["modularity"]
            # fp64 rounding of a different summation formula (the bound
            # test_quality.py uses for the same comparison)
            assert abs(got - want) <= 1e-12, (state, got, want)
        assert len({o["staged"][state]["num_communities"]
                    for o in outs}) == 1


def _check_halo(name, world, outs):
    for o in outs:
        s = o["staged"]
        assert s["ghosts"].numel() > 0
        assert torch.equal(s["exchanged"], s["ghosts"] * 10)
        assert s["wire_dtype"] == "torch.int32"


def check_scenario(name: str, world: int, outs, devtype: str):
    """Parent-side verdict on one scenario of a launch. `outs` is the
    per-rank list of launch_worker()[name]. First the staged side against
    the same-world oracle, field by field and exactly; then what the
    scenario promises beyond that (single-rank references, conservation,
    conditions on the inputs)."""
    assert len(outs) == world
    outs = [{side: dict(o[side]) for side in ("oracle", "staged")}
            for o in outs]
    for r, o in enumerate(outs):
        # where the results lived is not part of the comparison
        for key, want in (("on", devtype), ("buffers_on", [devtype])):
            if key in o["staged"]:
                assert o["staged"].pop(key) == want, (name, r, key)
                o["oracle"].pop(key)
        assert_same(o["oracle"], o["staged"], f"{name} rank {r}")
    if name.startswith("sweep_"):
        _check_sweeps(name, world, outs)
    elif name.startswith("louvain_"):
        _check_louvain(name, world, outs)
    else:
        {"halo": _check_halo, "coarsen": _check_coarsen,
         "coloring": _check_coloring, "scoring": _check_scoring}[name](
            name, world, outs)
