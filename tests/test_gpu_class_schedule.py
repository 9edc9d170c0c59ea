"""The HIP local-move kernels under the class schedule: the block classes
running beside the sub classes on an auxiliary stream that is forked from
and joined into the calling stream inside the binding, and the edge loop at
every degree where a lane's number of pipelined and remainder trips changes.

All data is integer-valued (schedule_cases.py), so every comparison is
torch.equal against the CPU oracle, no tolerance.
tests/test_schedule_cases.py shows on the CPU that the inputs have the
properties relied on here."""

import functools

import pytest
import torch

from cuvite_amd.generators import rmat_graph
from cuvite_amd.graph import single_partition
from cuvite_amd.local_move import local_move_torch
from cuvite_amd.louvain import (LouvainConfig, PhaseState, _modularity,
                                _one_sweep, _pick_move_fn)
from cuvite_amd.parallel import Comm

from fused_cases import (RMAT_STEP_CASES, aggregates_of, isolated_sizes,
                         with_isolated)
from kernel_cases import move_inputs_to
from schedule_cases import LADDER, STATES, crowded, pipeline_ladder

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
SENTINEL, PAD = -7, 64
# (CUVITE_CLASS_STREAMS, CUVITE_NO_OVERLAP)
SCHEDULES = {"default": (None, None),
             "streams_off": ("0", None),
             "no_overlap": (None, "1"),
             "one_stream": ("0", "1")}


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _set_schedule(monkeypatch, name):
    for var, val in zip(("CUVITE_CLASS_STREAMS", "CUVITE_NO_OVERLAP"),
                        SCHEDULES[name]):
        if val is None:
            monkeypatch.delenv(var, raising=False)
        else:
            monkeypatch.setenv(var, val)


def _assert_same(got, ref, inp_cpu, what=""):
    t, cw = got[0].cpu(), got[1].cpu()
    assert t.dtype == ref[0].dtype and cw.dtype == ref[1].dtype
    if torch.equal(t, ref[0]) and torch.equal(cw, ref[1]):
        return
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    bad = ((t != ref[0]) | (cw != ref[1])).nonzero(as_tuple=True)[0]
    pytest.fail(f"{what}: {bad.numel()} vertices differ from the oracle; "
                f"degrees of the first 40: {deg[bad][:40].tolist()}")


# ----------------------------- pipeline ladder -----------------------------

@functools.lru_cache(maxsize=None)
def _ladder(wdtype, state, dup):
    inp, L = pipeline_ladder(wdtype, state, dup)
    return inp, L, local_move_torch(inp)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("dup", [False, True], ids=["plain", "dup"])
@pytest.mark.parametrize("state", STATES)
def test_pipeline_ladder_matches_oracle(ops, dev, state, dup, wdtype):
    """One vertex at every degree where a lane's edge count changes
    (k * stride - 1, k * stride, k * stride + 1 for k = 1..5 and the
    strides 16, 64 and 256), and on both sides of every class bound and of
    the hub cut."""
    inp_cpu, L, ref = _ladder(wdtype, state, dup)
    inp = move_inputs_to(inp_cpu, dev)
    vlists, hubs, _ = ops._buckets_for(inp.rowptr)
    assert all(v.numel() > 0 for v in vlists)
    assert [LADDER[h] for h in hubs.tolist()] == [6145]
    _assert_same(ops.local_move(inp), ref, inp_cpu, f"{state} dup={dup}")


# ----------------------------- crowded classes -----------------------------

@functools.lru_cache(maxsize=None)
def _crowded(wdtype, state):
    inp, L = crowded(wdtype, state)
    return inp, L, local_move_torch(inp)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("state", STATES)
def test_crowded_same_under_every_schedule(ops, dev, monkeypatch, state,
                                           wdtype):
    """Hundreds of vertices per block class, so blocks of several classes
    share CUs: the class streams on and off, each with and without the
    hub overlap, all give the oracle's output."""
    inp_cpu, L, ref = _crowded(wdtype, state)
    inp = move_inputs_to(inp_cpu, dev)
    for name in SCHEDULES:
        _set_schedule(monkeypatch, name)
        _assert_same(ops.local_move(inp), ref, inp_cpu, name)


# --------------------- fused aggregates under the schedule -----------------

@functools.lru_cache(maxsize=None)
def _iso_crowded(wdtype, state):
    base_inp, L, (t0, _) = _crowded(wdtype, state)
    inp, _ = with_isolated(base_inp, L, t0)
    t, cw = local_move_torch(inp)
    size, degree = aggregates_of(inp, t)
    return inp, (t, cw), size, degree, isolated_sizes(inp)


def _guarded(nc, wdtype, dev, iso):
    size_buf = torch.full((nc + 2 * PAD,), SENTINEL, dtype=torch.int64,
                          device=dev)
    deg_buf = torch.full((nc + 2 * PAD,), SENTINEL, dtype=wdtype, device=dev)
    nsize, ndegree = size_buf[PAD:PAD + nc], deg_buf[PAD:PAD + nc]
    assert nsize.is_contiguous() and ndegree.is_contiguous()
    nsize.copy_(iso.to(dev))
    ndegree.zero_()
    return size_buf, deg_buf, nsize, ndegree


def _guards_intact(*bufs):
    for buf in bufs:
        assert bool((buf[:PAD] == SENTINEL).all())
        assert bool((buf[-PAD:] == SENTINEL).all())


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("schedule", ["default", "streams_off"])
def test_crowded_fused_aggregates(ops, dev, monkeypatch, schedule, state,
                                  wdtype):
    """next_size / next_degree equal bincount / index_add_ of the oracle's
    targets over all vertices when the accounting lanes of the block
    classes run beside those of the sub classes, and the sentinels around
    the buffers stay."""
    _set_schedule(monkeypatch, schedule)
    inp_cpu, ref, size_ref, degree_ref, iso = _iso_crowded(wdtype, state)
    inp = move_inputs_to(inp_cpu, dev)
    nc = inp.comm_size.numel()
    size_buf, deg_buf, nsize, ndegree = _guarded(nc, wdtype, dev, iso)
    got = ops.local_move(inp, next_size=nsize, next_degree=ndegree)
    _assert_same(got, ref, inp_cpu, schedule)
    assert torch.equal(nsize.cpu(), size_ref)
    assert torch.equal(ndegree.cpu(), degree_ref.to(wdtype))
    _guards_intact(size_buf, deg_buf)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("streams", [True, False], ids=["streams", "serial"])
def test_padded_class0_list_adds_nothing(ops, dev, streams, wdtype):
    """The binding with -1 entries inside and behind the class-0 list: the
    aggregates hold the listed vertices (everything but the hubs) once."""
    inp_cpu, ref, size_ref, degree_ref, iso = _iso_crowded(wdtype, "random")
    inp = move_inputs_to(inp_cpu, dev)
    vlists, hubs, _ = ops._buckets_for(inp.rowptr)
    vlists = list(vlists)
    pad = torch.full((37,), -1, dtype=torch.int32, device=dev)
    n0 = vlists[0].numel()
    vlists[0] = torch.cat([vlists[0][:n0 // 2], pad[:5], vlists[0][n0 // 2:],
                           pad])
    nc = inp.comm_size.numel()
    size_buf, deg_buf, nsize, ndegree = _guarded(nc, wdtype, dev, iso)
    t, cw = ops._require().local_move_bucketed(
        inp.rowptr, inp.tails, inp.weights, inp.curr_comm, inp.v_degree,
        inp.comm_size, inp.comm_degree, inp.comm_gid, float(inp.constant),
        vlists, next_size=nsize, next_degree=ndegree, class_streams=streams)
    hubs = hubs.cpu()
    t_hub = ref[0][hubs].to(torch.int64)
    size_want = size_ref - torch.bincount(t_hub, minlength=nc)
    degree_want = degree_ref.clone().index_add_(
        0, t_hub, -inp_cpu.v_degree[hubs].to(torch.float64))
    assert torch.equal(nsize.cpu(), size_want)
    assert torch.equal(ndegree.cpu(), degree_want.to(wdtype))
    _guards_intact(size_buf, deg_buf)
    rest = torch.ones(inp.nv, dtype=torch.bool)
    rest[hubs] = False
    assert torch.equal(t.cpu()[rest], ref[0][rest])
    assert torch.equal(cw.cpu()[rest], ref[1][rest])


# ---------------------------- join and allocator ---------------------------

@pytest.mark.parametrize("stream", ["main", "other"])
def test_outputs_complete_when_handed_out(ops, dev, stream):
    """Back-to-back calls whose results are dropped at once while tensors
    of the same sizes are allocated and filled on the calling stream: an
    auxiliary stream that was not joined shows up as sentinel values or
    stale labels in a later comparison."""
    wdtype = torch.float64
    inp_cpu, L, ref = _crowded(wdtype, "random")
    inp = move_inputs_to(inp_cpu, dev)
    t_ref, cw_ref = ref[0].to(dev), ref[1].to(dev)
    torch.cuda.synchronize()
    calling = (torch.cuda.current_stream(dev) if stream == "main"
               else torch.cuda.Stream(device=dev))
    n_calls = 20 if stream == "main" else 1
    oks = []
    with torch.cuda.stream(calling):
        for _ in range(n_calls):
            t, cw = ops.local_move(inp)
            oks.append((t == t_ref).all() & (cw == cw_ref).all())
            del t, cw
            a = torch.full((inp.nv,), SENTINEL, dtype=torch.int32, device=dev)
            b = torch.full((inp.nv,), float(SENTINEL), dtype=wdtype,
                           device=dev)
            del a, b
    calling.synchronize()
    assert [bool(ok) for ok in oks] == [True] * n_calls


# -------------------------------- multi-step -------------------------------

def _unit_rmat(scale):
    g = rmat_graph(scale, 16, seed=3)
    g.weights.fill_(1.0)
    return g


def _run_steps(g, dev, n_steps):
    """Drive PhaseState / _one_sweep / _modularity the way bench.py does."""
    dg = single_partition(g.to(dev))
    cfg = LouvainConfig(backend="hip")
    state = PhaseState(dg, Comm(dev))
    state.use_hip = True
    move_fn = _pick_move_fn(cfg, dev)
    out = []
    for _ in range(n_steps):
        target = _one_sweep(state, cfg, move_fn, None)
        q = _modularity(state)
        state.past_comm, state.curr_comm = state.curr_comm, target
        out.append((state.curr_comm.cpu().clone(),
                    state.local_size.cpu().clone(),
                    state.local_degree.cpu().clone(),
                    state.cluster_weight.cpu().clone(), q))
    return out, state


@pytest.mark.parametrize("schedule", ["streams_off", "one_stream"])
def test_four_steps_same_with_switches_off(ops, dev, monkeypatch, schedule):
    """Four fused steps at R-MAT scale 14, cut 3600 (class 6 and the hub
    list both non-empty): labels, sizes, degrees, cluster weights and Q
    after every step equal the default schedule's (unit weights: exact)."""
    scale, cut = RMAT_STEP_CASES[-1]
    assert (scale, cut) == (14, 3600)
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    g = _unit_rmat(scale)
    _set_schedule(monkeypatch, "default")
    on, st = _run_steps(g, dev, 4)
    assert st._agg_spare is not None          # the fused path did run
    ops.clear_phase_caches()
    _set_schedule(monkeypatch, schedule)
    off, _ = _run_steps(g, dev, 4)
    for i, (a, b) in enumerate(zip(on, off)):
        for x, y, name in zip(a[:4], b[:4], ("curr_comm", "local_size",
                                             "local_degree",
                                             "cluster_weight")):
            assert torch.equal(x, y), (i, name)
        assert a[4] == b[4], (i, a[4], b[4])
    assert torch.equal(on[-1][1], torch.bincount(on[-1][0], minlength=g.nv))
