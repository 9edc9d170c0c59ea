"""The HIP refine-move kernels (one Leiden refinement round) against their
torch twin, on the refine cases of refine_cases.py: every degree class, the
hub pipeline at hub cuts 2049 and 6144 (the default), fp32 and fp64, with
and without ghosts.

All data is integer-valued (see kernel_cases.py), so every comparison is
bit-for-bit: torch.equal against `refine_move_torch` computed on the CPU.
tests/test_refine_cases.py shows on the CPU that the inputs make the bound
filter, the ineligible candidates, the vertices without a candidate and the
non-movers beside movers decide the answer on every route."""

import functools

import pytest
import torch

from cuvite_amd.local_move import local_move_torch, refine_move_torch

from kernel_cases import LADDER, move_inputs_to
from refine_cases import CASES, refine_case

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
SHAPES = [False, True]
_sh = {False: "plain", True: "ghostdup"}.get
CUTS = [2049, 6144]
PAD = 64


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
def _case(name, wdtype, ghostdup):
    """CPU inputs and the CPU twin's answer, computed once per case."""
    inp, L, mover, cand, _ = refine_case(name, wdtype, ghostdup)
    t_ref, cw_ref = refine_move_torch(inp, mover, cand)
    return inp, L, mover, cand, t_ref, cw_ref


@functools.lru_cache(maxsize=None)
def _plain_ref(name, wdtype, ghostdup):
    return local_move_torch(_case(name, wdtype, ghostdup)[0])


def _assert_same(got, ref, inp_cpu):
    t, cw = got[0].cpu(), got[1].cpu()
    t_ref, cw_ref = ref
    assert t.dtype == t_ref.dtype and cw.dtype == cw_ref.dtype
    if torch.equal(t, t_ref) and torch.equal(cw, cw_ref):
        return
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    bad = ((t != t_ref) | (cw != cw_ref)).nonzero(as_tuple=True)[0]
    pytest.fail(f"{bad.numel()} vertices differ from the twin; degrees of "
                f"the first 40: {deg[bad][:40].tolist()}")


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("cut", CUTS)
def test_refine_move_matches_twin(ops, dev, monkeypatch, cut, name, ghostdup,
                                  wdtype):
    """cut 6144: hubs 6145..8001, class 6 holds 2049..6144. cut 2049: class
    6 holds the single deg-2049 vertex, eight hubs. The results are written
    into buffers with sentinels on both sides."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    inp_cpu, L, mover, cand, t_ref, cw_ref = _case(name, wdtype, ghostdup)
    inp = move_inputs_to(inp_cpu, dev)
    vlists, hubs, _ = ops._buckets_for(inp.rowptr)
    assert all(v.numel() > 0 for v in vlists)
    hub_degs = [LADDER[h] for h in hubs.tolist()]
    if cut == 2049:
        assert hub_degs == [4096, 4097, 6143, 6144, 6145, 7999, 8000, 8001]
    else:
        assert hub_degs == [6145, 7999, 8000, 8001]
    nv = inp.nv
    t_buf = torch.full((nv + 2 * PAD,), -7, dtype=torch.int32, device=dev)
    cw_buf = torch.full((nv + 2 * PAD,), -7, dtype=wdtype, device=dev)
    out = (t_buf[PAD:PAD + nv], cw_buf[PAD:PAD + nv])
    got = ops.refine_move(inp, mover.to(dev), cand.to(dev), out=out)
    assert got[0].data_ptr() == out[0].data_ptr()
    assert got[1].data_ptr() == out[1].data_ptr()
    _assert_same(got, (t_ref, cw_ref), inp_cpu)
    for buf in (t_buf, cw_buf):
        assert bool((buf[:PAD] == -7).all()) and bool((buf[-PAD:] == -7).all())


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("name", ["foreign", "random"])
def test_local_move_unchanged_on_the_same_inputs(ops, dev, name, ghostdup,
                                                 wdtype):
    """The plain kernels share their bodies with the refine ones: they still
    give their own oracle's answer, before and after a refine call."""
    inp_cpu, L, mover, cand, _, _ = _case(name, wdtype, ghostdup)
    ref = _plain_ref(name, wdtype, ghostdup)
    inp = move_inputs_to(inp_cpu, dev)
    _assert_same(ops.local_move(inp), ref, inp_cpu)
    ops.refine_move(inp, mover.to(dev), cand.to(dev))
    _assert_same(ops.local_move(inp), ref, inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("name", ["ineligible", "random"])
@pytest.mark.parametrize("env", ["CUVITE_HUB_SEGSORT=0",
                                 "CUVITE_NO_OVERLAP=1",
                                 "CUVITE_CLASS_STREAMS=0"])
def test_refine_env_variants_identical(ops, dev, monkeypatch, env, name,
                                       wdtype):
    """The torch-sort hub fallback and the serial schedules give the default
    path's output (and the twin's)."""
    inp_cpu, L, mover, cand, t_ref, cw_ref = _case(name, wdtype, True)
    inp = move_inputs_to(inp_cpu, dev)
    mb, cb = mover.to(dev), cand.to(dev)
    t0, cw0 = ops.refine_move(inp, mb, cb)
    ops.clear_phase_caches()
    key, val = env.split("=")
    monkeypatch.setenv(key, val)
    t1, cw1 = ops.refine_move(inp, mb, cb)
    assert torch.equal(t0, t1) and torch.equal(cw0, cw1)
    _assert_same((t1, cw1), (t_ref, cw_ref), inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_round_without_hub_movers_skips_the_hub_pipeline(ops, dev, wdtype):
    """No hub moves: the hub statics are not even built, hubs keep their
    labels, everyone else matches the twin."""
    inp_cpu, L, mover, cand, _, _ = _case("foreign", wdtype, False)
    mover = mover.clone()
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    mover[deg > 6144] = -1
    t_ref, cw_ref = refine_move_torch(inp_cpu, mover, cand)
    inp = move_inputs_to(inp_cpu, dev)
    got = ops.refine_move(inp, mover.to(dev), cand.to(dev))
    assert len(ops._hub_static_cache) == 0
    _assert_same(got, (t_ref, cw_ref), inp_cpu)
