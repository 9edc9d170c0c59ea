"""The HIP side of the V-cycle against its CPU oracle: the MARK
instantiation of the intra_weight kernel (ops.intra_boundary) at its span and
chunk boundaries, one refinement phase, and whole louvain(vcycle=True) runs
on one rank and on two ranks sharing the GPU.

Kernel inputs carry integer weights (quality_cases.csr_from_degrees), so cw
is exact in fp32 and fp64 in any order."""

import pytest
import torch

from cuvite_amd.graph import single_partition
from cuvite_amd.louvain import LouvainConfig, louvain
from cuvite_amd.parallel import Comm
from cuvite_amd.uncoarsen import intra_boundary_torch, run_uncoarsen_phase

from tests.dist_utils import run_dist

import vcycle_cases as vc
from quality_cases import csr_from_degrees

pytestmark = pytest.mark.gpu

WDTYPES = [torch.float32, torch.float64]
LDTYPES = [torch.int32, torch.int64]
_dt = {torch.float32: "fp32", torch.float64: "fp64", torch.int32: "i32",
       torch.int64: "i64"}.get
N_GHOST = 3
CUTS = [2049, 6144]


def _deg_lists(S):
    return [[0, 1, S - 1, S, S + 1, 0, 0, 3 * S + 1, 1],
            [S, S, 2 * S, 5, S - 5, 7],
            [3 * S + 1],
            [S // 2] * 3,
            [0] * 5,
            []]


@pytest.fixture
def ops():
    from cuvite_amd import ops as _ops
    _ops.clear_phase_caches()
    yield _ops
    _ops.clear_phase_caches()


@pytest.fixture
def dev():
    return torch.device("cuda:0")


def _case(S, which):
    """CSR with the degree list `which`, tails in [0, nv + N_GHOST), and a
    label array with one more slot: dense id nv + N_GHOST is a ghost no
    random tail points to."""
    degs = _deg_lists(S)[which]
    rowptr, tails, w, labels = csr_from_degrees(degs, N_GHOST, seed=40 + which)
    labels = torch.cat([labels, torch.tensor([1])])
    return degs, rowptr, tails, w, labels


def _run(ops, dev, rowptr, tails, w, labels, wdtype, ldtype):
    args = (rowptr.to(dev), tails.to(dev), w.to(wdtype).to(dev),
            labels.to(ldtype).to(dev))
    cw, mask = ops.intra_boundary(*args)
    assert mask.dtype == torch.uint8 and mask.shape == (rowptr.numel() - 1,)
    assert cw.dtype == wdtype
    assert torch.equal(cw, ops.intra_weight(*args))   # bit for bit
    return cw.cpu(), mask.cpu()


def _row_of(rowptr, e):
    return int(torch.searchsorted(rowptr, torch.tensor(e), right=True)) - 1


def _positions(S, degs, rowptr):
    """Edge indices at the places where the lane that owns an edge is
    special; only those the degree list has."""
    ne = int(rowptr[-1])
    pos = {}
    if ne > 0:
        pos["first_edge_of_a_span"] = S if ne > S else 0
        if ne % S:
            pos["last_edge_of_partial_last_span"] = ne - 1
    if ne >= S:
        pos["last_edge_of_a_span"] = S - 1
    if ne > 127:
        pos["lane_0_of_a_chunk"] = 64
        pos["lane_63_of_a_chunk"] = 127
    if 3 * S + 1 in degs:
        r = degs.index(3 * S + 1)
        first_inside = (int(rowptr[r]) + S - 1) // S   # first span inside
        e = (first_inside + 1) * S + S // 2            # the one after it
        assert int(rowptr[r]) <= (first_inside + 1) * S
        assert (first_inside + 2) * S <= int(rowptr[r + 1])
        pos["middle_span_of_the_long_row"] = e
    return pos


@pytest.mark.parametrize("ldtype", LDTYPES, ids=_dt)
@pytest.mark.parametrize("wdtype", WDTYPES, ids=_dt)
@pytest.mark.parametrize("which", range(6))
def test_intra_boundary_matches_twin(ops, dev, which, wdtype, ldtype):
    S = ops.intra_weight_span()
    degs, rowptr, tails, w, labels = _case(S, which)
    nv = len(degs)
    # random labels
    cw_ref, mask_ref = intra_boundary_torch(rowptr, tails, w, labels)
    assert torch.equal(mask_ref, vc.boundary_loop(rowptr, tails, labels))
    cw, mask = _run(ops, dev, rowptr, tails, w, labels, wdtype, ldtype)
    assert torch.equal(mask, mask_ref)
    assert torch.equal(cw.to(torch.float64), cw_ref)
    # one community: nothing is on the boundary
    one = torch.full_like(labels, 7)
    _, mask = _run(ops, dev, rowptr, tails, w, one, wdtype, ldtype)
    assert int(mask.sum()) == 0

    # all labels equal but for the one node behind a single chosen edge, a
    # node no other edge points to: a row without edges where the list has
    # one (tails that hit it go to ghost 0), else the spare ghost
    spare = nv + N_GHOST
    x_local = degs.index(0) if 0 in degs else None
    base_tails = tails.clone()
    if x_local is not None:
        base_tails[base_tails == x_local] = nv
    cases = [(name, e, x_local if x_local is not None else spare)
             for name, e in _positions(S, degs, rowptr).items()]
    if int(rowptr[-1]):
        cases.append(("ghost_tail", int(rowptr[-1]) // 3, spare))
    for name, e, x in cases:
        t = base_tails.clone()
        t[e] = x
        lab = one.clone()
        lab[x] = 9
        cw_ref, mask_ref = intra_boundary_torch(rowptr, t, w, lab)
        want = torch.zeros(nv, dtype=torch.uint8)
        want[_row_of(rowptr, e)] = 1
        assert torch.equal(mask_ref, want), name
        cw, mask = _run(ops, dev, rowptr, t, w, lab, wdtype, ldtype)
        assert torch.equal(mask, want), (name, e, mask.nonzero().tolist())
        assert torch.equal(cw.to(torch.float64), cw_ref), name


def test_zero_degree_rows_between_marked_rows_stay_zero(ops, dev):
    S = ops.intra_weight_span()
    degs, rowptr, tails, w, labels = _case(S, 0)
    assert degs[5] == degs[6] == 0 and degs[4] and degs[7]
    spare = len(degs) + N_GHOST
    t = tails.clone()
    t[int(rowptr[5]) - 1] = spare       # last edge of row 4
    t[int(rowptr[7])] = spare           # first edge of row 7
    lab = torch.full_like(labels, 7)
    lab[spare] = 9
    for wdtype in WDTYPES:
        _, mask = _run(ops, dev, rowptr, t, w, lab, wdtype, torch.int64)
        assert mask.nonzero(as_tuple=True)[0].tolist() == [4, 7]


def test_out_of_range_tails_mark_nothing(ops, dev):
    S = ops.intra_weight_span()
    degs, rowptr, tails, w, labels = _case(S, 1)
    short = labels[:len(degs) + 1]      # ghosts 1.. are outside the labels
    cw_ref, mask_ref = intra_boundary_torch(rowptr, tails, w, short)
    cw, mask = _run(ops, dev, rowptr, tails, w, short, torch.float64,
                    torch.int64)
    assert torch.equal(mask, mask_ref) and torch.equal(cw, cw_ref)
    one = torch.full_like(short, 3)
    _, mask = _run(ops, dev, rowptr, tails, w, one, torch.float64,
                   torch.int64)
    assert int(mask.sum()) == 0


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", ["rgg", "rmat10u"])
def test_refinement_phase_matches_cpu_oracle(ops, dev, monkeypatch, name,
                                             cut):
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    lab, rep, events = vc.phase_oracle(name)
    rec = vc.QRecorder()
    dg = single_partition(vc.graph(name)).to(dev)
    lab_d, _, rep_d = run_uncoarsen_phase(
        dg, Comm(dev), LouvainConfig(backend="hip"),
        vc.plain_run(name).communities.to(dev), observe=rec)
    print(f"{name}: sizes {rep_d.sizes_per_sweep} of {dg.nv} "
          f"q {rep_d.q_per_sweep}")
    assert rep_d.sizes_per_sweep == rep.sizes_per_sweep
    assert rep_d.boundary == rep.boundary and rep_d.sweeps == rep.sweeps
    assert torch.equal(lab_d.cpu(), lab)
    assert len(rep_d.q_per_sweep) == len(rep.q_per_sweep)
    for a, b in zip(rep_d.q_per_sweep, rep.q_per_sweep):
        assert abs(a - b) < 1e-12
    for e_d, e in zip(rec.q, events):
        assert torch.equal(e_d["labels"].cpu(), e["labels"])
    assert vc.same_reports([rep_d], [rep])


@pytest.mark.parametrize("name", ["karate", "rgg", "rmat10u"])
def test_whole_run_matches_cpu_oracle(ops, dev, name):
    want = vc.vcycle_run(name)
    dg = single_partition(vc.graph(name)).to(dev)
    res = louvain(dg, Comm(dev), LouvainConfig(backend="hip", vcycle=True))
    for lv in res.vcycle:
        print(f"{name}: {lv}")
    assert torch.equal(res.communities.cpu(), want.communities)
    assert vc.same_reports(res.vcycle, want.vcycle)
    assert abs(res.modularity - want.modularity) < 1e-12


def _w_two_ranks(rank, world, name):
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(8)
    dev = torch.device("cuda:0")
    return vc.dist_vcycle(rank, world, HostStagedComm(dev), dev, "hip", name,
                          False)


@pytest.mark.parametrize("name", ["karate2", "rgg"])
def test_two_ranks_on_one_gpu_match_cpu_oracle(name):
    """Both rank processes compute on cuda:0, the wire is gloo on host
    copies: labels and reports equal the one-rank CPU oracle's."""
    want = vc.vcycle_run(name)
    parts = run_dist(2, _w_two_ranks, name, timeout_s=60)
    assert torch.equal(torch.cat([p["labels"] for p in parts]),
                       want.communities)
    for p in parts:
        assert vc.same_reports(p["vcycle"], want.vcycle)
