"""HIP kernels at the edges the R-MAT tests reach only by chance: degree-class
boundaries with worst-case table load, distributed-shaped inputs (ghost
tails, remote communities), non-identity global ids above 2^32, fp32, and
the small kernels at odd sizes.

All data is integer-valued (see kernel_cases.py), so every comparison is
bit-for-bit: torch.equal against a plain torch reference computed on the
CPU, no tolerance and no allowed mismatches. tests/test_kernel_cases.py
shows on the CPU that the inputs have the properties relied on here."""

import functools

import pytest
import torch

from cuvite_amd.local_move import local_move_torch

from kernel_cases import LADDER, STATES, ladder_inputs, move_inputs_to

pytestmark = pytest.mark.gpu

SEED = 20
DTYPES = [torch.float32, torch.float64]
_dt = {torch.float32: "fp32", torch.float64: "fp64"}.get
SHAPES = [False, True]          # (ghosts, dup) in {(F, F), (T, T)}
_sh = {False: "plain", True: "ghostdup"}.get


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
def _ladder(wdtype, state, ghostdup):
    """CPU inputs and the CPU oracle's answer, computed once per case."""
    inp, L = ladder_inputs(wdtype, state, ghostdup, ghostdup, SEED)
    t_ref, cw_ref = local_move_torch(inp)
    return inp, L, t_ref, cw_ref


def _assert_same(got, ref, inp_cpu, only=None):
    """torch.equal on targets and cluster weights; on failure name the
    degrees of the mismatching vertices (ladder vertices first)."""
    t, cw = got[0].cpu(), got[1].cpu()
    t_ref, cw_ref = ref
    assert t.dtype == t_ref.dtype and cw.dtype == cw_ref.dtype
    if only is not None:
        t, cw, t_ref, cw_ref = t[only], cw[only], t_ref[only], cw_ref[only]
    if torch.equal(t, t_ref) and torch.equal(cw, cw_ref):
        return
    deg = inp_cpu.rowptr[1:] - inp_cpu.rowptr[:-1]
    if only is not None:
        deg = deg[only]
    bad = ((t != t_ref) | (cw != cw_ref)).nonzero(as_tuple=True)[0]
    pytest.fail(f"{bad.numel()} vertices differ from the oracle; degrees of "
                f"the first 40: {deg[bad][:40].tolist()}")


# ------------------------------ local move --------------------------------

@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("state", STATES)
def test_ladder_default_cut(ops, dev, state, ghostdup, wdtype):
    inp_cpu, L, t_ref, cw_ref = _ladder(wdtype, state, ghostdup)
    inp = move_inputs_to(inp_cpu, dev)
    vlists, hubs, _ = ops._buckets_for(inp.rowptr)
    assert all(v.numel() > 0 for v in vlists)
    assert [LADDER[h] for h in hubs.tolist()] == [6145, 7999, 8000, 8001]
    _assert_same(ops.local_move(inp), (t_ref, cw_ref), inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("ghostdup", SHAPES, ids=_sh)
@pytest.mark.parametrize("state", ["singleton", "random", "tied"])
@pytest.mark.parametrize("cut", [8000, 2049])
def test_ladder_hub_cut_extremes(ops, dev, monkeypatch, cut, state, ghostdup,
                                 wdtype):
    """cut=8000: the deg-7999 and deg-8000 rows fill the 8192-slot table
    with all-distinct keys (singleton state), 8001 stays on the hub path.
    cut=2049: class 6 holds the single deg-2049 vertex, eight hubs."""
    monkeypatch.setenv("CUVITE_HUB_CUT", str(cut))
    inp_cpu, L, t_ref, cw_ref = _ladder(wdtype, state, ghostdup)
    inp = move_inputs_to(inp_cpu, dev)
    vlists, hubs, _ = ops._buckets_for(inp.rowptr)
    hub_degs = [LADDER[h] for h in hubs.tolist()]
    cls6 = sorted(LADDER[v] for v in vlists[6].tolist() if v < L)
    if cut == 8000:
        assert hub_degs == [8001]
        assert cls6[-2:] == [7999, 8000]
    else:
        assert hub_degs == [4096, 4097, 6143, 6144, 6145, 7999, 8000, 8001]
        assert cls6 == [2049]
    _assert_same(ops.local_move(inp), (t_ref, cw_ref), inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("state,ghostdup", [("random", True),
                                            ("tied", False)])
@pytest.mark.parametrize("env", ["CUVITE_HUB_SEGSORT=0",
                                 "CUVITE_NO_OVERLAP=1"])
def test_ladder_env_variants_identical(ops, dev, monkeypatch, env, state,
                                       ghostdup, wdtype):
    """The torch-sort hub fallback and the single-stream schedule give the
    default path's output (and the oracle's)."""
    inp_cpu, L, t_ref, cw_ref = _ladder(wdtype, state, ghostdup)
    inp = move_inputs_to(inp_cpu, dev)
    t0, cw0 = ops.local_move(inp)
    ops.clear_phase_caches()
    name, val = env.split("=")
    monkeypatch.setenv(name, val)
    t1, cw1 = ops.local_move(inp)
    assert torch.equal(t0, t1) and torch.equal(cw0, cw1)
    _assert_same((t1, cw1), (t_ref, cw_ref), inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("state", ["few", "random"])
def test_ladder_hub_chunk_groups(ops, dev, monkeypatch, state, wdtype):
    """Four hubs (28k deduped edges) under a 9000-edge sort cap: one group
    per hub on the rocPRIM path; same answer as the single-group run."""
    inp_cpu, L, t_ref, cw_ref = _ladder(wdtype, state, True)
    inp = move_inputs_to(inp_cpu, dev)
    t0, cw0 = ops.local_move(inp)
    ops.clear_phase_caches()
    monkeypatch.setattr(ops, "_HUB_SORT_CHUNK", 9000)
    t1, cw1 = ops.local_move(inp)
    _, hubs, hdeg = ops._buckets_for(inp.rowptr)
    assert len(ops._hub_groups(inp, hubs, hdeg)) == 4
    assert torch.equal(t0, t1) and torch.equal(cw0, cw1)
    _assert_same((t1, cw1), (t_ref, cw_ref), inp_cpu)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("empty", [(), (2,), (0, 6)])
def test_vlist_padding_and_empty_classes(ops, dev, empty, wdtype):
    """Class lists whose lengths are no multiple of the vertices per block
    (16 for class 0, 4 for classes 1-3), and empty classes: listed vertices
    match the oracle, every other vertex keeps (curr_comm, 0)."""
    inp_cpu, L, t_ref, cw_ref = _ladder(wdtype, "random", True)
    inp = move_inputs_to(inp_cpu, dev)
    vlists, _, _ = ops._buckets_for(inp.rowptr)
    vlists = list(vlists)
    for c, per_block, rem in ((0, 16, 13), (1, 4, 3), (2, 4, 1), (3, 4, 2)):
        n = vlists[c].numel()
        n -= (n - rem) % per_block
        assert n >= 1
        vlists[c] = vlists[c][:n].contiguous()
        assert vlists[c].numel() % per_block == rem
    for c in empty:
        vlists[c] = vlists[c][:0]
    t, cw = ops._require().local_move_bucketed(
        inp.rowptr, inp.tails, inp.weights, inp.curr_comm, inp.v_degree,
        inp.comm_size, inp.comm_degree, inp.comm_gid, float(inp.constant),
        vlists)
    listed = torch.zeros(inp.nv, dtype=torch.bool)
    listed[torch.cat(vlists).cpu().to(torch.int64)] = True
    assert int(listed.sum()) == sum(v.numel() for v in vlists)
    _assert_same((t, cw), (t_ref, cw_ref), inp_cpu, only=listed)
    rest = ~listed
    assert int(rest.sum()) >= 4
    assert torch.equal(t.cpu()[rest], inp_cpu.curr_comm[:inp.nv][rest])
    assert not bool(cw.cpu()[rest].any())


# ----------------------------- small kernels ------------------------------

@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("n", [0, 1, 255, 257, 65535 * 256 + 7])
def test_scatter_add_sizes(ops, dev, n, wdtype):
    """Values 0..3 over 1000 bins: every partial sum is an integer below
    2^24 (n * 3 / 1000 plus the start value), exact in fp32 in any order.
    The last size is one grid-stride step past the 65535-block cap."""
    g = torch.Generator(device=dev).manual_seed(n)
    nb = 1000
    idx = torch.randint(0, nb, (n,), generator=g, device=dev)
    val = torch.randint(0, 4, (n,), generator=g, device=dev)
    start = torch.arange(nb, device=dev) % 7
    out = start.to(wdtype)
    ops.scatter_add_(out, idx, val.to(wdtype))
    ref = start.cpu().index_add_(0, idx.cpu(), val.cpu())
    assert out.dtype == wdtype
    assert torch.equal(out.cpu(), ref.to(wdtype))


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_scatter_add_one_hot_bin(ops, dev, wdtype):
    n = 1 << 20                        # sum <= 3 * 2^20 < 2^24
    g = torch.Generator(device=dev).manual_seed(1)
    idx = torch.full((n,), 5, dtype=torch.int64, device=dev)
    val = torch.randint(0, 4, (n,), generator=g, device=dev)
    out = torch.zeros(9, dtype=wdtype, device=dev)
    ops.scatter_add_(out, idx, val.to(wdtype))
    ref = torch.zeros(9, dtype=torch.int64)
    ref[5] = int(val.sum())
    assert torch.equal(out.cpu(), ref.to(wdtype))


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("nv", [1, 63, 64, 65, 255, 257, 2048 * 256 + 3])
def test_modularity_parts_sizes(ops, dev, nv, wdtype):
    """Integers: sum(cw) < 2^23 and sum(cd^2) < 2^40, exact in fp64."""
    g = torch.Generator(device=dev).manual_seed(nv)
    cw = torch.randint(0, 8, (nv,), generator=g, device=dev)
    cd = torch.randint(0, 1024, (nv,), generator=g, device=dev)
    got = ops.modularity_parts(cw.to(wdtype), cd.to(wdtype))
    cwc, cdc = cw.cpu(), cd.cpu()
    ref = torch.stack([cwc.sum(), (cdc * cdc).sum()]).to(torch.float64)
    assert got.dtype == torch.float64
    assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_row_sum_hand_built_rows(ops, dev, wdtype):
    lens = torch.tensor([0, 0, 1, 63, 64, 65, 0, 129, 1000, 0, 0, 7, 0])
    nv = lens.numel()
    assert nv % 4 != 0
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, dim=0)
    w = torch.randint(1, 5, (int(rowptr[-1]),),
                      generator=torch.Generator().manual_seed(2))
    got = ops.row_sum(rowptr.to(dev), w.to(wdtype).to(dev))
    ref = torch.zeros(nv, dtype=torch.int64).index_add_(
        0, torch.repeat_interleave(torch.arange(nv), lens), w)
    assert got.dtype == wdtype
    assert torch.equal(got.cpu(), ref.to(wdtype))


def _deltas_case(case, nv, base, bound, g):
    if case == "none_moved":
        curr = torch.randint(base - 50, bound + 50, (nv,), generator=g)
        target = curr.clone()
    elif case == "all_moved":
        curr = torch.randint(base - 50, bound + 50, (nv,), generator=g)
        target = curr + 1 + torch.randint(0, 40, (nv,), generator=g)
    elif case == "mixed":
        curr = torch.randint(base - 50, bound + 50, (nv,), generator=g)
        target = torch.where(torch.rand(nv, generator=g) < 0.4,
                             torch.randint(base - 50, bound + 50, (nv,),
                                           generator=g), curr)
    elif case == "one_to_one":
        # every vertex leaves community base+3 and enters base+5
        curr = torch.full((nv,), base + 3, dtype=torch.int64)
        target = torch.full((nv,), base + 5, dtype=torch.int64)
    else:
        raise AssertionError(case)
    return curr, target


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", ["none_moved", "all_moved", "mixed",
                                  "one_to_one", "no_local"])
def test_apply_deltas_cases(ops, dev, case, wdtype):
    """Integer degrees 0..3 on 100003 vertices: every partial sum stays an
    integer of magnitude < 2^24, exact in fp32 in any atomic order."""
    g = torch.Generator().manual_seed(5)
    nv, base = 100003, 1000
    bound = base if case == "no_local" else base + 300
    curr, target = _deltas_case("mixed" if case == "no_local" else case,
                                nv, base, base + 300, g)
    vdeg = torch.randint(0, 4, (nv,), generator=g)
    size0 = torch.randint(1, 9, (300,), generator=g)
    degree0 = torch.randint(0, 1000, (300,), generator=g)
    size, degree = size0.to(dev), degree0.to(wdtype).to(dev)
    ops.apply_deltas_(target.to(dev), curr.to(dev), vdeg.to(wdtype).to(dev),
                      base, bound, size, degree)
    size_ref, degree_ref = size0.clone(), degree0.clone()
    moved = target != curr
    for lab, sign in ((curr, -1), (target, 1)):
        m = moved & (lab >= base) & (lab < bound)
        size_ref.index_add_(0, lab[m] - base,
                            torch.full((int(m.sum()),), sign))
        degree_ref.index_add_(0, lab[m] - base, sign * vdeg[m])
    if case in ("none_moved", "no_local"):
        assert torch.equal(size_ref, size0) and torch.equal(degree_ref,
                                                            degree0)
    else:
        assert not torch.equal(size_ref, size0)
    assert torch.equal(size.cpu(), size_ref)
    assert degree.dtype == wdtype
    assert torch.equal(degree.cpu(), degree_ref.to(wdtype))


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_recount_ignores_out_of_range_labels(ops, dev, wdtype):
    """Labels below base and at or above base+ncomm are skipped (the
    kernel's documented guard); buffers around the output slices keep their
    sentinels."""
    g = torch.Generator().manual_seed(6)
    nv, base, ncomm, pad = 40003, 500, 777, 64
    labels = torch.randint(base - 200, base + ncomm + 200, (nv,), generator=g)
    labels[:4] = torch.tensor([base - 1, base, base + ncomm - 1, base + ncomm])
    vdeg = torch.randint(0, 4, (nv,), generator=g)
    size_buf = torch.full((ncomm + 2 * pad,), -7, dtype=torch.int64,
                          device=dev)
    deg_buf = torch.full((ncomm + 2 * pad,), -7, dtype=wdtype, device=dev)
    size = size_buf[pad:pad + ncomm]
    degree = deg_buf[pad:pad + ncomm]
    assert size.is_contiguous() and degree.is_contiguous()
    ops._require().recount_(labels.to(dev), vdeg.to(wdtype).to(dev), base,
                            size, degree)
    ok = (labels >= base) & (labels < base + ncomm)
    assert 0 < int(ok.sum()) < nv
    size_ref = torch.bincount(labels[ok] - base, minlength=ncomm)
    degree_ref = torch.zeros(ncomm, dtype=torch.int64).index_add_(
        0, labels[ok] - base, vdeg[ok])
    assert torch.equal(size.cpu(), size_ref)
    assert torch.equal(degree.cpu(), degree_ref.to(wdtype))
    for buf in (size_buf, deg_buf):
        assert bool((buf[:pad] == -7).all()) and bool((buf[-pad:] == -7).all())


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
def test_csr_from_edges_every_row(ops, dev, wdtype):
    """Empty rows (first, last, every odd one), one row with half of all
    edges, base != 0; all rows compared as multisets of (tail, weight)."""
    g = torch.Generator().manual_seed(8)
    nv, base, ne = 301, 1000, 40000
    rows = 6 + 2 * torch.randint(0, 144, (ne,), generator=g)   # even, 6..292
    rows[: ne // 2] = 18
    rows = rows[torch.randperm(ne, generator=g)]
    dst = torch.randint(0, 8192, (ne,), generator=g)
    w = torch.randint(1, 8, (ne,), generator=g)
    rowptr, tails, weights = ops.csr_from_edges(
        nv, base, (rows + base).to(dev), dst.to(dev), w.to(wdtype).to(dev))
    deg = torch.bincount(rows, minlength=nv)
    assert int(deg[0]) == 0 and int(deg[-1]) == 0 and int(deg[18]) >= ne // 2
    rowptr_ref = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr_ref[1:] = torch.cumsum(deg, dim=0)
    assert torch.equal(rowptr.cpu(), rowptr_ref)
    assert weights.dtype == wdtype and tails.dtype == torch.int64
    row_of = torch.repeat_interleave(torch.arange(nv, device=dev),
                                     (rowptr[1:] - rowptr[:-1]))
    # (row, tail, weight) packed into one sortable integer: tail < 2^13,
    # weight < 2^3 and integral
    assert torch.equal(weights, weights.round())
    got = (row_of * 8192 + tails) * 8 + weights.to(torch.int64)
    ref = ((rows * 8192 + dst) * 8 + w).to(dev)
    assert torch.equal(torch.sort(got)[0], torch.sort(ref)[0])


def _agg_ref(key, w):
    uniq, inv = torch.unique(key, return_inverse=True)
    return uniq, torch.zeros(uniq.numel(), dtype=torch.int64).index_add_(
        0, inv, w)


def _key_cases():
    g = torch.Generator().manual_seed(9)
    cases = {
        "n1": torch.tensor([12345], dtype=torch.int64),
        "all_equal": torch.full((5000,), 77, dtype=torch.int64),
        "all_distinct": torch.randperm(5000, generator=g) * 3 + 1,
    }
    for k in (1, 31, 32, 50):
        for top, name in (((1 << k) - 1, f"max_2p{k}_minus1"),
                          (1 << k, f"max_2p{k}")):
            key = torch.randint(0, top + 1, (4000,), generator=g)
            key[::7] = top                       # the maximum, repeated
            key[1::7] = key[2::7][: key[1::7].numel()]   # more duplicates
            cases[name] = key
    return cases


_KEYS = _key_cases()


@pytest.mark.parametrize("wdtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("name", list(_KEYS))
def test_aggregate_keys_end_bit_boundaries(ops, dev, name, wdtype):
    """coarsen._aggregate_keys sorts only bit_length(max key) bits; the
    maximum key sits exactly below and exactly on a power of two."""
    from cuvite_amd.coarsen import _aggregate_keys
    key = _KEYS[name]
    w = torch.randint(1, 5, (key.numel(),),
                      generator=torch.Generator().manual_seed(10))
    uniq_ref, sums_ref = _agg_ref(key, w)
    uniq, sums = _aggregate_keys(key.to(dev), w.to(wdtype).to(dev))
    assert torch.equal(uniq.cpu(), uniq_ref)
    assert sums.dtype == wdtype
    assert torch.equal(sums.cpu(), sums_ref.to(wdtype))
    # the binding itself in this dtype (the wrapper always passes fp64)
    end_bit = max(1, int(key.max()).bit_length())
    u2, s2, cnt = ops._require().sort_reduce_pairs(
        key.to(dev), w.to(wdtype).to(dev), end_bit)
    m = int(cnt[0])
    assert m == uniq_ref.numel()
    assert torch.equal(u2[:m].cpu(), uniq_ref)
    assert torch.equal(s2[:m].cpu(), sums_ref.to(wdtype))


def test_aggregate_pairs_fp32(ops, dev):
    from cuvite_amd.coarsen import _aggregate
    g = torch.Generator().manual_seed(11)
    n, gnc = 30000, 997
    s = torch.randint(0, gnc, (n,), generator=g)
    t = torch.randint(0, gnc, (n,), generator=g)
    s[0], t[0] = gnc - 1, gnc - 1                 # largest possible key
    w = torch.randint(1, 5, (n,), generator=g)
    uniq_ref, sums_ref = _agg_ref(s * gnc + t, w)
    gs, gt, gw = _aggregate(s.to(dev), t.to(dev),
                            w.to(torch.float32).to(dev), gnc)
    assert torch.equal(gs.cpu(), uniq_ref // gnc)
    assert torch.equal(gt.cpu(), uniq_ref % gnc)
    assert gw.dtype == torch.float32
    assert torch.equal(gw.cpu(), sums_ref.to(torch.float32))


def _coloring_state():
    """Partly coloured distributed-shaped round state on the CPU."""
    g = torch.Generator().manual_seed(12)
    base, ng = 1000, 48
    lens = torch.tensor([0, 63, 64, 65, 129, 1, 0, 0, 7, 200, 3] * 13)
    nv = lens.numel()                                  # 143
    assert nv % 4 != 0
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, dim=0)
    tails = torch.randint(0, nv + ng, (int(rowptr[-1]),), generator=g)
    seg = torch.repeat_interleave(torch.arange(nv), lens)
    # self-loops on a fifth of the edges' rows
    loop = torch.rand(tails.numel(), generator=g) < 0.05
    tails[loop] = seg[loop]
    colors = torch.where(torch.rand(nv, generator=g) < 0.4,
                         torch.randint(0, 8, (nv,), generator=g),
                         torch.full((nv,), -1))
    ghost_uncolored = torch.rand(ng, generator=g) < 0.5
    ghost_uncolored[:2] = True
    # ghost gids above 2^32; the first two share their low 32 bits with the
    # local vertices base+1 and base+2 (same hash, but not "self")
    ghosts = (5 << 32) + torch.randperm(1 << 20, generator=g)[:ng] * 4099
    ghosts[0] = (1 << 32) + base + 1
    ghosts[1] = (7 << 32) + base + 2
    # vertex 1 (63 edges, uncoloured): ghost 0 among its neighbours;
    # vertex 2 (64 edges, uncoloured): every neighbour coloured or itself
    colors[1] = colors[2] = -1
    tails[rowptr[1]] = nv
    coloured = torch.cat([(colors >= 0).nonzero(as_tuple=True)[0],
                          nv + (~ghost_uncolored).nonzero(as_tuple=True)[0]])
    pick = torch.randint(0, coloured.numel(), (64,), generator=g)
    tails[rowptr[2]:rowptr[3]] = coloured[pick]
    tails[rowptr[2] + 5] = 2
    gid_all = torch.cat([torch.arange(base, base + nv), ghosts])
    uncolored_all = torch.cat([colors < 0, ghost_uncolored])
    return (rowptr, tails.to(torch.int32), gid_all, uncolored_all, colors,
            base)


@pytest.mark.parametrize("n_hash", [1, 4, 8])
def test_coloring_minmax_matches_torch_path(ops, dev, n_hash):
    from cuvite_amd.coloring import _minmax_torch
    rowptr, tails, gid_all, uncolored_all, colors, base = _coloring_state()
    seeds = [(0xF0000000 + 1012 + 1043 * t) & 0xFFFFFFFF
             for t in range(n_hash)]
    mns, mxs = _minmax_torch(rowptr, tails, gid_all, uncolored_all, colors,
                             base, seeds)
    mn_ref, mx_ref = torch.stack(mns, dim=1), torch.stack(mxs, dim=1)
    # the state has what the test is about
    assert int(mn_ref[2, 0]) == 1 << 33 and int(mx_ref[2, 0]) == -1
    assert int(colors[1]) < 0 and int(mx_ref[1, 0]) >= 0
    done = colors >= 0
    assert bool(done.any()) and bool((mx_ref[done] == -1).all())
    assert int(((mx_ref[:, 0] >= 0) & ~done).sum()) > 50
    mn, mx = ops._require().coloring_minmax(
        rowptr.to(dev), tails.to(dev), gid_all.to(dev),
        uncolored_all.to(dev), colors.to(dev), base,
        torch.tensor(seeds, dtype=torch.int64, device=dev))
    assert torch.equal(mn.cpu(), mn_ref)
    assert torch.equal(mx.cpu(), mx_ref)
