"""CPU-only input builders for the computed-gid, fused-aggregate and hub
slice tests. Plain torch on the CPU, no GPU and no `cuvite_amd.ops` import;
`tests/test_fused_cases.py` shows on the oracle alone that these inputs have
the properties `tests/test_gpu_fused_step.py` relies on.

All data is integer-valued as in kernel_cases.py (unit or small integer
weights, a power-of-two `constant`), so every oracle answer is exact and
dtype-independent."""

from __future__ import annotations

import dataclasses

import torch

from cuvite_amd.local_move import MoveInputs

from kernel_cases import LADDER, N_GHOST, ladder_inputs

SEED = 20
GID_BASES = (0, 1 << 20, (3 << 32) + 7)
CLASS_BOUNDS = (16, 64, 256, 512, 1024, 2048)
SLICES = 32   # ops.hub_slices() of the built extension (asserted on GPU)
# (R-MAT scale, hub cut) of the fused-step test
RMAT_STEP_CASES = [(12, 2049), (14, 2049), (14, 3600)]


# ------------------------------ computed gids ------------------------------

def computed_gid_inputs(wdtype, base, seed=SEED):
    """The ladder with ghosts (no parallel edges, unit weights) in the `tied`
    state, reshaped so that `comm_gid[i] == base + i` for i < nv:

    - every ghost is alone in its own remote community (dense ids nv ..
      nv + N_GHOST - 1), and every remote row is (size 2, degree 8.0) like
      the pool rows, so a ghost neighbour ties exactly with every pool
      neighbour and only the global id decides;
    - for base > 0 half of the remote gids lie below `base` (but above every
      dense id, and above 2^32 when the base is) and half above base + nv;
      the remote community at dense id nv holds the global minimum. At
      base 0 nothing fits below the base: all remote gids lie above nv;
    - every second ladder row (odd index, degree >= 2) gets ghost vertex nv
      as a neighbour in place of its last one, so in every degree class
      some rows hinge on `comm_gid[nv]` itself and the others on the
      remaining remote ids.

    Returns (MoveInputs with local_gid_base=base, L)."""
    inp, L = ladder_inputs(wdtype, "tied", True, False, seed, unit=True)
    nv = inp.nv
    g = torch.Generator().manual_seed(seed + 1)
    tails = inp.tails.clone()
    for v in range(1, L, 2):
        e0, e1 = int(inp.rowptr[v]), int(inp.rowptr[v + 1])
        if e1 - e0 >= 2 and not bool((tails[e0:e1] == nv).any()):
            tails[e1 - 1] = nv
    curr = inp.curr_comm.clone()
    curr[nv:] = nv + torch.arange(N_GHOST, dtype=curr.dtype)
    size = torch.cat([inp.comm_size[:nv],
                      torch.full((N_GHOST,), 2, dtype=torch.int64)])
    cdeg = torch.cat([inp.comm_degree[:nv],
                      torch.full((N_GHOST,), 8.0, dtype=inp.comm_degree.dtype)])
    n_lo = N_GHOST // 2 if base > 0 else 0
    lo0 = (1 << 32) if base > (1 << 33) else nv + 8
    if n_lo:
        low = lo0 + torch.randperm(min(base - lo0, 1 << 20),
                                   generator=g)[:n_lo]
    else:
        low = torch.empty(0, dtype=torch.int64)
    high = base + nv + 1 + torch.randperm(1 << 20, generator=g)[:N_GHOST - n_lo]
    remote = torch.cat([low, high])
    remote = remote[torch.randperm(N_GHOST, generator=g)]
    # dense id nv: the smallest remote id (the global minimum for base > 0)
    j = int(torch.argmin(remote))
    remote[[0, j]] = remote[[j, 0]]
    gid = torch.cat([base + torch.arange(nv), remote])
    out = dataclasses.replace(inp, tails=tails, curr_comm=curr, comm_size=size,
                              comm_degree=cdeg, comm_gid=gid,
                              local_gid_base=base)
    return out, L


def wrong_gid_readings(inp: MoveInputs, base: int) -> dict:
    """comm_gid tables a faulty kernel would effectively use."""
    nv, nc = inp.nv, inp.comm_gid.numel()
    remote = inp.comm_gid[nv:]
    as_local = inp.comm_gid.clone()
    as_local[nv] = base + nv
    return {
        "dense_order": torch.arange(nc),
        "base_dropped": torch.cat([torch.arange(nv), remote]),
        "truncated": torch.cat([(base + torch.arange(nv)) & 0xFFFFFFFF,
                                remote]),
        "nv_as_local": as_local,
    }


def routes(deg: torch.Tensor, cut: int) -> dict:
    """Boolean masks over the vertices for the seven LDS classes and the
    hub path at hub cut `cut`."""
    out, lo = {}, 0
    for c, hi in enumerate(CLASS_BOUNDS + (cut,)):
        out[f"class{c}"] = (deg > lo) & (deg <= hi)
        lo = hi
    out["hub"] = deg > cut
    return out


# ---------------------------- fused aggregates -----------------------------

N_ISO = 7


def with_isolated(inp: MoveInputs, L: int, t_ref: torch.Tensor):
    """Append N_ISO vertices without edges to plain (ghost-free) ladder
    inputs: three in singleton communities of their own, three sharing the
    label of a pool vertex, and one sharing the label of a ladder vertex
    that moves (`t_ref`: the oracle's targets for `inp`). The community rows
    grow by N_ISO (fresh unique global ids) and the sizes count the new
    members. Returns (MoveInputs, mover) with `mover` the ladder vertex."""
    nv = inp.nv
    assert inp.curr_comm.numel() == nv and inp.comm_size.numel() == nv
    cc = inp.curr_comm.to(torch.int64)
    moved = (t_ref[:L].to(torch.int64) != cc[:L]).nonzero(as_tuple=True)[0]
    mover = int(moved[-1])
    labels = torch.tensor([nv, nv + 1, nv + 2,
                           int(cc[L + 5]), int(cc[L + 6]), int(cc[L + 700]),
                           int(cc[mover])])
    rowptr = torch.cat([inp.rowptr, inp.rowptr[-1:].expand(N_ISO)])
    curr = torch.cat([cc, labels]).to(inp.curr_comm.dtype)
    vdeg = torch.cat([inp.v_degree,
                      torch.zeros(N_ISO, dtype=inp.v_degree.dtype)])
    size = torch.cat([inp.comm_size, torch.zeros(N_ISO, dtype=torch.int64)])
    size += torch.bincount(labels, minlength=nv + N_ISO)
    cdeg = torch.cat([inp.comm_degree,
                      torch.zeros(N_ISO, dtype=inp.comm_degree.dtype)])
    gid = torch.cat([inp.comm_gid,
                     (3 << 32) + 3 * (nv + torch.arange(N_ISO)) + 1])
    assert gid.unique().numel() == gid.numel()
    out = dataclasses.replace(inp, rowptr=rowptr, curr_comm=curr,
                              v_degree=vdeg, comm_size=size, comm_degree=cdeg,
                              comm_gid=gid)
    return out, mover


def aggregates_of(inp: MoveInputs, target: torch.Tensor):
    """(size, degree) of the communities after every vertex took `target`:
    bincount / index_add_ over ALL vertices, integer-valued."""
    nc = inp.comm_size.numel()
    t = target.to(torch.int64)
    size = torch.bincount(t, minlength=nc)
    degree = torch.zeros(nc, dtype=torch.float64).index_add_(
        0, t, inp.v_degree.to(torch.float64))
    return size, degree


def isolated_sizes(inp: MoveInputs):
    """Per-community count of the vertices without edges (what the fused
    step pre-loads: the kernels never visit those vertices)."""
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    iso = (deg == 0).nonzero(as_tuple=True)[0]
    return torch.bincount(inp.curr_comm.to(torch.int64)[iso],
                          minlength=inp.comm_size.numel())


# ------------------------------- hub slices --------------------------------

HUB_KINDS = ("own", "absent", "single", "span", "tie")
N_TIE = 20          # edges in each of the two tied runs


@dataclasses.dataclass
class HubCase:
    """Hand-built hub segments for the hub_moves binding and the MoveInputs
    they describe: hub h is vertex h and its CSR row is its segment."""
    inp: MoveInputs
    nhub: int
    specs: list          # (kind, segment length) per hub
    tie_local: int       # dense id of the tie hub's local tied community
    tie_remote: int      # ... and of its remote one


def hub_lengths(slices: int):
    return [1, 2, 63, 64, 65, slices - 1, slices, slices + 1, 64 * slices + 1]


def span_run(n: int, slices: int):
    """(offset, length) of the long foreign run in a `span` segment: it
    starts a third into the segment and covers parts of at least three
    slices (a slice holds at most ceil(n / slices) elements)."""
    per = -(-n // slices)
    return n // 3, max(5, 2 * per + 2)


def hub_case(wdtype, slices: int, computed: bool, seed=SEED) -> HubCase:
    """One hub per (content, segment length). Vertices: the hubs, then one
    private block of leaf vertices per hub (its neighbours, all distinct,
    so a segment is a duplicate-free row), then N_TIE ghost vertices. Leaves
    and ghosts have no rows. A leaf is a singleton community (its own dense
    id) unless the content relabels it, so inside a segment the sorted
    position of a neighbour is its position in the block; ghosts carry the
    remote community nv + 1, which sorts behind every local one. Weights
    are integers 1..4 (1 in the tie segment) and every segment is stored in
    shuffled order.

    Contents (lengths: hub_lengths):
      own     every neighbour carries the hub's community: one run over the
              whole segment; the hub stays, cw is the total weight;
      absent  no neighbour carries it (cw 0); for n >= 8 the first n // 4
              neighbours share one community;
      single  every neighbour is a singleton of its own;
      span    (n >= 5) a foreign run over at least three slices (span_run)
              that wins by weight;
      tie     (longest length only) N_TIE neighbours at sorted positions
              60..79, a run cut by the slice boundary at 64, tie exactly
              with the N_TIE ghosts, a run inside the last slice. The
              remote community has the smaller global id and the larger
              dense id, so the two orders pick different winners.
    Sizes are the true member counts (the singleton guard is live), every
    candidate community has degree 8 and a hub's own community its hub's
    degree (plus 8 where leaves share it).

    `computed`: comm_gid[i] = base + i for the local communities and
    local_gid_base is set; otherwise comm_gid is an arbitrary non-monotone
    table above 2^32 and local_gid_base is None."""
    g = torch.Generator().manual_seed(seed)
    big = 64 * slices + 1
    specs = []
    for n in hub_lengths(slices):
        specs += [("own", n), ("absent", n), ("single", n)]
        if n >= 5:
            specs.append(("span", n))
    specs.append(("tie", big))
    nhub = len(specs)
    n_leaf = sum(n for _, n in specs) - N_TIE
    nv = nhub + n_leaf
    tie_remote = nv + 1
    labels = torch.arange(nv + N_TIE)
    labels[nv:] = tie_remote
    rows_t, rows_w = [], []
    a = nhub
    tie_local = -1
    for h, (kind, n) in enumerate(specs):
        w = torch.randint(1, 5, (n,), generator=g).to(torch.float64)
        t = a + torch.arange(n)
        if kind == "own":
            labels[a:a + n] = h
        elif kind == "absent" and n >= 8:
            labels[a:a + n // 4] = a
        elif kind == "span":
            off, k = span_run(n, slices)
            labels[a + off:a + off + k] = a + off
        elif kind == "tie":
            t = torch.cat([t[:n - N_TIE], nv + torch.arange(N_TIE)])
            w = torch.ones(n, dtype=torch.float64)
            tie_local = a + 60
            labels[a + 60:a + 60 + N_TIE] = tie_local
            n -= N_TIE                      # leaves used
        perm = torch.randperm(t.numel(), generator=g)
        rows_t.append(t[perm])
        rows_w.append(w[perm])
        a += n
    assert a == nv
    lens = torch.tensor([t.numel() for t in rows_t] + [0] * n_leaf)
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(lens, dim=0)
    tails, weights = torch.cat(rows_t), torch.cat(rows_w)
    vdeg = torch.zeros(nv, dtype=torch.float64).index_add_(
        0, torch.repeat_interleave(torch.arange(nv), lens), weights)
    nc = nv + 2
    size = torch.bincount(labels, minlength=nc)
    cdeg = torch.full((nc,), 8.0, dtype=torch.float64)
    cdeg[:nhub] = vdeg[:nhub] + 8.0 * (size[:nhub] > 1)
    if computed:
        base = (3 << 32) + 7
        gid = torch.cat([base + torch.arange(nv),
                         torch.tensor([1 << 33, 5])])
    else:
        base = None
        gid = torch.randperm(nc, generator=g) * 3 + (3 << 32)
        if int(gid[tie_remote]) > int(gid[tie_local]):
            gid[[tie_remote, tie_local]] = gid[[tie_local, tie_remote]]
    total = float(vdeg.sum())
    k = 0
    while (1 << (k + 1)) <= total:
        k += 1
    inp = MoveInputs(rowptr, tails.to(torch.int32), weights.to(wdtype),
                     labels.to(torch.int32), vdeg.to(wdtype), size,
                     cdeg.to(wdtype), gid, 1.0 / float(1 << k),
                     local_gid_base=base)
    return HubCase(inp, nhub, specs, tie_local, tie_remote)
