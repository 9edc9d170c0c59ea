"""CPU-only input builders for the class-schedule tests (block classes
beside the sub classes on an auxiliary stream, the edge loop at every trip
count). Plain torch on the CPU, no GPU and no `cuvite_amd.ops`
import; `tests/test_schedule_cases.py` shows on the oracle alone that these
inputs have the properties `tests/test_gpu_class_schedule.py` relies on.

All data is integer-valued as in kernel_cases.py (weights 1..4, a
power-of-two `constant`, integer aggregates), so every oracle answer is
exact in fp32 and fp64 and in any atomic order: a correct kernel matches it
bit for bit.

Two graphs:

- the *pipeline ladder*: one vertex at every degree where the number of
  edges of a lane in `insert_edges_pipelined` changes (and with it the
  split between the 4-deep pipelined loop and the remainder loop), i.e.
  k*STRIDE - 1, k*STRIDE and k*STRIDE + 1 for k = 1..5 and every STRIDE a
  class runs at (16 lanes, 64 lanes, blocks of 256 threads; wider blocks
  were measured and not kept), restricted to the degrees of the classes
  that use the stride, plus both sides of every class bound and of the
  default hub cut;
- the *crowded* graph: enough vertices in each block class that blocks of
  classes 4, 5 and 6 and of the sub classes are resident on the same CUs at
  once when the classes run on two streams, about 4 M edges.
"""

from __future__ import annotations

import torch

from cuvite_amd.local_move import MoveInputs

N_POOL = 8192
SEED = 41
STATES = ("singleton", "random", "tied")
CLASS_BOUNDS = (16, 64, 256, 512, 1024, 2048)
CUT = 6144                      # default hub cut
BLOCK_WIDTHS = (256,)           # block sizes of classes 4-6


def ladder_degrees():
    """Sorted, duplicate-free degrees of the pipeline ladder."""
    degs = {1}
    for stride, lo, hi in ((16, 1, 16), (64, 17, 512)) + tuple(
            (b, 513, CUT) for b in BLOCK_WIDTHS):
        for k in range(1, 6):
            for d in (k * stride - 1, k * stride, k * stride + 1):
                if lo <= d <= hi:
                    degs.add(d)
    for b in CLASS_BOUNDS + (CUT,):
        degs.update((b, b + 1))
    return tuple(sorted(degs))


LADDER = ladder_degrees()


def _constant(total: float) -> float:
    k = 0
    while (1 << (k + 1)) <= total:
        k += 1
    return 1.0 / float(1 << k)


def _finish(nv, s, t, w, pool, state, wdtype, g):
    """CSR, labels and aggregates for the edge list (s, t, w); `pool` are
    the vertex ids whose community rows the `tied` state equalises."""
    order = torch.argsort(s, stable=True)
    s, t, w = s[order], t[order], w[order]
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(s, minlength=nv), dim=0)
    vdeg = torch.zeros(nv, dtype=torch.float64).index_add_(0, s, w)
    if state == "random":
        curr = torch.randint(0, nv, (nv,), generator=g)
    else:
        curr = torch.arange(nv)
    size = torch.bincount(curr, minlength=nv)
    cdeg = torch.zeros(nv, dtype=torch.float64).index_add_(0, curr, vdeg)
    if state == "tied":
        # as in kernel_cases.ladder_inputs: identical rows for all pool
        # communities, size 2 switches the singleton guard off
        size[pool] = 2
        cdeg[pool] = 8.0
    gid = torch.randperm(nv, generator=g) * 3 + (3 << 32)
    return MoveInputs(rowptr, t.to(torch.int32), w.to(wdtype),
                      curr.to(torch.int32), vdeg.to(wdtype), size,
                      cdeg.to(wdtype), gid, _constant(float(vdeg.sum())))


def pipeline_ladder(wdtype, state, dup, seed=SEED):
    """Returns (MoveInputs on CPU, L). Vertices 0..L-1 have exactly the
    LADDER degrees with distinct neighbours drawn from the pool, vertices
    L..L+N_POOL-1; every pool vertex has the reverse edges and one ring
    edge, which leaves it in the low classes. `dup`: every ladder row of
    degree >= 8 gets deg // 8 parallel edges and one self-loop."""
    assert state in STATES
    g = torch.Generator().manual_seed(seed)
    L = len(LADDER)
    nv = L + N_POOL
    src, dst = [], []
    for v, d in enumerate(LADDER):
        nb = torch.randperm(N_POOL, generator=g)[:d] + L
        if dup and d >= 8:
            nb[:d // 8] = nb[0]
            nb[-1] = v
        src.append(torch.full((d,), v, dtype=torch.int64))
        dst.append(nb)
    lad_src, lad_dst = torch.cat(src), torch.cat(dst)
    pair = torch.unique(lad_src * nv + lad_dst)
    r_src, r_dst = pair % nv, pair // nv
    keep = r_src >= L
    pool = torch.arange(L, nv)
    ring = L + (pool - L + 1) % N_POOL
    s = torch.cat([lad_src, r_src[keep], pool])
    t = torch.cat([lad_dst, r_dst[keep], ring])
    w = torch.randint(1, 5, (s.numel(),), generator=g).to(torch.float64)
    return _finish(nv, s, t, w, pool, state, wdtype, g), L


# (number of vertices, lowest degree, highest degree) per group, in vertex
# order; the pool is the first N_POOL vertices of the last LDS group
CROWDED_GROUPS = ((600, 2100, 2300),     # class 6
                  (800, 1100, 1200),     # class 5
                  (1600, 550, 650),      # class 4
                  (4096, 65, 200),       # class 2
                  (32768, 1, 16))        # class 0
CROWDED_HUBS = (6200, 6500, 7000)


def crowded(wdtype, state, seed=SEED):
    """Returns (MoveInputs on CPU, L): the CROWDED_GROUPS in order, then
    the hubs. L is the first vertex of the degree 1..16 group, whose first
    N_POOL vertices are the neighbour pool of every row (neighbours are
    drawn with replacement, so parallel edges occur; the edges are
    directed, which the kernels and the oracle take as given). Every 97th
    edge is turned into a self-loop."""
    assert state in STATES
    g = torch.Generator().manual_seed(seed)
    degs = [torch.randint(lo, hi + 1, (n,), generator=g)
            for n, lo, hi in CROWDED_GROUPS]
    L = sum(n for n, _, _ in CROWDED_GROUPS[:-1])
    degs.append(torch.tensor(CROWDED_HUBS))
    deg = torch.cat(degs)
    nv = deg.numel()
    s = torch.repeat_interleave(torch.arange(nv), deg)
    t = L + torch.randint(0, N_POOL, (s.numel(),), generator=g)
    loop = torch.arange(0, s.numel(), 97)
    t[loop] = s[loop]
    w = torch.randint(1, 5, (s.numel(),), generator=g).to(torch.float64)
    pool = torch.arange(L, L + N_POOL)
    return _finish(nv, s, t, w, pool, state, wdtype, g), L


def class_counts(inp: MoveInputs, cut: int = CUT):
    """Vertices per LDS class 0..6 and on the hub path."""
    deg = inp.rowptr[1:] - inp.rowptr[:-1]
    out, lo = [], 0
    for hi in CLASS_BOUNDS + (cut,):
        out.append(int(((deg > lo) & (deg <= hi)).sum()))
        lo = hi
    out.append(int((deg > cut).sum()))
    return out
