"""CPU-only input builders for the kernel edge-case tests.

Everything here is plain torch on the CPU: no GPU, no `cuvite_amd.ops`
import. `tests/test_kernel_cases.py` checks on the oracle alone that these
inputs have the properties the GPU tests rely on; `tests/
test_gpu_kernel_edges.py` feeds them to the HIP kernels.

The "ladder" graph pins one vertex at every degree where the local-move
routing changes: the class bounds (16, 64, 256, 512, 1024, 2048, cut), the
`cap_for_degree` switch points inside the classes (7/8, 31/32, 127/128) and
both sides of the hub cut for the default (6144) and the largest (8000)
setting. Ladder neighbours are distinct, so in the singleton state every
LDS table sees its worst-case load (deg distinct keys).

States: `singleton`, `few` (five communities: a hub has fewer candidates
than argmax splits), `random`, and `tied` (singleton labels with identical
aggregate rows for all pool communities). In the first three a wrong
tie-break is visible on a handful of vertices at most, because exact ties
at the maximum are rare (what the global ids mostly decide there is the
singleton guard); `tied` makes every ladder vertex's answer hinge on the
tie-break.

Exactness. Weights are small integers, so every weight sum is exact in fp32
and fp64 and in any (atomic) order. `constant` is a power of two, so the
gain 2*(eiy - eix) - 2*vdeg*(ay - ax)*constant is an exact fp64 value as
well (integers below 2^40 scaled by 2^-k): it does not depend on evaluation
order or on fused multiply-adds. A correct kernel therefore matches the
oracle bit for bit, tie-breaks included.
"""

from __future__ import annotations

import dataclasses

import torch

from cuvite_amd.local_move import MoveInputs

LADDER = (1, 2, 7, 8, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, 255, 256, 257,
          511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097,
          6143, 6144, 6145, 7999, 8000, 8001)
N_POOL = 8192
N_GHOST = 512
N_REMOTE = 64
STATES = ("singleton", "few", "random", "tied")


def ladder_inputs(wdtype, state, ghosts, dup, seed, unit=False):
    """Returns (MoveInputs on CPU, L). Vertices 0..L-1 have exactly the
    LADDER degrees; vertices L..L+N_POOL-1 are the neighbour pool; with
    `ghosts`, dense vertex ids nv..nv+N_GHOST-1 are ghosts whose communities
    are N_REMOTE remote ones at dense ids >= nv."""
    assert state in STATES
    g = torch.Generator().manual_seed(seed)
    L = len(LADDER)
    nv = L + N_POOL
    n_cand = N_POOL + (N_GHOST if ghosts else 0)

    src, dst = [], []
    for v, d in enumerate(LADDER):
        # distinct neighbours; candidate c < N_POOL is pool vertex L + c,
        # c >= N_POOL is ghost nv + (c - N_POOL): dense id L + c either way
        nb = torch.randperm(n_cand, generator=g)[:d] + L
        if dup and d >= 8:
            nb[:d // 8] = nb[0]      # parallel edges
            nb[-1] = v               # self-loop
        src.append(torch.full((d,), v, dtype=torch.int64))
        dst.append(nb)
    lad_src, lad_dst = torch.cat(src), torch.cat(dst)
    # reverse edges: one per distinct (ladder, pool) pair, plus a ring edge
    pair = torch.unique(lad_src * (nv + N_GHOST) + lad_dst)
    r_src, r_dst = pair % (nv + N_GHOST), pair // (nv + N_GHOST)
    keep = (r_src >= L) & (r_src < nv)
    r_src, r_dst = r_src[keep], r_dst[keep]
    pool = torch.arange(L, nv)
    ring = L + (pool - L + 1) % N_POOL
    s = torch.cat([lad_src, r_src, pool])
    t = torch.cat([lad_dst, r_dst, ring])
    if unit:
        w = torch.ones(s.numel(), dtype=torch.float64)
    else:
        w = torch.randint(1, 5, (s.numel(),), generator=g).to(torch.float64)
    # CSR; the stable sort keeps each ladder row in construction order
    order = torch.argsort(s, stable=True)
    s, t, w = s[order], t[order], w[order]
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(s, minlength=nv), dim=0)
    vdeg = torch.zeros(nv, dtype=torch.float64).index_add_(0, s, w)

    if state in ("singleton", "tied"):
        curr = torch.arange(nv)
    elif state == "few":
        curr = torch.randint(0, 5, (nv,), generator=g)
    else:
        curr = torch.randint(0, nv, (nv,), generator=g)
    size = torch.bincount(curr, minlength=nv)
    cdeg = torch.zeros(nv, dtype=torch.float64).index_add_(0, curr, vdeg)
    if state == "tied":
        # the kernels take the aggregates as given (in a distributed run
        # they arrive from other ranks): give every pool community the same
        # row. Equal degrees make all maximum-weight neighbours of a ladder
        # vertex tie exactly, and size 2 switches the singleton guard off,
        # so the global-id tie-break alone picks the target.
        size[L:] = 2
        cdeg[L:] = 8.0
    if ghosts:
        curr = torch.cat(
            [curr, nv + torch.randint(0, N_REMOTE, (N_GHOST,), generator=g)])
        # remote rows: sizes 1..3 (size 1 trips the singleton guard)
        size = torch.cat(
            [size, torch.randint(1, 4, (N_REMOTE,), generator=g)])
        cdeg = torch.cat(
            [cdeg,
             torch.randint(1, 4096, (N_REMOTE,), generator=g).to(cdeg.dtype)])
    nc = size.numel()
    # non-monotone in the dense id, every value above 2^32
    gid = torch.randperm(nc, generator=g) * 3 + (3 << 32)
    total = float(vdeg.sum())
    k = 0
    while (1 << (k + 1)) <= total:
        k += 1
    inp = MoveInputs(rowptr, t.to(torch.int32), w.to(wdtype),
                     curr.to(torch.int32), vdeg.to(wdtype), size,
                     cdeg.to(wdtype), gid, 1.0 / float(1 << k))
    return inp, L


def with_arange_gid(inp: MoveInputs) -> MoveInputs:
    """Same inputs with the identity dense->global map the older tests use."""
    return dataclasses.replace(
        inp, comm_gid=torch.arange(inp.comm_gid.numel(), dtype=torch.int64))


def move_inputs_to(inp: MoveInputs, dev) -> MoveInputs:
    vals = [getattr(inp, f.name) for f in dataclasses.fields(inp)]
    return MoveInputs(*[x.to(dev) if torch.is_tensor(x) else x for x in vals])
