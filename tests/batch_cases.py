"""CPU-only builders shared by the edge-batch tests (test_batch_apply.py,
test_gpu_batch_apply.py). Plain torch, no GPU and no `cuvite_amd.ops` import.

`span_graph(span)` is built around the span length of the edge-batch kernels:
the rows the named batches touch have degrees on both sides of 64 (one
ballot) and of the span, one row covers more than three spans, and a pair
stored four times sits on both sides of span boundaries. Every weight is a
small integer, so fp32 and fp64 hold it exactly."""

from __future__ import annotations

import functools

import torch

from cuvite_amd.dynamic import EdgeBatch, _directed
from cuvite_amd.graph import Graph

import dynamic_cases as dyc

FILLERS = 64   # rows that only hold the reverse edges of the shaped rows
NAMED = ("empty", "first", "last", "boundary", "parallel", "whole_row",
         "loop", "into_empty", "all_rows", "mixed")


def _layout(span: int):
    """Row ids: the shaped rows first, then the fillers, then a degree-0 and
    a degree-2 row, so that vertex nv - 1 is the last non-empty row."""
    degs = [0, 1, 63, 64, 65, span - 1, span, span + 1, 3 * span + 5]
    nv = len(degs) + FILLERS + 2
    return degs, nv


@functools.lru_cache(maxsize=None)
def span_graph(span: int) -> Graph:
    """One rank. Row degrees 0, 1, 63, 64, 65, span-1, span, span+1,
    3*span+5, then FILLERS rows, then 0, 2. Tails of the shaped rows are
    drawn (seed 11) from the fillers, whose rows hold the reverse edges: the
    graph is symmetric and the shaped rows keep their degrees. The long row
    (LONG = 8) holds the pair (LONG, P) four times, at row indices span-1,
    span, 2*span and the last one, and a self-loop at index 7."""
    gen = torch.Generator().manual_seed(11)
    degs, nv = _layout(span)
    LONG, P = 8, len(degs)             # P: the first filler
    f_lo, f_hi = P + 1, P + FILLERS    # P itself is never drawn
    rows = [[] for _ in range(nv)]
    shaped = list(enumerate(degs)) + [(nv - 2, 0), (nv - 1, 2)]
    for v, d in shaped:
        t = torch.randint(f_lo, f_hi, (d,), generator=gen).tolist()
        w = torch.randint(1, 5, (d,), generator=gen).tolist()
        if v == LONG:
            for k in (span - 1, span, 2 * span, d - 1):
                t[k] = P
            t[7] = LONG
        for a, b in zip(t, w):
            rows[v].append((a, float(b)))
            if a != v:
                rows[a].append((v, float(b)))
    rowptr = torch.zeros(nv + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor([len(r) for r in rows]), 0)
    tails = torch.tensor([a for r in rows for a, _ in r], dtype=torch.int64)
    weights = torch.tensor([b for r in rows for _, b in r],
                           dtype=torch.float64)
    g = Graph(rowptr, tails, weights)
    assert g.degrees()[:len(degs)].tolist() == degs
    assert g.degrees()[-2:].tolist() == [0, 2]
    return g


def _batch(ins=(), dels=()) -> EdgeBatch:
    i64 = torch.int64
    return EdgeBatch(torch.tensor([e[0] for e in ins], dtype=i64),
                     torch.tensor([e[1] for e in ins], dtype=i64),
                     torch.tensor([e[2] for e in ins], dtype=torch.float64),
                     torch.tensor([e[0] for e in dels], dtype=i64),
                     torch.tensor([e[1] for e in dels], dtype=i64))


def named_batches(span: int) -> dict:
    """The named batches on span_graph(span), plus `absent`."""
    g = span_graph(span)
    degs, nv = _layout(span)
    LONG, P = 8, len(degs)
    rp, t = g.rowptr.tolist(), g.tails.tolist()

    def entry(v, k):
        return (v, t[rp[v] + k])

    def row(v):
        return sorted({(v, x) for x in t[rp[v]:rp[v + 1]]})

    b = {
        "empty": ((), ()),
        "first": ((), (entry(2, 0),)),
        "last": ((), (entry(nv - 1, 1),)),
        "boundary": ((), (entry(LONG, span - 1), entry(LONG, span))),
        "parallel": ((), ((LONG, P), (P, LONG), (LONG, P))),
        "whole_row": ((), tuple(row(4) + row(nv - 1))),
        "loop": (((LONG, LONG, 9.0),), ((LONG, LONG),)),
        "into_empty": (((0, nv - 2, 3.0), (0, 5, 2.0), (nv - 1, nv - 2, 5.0),
                        (nv - 2, nv - 2, 7.0)), ()),
        "all_rows": (tuple((v, (v + 1) % nv, float(1 + v % 4))
                           for v in range(nv)), ()),
    }
    assert entry(LONG, span - 1) == entry(LONG, span) == (LONG, P)
    assert entry(LONG, 7) == (LONG, LONG)
    b["mixed"] = (sum((list(v[0]) for v in b.values()), []),
                  sum((list(v[1]) for v in b.values()), []))
    b["absent"] = (((3, 4, 1.0),), (entry(2, 0), (0, 1)))
    return {k: _batch(*v) for k, v in b.items()}


def routed(batch: EdgeBatch):
    """The routed lists of a one-rank batch: (d_src, d_dst, i_src, i_dst,
    i_w), what dynamic._route_batch returns at world 1."""
    d_src, d_dst = _directed(batch.del_src, batch.del_dst)
    i_src, i_dst, i_w = _directed(batch.ins_src, batch.ins_dst,
                                  batch.ins_w.to(torch.float64))
    return d_src, d_dst, i_src, i_dst, i_w


def loop_apply(g: Graph, base: int, d_src, d_dst, i_src, i_dst, i_w):
    """The stable-rows contract by a python loop over the rows: (rowptr,
    tails, weights) as lists, or None if a deletion matches nothing."""
    rp, t, w = g.rowptr.tolist(), g.tails.tolist(), g.weights.tolist()
    dele = set(zip((d_src - base).tolist(), d_dst.tolist()))
    stored = {(v, t[e]) for v in range(g.nv) for e in range(rp[v], rp[v + 1])}
    if not dele <= stored:
        return None
    ins = list(zip((i_src - base).tolist(), i_dst.tolist(), i_w.tolist()))
    n_rp, n_t, n_w = [0], [], []
    for v in range(g.nv):
        for e in range(rp[v], rp[v + 1]):
            if (v, t[e]) not in dele:
                n_t.append(t[e])
                n_w.append(w[e])
        for s, d, x in ins:
            if s == v:
                n_t.append(d)
                n_w.append(x)
        n_rp.append(len(n_t))
    return n_rp, n_t, n_w


def sorted_rows(g: Graph):
    """(rowptr, tails, weights) with every row sorted by (dst, weight): what
    two CSRs that differ in row order only agree on."""
    src = torch.repeat_interleave(torch.arange(g.nv, device=g.device),
                                  g.degrees())
    w = g.weights.to(torch.float64)
    o = torch.argsort(w, stable=True)
    o = o[torch.argsort(g.tails[o], stable=True)]
    o = o[torch.argsort(src[o], stable=True)]
    return g.rowptr.cpu(), g.tails[o].cpu(), w[o].cpu()


def same_graph(a: Graph, b: Graph) -> bool:
    """Bit for bit, row order included."""
    return (torch.equal(a.rowptr.cpu(), b.rowptr.cpu())
            and torch.equal(a.tails.cpu(), b.tails.cpu())
            and a.weights.dtype == b.weights.dtype
            and torch.equal(a.weights.cpu(), b.weights.cpu()))


def concat_batches(batches) -> EdgeBatch:
    return EdgeBatch(*[torch.cat([getattr(b, f) for b in batches])
                       for f in ("ins_src", "ins_dst", "ins_w", "del_src",
                                 "del_dst")])


def stream_batches():
    """Three successive batches on lfr: the thirds of one 3 % recipe batch,
    so that their deletions are distinct stored pairs of the old graph and
    the concatenation of the three is itself a valid batch."""
    whole = dyc.recipe_batch(dyc.base_graph("lfr"), 0.03)
    return [dyc.share_of(whole, k, 3) for k in range(3)]
