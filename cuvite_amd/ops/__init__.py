"""HIP kernel ops for gfx950 (MI355X).

The extension `_hip_ops` is built in-tree by setup.py / __graft_entry__.build()
with hipcc --offload-arch=gfx950. On a GPU box the HIP path is mandatory: if a
CUDA/HIP tensor reaches these wrappers without the extension present, we raise
instead of silently falling back to eager PyTorch.
"""

from __future__ import annotations

import os

import torch

_ext = None
_import_error: Exception | None = None
try:
    from . import _hip_ops as _ext  # type: ignore
except Exception as e:  # pragma: no cover - exercised only on broken builds
    _import_error = e


def available() -> bool:
    return _ext is not None


def _require():
    if _ext is None:
        raise RuntimeError(
            "cuvite_amd HIP extension (_hip_ops) is not built; run "
            "`python setup.py build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). "
            f"Original import error: {_import_error!r}")
    return _ext


# Degree-class boundaries (see louvain_kernels.hip header comment): sized
# so the bulk classes' LDS tables stay at 24 KB/block (6 blocks/CU).
_CLASS_BOUNDS = (16, 64, 256, 512, 1024, 2048)
_bucket_cache: dict = {}


def _hub_cut() -> int:
    """Degree above which vertices leave the LDS classes for the rocPRIM
    hub pipeline. The 8192-slot table stays collision-safe up to 8000
    distinct neighbors (load <= 0.98 worst case, ~0.8 typical); R-MAT's
    lumpy degree spectrum clusters many "hubs" just above 4096, so raising
    the cut keeps them on the (cheaper) LDS path. A/B at s26 (gpurun r2c):
    cut 4096 = 150.1 ms/step, 6144 = 136.0, 8000 = 136.7 (identical
    trajectories; hub count 84k -> 18k, hub sort 74 -> 43 ms). Default 6144;
    CUVITE_HUB_CUT overrides (the reference's CUT_SIZE was 4096,
    louvain_cuda_constants.cuh:34)."""
    try:
        cut = int(os.environ.get("CUVITE_HUB_CUT", "6144"))
    except ValueError:
        cut = 6144
    return max(2049, min(cut, 8000))


def _buckets_for(rowptr: torch.Tensor):
    """Degree-class vertex lists for a CSR (static per phase; cached by the
    rowptr storage). Returns (vlists[7] for the LDS class kernels,
    hubs64 int64 hub vertex list, hdeg int64 hub degrees)."""
    cut = _hub_cut()
    key = (rowptr.data_ptr(), rowptr.numel(), cut)
    hit = _bucket_cache.get(key)
    if hit is not None and hit[0] is rowptr:  # identity check: ptr reuse safe
        return hit[1], hit[2], hit[3]
    deg = rowptr[1:] - rowptr[:-1]
    lo = 0
    vlists = []
    for b in _CLASS_BOUNDS + (cut,):
        vlists.append(((deg > lo) & (deg <= b)).nonzero(
            as_tuple=True)[0].to(torch.int32))
        lo = b
    hubs64 = (deg > cut).nonzero(as_tuple=True)[0]
    hdeg = deg[hubs64]
    if len(_bucket_cache) > 8:
        _bucket_cache.clear()
    _bucket_cache[key] = (rowptr, vlists, hubs64, hdeg)
    return vlists, hubs64, hdeg


_class_id_cache: dict = {}
FRONTIER_HUB_CLASS = 7        # class ids of frontier_lists beyond the seven
FRONTIER_EDGELESS_CLASS = 8   # LDS classes


def _class_ids_for(rowptr: torch.Tensor) -> torch.Tensor:
    """uint8 [nv] degree class of every vertex (static per phase; cached like
    _bucket_cache): 0-6 the LDS classes of _CLASS_BOUNDS and the hub cut, 7
    hubs, 8 vertices without edges."""
    cut = _hub_cut()
    key = (rowptr.data_ptr(), rowptr.numel(), cut)
    hit = _class_id_cache.get(key)
    if hit is not None and hit[0] is rowptr:
        return hit[1]
    deg = rowptr[1:] - rowptr[:-1]
    bounds = torch.tensor(_CLASS_BOUNDS + (cut,), dtype=torch.int64,
                          device=rowptr.device)
    # bucketize: class c holds bounds[c - 1] < deg <= bounds[c]
    cls = torch.bucketize(deg, bounds).to(torch.uint8)
    cls[deg == 0] = FRONTIER_EDGELESS_CLASS
    if len(_class_id_cache) > 8:
        _class_id_cache.clear()
    _class_id_cache[key] = (rowptr, cls)
    return cls


_side_streams: dict = {}


def clear_phase_caches():
    """Drop the phase-keyed caches (degree buckets, deduped hub adjacency,
    hub chunk groups). Called by the phase loop before coarsening: at s27
    the cached hub arrays are tens of GB and the next level re-keys anyway."""
    _bucket_cache.clear()
    _class_id_cache.clear()
    _hub_static_cache.clear()
    _hub_groups_cache.clear()


def _side_stream(dev):
    st = _side_streams.get(dev)
    if st is None:
        st = torch.cuda.Stream(device=dev)
        _side_streams[dev] = st
    return st


_HUB_SORT_CHUNK = 1 << 30  # max edges per sort batch (torch op INT_MAX cap)
_hub_groups_cache: dict = {}


def _hub_segsort_enabled() -> bool:
    """rocPRIM segsort hub path — the DEFAULT since the round-2 A/B at
    R-MAT s26 (gpurun_out/ab/, profiles/): 189.7 ms/step vs 549.8 ms for
    the torch global-sort path (identical modularity trajectory), i.e. the
    hub stage drops 0.44 s -> 0.083 s. Narrow-bit segmented radix sort +
    one sliced pass over the sorted pairs (run sums, gains, argmax), fully
    device-side (no host sync per iteration). CUVITE_HUB_SEGSORT=0 restores
    the torch-sort fallback."""
    return os.environ.get("CUVITE_HUB_SEGSORT", "1") not in ("0", "off")


def _hub_groups(inp, hubs, hdeg):
    """Phase-static chunking of the hub list into groups whose edge totals
    stay under the sort cap. The group tensors are cached per phase (keyed by
    the rowptr storage) so _hub_static's identity-keyed cache hits every
    iteration — fresh hubs[m] subsets each call would rebuild the multi-GB
    flattened hub adjacency per iteration."""
    key = (inp.rowptr.data_ptr(), hubs.data_ptr(), hubs.numel())
    hit = _hub_groups_cache.get(key)
    if hit is not None and hit[0] is inp.rowptr and hit[1] is hubs:
        return hit[2]
    total = int(hdeg.sum())
    if total <= _HUB_SORT_CHUNK or hubs.numel() <= 1:
        groups = [(hubs, hdeg, None)]
    else:
        cum = torch.cumsum(hdeg, dim=0)
        gidx = torch.div(cum - 1, _HUB_SORT_CHUNK, rounding_mode="floor")
        groups = []
        for g in range(int(gidx[-1]) + 1):
            m = gidx == g
            if bool(m.any()):
                groups.append((hubs[m].contiguous(), hdeg[m].contiguous(), m))
    if len(_hub_groups_cache) > 4:
        _hub_groups_cache.clear()
    _hub_groups_cache[key] = (inp.rowptr, hubs, groups)
    return groups


def _gid_args(inp) -> dict:
    """Keyword arguments that tell the kernels which global community ids
    they may compute instead of gathering (MoveInputs.local_gid_base)."""
    base = getattr(inp, "local_gid_base", None)
    if base is None:
        return dict(gid_base=0, n_local=0)
    return dict(gid_base=int(base), n_local=int(inp.nv))


def _hub_moves_sorted(inp, hubs, hdeg, nxt=None, bounds=None):
    """Chunk wrapper: split the hub list into phase-static groups whose edge
    totals stay under the torch sort cap; each hub's candidates are
    independent. Returns (target_dense int32 [nhub], wcc [nhub]) aligned
    with `hubs`. `nxt`: optional (next_size, next_degree) pair; every group's
    hub_moves call accounts its own hubs in it. `bounds`: optional
    (mover_bound, cand_bound) pair of a refine round (see refine_move)."""
    groups = _hub_groups(inp, hubs, hdeg)
    if len(groups) == 1:
        return _hub_moves_sorted_one(inp, groups[0][0], groups[0][1], nxt,
                                     bounds)
    tgt = torch.empty(hubs.numel(), dtype=torch.int32, device=hubs.device)
    wcc = torch.empty(hubs.numel(), dtype=inp.weights.dtype,
                      device=hubs.device)
    for hubs_g, hdeg_g, m in groups:
        t, w = _hub_moves_sorted_one(inp, hubs_g, hdeg_g, nxt, bounds)
        tgt[m] = t
        wcc[m] = w
    return tgt, wcc


_hub_static_cache: dict = {}


def _hub_static(inp, hubs, hdeg):
    """Phase-static hub data: flattened hub adjacency (tails, weights),
    per-hub segment ids and self-loop weights. None of it depends on the
    community labels, so it is gathered once per phase and reused every
    iteration (cache keyed like _bucket_cache)."""
    dev = inp.rowptr.device
    key = (inp.rowptr.data_ptr(), hubs.data_ptr(), hubs.numel())
    hit = _hub_static_cache.get(key)
    if hit is not None and hit[0] is inp.rowptr and hit[1] is hubs:
        return hit[2]
    nhub = hubs.numel()
    offs = torch.zeros(nhub + 1, dtype=torch.int64, device=dev)
    offs[1:] = torch.cumsum(hdeg, dim=0)
    tot = int(offs[-1])
    seg = torch.repeat_interleave(torch.arange(nhub, device=dev), hdeg)
    pos = torch.arange(tot, device=dev) - offs[seg]
    eidx = inp.rowptr[hubs][seg] + pos
    del pos
    tails_h = inp.tails[eidx].to(torch.int64)
    wts = inp.weights[eidx].to(torch.float64)
    del eidx
    # merge PARALLEL edges once per phase: duplicates of (hub, neighbor)
    # land in the same community every iteration, so summing their weights
    # here shrinks every per-iteration sort for identical results (R-MAT
    # hub adjacencies are duplicate-heavy). One-time cost = one sort.
    stride = inp.curr_comm.numel()  # > max dense tail id
    dkey = seg * stride + tails_h
    del seg, tails_h
    dkey_s, order = torch.sort(dkey)
    del dkey
    w_s = wts[order]
    del wts, order
    uniq, counts = torch.unique_consecutive(dkey_s, return_counts=True)
    del dkey_s
    ends = torch.cumsum(counts, dim=0) - 1
    del counts
    cs = torch.cumsum(w_s, dim=0)
    del w_s
    wts = cs[ends].clone()
    wts[1:] -= cs[ends[:-1]]
    del cs, ends
    seg = uniq // stride
    tails_h = uniq % stride
    del uniq
    selfmask = tails_h == hubs[seg]
    selfloop = torch.zeros(nhub, dtype=torch.float64, device=dev)
    if bool(selfmask.any()):
        selfloop.index_add_(0, seg[selfmask], wts[selfmask])
    del selfmask
    if _hub_segsort_enabled() and dev.type == "cuda":
        # int32 copies + deduped per-hub offsets for the rocPRIM path;
        # the int64 originals are not needed again on this path — drop them
        # (at s27 they are ~24 B per deduped hub edge, tens of GB)
        offs_d = torch.zeros(nhub + 1, dtype=torch.int64, device=dev)
        offs_d[1:] = torch.cumsum(
            torch.bincount(seg, minlength=nhub), dim=0)
        extra = (tails_h.to(torch.int32), offs_d,
                 wts.to(inp.weights.dtype), hubs.to(torch.int32))
        seg = tails_h = wts = None
    else:
        extra = None
    data = (seg, tails_h, wts, selfloop, extra)
    if len(_hub_static_cache) > 4:
        # evict only OTHER phases' entries: all chunk groups of the current
        # phase must stay resident together (one entry per group)
        stale = [k for k, v in _hub_static_cache.items()
                 if v[0] is not inp.rowptr]
        for k in stale:
            del _hub_static_cache[k]
    _hub_static_cache[key] = (inp.rowptr, hubs, data)
    return data


def _hub_moves_sorted_one(inp, hubs, hdeg, nxt=None, bounds=None):
    """Hub vertices (deg > hub cut, default 6144) via radix sort +
    segmented reduction.
    Default path: the fully-device rocPRIM pipeline (hub_moves binding).
    Fallback (CUVITE_HUB_SEGSORT=0): torch.sort of packed (hub, community)
    keys + cumsum segment sums + vectorized exact-tie-break argmax.
    Deterministic, atomic-free. A round-1 global-memory hash-table pipeline
    was deleted after showing pathological CAS slowdowns on tables past the
    4 MB XCD-L2 footprint (profiles/hub_pathology_and_s26.md) and losing
    the A/B to this pipeline (profiles/round2_hub_segsort_ab.md)."""
    dev = inp.rowptr.device
    nhub = hubs.numel()
    seg, tails_h, wts, selfloop, extra = _hub_static(inp, hubs, hdeg)
    C = inp.comm_degree.numel()
    if extra is not None:
        # rocPRIM path, fully device-side: segmented narrow-bit radix sort,
        # then one sliced pass over the sorted pairs for run sums, gains
        # and argmax (no host sync per iteration)
        tails32, offs, wts_w, hubs32 = extra
        if bounds is not None:
            tgt_hub, cw_hub = _require().hub_refine_moves(
                tails32, wts_w, offs, hubs32, selfloop,
                inp.curr_comm, inp.v_degree, inp.comm_degree, inp.comm_gid,
                float(inp.constant), bounds[0], bounds[1], **_gid_args(inp))
            return tgt_hub, cw_hub
        tgt_hub, cw_hub = _require().hub_moves(
            tails32, wts_w, offs, hubs32, selfloop,
            inp.curr_comm, inp.v_degree, inp.comm_size, inp.comm_degree,
            inp.comm_gid, float(inp.constant), **_gid_args(inp),
            next_size=None if nxt is None else nxt[0],
            next_degree=None if nxt is None else nxt[1])
        return tgt_hub, cw_hub
    if nxt is not None:
        raise RuntimeError("fused aggregates need the rocPRIM hub path "
                           "(CUVITE_HUB_SEGSORT=0 or a CPU tensor disables "
                           "it)")
    comm = inp.curr_comm[tails_h].to(torch.int64)
    key = seg * C + comm
    del comm
    key_s, order = torch.sort(key)
    del key
    w_s = wts[order]
    del order
    uniq, counts = torch.unique_consecutive(key_s, return_counts=True)
    del key_s
    ends = torch.cumsum(counts, dim=0) - 1
    del counts
    cs = torch.cumsum(w_s, dim=0)
    del w_s
    wsum = cs[ends].clone()
    wsum[1:] -= cs[ends[:-1]]
    del cs, ends
    hub_of = uniq // C
    y = uniq % C
    del uniq

    cc = inp.curr_comm[hubs].to(torch.int64)         # [nhub]
    vdeg = inp.v_degree[hubs].to(torch.float64)
    # weight to own community (includes self-loops)
    is_cc = y == cc[hub_of]
    wcc = torch.zeros(nhub, dtype=torch.float64, device=dev)
    wcc[hub_of[is_cc]] = wsum[is_cc]
    eix = wcc - selfloop
    ax = inp.comm_degree[cc].to(torch.float64) - vdeg
    ay = inp.comm_degree[y].to(torch.float64)
    g = 2.0 * (wsum - eix[hub_of]) - 2.0 * vdeg[hub_of] * \
        (ay - ax[hub_of]) * float(inp.constant)
    g = torch.where(is_cc, torch.full_like(g, -torch.inf), g)
    del ay, wsum
    if bounds is not None:
        # refine round: only candidates with the mover's bound count, and a
        # hub that does not move has none
        mb = bounds[0][hubs].to(torch.int64)
        ok = (mb[hub_of] >= 0) & (bounds[1].to(torch.int64)[y] == mb[hub_of])
        g = torch.where(ok, g, torch.full_like(g, -torch.inf))
        wcc = torch.where(mb >= 0, wcc, torch.zeros_like(wcc))

    gmax = torch.full((nhub,), 0.0, dtype=torch.float64, device=dev)
    gmax.scatter_reduce_(0, hub_of, g, reduce="amax")
    move = gmax > 0.0
    winner = (g == gmax[hub_of]) & move[hub_of] & ~is_cc
    gid_y = inp.comm_gid[y]
    gid_win = torch.full((nhub,), torch.iinfo(torch.int64).max,
                         dtype=torch.int64, device=dev)
    gid_win.scatter_reduce_(0, hub_of[winner], gid_y[winner], reduce="amin")
    final = winner & (gid_y == gid_win[hub_of])
    tgt_dense = cc.clone()
    tgt_dense[hub_of[final]] = y[final]
    if bounds is not None:
        return tgt_dense.to(torch.int32), wcc.to(inp.weights.dtype)
    # singleton-swap guard (louvain.cpp:2238-2239)
    guard = (inp.comm_size[tgt_dense] == 1) & (inp.comm_size[cc] == 1) & \
        (inp.comm_gid[tgt_dense] > inp.comm_gid[cc])
    tgt_dense = torch.where(guard, cc, tgt_dense)
    return tgt_dense.to(torch.int32), wcc.to(inp.weights.dtype)


def fused_aggregates_supported() -> bool:
    """Whether local_move can account the new community aggregates itself
    (next_size / next_degree): needs the rocPRIM hub path and the plain
    (not per-class diagnostic) schedule."""
    return _hub_segsort_enabled() and not os.environ.get("CUVITE_PROGRESS")


def _class_streams_enabled() -> bool:
    """Run the block classes 4-6 beside the sub classes 0-3 on an auxiliary
    stream inside the local_move binding (default; s26 step 70.5 -> 59 ms,
    profiles/round4_class_schedule.md). CUVITE_CLASS_STREAMS=0 restores the
    serial schedule: all seven class kernels one after another on the
    calling stream. Read per call."""
    return os.environ.get("CUVITE_CLASS_STREAMS", "1") not in ("0", "off")


def _classes_beside_hubs(dev, hubs64, run_hub_sort, classes, hub_moves,
                         hub_mask=None):
    """Shared tail of local_move, refine_move and frontier_move. `classes()`
    launches the degree-class kernels and returns (target [nv], cw [nv]);
    `hub_moves()` runs the hub pipeline and returns the per-hub pair aligned
    with hubs64, which is scattered into the class result. With
    `run_hub_sort` false only the classes run. `hub_mask` (bool, aligned
    with hubs64): scatter only those hubs' results."""
    if hub_mask is not None and run_hub_sort:
        inner = hub_moves
        hubs64 = hubs64[hub_mask]

        def hub_moves():
            t, w = inner()
            return t[hub_mask], w[hub_mask]
    if run_hub_sort and not os.environ.get("CUVITE_NO_OVERLAP"):
        # disjoint vertex sets: run the HIP class kernels on a side stream
        # concurrently with the (longer) hub pipeline on the main stream;
        # hub results come back as separate tensors and are scattered after
        # the join (no cross-stream writes into the class kernels' outputs)
        main = torch.cuda.current_stream(dev)
        side = _side_stream(dev)
        side.wait_stream(main)
        with torch.cuda.stream(side):
            target, cw = classes()
        hub_tgt, hub_cw = hub_moves()
        main.wait_stream(side)
        target.record_stream(main)
        cw.record_stream(main)
        target[hubs64] = hub_tgt
        cw[hubs64] = hub_cw
        return target, cw
    target, cw = classes()
    if run_hub_sort:
        hub_tgt, hub_cw = hub_moves()
        target[hubs64] = hub_tgt
        cw[hubs64] = hub_cw
    return target, cw


def local_move(inp, next_size=None, next_degree=None):
    """HIP local-move iteration (see local_move.MoveInputs for semantics).
    Returns (target dense comm ids [nv], cluster_weight [nv]).

    With `next_size` (int64) and `next_degree` (weight dtype), both of one
    length >= nv, every vertex that has edges is also added to the size and
    the degree of its target community in those buffers, by the kernel lane
    that stores its target. The caller pre-loads them with what the edgeless
    vertices contribute (those are never visited). The inputs' comm_size /
    comm_degree must be other tensors: they are read while these are written.

    Degree classes 0-6 run in the LDS hash-table kernels; hub vertices
    (deg > _hub_cut()) go through the rocPRIM segsort pipeline
    (_hub_moves_sorted), overlapped on separate HIP streams (disjoint
    vertex sets). Inside the class binding the block classes 4-6 run on an
    auxiliary stream beside the sub classes 0-3 and are joined before it
    returns (CUVITE_CLASS_STREAMS=0: one after another). At world 1 the
    process thus uses three streams: the caller's, the side stream here and
    the binding's auxiliary one."""
    ext = _require()
    vlists, hubs64, hdeg = _buckets_for(inp.rowptr)
    dev = inp.rowptr.device
    if (next_size is None) != (next_degree is None):
        raise ValueError("next_size and next_degree go together")
    nxt = None if next_size is None else (next_size, next_degree)
    if nxt is not None and not fused_aggregates_supported():
        raise RuntimeError("fused aggregates need the rocPRIM hub path and "
                           "the plain schedule (CUVITE_HUB_SEGSORT=0 or "
                           "CUVITE_PROGRESS is set)")
    kw = dict(_gid_args(inp), next_size=next_size, next_degree=next_degree,
              class_streams=_class_streams_enabled())
    if os.environ.get("CUVITE_PROGRESS"):
        import sys
        import time
        torch.cuda.synchronize()
        sizes = [int(v.numel()) for v in vlists]
        print(f"[move] classes {sizes} hubs={hubs64.numel()}",
              file=sys.stderr, flush=True)
        outs = []
        for i in range(len(vlists)):
            one = [v if j == i else v[:0] for j, v in enumerate(vlists)]
            t0 = time.perf_counter()
            outs.append(ext.local_move_bucketed(
                inp.rowptr, inp.tails, inp.weights, inp.curr_comm,
                inp.v_degree, inp.comm_size, inp.comm_degree, inp.comm_gid,
                float(inp.constant), one, **kw))
            torch.cuda.synchronize()
            print(f"[move] class {i} n={sizes[i]} "
                  f"{time.perf_counter() - t0:.3f}s", file=sys.stderr,
                  flush=True)
        # merge: each class wrote its own vertices; take per-class targets
        target = outs[0][0]
        cw = outs[0][1]
        for i in range(1, len(vlists)):
            vl = vlists[i].to(torch.int64)
            if vl.numel():
                target[vl] = outs[i][0][vl]
                cw[vl] = outs[i][1][vl]
        if hubs64.numel():
            t0 = time.perf_counter()
            hub_tgt, hub_cw = _hub_moves_sorted(inp, hubs64, hdeg)
            target[hubs64] = hub_tgt
            cw[hubs64] = hub_cw
            torch.cuda.synchronize()
            print(f"[move] hub-sort n={hubs64.numel()} "
                  f"{time.perf_counter() - t0:.3f}s", file=sys.stderr,
                  flush=True)
        return target, cw

    def classes():
        return ext.local_move_bucketed(
            inp.rowptr, inp.tails, inp.weights, inp.curr_comm, inp.v_degree,
            inp.comm_size, inp.comm_degree, inp.comm_gid, float(inp.constant),
            vlists, **kw)

    return _classes_beside_hubs(
        dev, hubs64, hubs64.numel() > 0, classes,
        lambda: _hub_moves_sorted(inp, hubs64, hdeg, nxt))


def refine_move(inp, mover_bound: torch.Tensor, cand_bound: torch.Tensor,
                out=None):
    """HIP Leiden refine round (semantics: local_move.refine_move_torch).
    `mover_bound` int32 [>= nv]: bound id of a vertex that moves this round,
    else -1; `cand_bound` int32 [nc]: bound id of a dense community that may
    be joined this round, else -1. Returns (target dense comm ids [nv],
    cluster_weight [nv]); a vertex that does not move keeps its label.

    Same routing as local_move: the refine variants of the degree-class
    kernels, and the hub pipeline with the refine argmax kernels. The hub
    adjacency is cached per phase for the full hub list, so the sort covers
    every hub whenever one of them moves (non-movers leave the argmax
    kernels at once); a round in which no hub moves skips the hub pipeline,
    at the price of one host sync. inp.comm_size is not read. `out`: optional
    (target int32 [nv], cluster_weight [nv]) pair of contiguous buffers to
    write the result into."""
    ext = _require()
    vlists, hubs64, hdeg = _buckets_for(inp.rowptr)
    dev = inp.rowptr.device
    kw = dict(_gid_args(inp), class_streams=_class_streams_enabled())
    run_hub_sort = hubs64.numel() > 0 and bool(
        (mover_bound[hubs64] >= 0).any())

    def classes():
        return ext.refine_move_bucketed(
            inp.rowptr, inp.tails, inp.weights, inp.curr_comm, inp.v_degree,
            inp.comm_degree, inp.comm_gid, float(inp.constant), vlists,
            mover_bound, cand_bound, **kw,
            out_target=None if out is None else out[0],
            out_cw=None if out is None else out[1])

    bounds = (mover_bound, cand_bound)
    return _classes_beside_hubs(
        dev, hubs64, run_hub_sort, classes,
        lambda: _hub_moves_sorted(inp, hubs64, hdeg, None, bounds))


def _as_u8(active: torch.Tensor) -> torch.Tensor:
    """A bool or uint8 mask as uint8 over the same storage."""
    if active.dtype == torch.bool:
        return active.view(torch.uint8)
    if active.dtype != torch.uint8:
        raise TypeError("active must be a bool or uint8 mask")
    return active


def frontier_span() -> int:
    """Edges per wave span of the frontier_expand kernel (tests build their
    shapes around it)."""
    return int(_require().frontier_span())


def frontier_expand(changed: torch.Tensor, rowptr: torch.Tensor,
                    tails_dense: torch.Tensor, g_rowptr: torch.Tensor,
                    g_heads: torch.Tensor, active: torch.Tensor) -> torch.Tensor:
    """active[u] = 1 for every changed local id and for every local
    neighbour u of a changed dense id, in place (twin:
    dynamic.frontier_expand_torch). `changed`: int32 dense ids in
    [0, nv + ng), locals and ghosts in any order; `rowptr` / `tails_dense`:
    the level CSR; `g_rowptr` int64 [ng + 1] / `g_heads` int32: the ghost ->
    local reverse adjacency (dynamic.ghost_reverse_csr); `active`: bool or
    uint8 [nv]. Work is proportional to the summed degree of the changed
    rows; no host sync. Returns `active`."""
    _require().frontier_expand(changed, rowptr, tails_dense, g_rowptr,
                               g_heads, _as_u8(active))
    return active


def frontier_lists(rowptr: torch.Tensor, active: torch.Tensor):
    """Per-class vertex lists of the active vertices, built on the device in
    one compaction with ONE host sync (the copy of the nine counts). Returns
    nine ascending int32 lists: the seven LDS degree classes (what
    local_move_bucketed takes), the active hubs (FRONTIER_HUB_CLASS) and the
    active vertices without edges (FRONTIER_EDGELESS_CLASS). The lists are
    views of one buffer."""
    cls = _class_ids_for(rowptr)
    lists, counts = _require().frontier_compact(_as_u8(active), cls)
    out, lo = [], 0
    for n in counts.tolist():  # the sweep's host sync
        out.append(lists[lo:lo + n])
        lo += n
    return out


def frontier_move(inp, active: torch.Tensor, cw_prev: torch.Tensor,
                  lists=None):
    """HIP local move over the vertices marked in `active` (bool or uint8
    [nv]) only; twin: dynamic.frontier_move_torch. Returns (target dense comm
    ids [nv], cluster_weight [nv]): an active vertex gets exactly what
    local_move gives it, an inactive one keeps its label and its entry of
    `cw_prev` (weight dtype [nv], not modified). `lists`: the result of
    frontier_lists(inp.rowptr, active) if the caller already has it.

    The degree-class kernels run over the compacted class lists as they are.
    Hubs: the pipeline is skipped when no hub is active; otherwise it runs
    over the phase's cached full hub list (the flattened hub adjacency is
    keyed by that list) and only the active hubs' results are scattered."""
    ext = _require()
    if lists is None:
        lists = frontier_lists(inp.rowptr, active)
    vlists = list(lists[:7])
    act_hubs = lists[FRONTIER_HUB_CLASS]
    edgeless = lists[FRONTIER_EDGELESS_CLASS]
    nv = inp.nv
    dev = inp.rowptr.device
    target = torch.empty(nv, dtype=torch.int32, device=dev)
    cw = cw_prev.to(inp.weights.dtype).clone().contiguous()
    if edgeless.numel():
        cw[edgeless.to(torch.int64)] = 0  # what the move gives an edgeless row
    kw = dict(_gid_args(inp), class_streams=_class_streams_enabled(),
              out_target=target, out_cw=cw, keep_cw=True)

    def classes():
        return ext.local_move_bucketed(
            inp.rowptr, inp.tails, inp.weights, inp.curr_comm, inp.v_degree,
            inp.comm_size, inp.comm_degree, inp.comm_gid, float(inp.constant),
            vlists, **kw)

    if act_hubs.numel() == 0:
        return _classes_beside_hubs(dev, None, False, classes, None)
    _, hubs64, hdeg = _buckets_for(inp.rowptr)
    hub_mask = active[hubs64].to(torch.bool)
    return _classes_beside_hubs(
        dev, hubs64, True, classes,
        lambda: _hub_moves_sorted(inp, hubs64, hdeg), hub_mask=hub_mask)


def batch_span() -> int:
    """Touched entries per wave span of the edge-batch kernels (tests build
    their shapes around it)."""
    return int(_require().batch_span())


def apply_batch(rowptr: torch.Tensor, tails: torch.Tensor,
                weights: torch.Tensor, base: int, nv_global: int,
                d_src: torch.Tensor, d_dst: torch.Tensor,
                i_src: torch.Tensor, i_dst: torch.Tensor, i_w: torch.Tensor):
    """The CSR (rowptr, tails, weights) of one rank after its routed lists
    (directed, global ids, every source in [base, base + nv)): deletions
    (d_src, d_dst), then insertions (i_src, i_dst, i_w). Rows come out in the
    stable order of the twin, dynamic.apply_routed_batch_torch, bit for bit.
    Returns (new_rowptr, new_tails, new_weights), fresh tensors, or None if a
    deletion matches no stored entry; the inputs are never modified.

    Host side: torch ops over batch-sized and nv-sized tensors only (sort and
    deduplicate the lists, the touched rows and their slices, the new
    degrees). Device: mark / copy / compact / insert kernels
    (louvain_kernels.hip). A constant number of host syncs: two explicit
    ones, the touched rows' entry count and then "any deletion unmatched"
    with the new edge count, plus those inside the two torch.unique calls,
    which size their outputs.
    Beside the new CSR it allocates one byte per touched entry, int64 per
    span and per touched row, and O(nv)."""
    ext = _require()
    dev = rowptr.device
    nv = rowptr.numel() - 1
    if d_src.numel() == 0 and i_src.numel() == 0:
        return rowptr.clone(), tails.clone(), weights.clone()
    i64 = dict(dtype=torch.int64, device=dev)
    dkey = torch.unique((d_src - base) * nv_global + d_dst)  # (row, dst) order
    drow = torch.div(dkey, nv_global, rounding_mode="floor")
    ddst = (dkey - drow * nv_global).contiguous()
    irow = i_src - base
    order = torch.argsort(irow, stable=True)
    irow = irow[order]
    idst = i_dst[order].contiguous()
    iw = i_w[order].to(weights.dtype).contiguous()
    t_rows = torch.unique(torch.cat([drow, irow]))
    nt = t_rows.numel()
    edges = torch.cat([t_rows, torch.full((1,), nv, **i64)])
    d_offs = torch.searchsorted(drow, edges).contiguous()
    i_offs = torch.searchsorted(irow, edges).contiguous()
    t_offs = torch.zeros(nt + 1, **i64)
    t_offs[1:] = torch.cumsum(rowptr[t_rows + 1] - rowptr[t_rows], dim=0)
    n_touched = int(t_offs[-1])  # host sync: sizes the keep flags
    keep, span_cnt, row_kept, matched = ext.batch_mark(
        rowptr, tails, t_rows, t_offs, n_touched, d_offs, ddst)
    deg = rowptr[1:] - rowptr[:-1]
    deg[t_rows] = row_kept + (i_offs[1:] - i_offs[:-1])
    new_rowptr = torch.zeros(nv + 1, **i64)
    new_rowptr[1:] = torch.cumsum(deg, dim=0)
    del deg
    touched = torch.zeros(nv, dtype=torch.uint8, device=dev)
    touched[t_rows] = 1
    absent, new_ne = torch.stack([
        (matched == 0).any().to(torch.int64), new_rowptr[-1]]).tolist()
    if absent:
        return None
    span_offs = torch.cumsum(span_cnt, dim=0) - span_cnt
    kept_offs = torch.cumsum(row_kept, dim=0) - row_kept
    new_tails, new_weights = ext.batch_write(
        rowptr, tails, weights, t_rows, t_offs, n_touched, keep, span_offs,
        kept_offs, row_kept, touched, new_rowptr, int(new_ne), i_offs, idst,
        iw)
    return new_rowptr, new_tails, new_weights


def modularity_parts(cluster_weight: torch.Tensor,
                     local_comm_degree: torch.Tensor) -> torch.Tensor:
    """HIP reduction of (sum cluster_weight, sum degree^2) in fp64."""
    ext = _require()
    return ext.modularity_parts(cluster_weight, local_comm_degree)


def intra_weight(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                 weights: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """out[v] = sum of w[e] over row v's edges whose tail carries v's label,
    for ARBITRARY labels (int32 dense or int64 global ids, [nv + ng], local
    vertices first): the `cw` that local_move returns, self-loops and
    parallel edges included, without the hash-table pass. Edge-balanced
    HIP kernel on the current stream; output has the weights' dtype."""
    return _require().intra_weight(rowptr, tails_dense, weights, labels)


def intra_boundary(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                   weights: torch.Tensor, labels: torch.Tensor):
    """(cw, mask) from one edge pass: cw is intra_weight's result bit for
    bit, mask (uint8 [nv]) is 1 for every row with an edge whose tail lies
    inside `labels` and carries another label than the row: the boundary
    vertices, the only ones a local move can move (twin:
    uncoarsen.intra_boundary_torch). Self-loops and out-of-range tails mark
    nothing."""
    return _require().intra_boundary(rowptr, tails_dense, weights, labels)


def intra_weight_span() -> int:
    """Edges per wave span of the intra_weight kernel (rows cut by a span
    boundary take the atomic path; tests build their shapes around it)."""
    return int(_require().intra_weight_span())


def cc_components(rowptr: torch.Tensor, tails_dense: torch.Tensor,
                  labels_all: torch.Tensor):
    """Connected components of the graph restricted to edges whose endpoints
    carry the same label, over the dense node space [0, nv + ng) of
    halo.tails_dense (locals first, then ghosts; labels int32 or int64).
    Returns (comp int32 [nv + ng], rounds): comp[x] is the smallest dense id
    in x's component, rounds the number of hook + compress rounds (one host
    sync each; 0 when there is no edge or no vertex). HIP kernels on the
    current stream; the oracle is connectivity.cc_components_torch."""
    comp, rounds = _require().cc_components(rowptr, tails_dense, labels_all)
    return comp, int(rounds)


def scatter_add_(out: torch.Tensor, idx: torch.Tensor,
                 val: torch.Tensor) -> torch.Tensor:
    """out[idx[i]] += val[i]. On GPU float tensors this MUST go through the
    HIP kernel (native fp64 atomics): torch's index_add_ lowers fp64 atomic
    adds to a CAS loop on ROCm, measured 16.5 s per call at R-MAT s22
    (profiles/bench_s22 first profile). Integer dtypes and CPU tensors use
    torch's fast path."""
    if out.is_cuda and out.is_floating_point():
        _require().scatter_add_(out, idx, val.to(out.dtype))
    else:
        out.index_add_(0, idx, val.to(out.dtype))
    return out


def apply_deltas_(target: torch.Tensor, curr: torch.Tensor,
                  v_degree: torch.Tensor, base: int, bound: int,
                  local_size: torch.Tensor, local_degree: torch.Tensor):
    """Fused post-sweep community-aggregate update: for every vertex whose
    label changed, apply the +-1 size / +-degree deltas to LOCALLY-owned
    communities with native atomics (one kernel; replaces the torch
    mask/compact/index_add chain measured at ~40 ms/sweep at s26)."""
    _require().apply_deltas_(target, curr, v_degree, base, bound,
                             local_size, local_degree)


def csr_from_edges(nv: int, base: int, src: torch.Tensor, dst: torch.Tensor,
                   w: torch.Tensor):
    """Sort-free device CSR assembly: (rowptr, tails, weights). Handles edge
    counts beyond INT_MAX (torch.argsort cannot)."""
    ext = _require()
    return ext.csr_from_edges(nv, base, src, dst, w)


def row_sum(rowptr: torch.Tensor, weights: torch.Tensor) -> torch.Tensor:
    """Per-vertex weighted degree on device (one wave per CSR row)."""
    ext = _require()
    return ext.row_sum(rowptr, weights)
