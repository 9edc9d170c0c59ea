"""Time the dynamic-frontier phase against the plain warm start and the cold
run after an edge batch.

    python scripts/measure_dynamic.py --scale 22 --out DIR

Same graph as bench.py (R-MAT, edge factor 16, fp64, degree-sorted
relabelling, one GPU). `prev` is the converged cold run's partition of the
old graph. For every batch fraction the batch is drawn with the recipe of
tests/dynamic_cases.py (seed 7: delete a random share of the undirected
pairs, insert as many random pairs; inserted weights uniform in [0, 1) like
the graph's), applied, and phase 0 of the new graph is run three ways,
alternating in one process: frontier (run_frontier_phase from prev and the
affected vertices), warm (run_phase from prev) and cold (run_phase from
singletons). Each is timed with a device synchronisation on both sides, 1
warm-up, median of `--reps` (default 5) with min..max. One more frontier run
with synchronising timers gives the split of its sweeps; in that run the
class kernels and the hub pipeline run one after the other
(CUVITE_NO_OVERLAP) so that the hub pipeline can be timed alone. The result
goes to stdout and DIR/dynamic_timing.json. Needs a GPU."""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvite_amd import ops  # noqa: E402
from cuvite_amd.dynamic import (EdgeBatch, affected_vertices,  # noqa: E402
                                apply_edge_batch, run_frontier_phase)
from cuvite_amd.generators import degree_sort_dist, rmat_dist_graph  # noqa: E402
from cuvite_amd.halo import build_halo  # noqa: E402
from cuvite_amd.louvain import LouvainConfig, louvain, run_phase  # noqa: E402
from cuvite_amd.parallel import Comm  # noqa: E402
from cuvite_amd.quality import partition_quality  # noqa: E402
from cuvite_amd.utils.timers import Timers  # noqa: E402


def recipe_batch(dg, frac):
    """tests/dynamic_cases.recipe_batch on a device graph; the draws come
    from a CPU generator so the batch does not depend on the device."""
    gen = torch.Generator().manual_seed(7)
    g = dg.g
    src = torch.repeat_interleave(torch.arange(g.nv, device=g.device),
                                  g.degrees())
    sel = (src < g.tails).nonzero(as_tuple=True)[0]
    m = sel.numel()
    k = max(1, int(frac * m))
    dele = sel[torch.randperm(m, generator=gen)[:k].to(g.device)]
    ins_u = torch.randint(0, g.nv, (k,), generator=gen)
    ins_v = torch.randint(0, g.nv, (k,), generator=gen)
    w = torch.rand(k, generator=gen, dtype=torch.float64)
    keep = ins_u != ins_v
    return EdgeBatch(ins_u[keep], ins_v[keep], w[keep], src[dele].cpu(),
                     g.tails[dele].cpu())


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fracs", default="0.0001,0.001,0.01")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="out")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.available(), \
        "needs a GPU and the built HIP extension"
    dev = torch.device("cuda:0")
    comm = Comm(dev)
    old = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm, dev,
                          weight_dtype=torch.float64)
    old = degree_sort_dist(old, comm)
    cfg = LouvainConfig(backend="hip")
    cold_full = louvain(old, comm, cfg)
    prev = cold_full.communities
    ops.clear_phase_caches()
    result = {"scale": args.scale, "edgefactor": args.edgefactor,
              "nv": old.nv, "ne_directed": old.ne,
              "cold_full_phases": cold_full.phases,
              "cold_full_iters": cold_full.total_iters,
              "hub_cut": ops._hub_cut(), "batches": []}
    for frac in [float(x) for x in args.fracs.split(",")]:
        batch = recipe_batch(old, frac)
        dg = apply_edge_batch(old, comm, batch)
        f0 = affected_vertices(dg, comm, prev, batch)
        halo = build_halo(dg, comm)

        def frontier(**kw):
            return run_frontier_phase(dg, comm, cfg, prev, f0, halo=halo,
                                      **kw)

        def warm():
            return run_phase(dg, comm, cfg, -1.0, cfg.threshold, halo=halo,
                             init_labels=prev)

        def cold():
            return run_phase(dg, comm, cfg, -1.0, cfg.threshold, halo=halo)

        # alternating: one round runs all three, the first round warms up
        ms = {"frontier": [], "warm": [], "cold": []}
        outs = {}
        for rnd in range(args.reps + 1):
            for name, fn in (("frontier", frontier), ("warm", warm),
                             ("cold", cold)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[name] = fn()
                torch.cuda.synchronize()
                if rnd:
                    ms[name].append((time.perf_counter() - t0) * 1e3)
        rep = outs["frontier"][4]

        def q(labels):
            return partition_quality(dg, labels, comm, halo=halo,
                                     backend="hip").modularity

        # the split of the frontier sweeps, classes and hubs in series
        os.environ["CUVITE_NO_OVERLAP"] = "1"
        timers = Timers(sync=True)
        hub_ms = []
        inner = ops._hub_moves_sorted

        def hub_timed(*a, **k):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = inner(*a, **k)
            torch.cuda.synchronize()
            hub_ms.append((time.perf_counter() - t0) * 1e3)
            return r

        ops._hub_moves_sorted = hub_timed
        try:
            frontier(timers=timers)
        finally:
            ops._hub_moves_sorted = inner
            del os.environ["CUVITE_NO_OVERLAP"]
        split = {k: v * 1e3 for k, v in timers.acc.items()}
        split["hub_pipeline"] = sum(hub_ms)
        split["class_kernels"] = split.pop("move") - split["hub_pipeline"]
        entry = {
            "frac": frac, "inserted": int(batch.ins_src.numel()),
            "deleted": int(batch.del_src.numel()),
            "frontier0": int(f0.sum()),
            "frontier_sizes": rep.sizes_per_sweep,
            "frontier_sweeps": rep.sweeps, "evaluated": rep.evaluated,
            "warm_sweeps": outs["warm"][2], "cold_sweeps": outs["cold"][2],
            "frontier": stats(ms["frontier"]), "warm": stats(ms["warm"]),
            "cold": stats(ms["cold"]),
            "warm_over_frontier": statistics.median(ms["warm"])
            / statistics.median(ms["frontier"]),
            "exact_q_frontier": q(outs["frontier"][1]),
            "exact_q_warm": q(outs["warm"][1]),
            "exact_q_prev_on_new": q(prev),
            "split_ms_sum_over_sweeps": split,
            "hub_sweeps": len(hub_ms),
        }
        print(json.dumps(entry), flush=True)
        result["batches"].append(entry)
        del dg, halo, outs
        ops.clear_phase_caches()
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "dynamic_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
