"""Measure the V-cycle (louvain(vcycle=True)) against the plain run.

    python scripts/measure_vcycle.py --cpu-table --out DIR
    python scripts/measure_vcycle.py --scale 22 --out DIR

--cpu-table: the quality table on the CPU oracle (backend="torch", one rank,
default options) over the quality graphs of tests/quality_cases.py and
rmat_graph(s, 16, seed=1), s = 10 and 14: exact Q of the plain run, of a warm
restart from it, of the V-cycle with full sweeps (every sweep over all
vertices) and of the V-cycle as built (boundary first, then moved +
neighbours), and what level 0 evaluated either way. Needs no GPU; times are
not taken.

--scale S: on one GPU, the graph of scripts/measure_dynamic.py (R-MAT, edge
factor 16, fp64, degree-sorted relabelling). The plain and the V-cycle run
alternate in one process, each between device synchronisations: 1 warm-up
round, then `--reps` rounds, median with min..max, and the exact Q of both
results. The per-level split comes from the report of the last V-cycle run
(host clock; every part ends in a host read). ops.intra_boundary and
ops.intra_weight are timed by device events on the input graph under the
plain run's labels, alternating, `--kernel-reps` launches each. Results go to
stdout and DIR/vcycle_cpu.json or DIR/vcycle_timing.json."""

import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cuvite_amd import uncoarsen  # noqa: E402
from cuvite_amd.generators import rmat_graph  # noqa: E402
from cuvite_amd.graph import single_partition  # noqa: E402
from cuvite_amd.louvain import LouvainConfig, louvain  # noqa: E402
from cuvite_amd.parallel import Comm  # noqa: E402
from cuvite_amd.quality import partition_quality  # noqa: E402


def level_dict(lv):
    return {"level": lv.level, "vertices": lv.nv_global,
            "boundary": lv.boundary, "sweeps": lv.sweeps,
            "sizes": lv.sizes_per_sweep, "evaluated": lv.evaluated,
            "moved": lv.moved, "q_before": lv.q_before,
            "q_after": lv.q_after, "setup_ms": lv.setup_s * 1e3,
            "sweeps_ms": lv.sweeps_s * 1e3}


def cpu_table(out_dir):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from quality_cases import whole_graph

    rows = []
    for name in ("karate", "karate2", "lfr", "rgg", "rmat10", "rmat14"):
        g = rmat_graph(int(name[4:]), 16, seed=1) \
            if name.startswith("rmat") else whole_graph(name)
        dg = single_partition(g)

        def q(labels):
            return partition_quality(dg, labels, Comm(),
                                     backend="torch").modularity

        plain = louvain(dg, Comm(), LouvainConfig(backend="torch"))
        warm = louvain(dg, Comm(), LouvainConfig(backend="torch"),
                       init_labels=plain.communities.clone())
        vcy = louvain(dg, Comm(), LouvainConfig(backend="torch", vcycle=True))
        # the full-sweep variant: refine_up's test hook
        real = uncoarsen.refine_up
        uncoarsen.refine_up = lambda *a, **k: real(*a, full=True, **k)
        try:
            full = louvain(dg, Comm(),
                           LouvainConfig(backend="torch", vcycle=True))
        finally:
            uncoarsen.refine_up = real
        row = {"graph": name, "nv": g.nv, "q_plain": q(plain.communities),
               "q_warm": q(warm.communities), "q_full": q(full.communities),
               "q_frontier": q(vcy.communities),
               "level0_evaluated_frontier": vcy.vcycle[-1].evaluated,
               "level0_evaluated_full": full.vcycle[-1].evaluated,
               "levels": [level_dict(lv) for lv in vcy.vcycle]}
        row["gain"] = row["q_frontier"] - row["q_plain"]
        print(json.dumps({k: v for k, v in row.items() if k != "levels"}),
              flush=True)
        rows.append(row)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "vcycle_cpu.json"), "w") as f:
        json.dump(rows, f, indent=1)


def stats(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "reps": len(ms)}


def gpu_timing(args):
    from cuvite_amd import ops
    from cuvite_amd.generators import degree_sort_dist, rmat_dist_graph
    from cuvite_amd.halo import build_halo, exchange_ghost_labels

    assert torch.cuda.is_available() and ops.available(), \
        "needs a GPU and the built HIP extension"
    dev = torch.device("cuda:0")
    comm = Comm(dev)
    dg = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm, dev,
                         weight_dtype=torch.float64)
    dg = degree_sort_dist(dg, comm)
    cfgs = {"plain": LouvainConfig(backend="hip"),
            "vcycle": LouvainConfig(backend="hip", vcycle=True)}
    ms = {k: [] for k in cfgs}
    outs = {}
    for rnd in range(args.reps + 1):
        for name, cfg in cfgs.items():
            ops.clear_phase_caches()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[name] = louvain(dg, comm, cfg)
            torch.cuda.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3)
    halo = build_halo(dg, comm)

    def q(labels):
        return partition_quality(dg, labels, comm, halo=halo,
                                 backend="hip").modularity

    result = {"scale": args.scale, "edgefactor": args.edgefactor,
              "nv": dg.nv, "ne_directed": dg.ne}
    for name, res in outs.items():
        result[name] = dict(stats(ms[name]), exact_q=q(res.communities),
                            estimate=res.modularity, phases=res.phases,
                            iters=res.total_iters,
                            times_last_run_s=res.times)
    result["vcycle"]["levels"] = [level_dict(lv)
                                  for lv in outs["vcycle"].vcycle]

    # the setup pass against plain intra_weight, by device events
    labels = torch.cat([outs["plain"].communities,
                        exchange_ghost_labels(halo,
                                              outs["plain"].communities)])
    a = (dg.g.rowptr, halo.tails_dense, dg.g.weights, labels)
    kern = {"intra_weight": lambda: ops.intra_weight(*a),
            "intra_boundary": lambda: ops.intra_boundary(*a)}
    kms = {k: [] for k in kern}
    for rnd in range(args.kernel_reps + 3):
        for name, fn in kern.items():
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= 3:
                kms[name].append(e0.elapsed_time(e1))
    cw, mask = ops.intra_boundary(*a)
    result["kernels"] = {k: stats(v) for k, v in kms.items()}
    result["kernels"]["boundary_vertices"] = int(mask.sum())
    # rows cut by a span boundary are summed with float atomics, so on fp
    # weights two launches of ONE kernel may differ in the last bits: report
    # the difference between the two kernels beside that of two intra_weight
    # launches
    iw1, iw2 = ops.intra_weight(*a), ops.intra_weight(*a)
    result["kernels"]["cw_max_abs_diff_boundary_vs_weight"] = float(
        (cw - iw1).abs().max())
    result["kernels"]["cw_max_abs_diff_weight_vs_weight"] = float(
        (iw1 - iw2).abs().max())
    result["kernels"]["cw_rows_differing_boundary_vs_weight"] = int(
        (cw != iw1).sum())
    result["kernels"]["cw_rows_differing_weight_vs_weight"] = int(
        (iw1 != iw2).sum())
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "vcycle_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-table", action="store_true")
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--out", default="out")
    args = ap.parse_args()
    if args.cpu_table:
        cpu_table(args.out)
    else:
        gpu_timing(args)


if __name__ == "__main__":
    main()
