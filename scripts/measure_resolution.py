"""Measure the resolution parameter (LouvainConfig.resolution).

    python scripts/measure_resolution.py --cpu-table --out DIR
    python scripts/measure_resolution.py --scale 22 --out DIR

--cpu-table: on the CPU oracle (backend="torch", one rank) over two clique
rings and the quality graphs of tests/quality_cases.py, for gamma in 0.25,
0.5, 1, 2, 4: community count, sweeps and exact Q_gamma of the plain run, of
vcycle=True and of algorithm="leiden"; then resolution_scan over 4, 2, 1,
0.5, 0.25 against five cold runs (sweeps and Q_gamma of either). Needs no
GPU; times are not taken.

--scale S: on one GPU, R-MAT (edge factor 16, fp64, natural vertex order),
one plain run per gamma in --gammas after one untimed warm-up run at gamma
1: wall time between device synchronisations, sweeps, phases, communities,
the estimate and the exact Q_gamma of the result. ONE run each: no spread is
known. Results go to stdout and DIR/resolution_cpu.json or
DIR/resolution_gpu.json."""

import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cuvite_amd.graph import single_partition  # noqa: E402
from cuvite_amd.louvain import (LouvainConfig, louvain,  # noqa: E402
                                resolution_scan)
from cuvite_amd.parallel import Comm  # noqa: E402
from cuvite_amd.quality import partition_quality  # noqa: E402

GAMMAS = (0.25, 0.5, 1.0, 2.0, 4.0)
MODES = {"plain": {}, "vcycle": dict(vcycle=True),
         "leiden": dict(algorithm="leiden")}


def cpu_table(out_dir):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from resolution_cases import graph

    rows, scans = [], []
    for name in ("ring32k4", "ring30k5", "karate", "lfr", "rgg"):
        dg = single_partition(graph(name))

        def q(labels, gamma):
            return partition_quality(dg, labels, Comm(), backend="torch",
                                     resolution=gamma).modularity

        cold = {}
        for gamma in GAMMAS:
            row = {"graph": name, "gamma": gamma}
            for mode, kw in MODES.items():
                res = louvain(dg, Comm(), LouvainConfig(
                    backend="torch", resolution=gamma, **kw))
                row[mode] = {
                    "communities": int(torch.unique(res.communities).numel()),
                    "sweeps": res.total_iters, "phases": res.phases,
                    "q_gamma": q(res.communities, gamma)}
                if mode == "plain":
                    cold[gamma] = row[mode]
            print(json.dumps(row), flush=True)
            rows.append(row)
        order = sorted(GAMMAS, reverse=True)
        warm = resolution_scan(dg, order, Comm(),
                               LouvainConfig(backend="torch"))
        scan = {"graph": name, "gammas": order,
                "scan_sweeps": [r.total_iters for r in warm],
                "cold_sweeps": [cold[g]["sweeps"] for g in order],
                "scan_q_gamma": [q(r.communities, g)
                                 for r, g in zip(warm, order)],
                "cold_q_gamma": [cold[g]["q_gamma"] for g in order],
                "scan_communities": [int(torch.unique(r.communities).numel())
                                     for r in warm]}
        scan["scan_sweeps_total"] = sum(scan["scan_sweeps"])
        scan["cold_sweeps_total"] = sum(scan["cold_sweeps"])
        print(json.dumps(scan), flush=True)
        scans.append(scan)
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "resolution_cpu.json"), "w") as f:
        json.dump({"runs": rows, "scans": scans}, f, indent=1)


def gpu_runs(args):
    from cuvite_amd import ops
    from cuvite_amd.generators import rmat_dist_graph
    from cuvite_amd.halo import build_halo

    assert torch.cuda.is_available() and ops.available(), \
        "needs a GPU and the built HIP extension"
    dev = torch.device("cuda:0")
    comm = Comm(dev)
    dg = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm, dev,
                         weight_dtype=torch.float64)
    result = {"scale": args.scale, "edgefactor": args.edgefactor,
              "nv": dg.nv, "ne_directed": dg.ne, "runs": []}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "resolution_gpu.json")
    for i, gamma in enumerate([1.0] + list(args.gammas)):
        ops.clear_phase_caches()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = louvain(dg, comm, LouvainConfig(backend="hip",
                                              resolution=gamma))
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if i == 0:
            continue                    # warm-up
        halo = build_halo(dg, comm)
        pq = partition_quality(dg, res.communities, comm, halo=halo,
                               backend="hip", resolution=gamma)
        del halo
        row = {"gamma": gamma, "run_ms": ms, "sweeps": res.total_iters,
               "phases": res.phases, "communities": pq.num_communities,
               "estimate": res.modularity, "exact_q_gamma": pq.modularity,
               "exact_q_1": pq.at(1.0),
               "sweeps_per_phase": [lv["iters"] for lv in res.levels],
               "times_s": res.times}
        print(json.dumps(row), flush=True)
        result["runs"].append(row)
        with open(path, "w") as f:      # kept after every run
            json.dump(result, f, indent=1)
        del res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu-table", action="store_true")
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--gammas", type=float, nargs="+",
                    default=[0.5, 1.0, 2.0])
    ap.add_argument("--out", default="out")
    args = ap.parse_args()
    if args.cpu_table:
        cpu_table(args.out)
    else:
        gpu_runs(args)


if __name__ == "__main__":
    main()
