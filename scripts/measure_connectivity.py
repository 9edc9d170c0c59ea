"""Time split_disconnected against ops.intra_weight and one local-move sweep.

    python scripts/measure_connectivity.py --scale 22 --out DIR
    rocprofv3 --kernel-trace --stats ... -- \\
        python scripts/measure_connectivity.py --scale 22 --calls-only 3

Same graph as bench.py (R-MAT, edge factor 16, degree-sorted relabelling, one
GPU) and the labels phase 0 converges to. Each call is timed with device
events, 3 warm-up calls, median of 10; split_disconnected and
ops.cc_components sync with the host once per round, which the events
include. The result goes to stdout and to DIR/connectivity_timing.json.
`--calls-only N` just runs N split_disconnected calls after one warm-up, for
a kernel trace that gives the time per cc_hook / cc_compress launch. Needs a
GPU: there is no CPU fall-back."""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvite_amd import ops, split_disconnected  # noqa: E402
from cuvite_amd.generators import degree_sort_dist, rmat_dist_graph  # noqa: E402
from cuvite_amd.halo import exchange_ghost_labels  # noqa: E402
from cuvite_amd.local_move import MoveInputs  # noqa: E402
from cuvite_amd.louvain import LouvainConfig, PhaseState, run_phase  # noqa: E402
from cuvite_amd.parallel import Comm  # noqa: E402
from cuvite_amd.quality import partition_quality  # noqa: E402


def _time(fn, warmup=3, reps=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a = torch.cuda.Event(enable_timing=True)
        b = torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="out")
    ap.add_argument("--calls-only", type=int, default=0)
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.available(), \
        "needs a GPU and the built HIP extension"
    dev = torch.device("cuda:0")
    comm = Comm(dev)
    dg = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm, dev,
                         weight_dtype=torch.float64)
    dg = degree_sort_dist(dg, comm)
    cfg = LouvainConfig(backend="hip", one_phase=True)
    state = PhaseState(dg, comm)
    halo = state.halo
    _, labels, iters, _ = run_phase(dg, comm, cfg, -1.0, 1.0e-6, halo=halo)

    def split():
        return split_disconnected(dg, labels, comm, halo=halo, backend="hip")

    rep = split()
    if args.calls_only:
        for _ in range(args.calls_only):
            split()
        torch.cuda.synchronize()
        print(f"{args.calls_only} calls, rounds {rep.rounds}")
        return

    before = partition_quality(dg, labels, comm, halo=halo, backend="hip")
    after = partition_quality(dg, rep.labels, comm, halo=halo, backend="hip")
    st = PhaseState(dg, comm, halo=halo, init_labels=labels)
    st.use_hip = True
    ghost = exchange_ghost_labels(halo, st.curr_comm)
    dense, _, c_size, c_degree, c_gid = st.densify(ghost)
    inp = MoveInputs(dg.g.rowptr, halo.tails_dense, dg.g.weights, dense,
                     st.v_degree, c_size, c_degree, c_gid, st.constant)
    result = {
        "scale": args.scale, "edgefactor": args.edgefactor, "nv": dg.nv,
        "ne_directed": dg.ne, "phase0_sweeps": iters,
        "communities": rep.num_communities,
        "components": rep.num_components,
        "disconnected": rep.num_disconnected, "rounds": list(rep.rounds),
        "exact_q_before": before.modularity,
        "exact_q_after": after.modularity,
        "split_disconnected": _time(split),
        "cc_components_int64_labels": _time(lambda: ops.cc_components(
            dg.g.rowptr, halo.tails_dense, labels)),
        "cc_components_int32_labels": _time(lambda: ops.cc_components(
            dg.g.rowptr, halo.tails_dense, dense)),
        "intra_weight_int64_labels": _time(lambda: ops.intra_weight(
            dg.g.rowptr, halo.tails_dense, dg.g.weights, labels)),
        "local_move_sweep": _time(lambda: ops.local_move(inp)),
    }
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "connectivity_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
