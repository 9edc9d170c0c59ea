"""Time the Leiden refinement against one local-move sweep, and compare the
quality of louvain, connectivity="level" and leiden runs.

    python scripts/measure_leiden.py --scale 22 --out DIR          # GPU timing
    python scripts/measure_leiden.py --quality --device cpu        # quality

Timing (needs a GPU: there is no CPU fall-back). Same graph as bench.py
(R-MAT, edge factor 16, degree-sorted relabelling, one GPU) and the labels
phase 0 converges to. One refine round (the first of a refinement: every
vertex is a singleton, half of them move) and one local-move sweep from the
same singleton state are timed with device events, 3 warm-up calls, median
of 10; a whole refinement (all rounds, with its host sync per round) is
timed the same way with 1 warm-up and 5 repetitions. The result goes to
stdout and to DIR/leiden_timing.json.

Quality: exact Q, communities and communities split by the final pass, on
the four quality graphs of the tests and R-MAT s14."""

import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cuvite_amd import ops, refine_partition, split_disconnected  # noqa: E402
from cuvite_amd.generators import (degree_sort_dist, rmat_dist_graph,  # noqa: E402
                                   rmat_graph)
from cuvite_amd.graph import single_partition  # noqa: E402
from cuvite_amd.halo import exchange_ghost_labels  # noqa: E402
from cuvite_amd.local_move import MoveInputs  # noqa: E402
from cuvite_amd.louvain import (LouvainConfig, PhaseState, louvain,  # noqa: E402
                                run_phase)
from cuvite_amd.parallel import Comm  # noqa: E402
from cuvite_amd.quality import partition_quality  # noqa: E402
from cuvite_amd.refine import refine_coin  # noqa: E402


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


def quality(device: str, backend: str):
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from quality_cases import whole_graph
    dev = torch.device(device)
    graphs = [(n, whole_graph(n)) for n in ("karate", "karate2", "lfr",
                                            "rgg")]
    graphs.append(("rmat14", rmat_graph(14, 16, seed=1)))
    rows = []
    for name, g in graphs:
        dg = single_partition(g.to(dev))
        comm = Comm(dev)
        row = {"graph": name, "nv": g.nv}
        for label, kw in (("louvain", {}),
                          ("level", {"connectivity": "level"}),
                          ("leiden", {"algorithm": "leiden"})):
            res = louvain(dg, comm, LouvainConfig(backend=backend, **kw))
            pq = partition_quality(dg, res.communities, comm,
                                   backend=backend)
            rep = split_disconnected(dg, res.communities, comm,
                                     backend=backend)
            entry = {"exact_q": pq.modularity,
                     "communities": pq.num_communities,
                     "disconnected_in_result": rep.num_disconnected,
                     "phases": res.phases, "iters": res.total_iters}
            if label == "leiden":
                entry["split_by_final_pass"] = \
                    res.connectivity.num_disconnected
                entry["refine_rounds"] = [lv["refine"].rounds
                                          for lv in res.levels
                                          if "refine" in lv]
                entry["subcommunities"] = [lv["refine"].num_subcommunities
                                           for lv in res.levels
                                           if "refine" in lv]
            row[label] = entry
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="out")
    ap.add_argument("--quality", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.quality:
        backend = "torch" if args.device == "cpu" else "hip"
        rows = quality(args.device, backend)
        with open(os.path.join(args.out, "leiden_quality.json"), "w") as f:
            json.dump(rows, f, indent=1)
        return
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

    def refine():
        return refine_partition(dg, labels, comm, halo=halo, backend="hip")

    rep = refine()
    # the first round's inputs: singleton subs, coin-1 vertices move
    st = PhaseState(dg, comm, halo=halo)
    st.use_hip = True
    ghost = exchange_ghost_labels(halo, st.curr_comm)
    dense, _, c_size, c_degree, c_gid = st.densify(ghost)
    inp = MoveInputs(dg.g.rowptr, halo.tails_dense, dg.g.weights, dense,
                     st.v_degree, c_size, c_degree, c_gid, st.constant,
                     local_gid_base=dg.base)
    bid = torch.unique(labels, return_inverse=True)[1].to(torch.int32)
    coin = refine_coin(c_gid, 0)
    minus1 = torch.full((1,), -1, dtype=torch.int32, device=dev)
    mover_bound = torch.where(coin, bid, minus1)
    cand_bound = torch.where(coin, minus1, bid)
    result = {
        "scale": args.scale, "edgefactor": args.edgefactor, "nv": dg.nv,
        "ne_directed": dg.ne, "phase0_sweeps": iters,
        "communities": rep.num_communities,
        "subcommunities": rep.num_subcommunities, "rounds": rep.rounds,
        "moved_per_round": rep.moved_per_round,
        "first_round_movers": int(coin.sum()),
        "hubs": int(ops._buckets_for(dg.g.rowptr)[1].numel()),
        "refine_round": _time(lambda: ops.refine_move(inp, mover_bound,
                                                      cand_bound)),
        "local_move_sweep": _time(lambda: ops.local_move(inp)),
        "refine_partition": _time(refine, warmup=1, reps=5),
    }
    with open(os.path.join(args.out, "leiden_timing.json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps(result, indent=1))


if __name__ == "__main__":
    main()
