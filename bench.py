#!/usr/bin/env python3
"""Flagship benchmark: Louvain local-moving iterations on an R-MAT graph.

Metric (BASELINE.json): Louvain edges/sec (TEPS: global directed edge count x
timed iterations / elapsed, the reference's definition, main.cpp:448,509) plus
the final modularity, on R-MAT scale-26 with random edge weights, at 1-8
MI355X GPUs (strong scaling: the graph is fixed, ranks each own a 1-D slice).

One "step" = one full distributed local-moving iteration: ghost-label exchange
(RCCL p2p) + remote community-info fetch + HIP local-move kernel + community
delta push + modularity allreduce. Nothing is skipped inside the timed region.

Launch (the driver does this):
  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
      --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

A plain run only sets up, warms up, times the K steps and prints the result
line. --full adds everything else the benchmark measures (at world=1: the
converged multi-phase Louvain behind the "final modularity" half of the
metric). --dump-outputs DIR writes what the last timed step computed as
DIR/<name>.npy so two builds can be compared output for output.
"""

import argparse
import json
import os
import sys
import time

# expandable segments kill the fragmentation that OOM'd the s27 converged
# run at 254 GB allocated + 24 GB reserved-but-unallocated; must be set
# before torch initializes its allocator (all naming generations, ROCm
# reads the CUDA/HIP aliases)
for _k in ("PYTORCH_ALLOC_CONF", "PYTORCH_CUDA_ALLOC_CONF",
           "PYTORCH_HIP_ALLOC_CONF"):
    os.environ.setdefault(_k, "expandable_segments:True")

import torch  # noqa: E402


def _p(msg):
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr,
          flush=True)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cuvite_amd.generators import rmat_dist_graph  # noqa: E402
from cuvite_amd.louvain import (LouvainConfig, PhaseState, _modularity,
                                _one_sweep, _pick_move_fn)  # noqa: E402
from cuvite_amd.parallel import init_from_env  # noqa: E402


_DUMP_SAMPLE = 1 << 20  # per-array element cap: 4 fp64 arrays stay at 32 MB


def _dump_outputs(out_dir, state, target, q, comm, seed):
    """Write what the last timed step handed back: the step's modularity,
    the per-vertex community labels it chose (global ids, exact in fp64),
    the per-vertex weight into the own community, and the per-community
    degree/size aggregates it left behind. Arrays longer than _DUMP_SAMPLE
    are sampled at fixed positions drawn from a CPU generator seeded by
    --seed and the array length only, so two runs with the same arguments
    write the same positions."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    sfx = "" if comm.world == 1 else f"_rank{comm.rank}"
    n = target.numel()
    if n > _DUMP_SAMPLE:
        gen = torch.Generator().manual_seed(seed * 1000003 + n)
        pos = torch.randint(0, n, (_DUMP_SAMPLE,), generator=gen)
        pos = pos.sort().values.to(target.device)
    else:
        pos = None
    arrays = {
        "communities": target,
        "cluster_weight": state.cluster_weight,
        "community_degree": state.local_degree,
        "community_size": state.local_size,
    }
    for name, t in arrays.items():
        if pos is not None:
            t = t[pos]
        np.save(os.path.join(out_dir, f"{name}{sfx}.npy"),
                t.to(torch.float64).cpu().numpy())
    np.save(os.path.join(out_dir, f"modularity{sfx}.npy"),
            np.asarray([q], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=int, default=26)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dtype", choices=["fp64", "fp32"], default="fp64")
    ap.add_argument("--backend", default="auto",
                    help="auto|hip|torch (torch = eager fallback, CPU test only)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region also run everything beyond "
                         "the headline figure (at world=1: the converged "
                         "multi-phase Louvain, reported under config)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's outputs as DIR/*.npy")
    ap.add_argument("--converge", action="store_true",
                    help="also run a full multi-phase Louvain to convergence "
                         "AFTER the timed region and report final modularity "
                         "(what --full turns on at world=1; this forces it "
                         "at any world size)")
    ap.add_argument("--no-converge", action="store_true")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    comm = init_from_env()
    device = comm.device
    wdtype = torch.float64 if args.dtype == "fp64" else torch.float32

    t_gen0 = time.perf_counter()
    _p(f"generating rmat s{args.scale} on {device}")
    dg = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm,
                         device, weight_dtype=wdtype)
    if device.type == "cuda":
        torch.cuda.synchronize()
    _p(f"graph built: nv_local={dg.nv} ne_local={dg.ne}")
    vertex_order = "natural"
    if (device.type == "cuda"
            and os.environ.get("CUVITE_DEGSORT", "1") != "0"):
        # isomorphic per-rank degree-descending relabeling (outside the
        # timed region, declared in config): hub labels pack into per-rank
        # hot prefixes so the per-edge curr_comm gathers hit the XCD L2s.
        # Same edges, same degrees, same modularity landscape; measured
        # +23% at s26 world=1 (profiles/). CUVITE_DEGSORT=0 disables.
        from cuvite_amd.generators import degree_sort_dist
        dg = degree_sort_dist(dg, comm)
        torch.cuda.synchronize()
        vertex_order = "degree"
        _p("degree-sorted relabeling applied")
    ne_global = float(comm.allreduce_scalar(float(dg.ne)))
    t_gen = time.perf_counter() - t_gen0

    cfg = LouvainConfig(backend=args.backend)
    state = PhaseState(dg, comm)
    if device.type == "cuda":
        torch.cuda.synchronize()
    _p("phase state + halo ready")
    state.use_hip = device.type == "cuda" and args.backend in ("auto", "hip")
    move_fn = _pick_move_fn(cfg, device)

    dbg = os.environ.get("CUVITE_PROGRESS")

    def step():
        target = _one_sweep(state, cfg, move_fn, None)
        if dbg and device.type == "cuda":
            torch.cuda.synchronize()
            _p("sweep done")
        q = _modularity(state)
        if dbg and device.type == "cuda":
            torch.cuda.synchronize()
            _p("modularity done")
        state.past_comm, state.curr_comm = state.curr_comm, target
        return q

    for i in range(args.warmup):
        q = step()
        if device.type == "cuda":
            torch.cuda.synchronize()
        _p(f"warmup {i} done q={q:.6f}")

    comm.barrier()
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        q = step()
    if device.type == "cuda":
        torch.cuda.synchronize()
    comm.barrier()
    elapsed = time.perf_counter() - t0
    # max over ranks
    if comm.world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t[0])

    teps = ne_global * args.steps / elapsed

    if args.dump_outputs:
        # step() leaves the labels it chose in state.curr_comm
        _dump_outputs(args.dump_outputs, state, state.curr_comm, q, comm,
                      args.seed)
        _p(f"outputs written to {args.dump_outputs}")

    # Converged full run (outside the timed region): evidences the "final
    # modularity" half of the BASELINE metric. Only with --full, where it is
    # on at world=1; opt-in for multi-GPU (--converge) so the SCALE sweep
    # stays a pure per-iteration measurement.
    conv = None
    do_conv = args.converge or (args.full and comm.world == 1
                                and not args.no_converge
                                and os.environ.get("CUVITE_NO_CONVERGE") != "1")
    if do_conv:
        from cuvite_amd.louvain import louvain
        _p("converged multi-phase run starting")
        # memory handoff for the giant-graph case (s27: the converged run
        # OOM'd twice before this): reuse the timed region's halo for phase
        # 0 (no duplicate 17 GB tails_dense), drop the timed PhaseState, and
        # release the int64 CSR tails (34 GB; ne stays valid via
        # release_tails). The halo travels through a single-ref handoff so
        # louvain() can drop it once phase 0's coarsening is done.
        conv_halo = [state.halo]
        del state, step  # step's closure cell would otherwise keep state
        if device.type == "cuda" and comm.world == 1:
            dg.g.release_tails()
            torch.cuda.empty_cache()
        t0 = time.perf_counter()
        try:
            res = louvain(dg, comm, LouvainConfig(backend=args.backend),
                          halo=conv_halo.pop())
            if device.type == "cuda":
                torch.cuda.synchronize()
            conv_s = time.perf_counter() - t0
            conv = {
                "final_modularity": res.modularity,
                "phases": res.phases,
                "total_iters": res.total_iters,
                "seconds": round(conv_s, 3),
                "teps_converged": res.teps_numerator / conv_s
                if conv_s else None,
                "levels": [{k: (round(v, 6) if isinstance(v, float) else v)
                            for k, v in lv.items()} for lv in res.levels[:12]],
            }
            _p(f"converged: Q={res.modularity:.6f} phases={res.phases} "
               f"iters={res.total_iters} in {conv_s:.1f}s")
        except Exception as e:  # the PRIMARY timed metric must still print
            conv = {"error": f"{type(e).__name__}: {e}"[:300]}
            _p(f"converged run failed: {conv['error']}")
            import traceback
            traceback.print_exc(file=sys.stderr)
            if device.type == "cuda":
                # live-tensor census for memory debugging
                import gc
                sizes = {}
                for o in gc.get_objects():
                    try:
                        if torch.is_tensor(o) and o.is_cuda:
                            k = (tuple(o.shape), str(o.dtype))
                            sizes[k] = sizes.get(k, 0) + \
                                o.numel() * o.element_size()
                    except Exception:
                        pass
                top = sorted(sizes.items(), key=lambda kv: -kv[1])[:15]
                for (shape, dt), b in top:
                    _p(f"live {b/2**30:7.2f} GiB  {dt}  {shape}")
                _p(f"allocated {torch.cuda.memory_allocated()/2**30:.1f} "
                   f"GiB reserved {torch.cuda.memory_reserved()/2**30:.1f}")

    if comm.rank == 0:
        out = {
            "metric": "louvain_edges_per_sec",
            "value": teps,
            "unit": "edges/s",
            "n_gpus": comm.world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1e3,
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic",
            "config": {
                "model": f"louvain-rmat-s{args.scale}-ef{args.edgefactor}",
                "scale": args.scale,
                "edgefactor": args.edgefactor,
                "nv": 1 << args.scale,
                "ne_directed": int(ne_global),
                "modularity_last_step": q,
                "gen_seconds": round(t_gen, 2),
                "parallelism": f"graph1d-p{comm.world}",
                "backend": args.backend,
                "vertex_order": vertex_order,
            },
        }
        if conv is not None:
            out["config"]["converged"] = conv
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
