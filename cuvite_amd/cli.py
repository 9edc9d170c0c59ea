"""Command-line driver: the MI355X-native equivalent of the reference's
`graphClustering` binary (main.cpp:63-585, 587-712).

Flag surface mirrors the reference's getopt string "f:bc:od:r:t:a:ig:zpn:e:s:j"
with the same semantics, plus long-form extras for the MI355X build (R-MAT
generation, device/backend selection). Distributed runs launch one process
per GPU via `torch.distributed.run` (RCCL over xGMI on a GPU node, gloo on
CPU); single-process runs need no launcher.

Examples:
    python -m cuvite_amd -f karate.bin -c 8 -i
    python -m cuvite_amd -n 16384 -e 5 -o
    python -m cuvite_amd --karate --resolution 2 --exact-modularity
    torchrun --standalone --nproc-per-node 8 -m cuvite_amd --rmat 26
"""

from __future__ import annotations

import argparse
import math
import sys
import time

import torch

from .compare import compare_communities
from .connectivity import split_disconnected
from .generators import (rgg_dist_graph, rmat_dist_graph, karate_graph,
                         lfr_dist_graph)
from .graph import DistGraph, Graph, Partition
from .io import (load_dist_graph, load_ground_truth, write_communities,
                 write_dist_graph)
from .louvain import LouvainConfig, louvain
from .parallel import Comm, init_from_env
from .quality import partition_quality
from .utils.stats import print_dist_stats


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(
        prog="cuvite_amd",
        description="Distributed Louvain community detection on MI355X "
                    "(flag-compatible with the reference graphClustering; "
                    "ref main.cpp:587-712)")
    ap.add_argument("-f", dest="input", metavar="FILE", default="",
                    help="input binary graph (Vite format)")
    ap.add_argument("-b", dest="balanced", action="store_true",
                    help="edge-balanced 1-D partition for file inputs")
    ap.add_argument("-c", dest="coloring", metavar="NCOLORS", type=int,
                    default=0, help="coloring-ordered moves, sync per color")
    ap.add_argument("-d", dest="ordering", metavar="NCOLORS", type=int,
                    default=0, help="color-ordered moves, no per-color sync")
    ap.add_argument("-o", dest="output", action="store_true",
                    help="write <input>.communities")
    ap.add_argument("-r", dest="ranks_per_node", metavar="N", type=int,
                    default=1, help="I/O aggregator hint (accepted; POSIX "
                    "pread per rank needs no aggregation)")
    ap.add_argument("-t", dest="early_term", metavar="TYPE", type=int,
                    default=0, help="early termination type 1-4")
    ap.add_argument("-a", dest="et_alpha", metavar="ALPHA", type=float,
                    default=1.0, help="early termination alpha (types 2/4)")
    ap.add_argument("-i", dest="threshold_cycling", action="store_true",
                    help="threshold cycling across phases")
    ap.add_argument("-g", dest="ground_truth", metavar="FILE", default="",
                    help="ground-truth community file for comparison")
    ap.add_argument("-z", dest="one_based", action="store_true",
                    help="ground-truth file is 1-based")
    ap.add_argument("-p", dest="one_phase", action="store_true",
                    help="run a single Louvain phase")
    ap.add_argument("-n", dest="gen_nv", metavar="NV", type=int, default=0,
                    help="generate an in-memory RGG with NV vertices")
    ap.add_argument("-e", dest="random_edge_percent", metavar="PCT",
                    type=float, default=0.0,
                    help="add PCT%% random edges to the generated graph")
    ap.add_argument("-s", dest="gen_out", metavar="FILE", default="",
                    help="write the generated graph to FILE (Vite binary)")
    ap.add_argument("-j", dest="just_process", action="store_true",
                    help="load/generate the graph, print stats, exit")
    # MI355X-native extras
    ap.add_argument("--rmat", metavar="SCALE", type=int, default=0,
                    help="generate an R-MAT graph of 2^SCALE vertices")
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--karate", action="store_true",
                    help="use the built-in Zachary karate club graph")
    ap.add_argument("--lfr", metavar="NV", type=int, default=0,
                    help="generate an LFR-style benchmark with NV vertices "
                    "and planted ground-truth communities")
    ap.add_argument("--mu", type=float, default=0.4,
                    help="LFR mixing parameter")
    ap.add_argument("--device", choices=["auto", "cpu", "cuda"],
                    default="auto")
    ap.add_argument("--backend", choices=["auto", "hip", "torch"],
                    default="auto", help="local-move backend")
    ap.add_argument("--vertex-order", choices=["natural", "degree"],
                    default="natural",
                    help="degree: isomorphic per-rank degree-descending "
                         "relabeling before clustering (hub-label locality, "
                         "+23%% at R-MAT s26 on MI355X); outputs are mapped "
                         "back to the input vertex order")
    ap.add_argument("--threshold", type=float, default=1.0e-6)
    ap.add_argument("--max-phases", type=int, default=0,
                    help="cap the number of phases (0 = reference default)")
    ap.add_argument("--diag-files", action="store_true",
                    help="write per-rank diagnostics to dat.out.<rank> "
                    "instead of stdout (ref main.cpp:101-110)")
    ap.add_argument("--verbose", action="store_true",
                    help="per-iteration modularity + timing breakdown "
                    "(ref PRINT_TIMEDS, louvain_cuda.cu:2380-2730)")
    ap.add_argument("--unit-weights", action="store_true",
                    help="force all edge weights to 1.0 for file inputs "
                    "(ref SET_EDGE_WEIGHTS_TO_ONE, distgraph.cpp:200-202)")
    ap.add_argument("--score-communities", metavar="FILE", default="",
                    help="print the exact modularity of the partition in "
                    "FILE (a -o dump or a ground-truth file; -z applies) on "
                    "this graph and exit without clustering")
    ap.add_argument("--init-communities", metavar="FILE", default="",
                    help="warm start: begin clustering from the partition "
                    "in FILE instead of singletons (-z applies)")
    ap.add_argument("--update-edges", metavar="FILE", action="append",
                    default=[],
                    help="dynamic update: the graph given by -f or a "
                    "generator is the OLD graph, --init-communities its "
                    "partition; FILE holds the edge changes, one per line, "
                    "'a u v [w]' to add and 'd u v' to delete (0-based ids, "
                    "# comments). Phase 0 then sweeps only the affected "
                    "vertices and what their moves reach. May be given "
                    "several times: the files are applied in order, every "
                    "run starts from the partition the one before returned, "
                    "and -o, --exact-modularity and --check-connected act "
                    "on the last result")
    ap.add_argument("--exact-modularity", action="store_true",
                    help="after the run, print the exact modularity of the "
                    "returned partition (\"Final modularity\" is the "
                    "convergence estimate)")
    ap.add_argument("--connectivity", choices=["final", "level"],
                    default="off",
                    help="final: split the returned communities into their "
                    "connected components (never lowers the exact "
                    "modularity); level: split every phase's communities "
                    "before coarsening (all communities connected; the "
                    "exact modularity may end higher or lower)")
    ap.add_argument("--leiden", action="store_true",
                    help="Leiden mode: refine every phase's communities "
                    "into connected sub-communities before coarsening and "
                    "start the next phase from the parent communities; the "
                    "result always passes through the final split "
                    "(--connectivity final is implied, level is rejected; "
                    "-p skips refinement)")
    ap.add_argument("--vcycle", action="store_true",
                    help="keep every level on the way down and refine the "
                    "partition level by level on the way back up to the "
                    "input graph (never lowers the exact modularity; costs "
                    "the memory of the kept levels; not with --leiden or "
                    "--connectivity level)")
    ap.add_argument("--resolution", metavar="G", type=float, default=None,
                    help="resolution gamma of the modularity that is "
                    "optimised and reported, Q = sum_c [in_c/2m - G "
                    "(a_c/2m)^2] (default 1): above 1 more and smaller "
                    "communities, below 1 fewer and larger ones. Applies to "
                    "the run in every mode and to --score-communities, "
                    "--init-communities, --exact-modularity and "
                    "--update-edges")
    ap.add_argument("--check-connected", action="store_true",
                    help="print how many communities of the partition (the "
                    "returned one, or the one --score-communities reads) "
                    "are not connected, and into how many components they "
                    "fall")
    ap.add_argument("--stats", action="store_true",
                    help="print the graph distribution table "
                    "(ref printStats, distgraph.hpp:100-149)")
    return ap


def validate(args, world: int):
    if args.coloring and args.ordering:
        sys.exit("Cannot enable both -c and -d")
    if args.one_phase and args.threshold_cycling:
        sys.exit("Cannot enable both -p and -i")
    if args.leiden and args.connectivity == "level":
        sys.exit("Cannot enable both --leiden and --connectivity level")
    if args.vcycle and (args.leiden or args.connectivity == "level"):
        sys.exit("Cannot combine --vcycle with --leiden or --connectivity "
                 "level")
    if args.update_edges:
        if not args.init_communities:
            sys.exit("--update-edges needs --init-communities")
        if args.score_communities:
            sys.exit("--update-edges does not combine with "
                     "--score-communities")
        if (args.coloring or args.ordering or args.early_term
                or args.threshold_cycling):
            sys.exit("--update-edges cannot be combined with -c, -d, -t "
                     "or -i")
    if args.resolution is not None and not (
            math.isfinite(args.resolution) and args.resolution > 0.0):
        sys.exit("--resolution must be a finite number > 0")
    if args.early_term and not 1 <= args.early_term <= 4:
        sys.exit("-t must be 1..4")
    if args.early_term in (2, 4) and not 0.0 <= args.et_alpha <= 1.0:
        sys.exit("-a must be in [0,1]")
    n_sources = sum(bool(x) for x in
                    (args.input, args.gen_nv, args.rmat, args.karate,
                     args.lfr))
    if n_sources != 1:
        sys.exit("Specify exactly one graph source: -f FILE, -n NV, "
                 "--rmat SCALE, --lfr NV, or --karate")
    if args.random_edge_percent and not args.gen_nv:
        sys.exit("-e needs -n (generated graph)")
    if args.gen_nv and args.gen_nv % world != 0:
        sys.exit("-n NV must be divisible by the process count")


def _ingest(args, comm: Comm) -> DistGraph:
    dev = comm.device
    wdtype = torch.float64
    if args.input:
        return load_dist_graph(args.input, comm.rank, comm.world,
                               balanced=args.balanced,
                               unit_weights=args.unit_weights,
                               weight_dtype=wdtype).to(dev)
    if args.karate:
        g = karate_graph(wdtype)
        part = Partition.contiguous(g.nv, comm.world)
        # re-slice the single CSR by partition for multi-rank runs
        if comm.world == 1:
            return DistGraph(g, part, comm.rank).to(dev)
        base, bound = int(part.parts[comm.rank]), int(part.parts[comm.rank + 1])
        e0, e1 = int(g.rowptr[base]), int(g.rowptr[bound])
        lg = Graph(g.rowptr[base:bound + 1] - g.rowptr[base],
                   g.tails[e0:e1], g.weights[e0:e1])
        return DistGraph(lg, part, comm.rank).to(dev)
    if args.gen_nv:
        dg = rgg_dist_graph(args.gen_nv, comm.rank, comm.world,
                            seed=args.seed,
                            random_edge_percent=args.random_edge_percent,
                            weight_dtype=wdtype)
        if args.gen_out:
            write_dist_graph_collect(args.gen_out, dg, comm)
        return dg.to(dev)
    if args.lfr:
        dg, truth = lfr_dist_graph(args.lfr, comm.rank, comm.world,
                                   mu=args.mu, seed=args.seed, device=dev)
        args._lfr_truth = truth
        return dg
    # --rmat
    return rmat_dist_graph(args.rmat, args.edgefactor, args.seed, comm, dev,
                           weight_dtype=wdtype)


def _load_partition_slice(path: str, args, dg: DistGraph) -> torch.Tensor:
    """This rank's slice of the partition in `path`, in INPUT vertex order.
    Every rank reads the whole file, so every rank takes the same exit on a
    bad one. Label values are compacted to [0, k): ground-truth files with
    ids >= N or with gaps then satisfy the [0, nv_global) label contract."""
    import numpy as np
    try:
        lab = load_ground_truth(path, zero_based=not args.one_based)
    except FileNotFoundError:
        sys.exit(f"Error opening community file: {path}")
    if lab.numel() != dg.nv_global:
        sys.exit(f"Community file {path} has {lab.numel()} entries; the "
                 f"graph has {dg.nv_global} vertices")
    _, inv = np.unique(lab.numpy(), return_inverse=True)
    inv = torch.from_numpy(inv.astype(np.int64).reshape(-1))
    return inv[dg.base:dg.bound].to(dg.g.device)


def _load_edge_batch(path: str, nv_global: int):
    """The edge batch in `path`: lines 'a u v [w]' (add, weight 1 if absent)
    and 'd u v' (delete), 0-based ids, '#' starts a comment. Every rank reads
    the whole file, so every rank takes the same exit on a bad one."""
    from .dynamic import EdgeBatch
    ins, dels = [], []
    try:
        with open(path) as f:
            lines = f.readlines()
    except FileNotFoundError:
        sys.exit(f"Error opening edge update file: {path}")
    for no, line in enumerate(lines, 1):
        tok = line.split("#", 1)[0].split()
        if not tok:
            continue
        try:
            if tok[0] == "a" and len(tok) in (3, 4):
                ins.append((int(tok[1]), int(tok[2]),
                            float(tok[3]) if len(tok) == 4 else 1.0))
            elif tok[0] == "d" and len(tok) == 3:
                dels.append((int(tok[1]), int(tok[2])))
            else:
                raise ValueError
            u, v = int(tok[1]), int(tok[2])
            if not (0 <= u < nv_global and 0 <= v < nv_global):
                raise ValueError
        except ValueError:
            sys.exit(f"{path}:{no}: expected 'a u v [w]' or 'd u v' with "
                     f"vertex ids in [0, {nv_global})")
    i64 = torch.int64
    return EdgeBatch(
        torch.tensor([e[0] for e in ins], dtype=i64),
        torch.tensor([e[1] for e in ins], dtype=i64),
        torch.tensor([e[2] for e in ins], dtype=torch.float64),
        torch.tensor([e[0] for e in dels], dtype=i64),
        torch.tensor([e[1] for e in dels], dtype=i64))


def _print_connectivity(dg: DistGraph, labels: torch.Tensor, comm: Comm,
                        backend: str):
    """The --check-connected line for `labels` on `dg` (collective)."""
    rep = split_disconnected(dg, labels, comm, backend=backend)
    if comm.rank == 0:
        print(f"Connectivity: communities={rep.num_communities} "
              f"disconnected={rep.num_disconnected} "
              f"components={rep.num_components}")


def write_dist_graph_collect(path: str, dg: DistGraph, comm: Comm):
    """Root-gathers shards and writes one Vite binary (ref writeGraph,
    distgraph.cpp:936-1014; cold path, host-side)."""
    dev = comm.device
    rp = comm.gather_cat(dg.g.rowptr.to(dev), root=0)
    tl = comm.gather_cat(dg.g.tails.to(dev), root=0)
    wt = comm.gather_cat(dg.g.weights.to(dev), root=0)
    if comm.rank == 0:
        shards = []
        vo = 0
        eo = 0
        for p in range(comm.world):
            nvp = dg.partition.nv_local(p)
            rpp = rp[vo:vo + nvp + 1].cpu()
            nep = int(rpp[-1])
            shards.append(DistGraph(
                Graph(rpp, tl[eo:eo + nep].cpu(), wt[eo:eo + nep].cpu()),
                dg.partition, p))
            vo += nvp + 1
            eo += nep
        write_dist_graph(path, shards)
        print(f"Wrote generated graph to {path}")


def _cluster(args, comm: Comm, cfg: LouvainConfig, dg: DistGraph,
             init_labels, init_frontier, ne_global: float):
    """One clustering run and its report lines: the optional degree
    relabelling, the "Initial partition" line, louvain, and rank 0's summary.
    Returns (result, the graph that was clustered, vo_inv, vo_gmap); the two
    maps are None unless --vertex-order degree relabelled the graph."""
    gamma = cfg.resolution
    vo_inv = None     # new local pos -> old local pos (inverse applied later)
    vo_gmap = None    # old gid -> new gid
    if args.vertex_order == "degree":
        from .generators import degree_sort_dist
        dg, vo_order, vo_gmap = degree_sort_dist(dg, comm, return_maps=True)
        vo_inv = torch.empty_like(vo_order)
        vo_inv[vo_order] = torch.arange(vo_order.numel(),
                                        device=vo_order.device)

    if init_labels is not None:
        if vo_inv is not None:
            # relabelled local position p holds input-order vertex
            # vo_order[p]; community ids are opaque, so values stay
            init_labels = init_labels[vo_order]
            if init_frontier is not None:
                init_frontier = init_frontier[vo_order]
        pq = partition_quality(dg, init_labels, comm, backend=args.backend,
                               resolution=gamma)
        if comm.rank == 0:
            print(f"Initial partition: modularity={pq.modularity:.15g} "
                  f"communities={pq.num_communities}")

    comm.barrier()
    t0 = time.perf_counter()
    res = louvain(dg, comm, cfg, init_labels=init_labels,
                  init_frontier=init_frontier)
    comm.barrier()
    t_total = time.perf_counter() - t0

    if comm.rank == 0:
        fr = res.levels[0].get("frontier") if res.levels else None
        if fr is not None:
            # against what as many full sweeps would have evaluated
            print(f"Frontier phase: sweeps={fr.sweeps} "
                  f"evaluated={fr.evaluated} of {fr.sweeps * dg.nv_global}")
        for lvl, q in enumerate(res.modularity_per_level):
            print(f"Level {lvl}: modularity = {q:.6f}")
        for lvl, entry in enumerate(res.levels):
            rep = entry.get("refine")
            if rep is not None:
                print(f"Refinement: level={lvl} "
                      f"communities={rep.num_communities} "
                      f"subcommunities={rep.num_subcommunities} "
                      f"rounds={rep.rounds}")
        for lv in res.vcycle or []:
            print(f"V-cycle: level={lv.level} vertices={lv.nv_global} "
                  f"boundary={lv.boundary} sweeps={lv.sweeps} "
                  f"evaluated={lv.evaluated} moved={lv.moved} "
                  f"Q={lv.q_before:.15g}->{lv.q_after:.15g}")
        if args.leiden and res.connectivity is not None:
            print(f"Final split: communities="
                  f"{res.connectivity.num_communities} "
                  f"disconnected={res.connectivity.num_disconnected} "
                  f"components={res.connectivity.num_components}")
        # TEPS following the reference definition (main.cpp:448,509) with
        # one fix: the reference multiplies each level's ne by the CUMULATIVE
        # iteration count (inflating later levels); we use the original ne x
        # total iterations, which is conservative (coarse levels are smaller)
        teps = ne_global * res.total_iters / t_total if t_total > 0 else 0.0
        print(f"Final modularity: {res.modularity:.6f}")
        print(f"Phases: {res.phases}  Iterations: {res.total_iters}")
        print(f"Coloring time: {res.times.get('coloring', 0.0):.3f}s")
        print(f"Clustering time: {res.times.get('clustering', 0.0):.3f}s")
        print(f"Rebuild time: {res.times.get('rebuild', 0.0):.3f}s")
        print(f"Total time: {t_total:.3f}s  TEPS: {teps:.4g}")
        # memory observability (ref getrusage ru_maxrss, main.cpp:142-150)
        import resource
        rss_mb = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1024
        if comm.device.type == "cuda":
            hbm_gb = torch.cuda.max_memory_allocated() / (1 << 30)
            print(f"Peak memory: host rss {rss_mb:.0f} MB, "
                  f"device {hbm_gb:.2f} GB")
        else:
            print(f"Peak memory: host rss {rss_mb:.0f} MB")
    return res, dg, vo_inv, vo_gmap


def _input_order(labels: torch.Tensor, vo_inv, vo_gmap) -> torch.Tensor:
    """Labels of a clustered graph in the INPUT vertex order and id space:
    original local vertex v sits at relabelled position vo_inv[v]; label
    values (new gids) map through the global inverse."""
    if vo_inv is None:
        return labels
    labels = labels[vo_inv]
    inv_gmap = torch.empty_like(vo_gmap)
    inv_gmap[vo_gmap] = torch.arange(vo_gmap.numel(), device=vo_gmap.device)
    return inv_gmap[labels]


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    comm = init_from_env(prefer=args.device)
    validate(args, comm.world)
    if args.diag_files:
        # reference default: per-rank dat.out.<rank> diagnostic files
        sys.stdout = open(f"dat.out.{comm.rank}", "w")

    t0 = time.perf_counter()
    try:
        dg = _ingest(args, comm)
    except FileNotFoundError as e:
        sys.exit(f"Error opening graph file: {e.filename}")
    t_ingest = time.perf_counter() - t0
    ne_global = comm.allreduce_scalar(float(dg.ne))
    if comm.rank == 0:
        print(f"Graph: nv={dg.nv_global} ne(directed)={int(ne_global)} "
              f"ranks={comm.world} device={comm.device.type} "
              f"ingest={t_ingest:.3f}s")
    if args.stats or args.just_process:
        print_dist_stats(dg, comm)
    if args.just_process:
        return 0
    gamma = 1.0 if args.resolution is None else args.resolution
    if args.resolution is not None and comm.rank == 0:
        print(f"Resolution: {gamma:g}")

    if args.score_communities:
        part_labels = _load_partition_slice(args.score_communities, args, dg)
        pq = partition_quality(dg, part_labels, comm, backend=args.backend,
                               resolution=gamma)
        if comm.rank == 0:
            print(f"Partition {args.score_communities}: "
                  f"modularity={pq.modularity:.15g} "
                  f"communities={pq.num_communities} "
                  f"coverage={pq.coverage:.15g}")
        if args.check_connected:
            _print_connectivity(dg, part_labels, comm, args.backend)
        return 0
    init_labels = None
    if args.init_communities:
        init_labels = _load_partition_slice(args.init_communities, args, dg)
    cfg = LouvainConfig(
        threshold=args.threshold,
        threshold_scaling=args.threshold_cycling,
        one_phase=args.one_phase,
        early_term=args.early_term,
        et_delta=args.et_alpha,
        coloring=args.coloring > 0,
        ordering=args.ordering > 0,
        max_colors=max(args.coloring, args.ordering) or 8,
        backend=args.backend,
        verbose=args.verbose,
        connectivity=args.connectivity,
        algorithm="leiden" if args.leiden else "louvain",
        vcycle=args.vcycle,
        resolution=gamma,
    )
    if args.max_phases:
        cfg.max_phases = args.max_phases

    # every update file is read before any work is done. Rank 0 passes the
    # whole batch, the other ranks an empty share
    batches = [(path, _load_edge_batch(path, dg.nv_global))
               for path in args.update_edges]
    runs = batches or [None]
    for k, item in enumerate(runs, 1):
        init_frontier = None
        if item is not None:
            # the graph so far is the old one
            from .dynamic import (EdgeBatch, affected_vertices,
                                  apply_edge_batch)
            path, batch = item
            if len(runs) > 1 and comm.rank == 0:
                print(f"Batch {k}/{len(runs)}: {path}")
            n_ins, n_del = batch.ins_src.numel(), batch.del_src.numel()
            share = batch if comm.rank == 0 else EdgeBatch.empty()
            try:
                dg = apply_edge_batch(dg, comm, share)
            except ValueError as e:
                sys.exit(f"{path}: {e}")
            init_frontier = affected_vertices(dg, comm, init_labels, share)
            n_aff = int(comm.allreduce_scalar(float(init_frontier.sum())))
            if comm.rank == 0:
                print(f"Edge batch: inserted={n_ins} deleted={n_del} "
                      f"affected={n_aff}")
        res, run_dg, vo_inv, vo_gmap = _cluster(
            args, comm, cfg, dg, init_labels, init_frontier, ne_global)
        if k < len(runs):
            # the next batch starts from this result, in input vertex order
            init_labels = _input_order(res.communities, vo_inv, vo_gmap)
    dg = run_dg  # what the last run clustered

    if args.exact_modularity:
        # res.communities labels the graph that was clustered (after
        # --vertex-order degree the relabelled, isomorphic one)
        pq = partition_quality(dg, res.communities, comm,
                               backend=args.backend, resolution=gamma)
        if comm.rank == 0:
            print(f"Exact modularity: {pq.modularity:.15g} "
                  f"({pq.num_communities} communities)")

    if args.check_connected:
        _print_connectivity(dg, res.communities, comm, args.backend)

    builtin_truth = getattr(args, "_lfr_truth", None)
    if args.output or args.ground_truth or builtin_truth is not None:
        # map back to the INPUT vertex order so dumps match the input id
        # space
        final_comm = _input_order(res.communities, vo_inv, vo_gmap)
        # gather final communities to root in vertex order
        allc = comm.gather_cat(final_comm.to(comm.device), root=0)
        if comm.rank == 0:
            allc = allc.cpu()
            if args.output:
                out_path = (args.input or args.gen_out or "graph") + \
                    ".communities"
                write_communities(out_path, allc)
                print(f"Wrote communities to {out_path}")
            if args.ground_truth or builtin_truth is not None:
                try:
                    truth = builtin_truth if builtin_truth is not None else \
                        load_ground_truth(args.ground_truth,
                                          zero_based=not args.one_based)
                except FileNotFoundError as e:
                    sys.exit(f"Error opening ground truth file: {e.filename}")
                m = compare_communities(truth, allc)
                print(f"Ground truth: precision={m['precision']:.4f} "
                      f"recall={m['recall']:.4f} f-score={m['f_score']:.4f} "
                      f"f-mean={m['f_mean']:.4f} "
                      f"gini(pred)={m['gini_pred']:.4f} "
                      f"gini(truth)={m['gini_truth']:.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
