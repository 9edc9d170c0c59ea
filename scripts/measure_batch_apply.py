"""Time the application of an edge batch to the CSR: the device path
(ops.apply_batch) against the whole-graph rebuild (CUVITE_BATCH_DEVICE=0),
and a stream of three batches split into its parts.

    python scripts/measure_batch_apply.py --scale 22 --out DIR
    python scripts/measure_batch_apply.py --scale 26 --apply-only --out DIR

Same graph as scripts/measure_dynamic.py (R-MAT, edge factor 16, fp64,
degree-sorted relabelling, one GPU) and the same batch recipe (seed 7). For
every fraction apply_edge_batch is run both ways, alternating in one process,
each call between two device synchronisations, 1 warm-up, median of `--reps`
(default 5) with min..max. Beside the times: the bytes the copy has to move
(old plus new CSR), the bytes/s the device path reaches on them, and the
share of the `ne` entries that lie in touched rows. Then update_stream's
loop over three batches (the thirds of one 0.3 % recipe batch) from the
converged cold run's partition, with apply / affected / run timed apart.

--apply-only: no rebuild, no stream, no relabelling and a batch drawn from
sampled rows, so that nothing but the device path runs over the graph: the
one mode that fits a graph past 2^31 edges. The result goes to stdout and
DIR/batch_apply_s<scale>.json. Needs a GPU."""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cuvite_amd import ops  # noqa: E402
from cuvite_amd.dynamic import (EdgeBatch, StreamStep,  # noqa: E402
                                affected_vertices, apply_edge_batch)
from cuvite_amd.generators import degree_sort_dist, rmat_dist_graph  # noqa: E402
from cuvite_amd.louvain import LouvainConfig, louvain  # noqa: E402
from cuvite_amd.parallel import Comm  # noqa: E402

from measure_dynamic import recipe_batch, stats  # noqa: E402


def sampled_batch(dg, k):
    """k deletions (the first stored entry of k sampled rows, self-loops
    skipped) and k random insertions; batch-sized work only."""
    gen = torch.Generator().manual_seed(7)
    g = dg.g
    rows = torch.randint(0, g.nv, (k,), generator=gen).to(g.device)
    rows = rows[(g.rowptr[rows + 1] - g.rowptr[rows]) > 0]
    dst = g.tails[g.rowptr[rows]]
    m = rows != dst
    ins_u = torch.randint(0, g.nv, (k,), generator=gen)
    ins_v = torch.randint(0, g.nv, (k,), generator=gen)
    w = torch.rand(k, generator=gen, dtype=torch.float64)
    keep = ins_u != ins_v
    return EdgeBatch(ins_u[keep], ins_v[keep], w[keep], rows[m].cpu(),
                     dst[m].cpu())


def touched_entries(dg, batch):
    """Entries of the rows the batch touches (one rank: every endpoint)."""
    rows = torch.unique(torch.cat([batch.ins_src, batch.ins_dst,
                                   batch.del_src, batch.del_dst])).to(
        dg.g.device)
    return int((dg.g.rowptr[rows + 1] - dg.g.rowptr[rows]).sum()), \
        int(rows.numel())


def csr_bytes(g):
    return g.rowptr.numel() * 8 + g.ne * (8 + g.weights.element_size())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def split(batch, k, n):
    return EdgeBatch(batch.ins_src[k::n], batch.ins_dst[k::n],
                     batch.ins_w[k::n], batch.del_src[k::n],
                     batch.del_dst[k::n])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--edgefactor", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--fracs", default="0.0001,0.001,0.01")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--apply-only", action="store_true")
    ap.add_argument("--out", default="out")
    args = ap.parse_args()
    assert torch.cuda.is_available() and ops.available(), \
        "needs a GPU and the built HIP extension"
    dev = torch.device("cuda:0")
    comm = Comm(dev)
    old = rmat_dist_graph(args.scale, args.edgefactor, args.seed, comm, dev,
                          weight_dtype=torch.float64)
    result = {"scale": args.scale, "edgefactor": args.edgefactor,
              "nv": old.nv, "ne_directed": old.ne, "span": ops.batch_span(),
              "batches": []}
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, f"batch_apply_s{args.scale}.json")

    if args.apply_only:
        batch = sampled_batch(old, 100000)
        n_t, n_rows = touched_entries(old, batch)
        new, ms = timed(lambda: apply_edge_batch(old, comm, batch))
        # the batch's own entries, read back from the new graph
        g = new.g
        u, v = batch.ins_src[:1000].to(dev), batch.ins_dst[:1000].to(dev)
        found = sum(bool((g.tails[g.rowptr[a]:g.rowptr[a + 1]] == b).any())
                    for a, b in zip(u.tolist(), v.tolist()))
        entry = {"inserted": int(batch.ins_src.numel()),
                 "deleted": int(batch.del_src.numel()),
                 "touched_rows": n_rows, "touched_entries": n_t,
                 "touched_share": n_t / old.ne, "device_ms_first_call": ms,
                 "ne_after": new.ne, "past_2_31": new.ne > 2 ** 31,
                 "inserted_found_of_1000": found,
                 "copy_bytes": csr_bytes(old.g) + csr_bytes(new.g)}
        print(json.dumps(entry), flush=True)
        result["batches"].append(entry)
        with open(path, "w") as f:
            json.dump(result, f, indent=1)
        return

    old = degree_sort_dist(old, comm)
    for frac in [float(x) for x in args.fracs.split(",")]:
        batch = recipe_batch(old, frac)
        n_t, n_rows = touched_entries(old, batch)
        ms = {"device": [], "rebuild": []}
        ne_after = {}
        for rnd in range(args.reps + 1):  # the first round warms up
            for name, knob in (("device", "1"), ("rebuild", "0")):
                os.environ["CUVITE_BATCH_DEVICE"] = knob
                new, t = timed(lambda: apply_edge_batch(old, comm, batch))
                ne_after[name] = new.ne
                nbytes = csr_bytes(old.g) + csr_bytes(new.g)
                del new
                if rnd:
                    ms[name].append(t)
        os.environ.pop("CUVITE_BATCH_DEVICE")
        assert ne_after["device"] == ne_after["rebuild"]
        med = statistics.median(ms["device"])
        entry = {"frac": frac, "inserted": int(batch.ins_src.numel()),
                 "deleted": int(batch.del_src.numel()),
                 "touched_rows": n_rows, "touched_entries": n_t,
                 "touched_share": n_t / old.ne,
                 "device": stats(ms["device"]),
                 "rebuild": stats(ms["rebuild"]),
                 "rebuild_over_device":
                 statistics.median(ms["rebuild"]) / med,
                 "copy_bytes": nbytes,
                 "device_gbytes_per_s": nbytes / (med * 1e-3) / 1e9}
        print(json.dumps(entry), flush=True)
        result["batches"].append(entry)

    with open(path, "w") as f:
        json.dump(result, f, indent=1)

    # a stream of three batches, its parts timed apart
    prev = louvain(old, comm, LouvainConfig(backend="hip")).communities
    ops.clear_phase_caches()
    whole = recipe_batch(old, 0.003)
    # the recipe lists a pair once per parallel copy and a deletion removes
    # every copy: each pair goes to one batch only
    dkey = torch.unique(whole.del_src * old.nv + whole.del_dst)
    whole.del_src = torch.div(dkey, old.nv, rounding_mode="floor")
    whole.del_dst = dkey - whole.del_src * old.nv
    shares = [split(whole, k, 3) for k in range(3)]
    # the loop update_stream runs (tests/test_batch_apply.py holds the two
    # equal step for step), with each part between two synchronisations
    parts = {"apply": [], "affected": [], "run": []}
    cfg = LouvainConfig(backend="hip")
    dg, labels, steps = old, prev, []
    torch.cuda.synchronize()
    t_start = time.perf_counter()
    for share in shares:
        dg, t = timed(lambda: apply_edge_batch(dg, comm, share))
        parts["apply"].append(t)
        mask, t = timed(lambda: affected_vertices(dg, comm, labels, share))
        parts["affected"].append(t)
        res, t = timed(lambda: louvain(dg, comm, cfg, init_labels=labels,
                                       init_frontier=mask))
        parts["run"].append(t)
        steps.append(StreamStep(int(share.ins_src.numel()),
                                int(share.del_src.numel()), int(mask.sum()),
                                res))
        labels = res.communities
    total = (time.perf_counter() - t_start) * 1e3
    result["stream"] = {
        "total_ms": total, "parts_ms": parts,
        "steps": [{"inserted": s.inserted, "deleted": s.deleted,
                   "affected": s.affected, "phases": s.result.phases,
                   "iters": s.result.total_iters,
                   "frontier_sweeps": s.result.levels[0]["frontier"].sweeps}
                  for s in steps]}
    print(json.dumps(result["stream"]), flush=True)
    with open(path, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
