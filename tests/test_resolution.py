"""The resolution parameter on the CPU oracle: what gamma does to the
partition, exact scoring under gamma, every mode (plain, V-cycle, Leiden,
final split, frontier update) at gamma != 1, the scan, validation, rank
invariance, the CLI, and the precondition of the GPU kernel test (scaling
`constant` changes targets on every kernel route)."""

import dataclasses
import os
import subprocess
import sys

import pytest
import torch

from tests.dist_utils import run_dist

import cuvite_amd
from cuvite_amd import (affected_vertices, apply_edge_batch,
                        partition_quality, resolution_scan,
                        run_frontier_phase)
from cuvite_amd.graph import single_partition
from cuvite_amd.io import write_communities
from cuvite_amd.louvain import (LouvainConfig, PhaseState, _modularity,
                                _one_sweep, _pick_move_fn, louvain)
from cuvite_amd.parallel import Comm
from cuvite_amd.quality import intra_weight_torch

import dynamic_cases as dyc
import resolution_cases as rc
from fused_cases import routes
from quality_cases import cold_run, shard
from vcycle_cases import QUALITY_GRAPHS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def _cfg(gamma, **kw):
    return LouvainConfig(backend="torch", resolution=gamma, **kw)


# ---- what gamma does --------------------------------------------------------

@pytest.mark.parametrize("mode", list(rc.MODES))
def test_clique_ring_gamma_2_returns_the_cliques(mode):
    g = rc.graph("ring32k4")
    res = rc.gamma_run("ring32k4", 2.0, **rc.MODES[mode])
    lab = res.communities
    assert rc.num_communities(lab) == 32
    cliques = lab.view(32, 4)
    assert bool((cliques == cliques[:, :1]).all())
    q2 = partition_quality(single_partition(g), lab, Comm(), backend="torch",
                           resolution=2.0).modularity
    assert abs(q2 - (6.0 / 7.0 - 2.0 / 32.0)) < 1e-12
    assert abs(q2 - 0.794643) < 5e-7


def test_clique_ring_gamma_1_merges_cliques_whole():
    lab = rc.gamma_run("ring32k4", 1.0).communities
    assert rc.num_communities(lab) == 15
    cliques = lab.view(32, 4)
    assert bool((cliques == cliques[:, :1]).all())      # no clique is split
    # and the default config is the gamma = 1 run
    ref = louvain(single_partition(rc.graph("ring32k4")), Comm(),
                  LouvainConfig(backend="torch"))
    assert torch.equal(ref.communities, lab)


def test_karate_community_counts():
    got = {g: rc.num_communities(rc.gamma_run("karate", g).communities)
           for g in rc.GAMMAS}
    assert got == rc.KARATE_COUNTS


def test_rgg_community_count_grows_with_gamma():
    counts = [rc.num_communities(rc.gamma_run("rgg", g).communities)
              for g in rc.GAMMAS]
    print(f"rgg communities over gamma {rc.GAMMAS}: {counts}")
    assert all(a < b for a, b in zip(counts, counts[1:]))


# ---- scoring ----------------------------------------------------------------

def _cold_labels(name):
    if name == "dup":
        return rc.gamma_run("dup", 1.0).communities
    return cold_run(name).communities


@pytest.mark.parametrize("gamma", [0.25, 1.0, 3.5])
@pytest.mark.parametrize("name", ["dup", "karate", "lfr"])
def test_partition_quality_against_brute_force(name, gamma):
    g = rc.graph(name)
    lab = _cold_labels(name)
    dg = single_partition(g)
    pq = partition_quality(dg, lab, Comm(), backend="torch",
                           resolution=gamma)
    brute = rc.brute_q_gamma(g, lab, gamma)
    print(f"{name} gamma {gamma}: {pq.modularity:.15g} brute {brute:.15g}")
    assert abs(pq.modularity - brute) < 1e-12
    assert pq.resolution == gamma
    plain = partition_quality(dg, lab, Comm(), backend="torch")
    # the sums do not depend on gamma; at() rescores from them
    assert pq.degree_sq == plain.degree_sq
    assert (pq.intra_weight, pq.total_weight, pq.coverage,
            pq.num_communities) == (plain.intra_weight, plain.total_weight,
                                    plain.coverage, plain.num_communities)
    assert pq.at(gamma) == pq.modularity
    assert plain.at(gamma) == pq.modularity
    for other in (0.25, 1.0, 3.5):
        fresh = partition_quality(dg, lab, Comm(), backend="torch",
                                  resolution=other)
        assert pq.at(other) == fresh.modularity
    if gamma == 1.0:
        # the same bits as the call without the argument, and as the
        # expression the parent used
        assert pq.modularity == plain.modularity
        c = 1.0 / plain.total_weight
        assert plain.modularity == plain.intra_weight * c \
            - plain.degree_sq * c * c
        assert plain.resolution == 1.0


def test_phase_state_keeps_both_constants():
    dg = single_partition(rc.graph("dup"))
    tw = float(dg.local_degree_sum().sum())
    one = PhaseState(dg, Comm())
    assert one.resolution == 1.0
    assert one.constant == one.inv_2m == 1.0 / tw
    st = PhaseState(dg, Comm(), resolution=3.5)
    assert st.resolution == 3.5 and st.inv_2m == 1.0 / tw
    assert st.constant == 3.5 * (1.0 / tw)
    from cuvite_amd.graph import Graph
    empty = Graph(torch.zeros(4, dtype=torch.int64),
                  torch.empty(0, dtype=torch.int64),
                  torch.empty(0, dtype=torch.float64))
    st0 = PhaseState(single_partition(empty), Comm(), resolution=2.0)
    assert st0.constant == 0.0 and st0.inv_2m == 0.0


@pytest.mark.parametrize("gamma", [0.25, 2.0, 3.5])
def test_sweep_estimate_with_integer_weights(gamma):
    """_modularity(state) after every sweep of a phase: the intra weight
    under the labels the sweep read, the degrees after it, combined as
    Q_gamma."""
    g = rc.graph("dup")
    dg = single_partition(g)
    cfg = _cfg(gamma)
    state = PhaseState(dg, Comm(), resolution=gamma)
    move_fn = _pick_move_fn(cfg, CPU)
    vdeg = dg.local_degree_sum()
    c = 1.0 / float(vdeg.sum())
    t32 = g.tails.to(torch.int32)
    moved = False
    for _ in range(4):
        before = state.curr_comm.clone()
        target = _one_sweep(state, cfg, move_fn, None)
        est = _modularity(state)
        iw = intra_weight_torch(g.rowptr, t32, g.weights, before)
        deg = torch.zeros(g.nv, dtype=torch.float64).index_add_(
            0, target, vdeg)
        full = float(iw.sum()) * c - gamma * float((deg ** 2).sum()) * c * c
        assert abs(est - full) < 1e-12
        moved |= bool((target != before).any())
        state.past_comm, state.curr_comm = state.curr_comm, target
    assert moved


class _Recorder:
    def __init__(self):
        self.begin, self.end = [], []

    def __call__(self, event, **kw):
        getattr(self, event).append(kw)


@pytest.mark.parametrize("gamma", [0.5, 2.0])
def test_frontier_phase_estimate_with_integer_weights(gamma):
    """test_dynamic's estimate check, under gamma."""
    g, _, prev, f0 = dyc.perturbed("dup", 0.3)
    dg = single_partition(g)
    rec = _Recorder()
    _, _, it, _, rep = run_frontier_phase(dg, Comm(), _cfg(gamma),
                                          prev.clone(), f0.clone(),
                                          observe=rec)
    assert len(rec.end) == it >= 1
    vdeg = dg.local_degree_sum()
    c = 1.0 / float(vdeg.sum())
    t32 = g.tails.to(torch.int32)
    for b, e in zip(rec.begin, rec.end):
        iw = intra_weight_torch(g.rowptr, t32, g.weights, b["curr"])
        assert torch.equal(e["cw"], iw)
        deg = torch.zeros(g.nv, dtype=torch.float64).index_add_(
            0, e["target"], vdeg)
        full = float(iw.sum()) * c - gamma * float((deg ** 2).sum()) * c * c
        assert abs(e["estimate"] - full) < 1e-12
    assert rep.estimates == [e["estimate"] for e in rec.end]


# ---- the modes --------------------------------------------------------------

@pytest.mark.parametrize("gamma", [0.25, 0.5, 2.0, 4.0])
@pytest.mark.parametrize("name", QUALITY_GRAPHS)
def test_vcycle_never_lower_and_reports_q_gamma(monkeypatch, name, gamma):
    from cuvite_amd import uncoarsen
    seen = []
    real = uncoarsen.run_uncoarsen_phase

    def spy(dg, comm, cfg, start, halo=None, **kw):
        out = real(dg, comm, cfg, start, halo, **kw)
        seen.append((dg, start.clone(), out[0].clone(), out[2]))
        return out

    monkeypatch.setattr(uncoarsen, "run_uncoarsen_phase", spy)
    res = louvain(single_partition(rc.graph(name)), Comm(),
                  _cfg(gamma, vcycle=True))
    q_plain = rc.q_gamma(name, rc.gamma_run(name, gamma).communities, gamma)
    q_v = rc.q_gamma(name, res.communities, gamma)
    print(f"{name} gamma {gamma}: plain {q_plain:.6f} vcycle {q_v:.6f}")
    assert q_v >= q_plain
    assert len(seen) == len(res.vcycle) >= 1
    for (dg, start, lab, rep), lv in zip(seen, res.vcycle):
        assert rep is lv
        for labels, q in ((start, lv.q_before), (lab, lv.q_after)):
            exact = partition_quality(dg, labels, Comm(), backend="torch",
                                      resolution=gamma).modularity
            assert abs(q - exact) < 1e-12
        assert lv.q_after >= lv.q_before
    for coarse, fine in zip(res.vcycle, res.vcycle[1:]):
        assert abs(fine.q_before - coarse.q_after) < 1e-12
    assert abs(res.vcycle[-1].q_after - q_v) < 1e-12
    # the way down is the plain run's
    assert res.modularity == rc.gamma_run(name, gamma).modularity


@pytest.mark.parametrize("gamma", [0.25, 0.5, 2.0, 4.0])
@pytest.mark.parametrize("name", QUALITY_GRAPHS + ("rmat10u",))
def test_final_split_never_lowers_q_gamma(name, gamma):
    plain = rc.gamma_run(name, gamma)
    res = rc.gamma_run(name, gamma, connectivity="final")
    q_plain = rc.q_gamma(name, plain.communities, gamma)
    q_split = rc.q_gamma(name, res.communities, gamma)
    print(f"{name} gamma {gamma}: plain {q_plain:.6f} split {q_split:.6f} "
          f"disconnected {res.connectivity.num_disconnected}")
    assert q_split >= q_plain
    assert rc.connected_communities(rc.graph(name), res.communities)


@pytest.mark.parametrize("gamma", [0.5, 2.0])
@pytest.mark.parametrize("name", QUALITY_GRAPHS + ("rmat10u",))
def test_leiden_communities_are_connected(name, gamma):
    res = rc.gamma_run(name, gamma, algorithm="leiden")
    assert rc.connected_communities(rc.graph(name), res.communities)
    assert any("refine" in lv for lv in res.levels)


def test_refine_partition_takes_the_resolution():
    """At gamma = 4 the refinement of the gamma = 1 communities of the ring
    leaves more sub-communities than at gamma = 1: the keyword reaches the
    gain."""
    from cuvite_amd import refine_partition
    dg = single_partition(rc.graph("ring32k4"))
    lab = rc.gamma_run("ring32k4", 1.0).communities
    one = refine_partition(dg, lab, Comm(), backend="torch")
    same = refine_partition(dg, lab, Comm(), backend="torch", resolution=1.0)
    assert torch.equal(one.labels, same.labels)
    hi = refine_partition(dg, lab, Comm(), backend="torch", resolution=64.0)
    print(f"subs: gamma 1 {one.num_subcommunities}, gamma 64 "
          f"{hi.num_subcommunities}")
    assert hi.num_subcommunities > one.num_subcommunities


# ---- dynamic ----------------------------------------------------------------

def _gamma2_update(name, frac):
    """(new graph, prev = the gamma = 2 cold run on the old graph, first
    frontier) for the recipe batch of dynamic_cases.py."""
    g = dyc.base_graph(name)
    batch = dyc.recipe_batch(g, frac)
    dg = apply_edge_batch(single_partition(g), Comm(), batch)
    prev = rc.gamma_run(name, 2.0).communities
    f0 = affected_vertices(dg, Comm(), prev, batch)
    return dg, prev, f0


@pytest.mark.parametrize("name", ["karate", "lfr", "dup"])
def test_full_frontier_without_expansion_is_warm_start_at_gamma_2(name):
    dg, prev, _ = _gamma2_update(name, 0.05)
    ref = louvain(dg, Comm(), _cfg(2.0, one_phase=True),
                  init_labels=prev.clone())
    est, lab, it, _, rep = run_frontier_phase(
        dg, Comm(), _cfg(2.0), prev.clone(),
        torch.ones(dg.nv, dtype=torch.bool), expand=False)
    assert it == ref.total_iters and rep.sweeps == it
    if ref.modularity_per_level:
        assert torch.equal(lab, ref.communities)
        assert est == ref.modularity


def test_lfr_batch_keeps_q_2():
    dg, prev, f0 = _gamma2_update("lfr", 0.01)
    res = louvain(dg, Comm(), _cfg(2.0), init_labels=prev.clone(),
                  init_frontier=f0.clone())
    rep = res.levels[0]["frontier"]

    def q2(labels):
        return partition_quality(dg, labels, Comm(), backend="torch",
                                 resolution=2.0).modularity

    q_new, q_prev = q2(res.communities), q2(prev)
    print(f"lfr 1 % batch at gamma 2: sizes {rep.sizes_per_sweep} "
          f"Q_2 {q_new:.6f} (prev on new graph {q_prev:.6f})")
    assert q_new >= q_prev
    assert rep.evaluated < rep.sweeps * dg.nv


# ---- scan -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["karate", "rgg"])
def test_scan_equals_explicit_warm_starts(name):
    dg = single_partition(rc.graph(name))
    scan = rc.scan_run(name)
    assert len(scan) == len(rc.SCAN_GAMMAS)
    prev = None
    for g, got in zip(rc.SCAN_GAMMAS, scan):
        want = louvain(dg, Comm(), _cfg(g), init_labels=prev)
        assert torch.equal(got.communities, want.communities)
        assert got.total_iters == want.total_iters
        assert got.modularity == want.modularity
        prev = got.communities
    # the first run is an ordinary cold run
    assert torch.equal(scan[0].communities,
                       rc.gamma_run(name, rc.SCAN_GAMMAS[0]).communities)


@pytest.mark.parametrize("name", ["lfr", "rgg"])
def test_scan_needs_fewer_sweeps_than_cold_runs(name):
    warm = sum(r.total_iters for r in rc.scan_run(name))
    cold = sum(rc.gamma_run(name, g).total_iters for g in rc.SCAN_GAMMAS)
    print(f"{name}: scan {warm} sweeps, five cold runs {cold}")
    assert warm < cold


def test_scan_keeps_the_config_and_takes_init_labels():
    dg = single_partition(rc.graph("karate"))
    cfg = LouvainConfig(backend="torch", vcycle=True, resolution=7.0)
    out = resolution_scan(dg, [2.0, 1.0], Comm(), cfg)
    assert all(r.vcycle is not None for r in out)
    assert cfg.resolution == 7.0                      # not written to
    init = rc.gamma_run("karate", 4.0).communities
    out = resolution_scan(dg, [2.0], Comm(), _cfg(1.0),
                          init_labels=init.clone())
    want = louvain(dg, Comm(), _cfg(2.0), init_labels=init.clone())
    assert torch.equal(out[0].communities, want.communities)
    assert cuvite_amd.resolution_scan is resolution_scan


@pytest.mark.parametrize("gammas", [[1.0, 2.0], [2.0, 2.0], [4.0, 1.0, 1.0],
                                    [2.0, 0.0], [float("nan")]])
def test_scan_rejects(gammas):
    dg = single_partition(rc.graph("karate"))
    with pytest.raises(ValueError):
        resolution_scan(dg, gammas, Comm(), _cfg(1.0))


# ---- validation -------------------------------------------------------------

BAD_GAMMAS = (0.0, -1.0, float("nan"), float("inf"))


@pytest.mark.parametrize("gamma", BAD_GAMMAS)
def test_bad_resolution_raises(gamma):
    dg = single_partition(rc.graph("karate"))
    with pytest.raises(ValueError, match="resolution"):
        louvain(dg, Comm(), _cfg(gamma))


def _w_bad_gamma(rank, world):
    dg = shard(rc.graph("karate"), rank, world)
    raised = []
    for gamma in BAD_GAMMAS:
        try:
            louvain(dg, Comm(), _cfg(gamma))
            raised.append(False)
        except ValueError:
            raised.append(True)
    # the ranks are still in step: a good run goes through
    res = louvain(dg, Comm(), _cfg(2.0))
    return raised, res.communities


def test_bad_resolution_raises_on_every_rank_before_any_collective():
    outs = run_dist(2, _w_bad_gamma, timeout_s=120)
    assert [o[0] for o in outs] == [[True] * 4, [True] * 4]
    assert torch.equal(torch.cat([o[1] for o in outs]),
                       rc.gamma_run("karate", 2.0).communities)


# ---- ranks ------------------------------------------------------------------

def _update_pieces(rank, world, comm, name, balanced, prev):
    g = dyc.base_graph(name)
    batch = dyc.recipe_batch(g, 0.01)
    share = dyc.share_of(batch, rank, world)
    dg = apply_edge_batch(shard(g, rank, world, balanced), comm, share)
    mine = prev[dg.base:dg.bound].clone()
    f0 = affected_vertices(dg, comm, mine, share)
    res = louvain(dg, comm, _cfg(2.0), init_labels=mine, init_frontier=f0)
    return {"labels": res.communities, "iters": res.total_iters,
            "sizes": list(res.levels[0]["frontier"].sizes_per_sweep)}


def _w_modes(rank, world, name, balanced, prev):
    if world > 1:
        torch.set_num_threads(4)    # the rank processes share the cores
    out = {m: rc.dist_run(rank, world, Comm(), CPU, "torch", name, balanced,
                          2.0, kw) for m, kw in rc.MODES.items()}
    out["update"] = _update_pieces(rank, world, Comm(), name, balanced, prev)
    return out


@pytest.mark.parametrize("balanced", [False, True],
                         ids=["contiguous", "balanced"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_gamma_2_runs_are_rank_invariant(world, balanced):
    name = "lfr"
    prev = rc.gamma_run(name, 2.0).communities
    dg_new, _, f0 = _gamma2_update(name, 0.01)
    want_update = louvain(dg_new, Comm(), _cfg(2.0),
                          init_labels=prev.clone(),
                          init_frontier=f0.clone())
    if world == 1:
        parts = [_w_modes(0, 1, name, balanced, prev)]
    else:
        parts = run_dist(world, _w_modes, name, balanced, prev)
    for mode, kw in rc.MODES.items():
        want = rc.gamma_run(name, 2.0, **kw)
        assert torch.equal(torch.cat([p[mode]["labels"] for p in parts]),
                           want.communities), mode
        for p in parts:
            assert p[mode]["iters"] == want.total_iters, mode
    assert torch.equal(torch.cat([p["update"]["labels"] for p in parts]),
                       want_update.communities)
    for p in parts:
        assert p["update"]["iters"] == want_update.total_iters
        assert p["update"]["sizes"] == \
            want_update.levels[0]["frontier"].sizes_per_sweep


# ---- CLI --------------------------------------------------------------------

def _cli(args, cwd):
    env = dict(os.environ, PYTHONPATH=REPO)
    return subprocess.run(
        [sys.executable, "-m", "cuvite_amd", "--device", "cpu", "--backend",
         "torch"] + args,
        capture_output=True, text=True, cwd=cwd, env=env, timeout=300)


def _line(out, prefix):
    return [ln for ln in out.splitlines() if ln.startswith(prefix)]


def test_cli_resolution_run_and_score(tmp_path):
    r = _cli(["--karate", "--resolution", "2", "--exact-modularity"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    assert _line(r.stdout, "Resolution:") == ["Resolution: 2"]
    assert r.stdout.index("Resolution: 2") < r.stdout.index("Final modularity")
    want = rc.gamma_run("karate", 2.0)
    exact = _line(r.stdout, "Exact modularity:")[0]
    assert exact.endswith("(6 communities)")
    assert abs(float(exact.split()[2])
               - rc.q_gamma("karate", want.communities, 2.0)) < 1e-12
    assert f"Final modularity: {want.modularity:.6f}" in r.stdout

    # --score-communities and --init-communities print Q_gamma
    cfile = str(tmp_path / "k.communities")
    write_communities(cfile, want.communities)
    for gamma in (2.0, 0.5):
        q = rc.q_gamma("karate", want.communities, gamma)
        r = _cli(["--karate", "--score-communities", cfile, "--resolution",
                  str(gamma)], tmp_path)
        assert r.returncode == 0, r.stderr
        assert _line(r.stdout, "Resolution:") == [f"Resolution: {gamma:g}"]
        part = _line(r.stdout, "Partition ")[0]
        assert abs(float(part.split("modularity=")[1].split()[0]) - q) < 1e-12
        r = _cli(["--karate", "--init-communities", cfile, "--resolution",
                  str(gamma), "-p"], tmp_path)
        assert r.returncode == 0, r.stderr
        init = _line(r.stdout, "Initial partition:")[0]
        assert abs(float(init.split("modularity=")[1].split()[0]) - q) < 1e-12


def test_cli_without_the_flag_is_unchanged(tmp_path):
    r = _cli(["--karate", "--exact-modularity"], tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Resolution" not in r.stdout
    want = cold_run("karate")
    assert f"Final modularity: {want.modularity:.6f}" in r.stdout
    assert _line(r.stdout, "Exact modularity:")[0].endswith(
        f"({rc.num_communities(want.communities)} communities)")
    one = _cli(["--karate", "--resolution", "1", "--exact-modularity"],
               tmp_path)
    assert one.returncode == 0
    assert _line(one.stdout, "Exact modularity:") == \
        _line(r.stdout, "Exact modularity:")


def test_cli_resolution_composes_and_is_checked(tmp_path):
    from cuvite_amd.cli import build_parser, validate
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit, match="--resolution"):
            validate(build_parser().parse_args(
                ["--karate", "--resolution", bad]), 1)
    for extra in (["--vcycle"], ["--leiden"], ["--connectivity", "final"],
                  ["-c", "4"], ["-t", "1"], ["-i"]):
        validate(build_parser().parse_args(
            ["--karate", "--resolution", "0.5"] + extra), 1)
    # an update at gamma = 2: the partition of the old graph, one deleted
    # edge
    prev = rc.gamma_run("karate", 2.0).communities
    cfile, ufile = str(tmp_path / "c.communities"), str(tmp_path / "u.txt")
    write_communities(cfile, prev)
    with open(ufile, "w") as f:
        f.write("d 0 1\na 9 20\n")
    r = _cli(["--karate", "--init-communities", cfile, "--update-edges",
              ufile, "--resolution", "2", "--vcycle", "--exact-modularity"],
             tmp_path)
    assert r.returncode == 0, r.stderr
    for prefix in ("Resolution: 2", "Edge batch:", "Initial partition:",
                   "Frontier phase:", "Exact modularity:"):
        assert len(_line(r.stdout, prefix)) == 1, prefix


# ---- the precondition of the GPU kernel test ---------------------------------

LADDER_PAIRS = [(s, gh) for s in rc.LADDER_STATES for gh in (False, True)]


def test_scaling_the_constant_changes_targets_on_every_route():
    """Scaling `constant` by a power of two must decide argmaxes, else the
    GPU comparison at scaled constants shows nothing new: every (state,
    ghosts) pair changes a target under some factor, and over all cases a
    ladder vertex of every class and of the hub route changes, at hub cuts
    2049 and 6144."""
    hit = {cut: set() for cut in (2049, 6144)}
    for state, ghosts in LADDER_PAIRS:
        inp, L, (t0, _) = rc.base_ladder(torch.float64, state, ghosts)
        deg = (inp.rowptr[1:] - inp.rowptr[:-1])[:L]
        counts = []
        for f in rc.FACTORS:
            _, _, (t, _) = rc.scaled_ladder(torch.float64, state, ghosts, f)
            ch = t != t0
            counts.append(int(ch.sum()))
            for cut in hit:
                for route, mask in routes(deg, cut).items():
                    if bool((mask & ch[:L]).any()):
                        hit[cut].add(route)
        print(f"{state} ghosts={ghosts}: targets changed {counts}")
        assert max(counts) >= 1
    want = {f"class{c}" for c in range(7)} | {"hub"}
    for cut in hit:
        assert hit[cut] == want, (cut, sorted(want - hit[cut]))


def test_scaled_ladder_is_dtype_independent_and_exact():
    """fp32 and fp64 weights give the same targets (integer data, fp64 gain),
    and the dict model agrees with the torch twin on the ladder rows."""
    from cuvite_amd.local_move import local_move_pydict
    for f in rc.FACTORS:
        _, L, (t64, cw64) = rc.scaled_ladder(torch.float64, "few", True, f)
        _, _, (t32, cw32) = rc.scaled_ladder(torch.float32, "few", True, f)
        assert torch.equal(t64, t32)
        assert torch.equal(cw64, cw32.to(torch.float64))
    inp, L, (t, cw) = rc.scaled_ladder(torch.float64, "few", True, 1024.0)
    # the dict model over the first rows only (it is a python loop)
    n = 20
    head = dataclasses.replace(inp, rowptr=inp.rowptr[:n + 1])
    td, cwd = local_move_pydict(head)
    assert torch.equal(td, t[:n]) and torch.equal(cwd, cw[:n])
