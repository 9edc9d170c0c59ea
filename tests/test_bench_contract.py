"""The driver depends on bench.py's CLI + JSON contract; lock it down."""

import json
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DUMP_NAMES = ("modularity", "communities", "cluster_weight",
              "community_degree", "community_size")


def _run_bench(tmp_path, *extra):
    # the contract is checked on the CPU everywhere: with a GPU visible the
    # torch backend would run on it, where fp atomics make the fractional
    # weight sums differ in the last bit from run to run and the dumps of
    # two runs cannot be compared with array_equal
    env = dict(os.environ, PYTHONPATH=REPO, HIP_VISIBLE_DEVICES="",
               CUDA_VISIBLE_DEVICES="")
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--scale", "8",
         "--steps", "2", "--warmup", "1", "--backend", "torch", *extra],
        capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line on stdout: {r.stdout!r}"
    return json.loads(lines[0])


def test_bench_json_contract(tmp_path):
    out = _run_bench(tmp_path, "--dump-outputs", str(tmp_path / "plain"))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config"):
        assert key in out, key
    assert out["metric"] == "louvain_edges_per_sec"
    assert out["n_gpus"] == 1
    assert out["steps"] == 2
    assert out["warmup"] == 1
    assert out["higher_is_better"] is True
    assert out["data"] == "synthetic"
    assert out["value"] > 0
    assert out["ms_per_step"] > 0
    assert out["config"]["scale"] == 8
    assert out["config"]["ne_directed"] > 0
    # a plain run times the steps and nothing else
    assert "converged" not in out["config"]

    # --full adds the converged multi-phase run and leaves the headline
    # fields alone; the dumped outputs of the last timed step are the same
    # from run to run, whatever else the run does afterwards
    full = _run_bench(tmp_path, "--full", "--dump-outputs",
                      str(tmp_path / "full"))
    for key in ("metric", "unit", "higher_is_better", "dtype", "steps",
                "warmup"):
        assert full[key] == out[key], key
    assert full["ms_per_step"] > 0
    conv = full["config"]["converged"]
    assert "error" not in conv, conv
    assert conv["phases"] >= 1
    assert conv["final_modularity"] > 0

    nv = 1 << 8
    total = 0
    for name in DUMP_NAMES:
        a = np.load(tmp_path / "plain" / f"{name}.npy")
        b = np.load(tmp_path / "full" / f"{name}.npy")
        assert a.dtype == np.float64, name
        assert a.shape == ((1,) if name == "modularity" else (nv,)), name
        assert np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 << 20
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(
        f"{n}.npy" for n in DUMP_NAMES)
    q = np.load(tmp_path / "plain" / "modularity.npy")
    assert float(q[0]) == out["config"]["modularity_last_step"]
    labels = np.load(tmp_path / "plain" / "communities.npy")
    assert ((labels >= 0) & (labels < nv)).all()
    assert (labels == np.floor(labels)).all()
    size = np.load(tmp_path / "plain" / "community_size.npy")
    assert np.array_equal(size, np.bincount(labels.astype(np.int64),
                                            minlength=nv))
