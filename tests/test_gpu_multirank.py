"""The multi-rank (`world > 1`) code path on ONE GPU against the CPU oracle.

Two or three rank processes share `cuda:0`: all compute runs on the device
with backend "hip", the wire is gloo on host copies
(`dist_utils.HostStagedComm`), so neither a second GPU nor RCCL is needed.
What this covers is everything a rank does between collectives when it is
not alone: the HIP branch of `PhaseState.apply_moves` (apply_deltas_ on real
[base, bound) windows, the HIP scatter_add_ on the receive side of
push_remote_deltas), `densify` with its append-only universe and changed-
label remap feeding growing comm_* arrays to the move kernels and the hub
pipeline, the int32 halo wire format into device buffers, coarsening with
routed keys, coloring with ghosts and base != 0, scoring and warm start.
What it does not cover is the wire itself: RCCL / xGMI stay unverified.

One launch per world size runs every scenario of dist_cases.SCENARIOS, in
each rank process first on the CPU oracle over plain `Comm()`, then on the
device. The tests only read the cached launch. Inputs carry unit (or small
integer) weights, so every comparison is exact: torch.equal and ==.

Launch wall time measured on an MI355X (process start and imports
included): world 2 5.8 s, world 3 4.8 s. LAUNCH_TIMEOUT_S is three times
the slower one; the first test of a world prints what its launch took.
"""

import functools
import time

import pytest
import torch

from tests.dist_utils import run_dist

import dist_cases as dc

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)
LAUNCH_TIMEOUT_S = 18


@functools.lru_cache(maxsize=None)
def _launch(world):
    """One attempt per world size and session; a failed launch is cached as
    its exception, never repeated."""
    assert torch.cuda.is_available()
    t0 = time.perf_counter()
    try:
        outs = run_dist(world, dc.launch_worker, tuple(dc.SCENARIOS),
                        "cuda:0", timeout_s=LAUNCH_TIMEOUT_S)
    except Exception as e:
        outs = e
    print(f"world-{world} launch: {time.perf_counter() - t0:.1f} s "
          f"(limit {LAUNCH_TIMEOUT_S} s)")
    return outs


@pytest.mark.parametrize("name", list(dc.SCENARIOS))
@pytest.mark.parametrize("world", WORLDS)
def test_multirank_on_one_gpu_matches_cpu_oracle(world, name):
    outs = _launch(world)
    if isinstance(outs, Exception):
        raise AssertionError(f"world-{world} launch failed: {outs!r}")
    secs = [tuple(round(s, 2) for s in o[name]["seconds"]) for o in outs]
    print(f"{name} world {world}: (oracle, device) seconds per rank {secs}")
    dc.check_scenario(name, world, [o[name] for o in outs], "cuda")


@pytest.mark.parametrize("world", WORLDS)
def test_launch_left_no_process_behind(world):
    import multiprocessing
    outs = _launch(world)
    assert not isinstance(outs, Exception), repr(outs)
    assert len(outs) == world
    assert multiprocessing.active_children() == []
