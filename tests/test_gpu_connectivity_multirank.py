"""split_disconnected with more than one rank on ONE GPU.

Two or three rank processes share `cuda:0` (`dist_utils.HostStagedComm`:
compute on the device with backend "hip", the wire is gloo on host copies).
Each rank splits the cold-run labels of lfr and rgg on its contiguous shard,
first on the CPU over plain `Comm()`, then on the device. What this covers
beyond the single-rank tests: the cc kernels on shards with ghosts and
base != 0, the int32 halo wire carrying component values, and the cross-rank
stitching rounds on device tensors. Both sides must reproduce the
single-rank CPU labels exactly: the result is the smallest global vertex id
of the component, whatever the partition.

One launch per world size; the tests only read the cached launch. Launch
wall time measured on an MI355X (process start and imports included):
world 2 3.5 s, world 3 2.7 s. LAUNCH_TIMEOUT_S is three times the slower
one, rounded up; the first test of a world prints what its launch took.
"""

import functools
import time

import pytest
import torch

from cuvite_amd import split_disconnected
from cuvite_amd.graph import single_partition
from cuvite_amd.parallel import Comm

from tests.dist_utils import run_dist

from quality_cases import cold_run, shard, whole_graph

pytestmark = pytest.mark.gpu

WORLDS = (2, 3)
NAMES = ("lfr", "rgg")
LAUNCH_TIMEOUT_S = 11


def _worker(rank, world, labels_by_name, devname):
    from tests.dist_utils import HostStagedComm
    torch.set_num_threads(max(1, 16 // world))
    dev = torch.device(devname)
    out = {}
    for name, lab in labels_by_name.items():
        dg = shard(whole_graph(name), rank, world)
        mine = lab[dg.base:dg.bound].clone()
        cpu = split_disconnected(dg, mine, Comm(), backend="torch")
        gpu = split_disconnected(dg.to(dev), mine.to(dev),
                                 HostStagedComm(dev), backend="hip")
        out[name] = {
            "cpu": cpu.labels, "gpu": gpu.labels.cpu(),
            "on": gpu.labels.device.type,
            "counts": [(r.num_communities, r.num_components,
                        r.num_disconnected) for r in (cpu, gpu)],
            "rounds": (cpu.rounds, gpu.rounds)}
    return out


@functools.lru_cache(maxsize=None)
def _launch(world):
    """One attempt per world size and session; a failed launch is cached as
    its exception, never repeated."""
    assert torch.cuda.is_available()
    labels = {n: cold_run(n).communities for n in NAMES}
    t0 = time.perf_counter()
    try:
        outs = run_dist(world, _worker, labels, "cuda:0",
                        timeout_s=LAUNCH_TIMEOUT_S)
    except Exception as e:
        outs = e
    print(f"world-{world} launch: {time.perf_counter() - t0:.1f} s "
          f"(limit {LAUNCH_TIMEOUT_S} s)")
    return outs


@functools.lru_cache(maxsize=None)
def _single_rank(name):
    return split_disconnected(single_partition(whole_graph(name)),
                              cold_run(name).communities, Comm(),
                              backend="torch")


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("world", WORLDS)
def test_split_multirank_on_one_gpu(world, name):
    outs = _launch(world)
    if isinstance(outs, Exception):
        raise AssertionError(f"world-{world} launch failed: {outs!r}")
    assert len(outs) == world
    ref = _single_rank(name)
    print(f"{name} world {world}: (cpu, device) rounds per rank "
          f"{[o[name]['rounds'] for o in outs]}")
    for side in ("cpu", "gpu"):
        got = torch.cat([o[name][side] for o in outs])
        assert torch.equal(got, ref.labels), side
    want = (ref.num_communities, ref.num_components, ref.num_disconnected)
    for o in outs:
        assert o[name]["on"] == "cuda"
        assert o[name]["counts"] == [want, want]


@pytest.mark.parametrize("world", WORLDS)
def test_launch_left_no_process_behind(world):
    import multiprocessing
    outs = _launch(world)
    assert not isinstance(outs, Exception), repr(outs)
    assert multiprocessing.active_children() == []
