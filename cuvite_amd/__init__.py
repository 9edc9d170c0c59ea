"""cuvite_amd — MI355X-native distributed Louvain community detection.

A from-scratch CDNA4/ROCm framework with the capabilities of pnnl/cuVite:
multi-phase Louvain modularity maximization over graphs partitioned across
the GPUs of one MI355X node, with hand-written HIP kernels for the
local-moving phase and modularity reduction, RCCL-over-xGMI halo exchange,
on-device coarsening, coloring-ordered moves, early termination, and
Vite-compatible binary graph I/O.
"""

__version__ = "0.1.0"

from .graph import Graph, DistGraph, Partition
from .louvain import louvain, LouvainConfig, LouvainResult, resolution_scan
from .quality import (PartitionQuality, intra_weight_torch,
                      partition_quality)
from .connectivity import (ConnectivityReport, cc_components_torch,
                           split_disconnected)
from .refine import RefineReport, refine_coin, refine_partition
from .dynamic import (EdgeBatch, FrontierReport, StreamError, StreamStep,
                      affected_vertices, apply_edge_batch,
                      apply_routed_batch_torch, frontier_expand_torch,
                      frontier_move_torch, run_frontier_phase, update_stream)
from .uncoarsen import (VcycleLevel, intra_boundary_torch,
                        run_uncoarsen_phase)

__all__ = [
    "Graph",
    "DistGraph",
    "Partition",
    "louvain",
    "LouvainConfig",
    "LouvainResult",
    "resolution_scan",
    "PartitionQuality",
    "partition_quality",
    "intra_weight_torch",
    "ConnectivityReport",
    "split_disconnected",
    "cc_components_torch",
    "RefineReport",
    "refine_coin",
    "refine_partition",
    "EdgeBatch",
    "FrontierReport",
    "apply_edge_batch",
    "apply_routed_batch_torch",
    "update_stream",
    "StreamStep",
    "StreamError",
    "affected_vertices",
    "run_frontier_phase",
    "frontier_move_torch",
    "frontier_expand_torch",
    "VcycleLevel",
    "intra_boundary_torch",
    "run_uncoarsen_phase",
    "__version__",
]
