// MI355X (gfx950, CDNA4) kernels for Louvain local moving + modularity.
//
// Semantic spec: cuvite_amd/local_move.py (transcribed from the reference CPU
// path, louvain.cpp:2185-2431); this is a from-scratch wave64 design, not a
// port of the reference's CUDA kernels: the reference deduplicates neighbor
// communities with an O(deg^2) in-place sweep (distGetMaxIndex,
// louvain_cuda.cu:1190-1346); here every degree class builds an open-addressing
// LDS hash table (community id -> accumulated edge weight) with wave-
// cooperative inserts, then computes the dQ argmax by scanning the table.
//
// Degree-class routing (the reference's 3-bucket idea, count_size_clmap
// louvain_cuda.cu:1426-1592, rebuilt for wave64). Class boundaries are
// sized so the LDS table per block stays at <= 24 KB for the bulk classes
// (6 resident blocks/CU on 160 KB LDS — the round-1 two-class split left
// class (512,2048] on a 48 KB table at 3 blocks/CU, and PMC showed the
// kernels latency-bound at 80% SQ_WAIT_ANY, so residency is the lever):
//   class 0: deg in [1, 16]      16 lanes/vertex,  32-slot LDS table
//   class 1: deg in (16, 64]     one wave/vertex, 128-slot LDS table
//   class 2: deg in (64, 256]    one wave/vertex, 512-slot LDS (24 KB/blk)
//   class 3: deg in (256, 512]   one wave/vertex, 1024-slot LDS (48 KB/blk)
//   class 4: deg in (512, 1024]  256-thread block/vertex, 2048-slot (24 KB)
//   class 5: deg in (1024, 2048] 256-thread block/vertex, 4096-slot (48 KB)
//   class 6: deg in (2048, cut]  256-thread block/vertex, 8192-slot (96 KB;
//                                cut = CUVITE_HUB_CUT, default 6144 after
//                                the s26 A/B in profiles/)
//   hub    : deg > cut (6144)    hub_moves binding (rocPRIM narrow-bit
//                                segmented radix sort, then one pass over
//                                the sorted pairs in fixed element slices:
//                                run sums, gains and argmax, see "Hub
//                                argmax straight from the sorted pairs"
//                                below) — the sort pipeline is 2.9x faster
//                                than the torch global-sort fallback at s26
//                                (A/B in profiles/; CUVITE_HUB_SEGSORT=0
//                                restores the fallback). A global-memory
//                                hash-table hub pipeline existed in round
//                                1 but was DELETED: open-addressing CAS
//                                tables past the 4 MB XCD L2 measured
//                                pathologically slow with an unexplained
//                                hang at exactly 2^21 slots
//                                (profiles/hub_pathology_and_s26.md), and
//                                the sort pipeline beats it anyway.
//
// Schedule (local_move binding): classes 0-3 need 6 KB of LDS per block and
// fill all 32 wave slots of a CU; classes 4-6 are bound by their tables to
// 24, 12 and 4 resident waves per CU. The two groups run side by side, the
// block classes on an auxiliary stream (largest first), and share the CUs
// (s26 step 70.5 -> 59 ms, profiles/round4_class_schedule.md). Measured in
// the same round and NOT kept, each slower under that schedule: a
// predicated 4-deep edge loop without the remainder loop (a load under a
// per-lane condition makes the compiler branch around it and wait for all
// but one load in flight before every gather), 512- and 1024-thread blocks
// for classes 5 and 6 (faster only while the classes run one after
// another), a second auxiliary stream for class 6, and accounting class 0
// in a pass of its own (the pass alone takes 12.6 ms of atomics).
//
// All gain arithmetic is fp64 regardless of the weight dtype so trajectories
// match the fp64 CPU oracle (tie-break on equal gains -> smaller GLOBAL id).
// Global ids of locally owned communities are computed, not gathered
// (gid_of); with a second aggregate pair the lanes that store a target also
// account the new community sizes and degrees (account_target), which
// replaces the recount pass after a single-rank sweep.
//
// The move kernels (lv_move_sub, lv_move_block, hub_slice_kernel,
// hub_final_kernel) take a `bool REFINE` template parameter. false is the
// local move described above; its instantiations compile to the instructions
// they had before the parameter existed. true is one round of the Leiden
// refinement (cuvite_amd/refine.py): only the vertices with mover_bound[v] >=
// 0 move, a candidate y counts only if cand_bound[y] == mover_bound[v]
// (checked where its gain is folded into the argmax, one 4-byte gather per
// distinct candidate), and there is neither singleton guard nor aggregate
// accounting.
//
// Host interface: launch.h holds the argument structs (MoveArgs, HubArgs) and
// the declaration of every launcher defined at the end of this file. The
// degree classes are launched by launch_class, one kernel instantiation per
// row of CLASS_TABLE below.

#include "launch.h"

#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>

#include <cstdint>

#define DEV_INLINE __device__ __forceinline__

namespace cuvite {

// The degree classes of the header comment as code, and the only place their
// geometry is written. lanes > 0: lv_move_sub with that many lanes per
// vertex; lanes == 0: lv_move_block, one block per vertex. cap: LDS table
// slots per vertex. Every class runs CLASS_BLOCK threads per block.
struct ClassGeometry {
  int lanes, cap;
};
constexpr ClassGeometry CLASS_TABLE[] = {
    {16, 32},  {64, 128}, {64, 512}, {64, 1024},  // classes 0-3
    {0, 2048}, {0, 4096}, {0, 8192}};             // classes 4-6
constexpr int NUM_CLASSES = sizeof(CLASS_TABLE) / sizeof(CLASS_TABLE[0]);
constexpr int CLASS_BLOCK = 256;

static constexpr int32_t EMPTY_KEY = -1;

DEV_INLINE uint32_t hash_u32(uint32_t x) {
  x *= 0x9E3779B1u;
  x ^= x >> 16;
  return x;
}

template <typename W> DEV_INLINE void lds_atomic_add(W* p, W v);
template <> DEV_INLINE void lds_atomic_add<float>(float* p, float v) {
  unsafeAtomicAdd(p, v);
}
template <> DEV_INLINE void lds_atomic_add<double>(double* p, double v) {
  unsafeAtomicAdd(p, v);
}

// Candidate for the dQ argmax. Comparison implements the reference rule
// (louvain.cpp:2225-2233): strictly larger gain wins; equal nonzero gain with
// smaller global id wins. `gain == 0` entries represent "stay" (cc).
struct Best {
  double gain;
  int64_t gid;   // global community id (tie-break)
  int32_t dense; // dense community id (result)
};

DEV_INLINE void best_combine(Best& a, double g, int64_t gid, int32_t dense) {
  if (g > a.gain || (g == a.gain && g != 0.0 && gid < a.gid)) {
    a.gain = g;
    a.gid = gid;
    a.dense = dense;
  }
}

// Modularity gain (up to a constant factor) of moving a vertex of degree
// vdeg from its community (weight eix into it, degree ax without the vertex)
// to community y (weight eiy, degree ay). The one expression and operand
// order every move kernel uses, so equal inputs give equal bits.
DEV_INLINE double move_gain(double eiy, double eix, double vdeg, double ay,
                            double ax, double constant) {
  return 2.0 * (eiy - eix) - 2.0 * vdeg * (ay - ax) * constant;
}

// Global id of dense community y. Locally owned communities occupy the dense
// ids [0, n_local) and their global id is gid_base + y by construction, so
// the 8-byte random read of comm_gid[y] is needed for remote ones only.
// n_local == 0 reads the table for every id.
DEV_INLINE int64_t gid_of(const int64_t* __restrict__ comm_gid,
                          int64_t gid_base, int32_t n_local, int32_t y) {
  return y < n_local ? gid_base + (int64_t)y : comm_gid[y];
}

// Fused aggregate accounting: the lane that stores target[v] = tgt also adds
// v to the size and the degree of its new community in a second aggregate
// pair, so no recount pass over the labels is needed after the sweep. The
// atomics are fire-and-forget (no returned value). next_size == nullptr
// turns it off; the range check is the memory-safety guard recount_kernel
// has (an out-of-range label must not corrupt memory).
template <typename W>
DEV_INLINE void account_target(int64_t* __restrict__ next_size,
                               W* __restrict__ next_degree, int64_t n_next,
                               int32_t tgt, W vdeg) {
  if (next_size == nullptr) return;
  if (tgt < 0 || (int64_t)tgt >= n_next) return;
  atomicAdd((unsigned long long*)&next_size[tgt], 1ull);
  unsafeAtomicAdd(&next_degree[tgt], vdeg);
}

template <int WIDTH> DEV_INLINE void best_reduce(Best& b) {
#pragma unroll
  for (int off = WIDTH / 2; off > 0; off >>= 1) {
    double g = __shfl_down(b.gain, off, WIDTH);
    int64_t gid = __shfl_down(b.gid, off, WIDTH);
    int32_t dn = __shfl_down(b.dense, off, WIDTH);
    best_combine(b, g, gid, dn);
  }
}

template <int WIDTH> DEV_INLINE double sum_reduce(double v) {
#pragma unroll
  for (int off = WIDTH / 2; off > 0; off >>= 1)
    v += __shfl_down(v, off, WIDTH);
  return v;
}

// Probe (no insert): accumulated weight for key `k`, 0 if absent.
template <typename W>
DEV_INLINE W table_probe(const int32_t* keys, const W* vals, int cap,
                         int32_t k) {
  uint32_t h = hash_u32((uint32_t)k) & (cap - 1);
  while (true) {
    int32_t kk = keys[h];
    if (kk == k) return vals[h];
    if (kk == EMPTY_KEY) return (W)0;
    h = (h + 1) & (cap - 1);
  }
}

template <typename W>
DEV_INLINE void table_insert(int32_t* keys, W* vals, int cap, int32_t k, W w) {
  uint32_t h = hash_u32((uint32_t)k) & (cap - 1);
  while (true) {
    int32_t old = atomicCAS((int*)&keys[h], EMPTY_KEY, k);
    if (old == EMPTY_KEY || old == k) {
      lds_atomic_add(&vals[h], w);
      return;
    }
    h = (h + 1) & (cap - 1);
  }
}

// Edge-insert loop with a 4-deep software pipeline: the per-edge chain
// (load tail -> gather curr_comm[tail] -> LDS CAS insert) is latency-bound
// (PMC: ~80% SQ_WAIT_ANY at 3 blocks/CU); issuing 4 independent tail loads,
// then 4 independent label gathers, before any insert overlaps the two
// global-load latencies instead of serializing them per edge.
template <typename W, int STRIDE>
DEV_INLINE double insert_edges_pipelined(
    int64_t e0, int64_t e1, int lane, int32_t v,
    const int32_t* __restrict__ tails, const W* __restrict__ weights,
    const int32_t* __restrict__ curr_comm, int32_t* keys, W* vals, int cap) {
  constexpr int PIPE = 4;
  double selfloop = 0.0;
  int64_t e = e0 + lane;
  for (; e + (PIPE - 1) * (int64_t)STRIDE < e1; e += PIPE * (int64_t)STRIDE) {
    int32_t t[PIPE];
    W w[PIPE];
#pragma unroll
    for (int k = 0; k < PIPE; k++) {
      t[k] = tails[e + k * STRIDE];
      w[k] = weights[e + k * STRIDE];
    }
    int32_t c[PIPE];
#pragma unroll
    for (int k = 0; k < PIPE; k++) c[k] = curr_comm[t[k]];
#pragma unroll
    for (int k = 0; k < PIPE; k++) {
      if (t[k] == v) selfloop += (double)w[k];
      table_insert(keys, vals, cap, c[k], w[k]);
    }
  }
  for (; e < e1; e += STRIDE) {
    int32_t t = tails[e];
    W w = weights[e];
    if (t == v) selfloop += (double)w;
    table_insert(keys, vals, cap, curr_comm[t], w);
  }
  return selfloop;
}

// Scan the table slots owned by this lane and fold the argmax. REFINE: a
// candidate counts only if cand_bound[y] equals the mover's bound `mb` (one
// 4-byte gather per distinct candidate, here and not at insert, which would
// pay it per edge).
template <typename W, bool REFINE>
DEV_INLINE void scan_slots(const int32_t* keys, const W* vals, int cap,
                           int lane, int lanes, int32_t cc, double eix,
                           double ax, double vdeg, double constant,
                           const W* __restrict__ comm_degree,
                           const int64_t* __restrict__ comm_gid,
                           int64_t gid_base, int32_t n_local, Best& best,
                           int32_t mb,
                           const int32_t* __restrict__ cand_bound) {
  for (int s = lane; s < cap; s += lanes) {
    int32_t y = keys[s];
    if (y == EMPTY_KEY || y == cc) continue;
    if (REFINE && cand_bound[y] != mb) continue;
    double eiy = (double)vals[s];
    double ay = (double)comm_degree[y];
    double g = move_gain(eiy, eix, vdeg, ay, ax, constant);
    best_combine(best, g, gid_of(comm_gid, gid_base, n_local, y), y);
  }
}

// ---------------------------------------------------------------------------
// Sub-block kernel: LANES lanes per vertex, LDS table of CAP slots per group.
// vlist is padded to a multiple of (BLOCK/LANES) with -1.
// ---------------------------------------------------------------------------

// Smallest power of two >= 2*(deg+1), clamped to [lo, CAP]: distinct keys
// <= deg keeps the load factor under 1/2 while init/probe/scan touch only
// `cap` slots. rocprof at s26 showed the class-3 kernel (CAP 4096, typical
// deg ~600) spending most of its time on table init + argmax scan of slots
// that can never be occupied (profiles/round2_kernel_stats).
DEV_INLINE int cap_for_degree(int64_t deg, int CAP, int lo) {
  int cap = CAP;
  while (cap > lo && (cap >> 2) >= (int)(deg + 1)) cap >>= 1;
  return cap;
}

// REFINE = false is the plain local move (mover_bound and cand_bound are not
// read; the launcher passes null). REFINE = true is one Leiden refinement
// round (see local_move.refine_move_torch): a vertex with mover_bound[v] < 0
// does not move this round and is treated like the -1 padding, so it still
// reaches both barriers beside the movers of its block and keeps target = own
// label; candidates are filtered by their bound in scan_slots; no singleton
// guard and no fused aggregate accounting (comm_size, next_* are not read).
template <typename W, int LANES, int CAP, int BLOCK, bool REFINE>
__global__ __launch_bounds__(BLOCK) void lv_move_sub(
    const int32_t* __restrict__ vlist, int nlist,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ tails,
    const W* __restrict__ weights, const int32_t* __restrict__ curr_comm,
    const W* __restrict__ v_degree, const int64_t* __restrict__ comm_size,
    const W* __restrict__ comm_degree, const int64_t* __restrict__ comm_gid,
    double constant, int32_t* __restrict__ target,
    W* __restrict__ cluster_weight, int64_t gid_base, int32_t n_local,
    int64_t* __restrict__ next_size, W* __restrict__ next_degree,
    int64_t n_next, const int32_t* __restrict__ mover_bound,
    const int32_t* __restrict__ cand_bound) {
  constexpr int GROUPS = BLOCK / LANES;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  W* vals = (W*)smem;
  int32_t* keys = (int32_t*)(smem + (size_t)GROUPS * CAP * sizeof(W));

  const int group = threadIdx.x / LANES;
  const int lane = threadIdx.x % LANES;
  const int gidx = blockIdx.x * GROUPS + group;
  int32_t v = (gidx < nlist) ? vlist[gidx] : -1;
  int32_t mb = -1;
  if (REFINE && v >= 0) {
    mb = mover_bound[v];
    if (mb < 0) v = -1;
  }

  int32_t* gkeys = keys + (size_t)group * CAP;
  W* gvals = vals + (size_t)group * CAP;

  int64_t e0 = 0, e1 = 0;
  int32_t cc = 0;
  if (v >= 0) {
    e0 = rowptr[v];
    e1 = rowptr[v + 1];
    cc = curr_comm[v];
  }
  const int cap = cap_for_degree(e1 - e0, CAP, LANES);
#pragma unroll 4
  for (int s = lane; s < cap; s += LANES) {
    gkeys[s] = EMPTY_KEY;
    gvals[s] = (W)0;
  }
  __syncthreads();

  double selfloop = insert_edges_pipelined<W, LANES>(
      e0, e1, lane, v, tails, weights, curr_comm, gkeys, gvals, cap);
  __syncthreads();

  selfloop = sum_reduce<LANES>(selfloop);
  Best best{0.0, 0, cc};
  if (v >= 0 && e0 != e1) {
    W wcc = table_probe(gkeys, gvals, cap, cc);  // counter[cc]
    double eix = (double)wcc - __shfl(selfloop, 0, LANES);
    const W vdeg_w = v_degree[v];
    double vdeg = (double)vdeg_w;
    double ax = (double)comm_degree[cc] - vdeg;
    const int64_t gid_cc = gid_of(comm_gid, gid_base, n_local, cc);
    best.gid = gid_cc;
    scan_slots<W, REFINE>(gkeys, gvals, cap, lane, LANES, cc, eix, ax, vdeg,
                          constant, comm_degree, comm_gid, gid_base, n_local,
                          best, mb, cand_bound);
    best_reduce<LANES>(best);
    if (lane == 0) {
      int32_t tgt = best.dense;
      // singleton-swap guard (louvain.cpp:2238-2239)
      if (!REFINE && comm_size[tgt] == 1 && comm_size[cc] == 1 &&
          best.gid > gid_cc)
        tgt = cc;
      target[v] = tgt;
      cluster_weight[v] = wcc;
      if (!REFINE)
        account_target(next_size, next_degree, n_next, tgt, vdeg_w);
    }
  }
}

// ---------------------------------------------------------------------------
// Block kernel: one 256-thread block per vertex, CAP-slot LDS table.
// ---------------------------------------------------------------------------

// REFINE as in lv_move_sub; the whole block serves one vertex, so a
// non-mover leaves before any barrier (block-uniform) and keeps target = own
// label.
template <typename W, int CAP, int BLOCK, bool REFINE>
__global__ __launch_bounds__(BLOCK) void lv_move_block(
    const int32_t* __restrict__ vlist, int nlist,
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ tails,
    const W* __restrict__ weights, const int32_t* __restrict__ curr_comm,
    const W* __restrict__ v_degree, const int64_t* __restrict__ comm_size,
    const W* __restrict__ comm_degree, const int64_t* __restrict__ comm_gid,
    double constant, int32_t* __restrict__ target,
    W* __restrict__ cluster_weight, int64_t gid_base, int32_t n_local,
    int64_t* __restrict__ next_size, W* __restrict__ next_degree,
    int64_t n_next, const int32_t* __restrict__ mover_bound,
    const int32_t* __restrict__ cand_bound) {
  constexpr int WAVES = BLOCK / 64;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  W* vals = (W*)smem;
  int32_t* keys = (int32_t*)(smem + (size_t)CAP * sizeof(W));
  __shared__ double red_gain[WAVES];
  __shared__ int64_t red_gid[WAVES];
  __shared__ int32_t red_dense[WAVES];
  __shared__ double red_self[WAVES];

  const int32_t v = vlist[blockIdx.x];
  int32_t mb = -1;
  if (REFINE) {
    mb = mover_bound[v];
    if (mb < 0) return;
  }
  const int tid = threadIdx.x;
  const int wave = tid / 64, lane = tid % 64;

  const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
  const int cap = cap_for_degree(e1 - e0, CAP, BLOCK);
  for (int s = tid; s < cap; s += BLOCK) {
    keys[s] = EMPTY_KEY;
    vals[s] = (W)0;
  }
  __syncthreads();

  const int32_t cc = curr_comm[v];
  double selfloop = insert_edges_pipelined<W, BLOCK>(
      e0, e1, tid, v, tails, weights, curr_comm, keys, vals, cap);
  selfloop = sum_reduce<64>(selfloop);
  if (lane == 0) red_self[wave] = selfloop;
  __syncthreads();

  double self_total = 0.0;
#pragma unroll
  for (int i = 0; i < WAVES; i++) self_total += red_self[i];

  W wcc = table_probe(keys, vals, cap, cc);
  double eix = (double)wcc - self_total;
  const W vdeg_w = v_degree[v];
  double vdeg = (double)vdeg_w;
  double ax = (double)comm_degree[cc] - vdeg;
  const int64_t gid_cc = gid_of(comm_gid, gid_base, n_local, cc);
  Best best{0.0, gid_cc, cc};
  scan_slots<W, REFINE>(keys, vals, cap, tid, BLOCK, cc, eix, ax, vdeg,
                        constant, comm_degree, comm_gid, gid_base, n_local,
                        best, mb, cand_bound);
  best_reduce<64>(best);
  if (lane == 0) {
    red_gain[wave] = best.gain;
    red_gid[wave] = best.gid;
    red_dense[wave] = best.dense;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 1; i < WAVES; i++)
      best_combine(best, red_gain[i], red_gid[i], red_dense[i]);
    int32_t tgt = best.dense;
    if (!REFINE && comm_size[tgt] == 1 && comm_size[cc] == 1 &&
        best.gid > gid_cc)
      tgt = cc;
    target[v] = tgt;
    cluster_weight[v] = wcc;
    if (!REFINE) account_target(next_size, next_degree, n_next, tgt, vdeg_w);
  }
}

// ---------------------------------------------------------------------------
// Modularity reduction: (sum cluster_weight, sum comm_degree^2) in fp64.
// Reference analog: compute_modularity (modularity.cu:36-100), but fp64
// accumulation and a device-resident 2-double output the RCCL allreduce
// consumes directly (no D2H round trip).
// ---------------------------------------------------------------------------

template <typename W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void modularity_reduce(
    const W* __restrict__ cluster_weight, const W* __restrict__ comm_degree,
    int64_t nv, double* __restrict__ out) {
  double le = 0.0, la2 = 0.0;
  for (int64_t i = blockIdx.x * (int64_t)BLOCK + threadIdx.x; i < nv;
       i += (int64_t)gridDim.x * BLOCK) {
    le += (double)cluster_weight[i];
    double d = (double)comm_degree[i];
    la2 += d * d;
  }
  le = sum_reduce<64>(le);
  la2 = sum_reduce<64>(la2);
  if ((threadIdx.x % 64) == 0) {
    unsafeAtomicAdd(&out[0], le);
    unsafeAtomicAdd(&out[1], la2);
  }
}

// ---------------------------------------------------------------------------
// scatter_add: out[idx[i]] += val[i] with NATIVE fp32/fp64 atomics
// (unsafeAtomicAdd -> global_atomic_add_f64 on gfx950). PyTorch-ROCm's
// index_add_ lowers fp64 atomics to a CAS loop, which measured 16.5 s per
// call on an R-MAT s22 sweep (profiles/); this kernel replaces it on the
// hot paths (degree sums, community-aggregate deltas).
// ---------------------------------------------------------------------------

template <typename W>
__global__ void scatter_add_kernel(W* __restrict__ out,
                                   const int64_t* __restrict__ idx,
                                   const W* __restrict__ val, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    unsafeAtomicAdd(&out[idx[i]], val[i]);
}

// ---------------------------------------------------------------------------
// Fused community-aggregate update after a move sweep (ref 4-case update,
// louvain.cpp:2308-2376): one pass over the vertices applies the +-1 size
// and +-v_degree deltas for every moved vertex directly, with native int64/
// fp atomics. Replaces a 6-op torch chain (moved mask -> .any() host sync ->
// boolean compactions -> cat -> index_add_ -> scatter_add) that rocprof
// measured at ~40 ms/sweep at s26 (profiles/round2_kernel_stats). Only
// LOCALLY-owned community labels are applied here; remotely-owned deltas are
// compacted by the caller for the RCCL push (world>1 only).
// ---------------------------------------------------------------------------

template <typename W>
__global__ void apply_deltas_kernel(
    const int64_t* __restrict__ target, const int64_t* __restrict__ curr,
    const W* __restrict__ v_degree, int64_t nv, int64_t base, int64_t bound,
    int64_t* __restrict__ local_size, W* __restrict__ local_degree) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += stride) {
    const int64_t src = curr[i];
    const int64_t dst = target[i];
    if (src == dst) continue;
    const W d = v_degree[i];
    if (src >= base && src < bound) {
      atomicAdd((unsigned long long*)&local_size[src - base],
                (unsigned long long)(-1ll));
      unsafeAtomicAdd(&local_degree[src - base], (W)(-d));
    }
    if (dst >= base && dst < bound) {
      atomicAdd((unsigned long long*)&local_size[dst - base], 1ull);
      unsafeAtomicAdd(&local_degree[dst - base], d);
    }
  }
}

// ---------------------------------------------------------------------------
// Device-side CSR assembly (no sort; replaces torch.argsort which is capped
// at INT_MAX elements): degree histogram + atomic-cursor placement.
// Reference analog: processGraphData (utils.cpp:10-87) done host-side there.
// Row-internal edge order is nondeterministic; all consumers (local-move
// hash tables, degree sums) are order-invariant.
// ---------------------------------------------------------------------------

__global__ void degree_count_kernel(const int64_t* __restrict__ src, int64_t n,
                                    int64_t base, int32_t* __restrict__ cnt) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    atomicAdd(&cnt[src[i] - base], 1);
}

template <typename W>
__global__ void csr_place_kernel(const int64_t* __restrict__ src,
                                 const int64_t* __restrict__ dst,
                                 const W* __restrict__ w, int64_t n,
                                 int64_t base,
                                 const int64_t* __restrict__ rowptr,
                                 int32_t* __restrict__ cursor,
                                 int64_t* __restrict__ tails_out,
                                 W* __restrict__ w_out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride) {
    const int64_t s = src[i] - base;
    const int64_t o = rowptr[s] + atomicAdd(&cursor[s], 1);
    tails_out[o] = dst[i];
    w_out[o] = w[i];
  }
}

// ---------------------------------------------------------------------------
// Distance-1 coloring round: per-vertex strict min/max of every hash over
// COMPETING neighbors (uncolored at round start, not self), one wave per
// vertex with all n_hash hashes in a single edge pass and a wave reduction —
// no atomics, no edge-list materialization. Replaces 2*n_hash torch scatter
// passes over the full edge list per round (13.4 s for the whole coloring
// at R-MAT s26). Hash = the reference's 32-bit mix (coloring.cpp:74-85).
// ---------------------------------------------------------------------------

DEV_INLINE uint32_t color_hash(uint32_t a, uint32_t seed) {
  a ^= seed;
  a = (a + 0x7ED55D16u) + (a << 12);
  a = (a ^ 0xC761C23Cu) + (a >> 19);
  a = (a + 0x165667B1u) + (a << 5);
  a = (a ^ 0xD3A2646Cu) + (a << 9);
  a = (a + 0xFD7046C5u) + (a << 3);
  a = (a ^ 0xB55A4F09u) + (a >> 16);
  return a;
}

constexpr int MAX_NHASH = 8;

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void coloring_minmax_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ tails,
    const int64_t* __restrict__ gid_all, const bool* __restrict__ uncolored,
    const int64_t* __restrict__ colors, int64_t nv, int64_t base,
    const int64_t* __restrict__ seeds, int n_hash,
    int64_t* __restrict__ mn_out, int64_t* __restrict__ mx_out) {
  constexpr int WAVES = BLOCK / 64;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int64_t vstride = (int64_t)gridDim.x * WAVES;
  for (int64_t v = (int64_t)blockIdx.x * WAVES + wave; v < nv; v += vstride) {
    uint32_t mn[MAX_NHASH], mx[MAX_NHASH];
#pragma unroll
    for (int t = 0; t < MAX_NHASH; t++) {
      mn[t] = 0xFFFFFFFFu;
      mx[t] = 0u;
    }
    bool any = false;
    if (colors[v] < 0) {
      const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
      const int64_t vg = v + base;
      for (int64_t e = e0 + lane; e < e1; e += 64) {
        const int32_t td = tails[e];
        if (!uncolored[td]) continue;
        const int64_t g = gid_all[td];
        if (g == vg) continue;
        any = true;
        for (int t = 0; t < n_hash; t++) {
          const uint32_t h = color_hash((uint32_t)g, (uint32_t)seeds[t]);
          mn[t] = h < mn[t] ? h : mn[t];
          mx[t] = h > mx[t] ? h : mx[t];
        }
      }
    }
    any = __any(any);
    for (int t = 0; t < n_hash; t++) {
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const uint32_t omn = (uint32_t)__shfl_down((int)mn[t], off, 64);
        const uint32_t omx = (uint32_t)__shfl_down((int)mx[t], off, 64);
        mn[t] = omn < mn[t] ? omn : mn[t];
        mx[t] = omx > mx[t] ? omx : mx[t];
      }
    }
    if (lane == 0) {
      for (int t = 0; t < n_hash; t++) {
        // no competitor: same sentinels as the torch path (1<<33 / -1)
        mn_out[v * n_hash + t] =
            any ? (int64_t)mn[t] : ((int64_t)1 << 33);
        mx_out[v * n_hash + t] = any ? (int64_t)mx[t] : (int64_t)-1;
      }
    }
  }
}

void launch_coloring_minmax(const int64_t* rowptr, const int32_t* tails,
                            const int64_t* gid_all, const bool* uncolored,
                            const int64_t* colors, int64_t nv, int64_t base,
                            const int64_t* seeds, int n_hash, int64_t* mn_out,
                            int64_t* mx_out, hipStream_t stream) {
  if (nv == 0) return;
  constexpr int BLOCK = 256;
  constexpr int WAVES = BLOCK / 64;
  int64_t grid = (nv + WAVES - 1) / WAVES;
  if (grid > 1048576) grid = 1048576;
  hipLaunchKernelGGL((coloring_minmax_kernel<BLOCK>), dim3((uint32_t)grid),
                     dim3(BLOCK), 0, stream, rowptr, tails, gid_all,
                     uncolored, colors, nv, base, seeds, n_hash, mn_out,
                     mx_out);
}

// Per-vertex weighted degree: one wave per vertex, lane-strided row scan
// (ref distSumVertexDegree, louvain.cpp:2126-2151).
template <typename W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void row_sum_kernel(
    const int64_t* __restrict__ rowptr, const W* __restrict__ weights,
    int64_t nv, W* __restrict__ out) {
  constexpr int WAVES = BLOCK / 64;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  // wave-strided over vertices: grid stays under the 2^32-1 workitem cap
  const int64_t vstride = (int64_t)gridDim.x * WAVES;
  for (int64_t v = (int64_t)blockIdx.x * WAVES + wave; v < nv; v += vstride) {
    const int64_t e0 = rowptr[v], e1 = rowptr[v + 1];
    double acc = 0.0;
    for (int64_t e = e0 + lane; e < e1; e += 64) acc += (double)weights[e];
    acc = sum_reduce<64>(acc);
    if (lane == 0) out[v] = (W)acc;
  }
}

// ---------------------------------------------------------------------------
// intra_weight: out[v] = sum over row v of w[e] * [labels[tails[e]] ==
// labels[v]] for ARBITRARY labels (partition scoring, warm start) — the `cw`
// the move kernels produce, without the hash-table pass.
//
// Edge-balanced, not row-balanced: R-MAT rows range from < 16 edges to
// millions, so a wave-per-row layout (row_sum_kernel) leaves one wave
// walking a hub while the rest idle. Each wave owns a span of IW_SPAN
// consecutive edges and reads them lane-strided (coalesced tails/weights,
// one random label gather per edge). The span's first row comes from a
// binary search in rowptr and its last row from a gallop out of the first;
// every lane then finds the row of its own edge by a binary search inside
// that (wave-uniform, L1-resident) row range. Rows are contiguous runs of
// lanes, so a segmented shuffle scan sums them; a run that continues into
// the next 64-edge chunk is carried in registers. A row wholly inside the
// span gets one plain store; a row cut by a span boundary is added with a
// native float atomic into the zero-initialised output (at most two
// atomics per span). Sums inside a span are fp64 whatever the weight type.
// ---------------------------------------------------------------------------

constexpr int IW_SPAN = 4096;  // edges per wave: 64 chunks amortise the
                               // ~30 dependent loads of the row searches
constexpr int IW_PIPE = 4;     // chunks of loads in flight (as in
                               // insert_edges_pipelined)

// Largest r in [lo, hi] with rowptr[r] <= e (skips zero-degree rows).
DEV_INLINE int64_t row_of_edge(const int64_t* __restrict__ rowptr, int64_t lo,
                               int64_t hi, int64_t e) {
  while (lo < hi) {
    const int64_t m = (lo + hi + 1) >> 1;
    if (rowptr[m] <= e) lo = m; else hi = m - 1;
  }
  return lo;
}

// Wave-uniform row range [rlo, rhi] that holds the rows of the edges
// [s0, s1): the first row by a binary search over all of rowptr, the last by
// a gallop out of the first (rhi may overshoot the true last row).
DEV_INLINE void span_row_range(const int64_t* __restrict__ rowptr, int64_t nv,
                               int64_t s0, int64_t s1, int64_t& rlo,
                               int64_t& rhi) {
  rlo = row_of_edge(rowptr, 0, nv - 1, s0);
  rhi = rlo;
  int64_t step = 1;
  while (rhi + step < nv && rowptr[rhi + step] < s1) {
    rhi += step;
    step <<= 1;
  }
  rhi = (rhi + step - 1 < nv - 1) ? rhi + step - 1 : nv - 1;
}

// MARK: the same pass also flags the boundary vertices, mask[row] = 1 for
// every row with an edge whose tail is inside the label array and carries
// another label (the first frontier of an uncoarsening phase). The flag is a
// plain byte store by the lane that holds the edge: every writer stores the
// same 1 into a caller-zeroed array, so the order of the writers does not
// matter (frontier_expand_kernel's marks). Self-loops compare equal and
// out-of-range tails are skipped, so neither marks anything. Without MARK
// `mask` is null and never read.
template <typename W, typename L, int BLOCK, bool MARK>
__global__ __launch_bounds__(BLOCK) void intra_weight_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ tails,
    const W* __restrict__ weights, const L* __restrict__ labels, int64_t nv,
    int64_t ne, int64_t nl, W* __restrict__ out, uint8_t* __restrict__ mask) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t nspan = (ne + IW_SPAN - 1) / IW_SPAN;
  // wave-strided over spans: grid stays under the work-item cap
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * IW_SPAN;
    const int64_t s1 = (s0 + IW_SPAN < ne) ? s0 + IW_SPAN : ne;
    int64_t rlo, rhi;
    span_row_range(rowptr, nv, s0, s1, rlo, rhi);

    double carry_val = 0.0;
    int32_t carry_row = -1;  // row whose run continues from the last chunk
    for (int64_t c = s0; c < s1; c += (int64_t)IW_PIPE * 64) {
      int32_t t[IW_PIPE];
      W w[IW_PIPE];
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        const int64_t e = c + k * 64 + lane;
        const bool ok = e < s1;
        t[k] = ok ? tails[e] : 0;
        w[k] = ok ? weights[e] : (W)0;
      }
      L lt[IW_PIPE];
      bool inb[IW_PIPE];
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        // memory-safety guard: a tail outside the label array matches nothing
        inb[k] = (uint64_t)(int64_t)t[k] < (uint64_t)nl;
        lt[k] = inb[k] ? labels[t[k]] : (L)0;
      }
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        const int64_t cb = c + k * 64;
        if (cb >= s1) break;  // wave-uniform
        const int64_t e = cb + lane;
        const bool ok = e < s1;
        int32_t row = -2;  // lanes past the span: one inert run
        int64_t rend = 0;
        double val = 0.0;
        if (ok) {
          row = (int32_t)row_of_edge(rowptr, rlo, rhi, e);
          rend = rowptr[(int64_t)row + 1];
          if (inb[k]) {
            if (lt[k] == labels[row]) val = (double)w[k];
            else if (MARK) mask[row] = 1;  // row < nv: inside the mask
          }
        }
        if (lane == 0 && row == carry_row) val += carry_val;
        // segmented inclusive scan: equal rows are contiguous lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const double pv = __shfl_up(val, off, 64);
          const int32_t pr = __shfl_up(row, off, 64);
          if (lane >= off && pr == row) val += pv;
        }
        const bool tail = ok && (e == rend - 1 || e == s1 - 1);
        if (tail) {
          if (rowptr[row] >= s0 && rend <= s1)
            out[row] = (W)val;
          else
            unsafeAtomicAdd(&out[row], (W)val);
        }
        // only a full chunk can end inside a run (a partial chunk ends the
        // span, and its last edge is a tail)
        carry_val = __shfl(val, 63, 64);
        carry_row = __shfl(tail ? -1 : row, 63, 64);
        const int32_t last_row = __shfl(row, 63, 64);
        if (last_row >= 0) rlo = last_row;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// Connected components of the graph restricted to edges whose endpoints
// carry the same label (is a community connected? split it if not). Nodes
// are the dense ids [0, nl): local vertices first, then ghosts. The result
// comp[x] is the smallest dense id in x's component.
//
// Hook-and-compress rounds with a monotone min, driven by the host:
//   hook      every intra edge (u, t) reads ru = comp[u], rt = comp[t] and,
//             if they differ, does atomicMin(&comp[max], min) and raises
//             `changed`;
//   compress  every node chases comp to its root (comp[r] == r) and stores
//             it;
// until a hook pass raises no flag. Entering a hook pass comp is fully
// compressed, so every value in it is a root of that moment, and so is
// everything a pass writes: only roots are ever hooked, always under a
// smaller root of the same component. A root hooked twice in one pass keeps
// the smaller parent only; the edge behind the lost link sees two roots
// again next round, which is why the flag means "some intra edge saw two
// roots" and not "an atomicMin lowered something". When no edge raises it,
// comp is constant on every component, and since comp[x] <= x that constant
// is the component's smallest id.
//
// What makes this safe to run beside other work:
//   - comp[x] <= x holds at all times (it starts as x and only atomicMin
//     with a smaller value or a store of x's root ever writes it), so every
//     device loop walks strictly decreasing indices and ends after at most
//     x steps whatever other waves write meanwhile;
//   - no spin-wait, no CAS retry loop, no protocol between workgroups;
//   - a stale plain read of comp inside the hook pass (another XCD's L2
//     holds the fresh value) returns an older root of the same component: it
//     can only postpone a merge by a round, never merge two components;
//   - coherence between rounds comes from the kernel boundary.
// Every changing round removes at least one root, so nl + 1 rounds bound
// the host loop; real graphs take a handful.
//
// cc_hook_kernel is intra_weight_kernel's edge pass without the sums: each
// wave owns IW_SPAN consecutive edges, finds the span's row range with
// row_of_edge plus the gallop and every lane's row by a binary search
// inside it, keeps IW_PIPE chunks of loads in flight, and treats a tail
// outside the label array as matching nothing. No segmented scan and no
// per-row output.
// ---------------------------------------------------------------------------

template <typename L, int BLOCK>
__global__ __launch_bounds__(BLOCK) void cc_hook_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ tails,
    const L* __restrict__ labels, int64_t nv, int64_t ne, int64_t nl,
    int32_t* comp, int32_t* changed) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t nspan = (ne + IW_SPAN - 1) / IW_SPAN;
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  bool saw = false;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * IW_SPAN;
    const int64_t s1 = (s0 + IW_SPAN < ne) ? s0 + IW_SPAN : ne;
    int64_t rlo, rhi;
    span_row_range(rowptr, nv, s0, s1, rlo, rhi);

    for (int64_t c = s0; c < s1; c += (int64_t)IW_PIPE * 64) {
      int32_t t[IW_PIPE];
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        const int64_t e = c + k * 64 + lane;
        t[k] = (e < s1) ? tails[e] : -1;  // -1 fails the guard below
      }
      L lt[IW_PIPE];
      bool inb[IW_PIPE];
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        // memory-safety guard: a tail outside the label array matches nothing
        inb[k] = (uint64_t)(int64_t)t[k] < (uint64_t)nl;
        lt[k] = inb[k] ? labels[t[k]] : (L)0;
      }
#pragma unroll
      for (int k = 0; k < IW_PIPE; k++) {
        const int64_t cb = c + k * 64;
        if (cb >= s1) break;  // wave-uniform
        const int64_t e = cb + lane;
        int32_t row = -1;
        if (e < s1) {
          row = (int32_t)row_of_edge(rowptr, rlo, rhi, e);
          if (inb[k] && t[k] != row && lt[k] == labels[row]) {
            const int32_t ru = comp[row], rt = comp[t[k]];
            if (ru != rt) {
              atomicMin(&comp[ru > rt ? ru : rt], ru > rt ? rt : ru);
              saw = true;
            }
          }
        }
        const int32_t last_row = __shfl(row, 63, 64);
        if (last_row >= 0) rlo = last_row;
      }
    }
  }
  if (saw) changed[0] = 1;  // plain vector store; every writer stores 1
}

// One full chase per node. The chain from x walks strictly decreasing ids,
// so it ends within x steps; roots are fixed for the whole pass (a root is
// only ever stored its own id) and a concurrent store of another node's
// root only shortens the way. Workgroups are dispatched in index order, so
// even the depth-nl chain a hook pass builds on a path in natural vertex
// order is mostly met already compressed. The price of doing without
// pointer-doubling passes (a host sync each) is the worst case: a node whose
// whole chain is still uncompressed walks it alone, one dependent load per
// step. On R-MAT the pass takes 12 us at 4 M nodes (profiles/
// connectivity.md).
__global__ void cc_compress_kernel(int32_t* comp, int64_t nl) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < nl;
       x += stride) {
    int32_t r = comp[x];
    if (r == (int32_t)x) continue;
    int32_t p = comp[r];
    while (p < r) {  // p <= r always; equal at the root
      r = p;
      p = comp[r];
    }
    comp[x] = r;
  }
}

// ---------------------------------------------------------------------------
// Frontier sweeps (cuvite_amd/dynamic.py): a sweep evaluates only the
// vertices marked in a byte mask `active` [nv]. Two steps build that sweep's
// inputs on the device.
//
// Expand: given the dense ids whose label changed (locals in [0, nv), ghosts
// in [nv, nv + ng)), mark the changed locals and every local neighbour of a
// changed id. Neighbours of a local row come from the level CSR, those of a
// ghost from a ghost -> local reverse CSR. frontier_degrees_kernel stores the
// degree of every changed row (and marks the changed locals); the host side
// turns the degrees into the prefix array `offs`, which concatenates the
// changed rows into one edge space of offs[nc] edges. frontier_expand_kernel
// cuts that space into spans of FX_SPAN edges, one wave each, exactly as
// intra_weight_kernel cuts the whole edge list: first row of the span by a
// binary search in offs, last row by a gallop (span_row_range), each lane's
// row by a search inside that range. Work is proportional to the summed
// degree of the changed rows and a changed hub is spread over many waves.
// Marks are plain byte stores of 1: idempotent, so neither order nor
// duplicates matter and there are no atomics. Every loop is bounded by the
// span. An id outside [0, nv + ng) has degree 0; a neighbour outside [0, nv)
// (a ghost tail in a local row) is skipped.
//
// Compact: from `active` and the phase-static degree class of every vertex
// (0-6 the LDS classes, 7 hub, 8 edgeless) produce the ascending vertex list
// of every class in one buffer. A wave owns FC_UNIT consecutive vertices and
// ranks its members per class with ballots, so the lists are stable. Pass 1
// (WRITE = false) stores the per-wave class counts; the host side scans them
// into per-wave offsets and class bases with no sync; pass 2 (WRITE = true)
// repeats the ballots and stores the ids. No atomics.
// ---------------------------------------------------------------------------

constexpr int FX_SPAN = 1024;   // edges per wave in frontier_expand_kernel
constexpr int FC_CLASSES = 9;   // 7 LDS classes, hubs, edgeless
constexpr int FC_ITEMS = 16;    // 64-vertex chunks per wave
constexpr int FC_UNIT = 64 * FC_ITEMS;

// Degree of dense id x: a local row, a ghost row, or nothing.
DEV_INLINE int64_t fx_degree(const int64_t* __restrict__ rowptr, int64_t nv,
                             const int64_t* __restrict__ g_rowptr, int64_t ng,
                             int32_t x) {
  if (x < 0) return 0;
  if (x < nv) return rowptr[x + 1] - rowptr[x];
  const int64_t g = (int64_t)x - nv;
  return g < ng ? g_rowptr[g + 1] - g_rowptr[g] : 0;
}

__global__ void frontier_degrees_kernel(
    const int32_t* __restrict__ changed, int64_t nc,
    const int64_t* __restrict__ rowptr, int64_t nv,
    const int64_t* __restrict__ g_rowptr, int64_t ng,
    int64_t* __restrict__ deg_out, uint8_t* __restrict__ active) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nc;
       i += stride) {
    const int32_t x = changed[i];
    deg_out[i] = fx_degree(rowptr, nv, g_rowptr, ng, x);
    if (x >= 0 && x < nv) active[x] = 1;
  }
}

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void frontier_expand_kernel(
    const int32_t* __restrict__ changed, int64_t nc,
    const int64_t* __restrict__ offs, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ tails, int64_t nv, int64_t ne,
    const int64_t* __restrict__ g_rowptr, const int32_t* __restrict__ g_heads,
    int64_t ng, int64_t neg, uint8_t* __restrict__ active) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t total = offs[nc];
  const int64_t nspan = (total + FX_SPAN - 1) / FX_SPAN;
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * FX_SPAN;
    const int64_t s1 = (s0 + FX_SPAN < total) ? s0 + FX_SPAN : total;
    int64_t rlo, rhi;
    span_row_range(offs, nc, s0, s1, rlo, rhi);
    for (int64_t c = s0; c < s1; c += 64) {  // wave-uniform bounds
      const int64_t e = c + lane;
      int64_t r = -1;
      if (e < s1) {
        r = row_of_edge(offs, rlo, rhi, e);
        const int64_t k = e - offs[r];
        const int32_t x = changed[r];
        int32_t u = -1;
        if (x >= 0 && x < nv) {
          const int64_t idx = rowptr[x] + k;
          if (idx < ne) u = tails[idx];
        } else if (x >= nv && (int64_t)x - nv < ng) {
          const int64_t idx = g_rowptr[(int64_t)x - nv] + k;
          if (idx < neg) u = g_heads[idx];
        }
        if (u >= 0 && u < nv) active[u] = 1;
      }
      const int64_t last_row = __shfl(r, 63, 64);
      if (last_row >= 0) rlo = last_row;
    }
  }
}

template <bool WRITE>
__global__ __launch_bounds__(256) void frontier_compact_kernel(
    const uint8_t* __restrict__ active, const uint8_t* __restrict__ cls,
    int64_t nv, int64_t nunit, int32_t* __restrict__ unit_cnt,
    const int32_t* __restrict__ unit_off,
    const int32_t* __restrict__ class_base, int32_t* __restrict__ lists) {
  const int lane = threadIdx.x % 64;
  const int64_t unit = (int64_t)blockIdx.x * (blockDim.x / 64) +
                       threadIdx.x / 64;
  if (unit >= nunit) return;  // wave-uniform
  int32_t run[FC_CLASSES];
#pragma unroll
  for (int c = 0; c < FC_CLASSES; c++)
    run[c] = WRITE ? class_base[c] + unit_off[unit * FC_CLASSES + c] : 0;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const int64_t v0 = unit * FC_UNIT;
  for (int i = 0; i < FC_ITEMS; i++) {
    const int64_t v = v0 + (int64_t)i * 64 + lane;
    int k = -1;
    if (v < nv && active[v]) k = cls[v];
#pragma unroll
    for (int c = 0; c < FC_CLASSES; c++) {
      const uint64_t m = __ballot(k == c);
      if (WRITE && k == c) {
        // all lists together hold at most nv ids (memory-safety guard)
        const int64_t idx = (int64_t)run[c] + __popcll(m & below);
        if (idx < nv) lists[idx] = (int32_t)v;
      }
      run[c] += __popcll(m);
    }
  }
  if (!WRITE && lane == 0) {
#pragma unroll
    for (int c = 0; c < FC_CLASSES; c++)
      unit_cnt[unit * FC_CLASSES + c] = run[c];
  }
}

// ---------------------------------------------------------------------------
// Edge batches (cuvite_amd/dynamic.py, apply_edge_batch): the new CSR after
// a batch of deletions and insertions, rows in the stable order of
// dynamic.apply_routed_batch_torch. A batch of k edges touches at most 2k
// rows; every other row of the new CSR is the old row at another offset. The
// host side sorts the (batch-sized) lists and hands over the nt touched rows,
// each with its slice of the deletions (ascending tails, deduplicated) and of
// the insertions (list order). The touched rows' old entries are concatenated
// into one edge space of t_offs[nt] entries, cut into spans of BA_SPAN with
// one wave each, exactly as frontier_expand_kernel cuts the changed rows: a
// touched hub is spread over many waves.
//
// Mark     every lane binary-searches its entry's tail in its row's deletion
//          slice and stores the keep flag; a hit stores 1 into the matched
//          byte of that deletion (idempotent plain store). Kept counts: one
//          per span from the ballots, one per row from the runs of equal rows
//          in the ballots. A run that goes on into the next chunk is carried
//          in registers, so a row is written once per span it meets: a plain
//          store where the row lies inside the span, an integer atomic add
//          into the zeroed array where spans cut it (integer addition: the
//          order does not matter).
// Copy     over ALL old entries in spans of BA_COPY_SPAN as
//          intra_weight_kernel cuts them: an entry of an untouched row goes
//          to new_rowptr[row] + (e - rowptr[row]); consecutive lanes read
//          and write consecutive addresses. Entries of touched rows are
//          skipped before they are loaded.
// Compact  over the touched edge space again: a kept entry goes to its
//          stable position, span offset (exclusive scan of the span counts)
//          plus ballot prefix, rebased from the kept-entry space to the row's
//          start in the new CSR. Positions come from counts only, no atomics.
// Insert   entry j of the sorted insertion list goes behind its row's kept
//          entries, at its index inside the row's slice.
//
// Every loop is bounded by its span, there is no wait between waves and no
// float atomic; every store into the new CSR is bounds-checked.
// ---------------------------------------------------------------------------

constexpr int BA_SPAN = 1024;       // touched entries per wave (mark, compact)
constexpr int BA_COPY_SPAN = 4096;  // old entries per wave (copy)

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void batch_mark_kernel(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ tails,
    int64_t ne, const int64_t* __restrict__ t_rows,
    const int64_t* __restrict__ t_offs, int64_t nt, int64_t total,
    const int64_t* __restrict__ d_offs, const int64_t* __restrict__ d_dst,
    int64_t nd, uint8_t* __restrict__ d_matched, uint8_t* __restrict__ keep,
    int64_t* __restrict__ span_cnt, int64_t* __restrict__ row_kept) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const uint64_t from_lane = ~(((uint64_t)1 << lane) - 1);  // lanes >= lane
  const int64_t nspan = (total + BA_SPAN - 1) / BA_SPAN;
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * BA_SPAN;
    const int64_t s1 = (s0 + BA_SPAN < total) ? s0 + BA_SPAN : total;
    int64_t rlo, rhi;
    span_row_range(t_offs, nt, s0, s1, rlo, rhi);
    int64_t kept_span = 0;
    int64_t carry_row = -1;  // row whose run goes on from the last chunk
    int64_t carry_cnt = 0;
    for (int64_t c = s0; c < s1; c += 64) {  // wave-uniform bounds
      const int64_t e = c + lane;
      const bool valid = e < s1;
      int64_t r = -1;
      bool kp = false;
      if (valid) {
        r = row_of_edge(t_offs, rlo, rhi, e);
        const int64_t idx = rowptr[t_rows[r]] + (e - t_offs[r]);
        kp = true;
        if (idx >= 0 && idx < ne) {
          const int64_t t = tails[idx];
          int64_t lo = d_offs[r];
          int64_t end = d_offs[r + 1];
          if (lo < 0) lo = 0;
          if (end > nd) end = nd;
          int64_t hi = end;
          while (lo < hi) {  // first deletion of the row with d_dst >= t
            const int64_t m = (lo + hi) >> 1;
            if (d_dst[m] < t) lo = m + 1; else hi = m;
          }
          if (lo < end && d_dst[lo] == t) {
            kp = false;
            d_matched[lo] = 1;
          }
        }
        keep[e] = kp ? 1 : 0;
      }
      const uint64_t keptm = __ballot(kp);
      kept_span += __popcll(keptm);
      // runs of equal rows are contiguous lanes; the first lane of a run
      // counts the run's kept entries
      const int64_t prev_r = __shfl_up(r, 1, 64);
      const bool head = valid && (lane == 0 || prev_r != r);
      const uint64_t heads = __ballot(head);  // lane 0 is valid: not empty
      const uint64_t above = lane == 63 ? 0 : heads & (from_lane << 1);
      const int nh = above ? __ffsll((unsigned long long)above) - 1 : 64;
      const uint64_t upto = nh == 64 ? ~(uint64_t)0 : ((uint64_t)1 << nh) - 1;
      int64_t cnt = __popcll(keptm & upto & from_lane);
      if (head && r == carry_row) cnt += carry_cnt;
      const int64_t last_valid = (c + 64 < s1 ? c + 64 : s1) - 1;
      bool emit = false, carry = false;
      if (head) {
        if (nh < 64) emit = true;  // the run ends inside the chunk
        else if (t_offs[r + 1] - 1 <= last_valid || last_valid == s1 - 1)
          emit = true;             // the row or the span ends with the chunk
        else carry = true;
      }
      if (emit) {
        if (t_offs[r] >= s0 && t_offs[r + 1] <= s1)
          row_kept[r] = cnt;
        else
          atomicAdd((unsigned long long*)&row_kept[r],
                    (unsigned long long)cnt);
      }
      const int last_head = 63 - __clzll((long long)heads);
      const int carried = __shfl(carry ? 1 : 0, last_head, 64);
      const int64_t c_cnt = __shfl(cnt, last_head, 64);
      const int64_t c_row = __shfl(r, last_head, 64);
      carry_row = carried ? c_row : -1;
      carry_cnt = carried ? c_cnt : 0;
      const int64_t last_row = __shfl(r, 63, 64);
      if (last_row >= 0) rlo = last_row;
    }
    if (lane == 0) span_cnt[s] = kept_span;
  }
}

template <typename W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void batch_copy_kernel(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ tails,
    const W* __restrict__ weights, int64_t nv, int64_t ne,
    const uint8_t* __restrict__ touched,
    const int64_t* __restrict__ new_rowptr, int64_t new_ne,
    int64_t* __restrict__ new_tails, W* __restrict__ new_weights) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t nspan = (ne + BA_COPY_SPAN - 1) / BA_COPY_SPAN;
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * BA_COPY_SPAN;
    const int64_t s1 = (s0 + BA_COPY_SPAN < ne) ? s0 + BA_COPY_SPAN : ne;
    int64_t rlo, rhi;
    span_row_range(rowptr, nv, s0, s1, rlo, rhi);
    for (int64_t c = s0; c < s1; c += 64) {  // wave-uniform bounds
      const int64_t e = c + lane;
      int64_t r = -1;
      if (e < s1) {
        r = row_of_edge(rowptr, rlo, rhi, e);
        if (!touched[r]) {  // a touched row's entries are not even read
          const int64_t dst = new_rowptr[r] + (e - rowptr[r]);
          if (dst >= 0 && dst < new_ne) {
            new_tails[dst] = tails[e];
            new_weights[dst] = weights[e];
          }
        }
      }
      const int64_t last_row = __shfl(r, 63, 64);
      if (last_row >= 0) rlo = last_row;
    }
  }
}

template <typename W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void batch_compact_kernel(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ tails,
    const W* __restrict__ weights, int64_t ne,
    const int64_t* __restrict__ t_rows, const int64_t* __restrict__ t_offs,
    int64_t nt, int64_t total, const uint8_t* __restrict__ keep,
    const int64_t* __restrict__ span_offs,
    const int64_t* __restrict__ kept_offs,
    const int64_t* __restrict__ new_rowptr, int64_t new_ne,
    int64_t* __restrict__ new_tails, W* __restrict__ new_weights) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const uint64_t below = ((uint64_t)1 << lane) - 1;
  const int64_t nspan = (total + BA_SPAN - 1) / BA_SPAN;
  const int64_t sstride = (int64_t)gridDim.x * WAVES;
  for (int64_t s = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64; s < nspan;
       s += sstride) {
    const int64_t s0 = s * BA_SPAN;
    const int64_t s1 = (s0 + BA_SPAN < total) ? s0 + BA_SPAN : total;
    int64_t rlo, rhi;
    span_row_range(t_offs, nt, s0, s1, rlo, rhi);
    int64_t run = span_offs[s];  // kept entries before this span
    for (int64_t c = s0; c < s1; c += 64) {  // wave-uniform bounds
      const int64_t e = c + lane;
      const bool valid = e < s1;
      int64_t r = -1;
      bool kp = false;
      if (valid) {
        r = row_of_edge(t_offs, rlo, rhi, e);
        kp = keep[e] != 0;
      }
      const uint64_t m = __ballot(kp);
      if (kp) {
        const int64_t v = t_rows[r];
        const int64_t idx = rowptr[v] + (e - t_offs[r]);
        const int64_t rank = run + __popcll(m & below);
        const int64_t dst = new_rowptr[v] + (rank - kept_offs[r]);
        if (idx >= 0 && idx < ne && dst >= 0 && dst < new_ne) {
          new_tails[dst] = tails[idx];
          new_weights[dst] = weights[idx];
        }
      }
      run += __popcll(m);
      const int64_t last_row = __shfl(r, 63, 64);
      if (last_row >= 0) rlo = last_row;
    }
  }
}

template <typename W>
__global__ void batch_insert_kernel(
    const int64_t* __restrict__ t_rows, int64_t nt,
    const int64_t* __restrict__ i_offs, const int64_t* __restrict__ i_dst,
    const W* __restrict__ i_w, int64_t ni,
    const int64_t* __restrict__ row_kept,
    const int64_t* __restrict__ new_rowptr, int64_t new_ne,
    int64_t* __restrict__ new_tails, W* __restrict__ new_weights) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < ni;
       j += stride) {
    const int64_t r = row_of_edge(i_offs, 0, nt - 1, j);
    const int64_t dst = new_rowptr[t_rows[r]] + row_kept[r] + (j - i_offs[r]);
    if (dst >= 0 && dst < new_ne) {
      new_tails[dst] = i_dst[j];
      new_weights[dst] = i_w[j];
    }
  }
}

// ---------------------------------------------------------------------------
// Hub candidate generation via rocPRIM: gather the neighbours' community
// ids, then a per-hub segmented radix sort of those keys (only
// ceil(log2 C) bits) with the edge weights as payload. The torch fallback
// sorts full 64-bit packed keys; the narrow-bit segmented sort does about
// half the radix passes.
// ---------------------------------------------------------------------------

__global__ void gather_comm_kernel(const int32_t* __restrict__ tails_flat,
                                   const int32_t* __restrict__ curr_comm,
                                   int64_t n, int32_t* __restrict__ keys) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += stride)
    keys[i] = curr_comm[tails_flat[i]];
}

// ---------------------------------------------------------------------------
// Hub argmax straight from the sorted (community, weight) pairs: after the
// segmented sort every hub's segment [eoffs[h], eoffs[h+1]) of keys2/vals2
// holds its neighbour communities in ascending order, equal ones adjacent
// (a "run"). Three kernels read that once (12 B per hub edge) and write
// only O(nhub * HUB_SLICES) scratch:
//
//   hub_own_weight_kernel  the weight into the hub's own community cc is a
//       constant inside every gain, so it has to exist before any gain is
//       evaluated: a wave-cooperative 64-ary search finds the run of cc and
//       the run is summed in HUB_SLICES equal shares (it can hold 10^5-10^6
//       edges), one partial per wave.
//   hub_slice_kernel       the segment is cut into HUB_SLICES equal element
//       slices, one wave each, so the work per wave is bounded by elements
//       however long a run is (the mega-hub imbalance the split argmax was
//       introduced for, profiles/round2_kernel_stats). A wave walks its
//       slice in 64-element chunks with a segmented shuffle scan and a
//       (key, sum) carry between chunks (the intra_weight_kernel pattern),
//       evaluates the gain of every run that lies wholly inside the slice at
//       the run's last lane, and hands the slice's first and last run, which
//       may continue in a neighbour slice, on as (key, sum) records.
//   hub_final_kernel       one wave per hub, one record per lane: records
//       with equal keys are pieces of one run (the segment is sorted) and
//       are summed in slice order, their gains evaluated, the partial bests
//       folded, the singleton guard applied, target and cw written and, on
//       the fused path, the new community aggregates accounted.
//
// Every sum is fp64 in an order fixed by the slice layout (no float atomics
// on weights), rounded to the weight type once per run like the LDS tables'
// entries; gains come from move_gain, like the class kernels'.
// ---------------------------------------------------------------------------

constexpr int HUB_SLICES = 32;   // 2 records per slice = one per final lane
constexpr int HUB_PIPE = 4;      // chunks of loads in flight per wave
static_assert(2 * HUB_SLICES == 64, "hub_final_kernel: one record per lane");

// First index i in [lo, hi) with a[i] >= key, hi if none; a ascending on
// [lo, hi). All 64 lanes take part and get the same answer: each round
// probes 64 evenly spaced elements, so a 10^6-element segment takes 4
// dependent loads instead of 20.
DEV_INLINE int64_t wave_lower_bound(const int32_t* __restrict__ a, int64_t lo,
                                    int64_t hi, int32_t key, int lane) {
  while (hi - lo > 64) {
    const int64_t step = (hi - lo + 63) / 64;
    const int64_t p = lo + (int64_t)lane * step;
    const bool ge = (p < hi) ? (a[p] >= key) : true;
    const unsigned long long m = __ballot(ge);
    if (m == 0ull) {            // all 64 probes in range and below key
      lo = lo + 63 * step + 1;
      continue;
    }
    const int f = __ffsll(m) - 1;
    if (f == 0) return lo;      // a[lo] >= key
    const int64_t pf = lo + (int64_t)f * step;
    lo = lo + (int64_t)(f - 1) * step + 1;
    hi = pf < hi ? pf : hi;
  }
  const int64_t p = lo + lane;
  const bool ge = (p < hi) ? (a[p] >= key) : true;
  const unsigned long long m = __ballot(ge);
  return m ? lo + (__ffsll(m) - 1) : hi;
}

// Sum of the HUB_SLICES own-weight partials of hub `hidx`, in one fixed
// order (same bits in every wave that asks).
DEV_INLINE double hub_own_weight(const double* __restrict__ p_wcc, int hidx,
                                 int lane) {
  const double v =
      lane < HUB_SLICES ? p_wcc[(int64_t)hidx * HUB_SLICES + lane] : 0.0;
  return __shfl(sum_reduce<64>(v), 0, 64);
}

template <typename W, int BLOCK>
__global__ __launch_bounds__(BLOCK) void hub_own_weight_kernel(
    const int32_t* __restrict__ keys, const W* __restrict__ vals,
    const int64_t* __restrict__ eoffs, const int32_t* __restrict__ hubs,
    int nhub, const int32_t* __restrict__ curr_comm,
    double* __restrict__ p_wcc) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t w = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64;
  const int hidx = (int)(w / HUB_SLICES);
  const int part = (int)(w % HUB_SLICES);
  if (hidx >= nhub) return;
  const int32_t cc = curr_comm[hubs[hidx]];
  const int64_t b = eoffs[hidx], e = eoffs[hidx + 1];
  const int64_t r0 = wave_lower_bound(keys, b, e, cc, lane);
  // keys are dense community ids < 2^31 - 1, so cc + 1 does not overflow
  const int64_t r1 = wave_lower_bound(keys, r0, e, cc + 1, lane);
  const int64_t len = r1 - r0;
  const int64_t s0 = r0 + part * len / HUB_SLICES;
  const int64_t s1 = r0 + (part + 1) * len / HUB_SLICES;
  double acc = 0.0;
  for (int64_t i = s0 + lane; i < s1; i += 64) acc += (double)vals[i];
  acc = sum_reduce<64>(acc);
  if (lane == 0) p_wcc[w] = acc;
}

// REFINE (a refinement round, as in lv_move_sub): a hub that does not move
// this round leaves at once (wave-uniform; hub_final_kernel does not read
// its slice records), and a run's gain is folded only if the run's community
// has the mover's bound.
template <typename W, int BLOCK, bool REFINE>
__global__ __launch_bounds__(BLOCK) void hub_slice_kernel(
    const int32_t* __restrict__ keys, const W* __restrict__ vals,
    const int64_t* __restrict__ eoffs, const int32_t* __restrict__ hubs,
    int nhub, const double* __restrict__ hub_self,
    const double* __restrict__ p_wcc, const int32_t* __restrict__ curr_comm,
    const W* __restrict__ v_degree, const W* __restrict__ comm_degree,
    const int64_t* __restrict__ comm_gid, int64_t gid_base, int32_t n_local,
    double constant, double* __restrict__ p_gain, int64_t* __restrict__ p_gid,
    int32_t* __restrict__ p_dense, int32_t* __restrict__ r_key,
    double* __restrict__ r_sum, const int32_t* __restrict__ mover_bound,
    const int32_t* __restrict__ cand_bound) {
  constexpr int WAVES = BLOCK / 64;
  const int lane = threadIdx.x % 64;
  const int64_t w = (int64_t)blockIdx.x * WAVES + threadIdx.x / 64;
  const int hidx = (int)(w / HUB_SLICES);
  const int part = (int)(w % HUB_SLICES);
  if (hidx >= nhub) return;
  const int32_t v = hubs[hidx];
  int32_t mb = -1;
  if (REFINE) {
    mb = mover_bound[v];
    if (mb < 0) return;
  }
  const int32_t cc = curr_comm[v];
  const int64_t b = eoffs[hidx], e = eoffs[hidx + 1];
  const int64_t len = e - b;
  const int64_t s0 = b + part * len / HUB_SLICES;
  const int64_t s1 = b + (part + 1) * len / HUB_SLICES;
  Best best{0.0, gid_of(comm_gid, gid_base, n_local, cc), cc};
  if (s0 == s1) {  // wave-uniform: a segment shorter than HUB_SLICES
    if (lane == 0) {
      r_key[2 * w] = EMPTY_KEY;
      r_key[2 * w + 1] = EMPTY_KEY;
      p_gain[w] = best.gain;
      p_gid[w] = best.gid;
      p_dense[w] = best.dense;
    }
    return;
  }
  const W wcc = (W)hub_own_weight(p_wcc, hidx, lane);
  const double eix = (double)wcc - hub_self[hidx];
  const double vdeg = (double)v_degree[v];
  const double ax = (double)comm_degree[cc] - vdeg;
  // the runs of these two keys may go on in a neighbour slice
  const int32_t first_key = keys[s0], last_key = keys[s1 - 1];

  double carry_sum = 0.0;
  int32_t carry_key = EMPTY_KEY;  // key whose run the last chunk left open
  for (int64_t c = s0; c < s1; c += (int64_t)HUB_PIPE * 64) {
    int32_t k[HUB_PIPE], kn[HUB_PIPE];
    W x[HUB_PIPE];
#pragma unroll
    for (int j = 0; j < HUB_PIPE; j++) {
      const int64_t i = c + j * 64 + lane;
      k[j] = i < s1 ? keys[i] : -2;           // past the slice: inert run
      x[j] = i < s1 ? vals[i] : (W)0;
      kn[j] = i + 1 < s1 ? keys[i + 1] : -3;  // the slice's last lane: tail
    }
#pragma unroll
    for (int j = 0; j < HUB_PIPE; j++) {
      if (c + j * 64 >= s1) break;  // wave-uniform
      const int32_t kk = k[j];
      double val = (double)x[j];
      if (lane == 0 && kk == carry_key) val += carry_sum;
      // segmented inclusive scan: equal keys are contiguous lanes
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const double pv = __shfl_up(val, off, 64);
        const int32_t pk = __shfl_up(kk, off, 64);
        if (lane >= off && pk == kk) val += pv;
      }
      const bool tail = kk >= 0 && kn[j] != kk;
      if (tail) {
        if (kk == first_key) {
          r_key[2 * w] = kk;
          r_sum[2 * w] = val;
        } else if (kk == last_key) {
          r_key[2 * w + 1] = kk;
          r_sum[2 * w + 1] = val;
        } else if (kk != cc && (!REFINE || cand_bound[kk] == mb)) {
          const double eiy = (double)(W)val;
          const double ay = (double)comm_degree[kk];
          const double g = move_gain(eiy, eix, vdeg, ay, ax, constant);
          best_combine(best, g, gid_of(comm_gid, gid_base, n_local, kk), kk);
        }
      }
      // only a full chunk can end inside a run
      carry_sum = __shfl(val, 63, 64);
      carry_key = __shfl(tail ? EMPTY_KEY : kk, 63, 64);
    }
  }
  best_reduce<64>(best);
  if (lane == 0) {
    if (first_key == last_key) r_key[2 * w + 1] = EMPTY_KEY;
    p_gain[w] = best.gain;
    p_gid[w] = best.gid;
    p_dense[w] = best.dense;
  }
}

// REFINE: a hub that does not move this round keeps its label (cw 0, like a
// vertex the class kernels skip); the stitched runs pass the same bound
// filter as the runs inside a slice; no singleton guard, no aggregate
// accounting.
template <typename W, int BLOCK, bool REFINE>
__global__ __launch_bounds__(BLOCK) void hub_final_kernel(
    const int32_t* __restrict__ hubs, int nhub,
    const double* __restrict__ hub_self, const double* __restrict__ p_wcc,
    const int32_t* __restrict__ curr_comm, const W* __restrict__ v_degree,
    const int64_t* __restrict__ comm_size, const W* __restrict__ comm_degree,
    const int64_t* __restrict__ comm_gid, int64_t gid_base, int32_t n_local,
    double constant, const double* __restrict__ p_gain,
    const int64_t* __restrict__ p_gid, const int32_t* __restrict__ p_dense,
    const int32_t* __restrict__ r_key, const double* __restrict__ r_sum,
    int32_t* __restrict__ target_hub, W* __restrict__ cw_hub,
    int64_t* __restrict__ next_size, W* __restrict__ next_degree,
    int64_t n_next, const int32_t* __restrict__ mover_bound,
    const int32_t* __restrict__ cand_bound) {
  constexpr int WAVES = BLOCK / 64;
  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int hidx = blockIdx.x * WAVES + wave;
  if (hidx >= nhub) return;
  const int32_t v = hubs[hidx];
  const int32_t cc = curr_comm[v];
  int32_t mb = -1;
  if (REFINE) {
    mb = mover_bound[v];
    if (mb < 0) {  // wave-uniform
      if (lane == 0) {
        target_hub[hidx] = cc;
        cw_hub[hidx] = (W)0;
      }
      return;
    }
  }
  const W wcc = (W)hub_own_weight(p_wcc, hidx, lane);
  const double eix = (double)wcc - hub_self[hidx];
  const W vdeg_w = v_degree[v];
  const double vdeg = (double)vdeg_w;
  const double ax = (double)comm_degree[cc] - vdeg;
  const int64_t gid_cc = gid_of(comm_gid, gid_base, n_local, cc);
  Best best{0.0, gid_cc, cc};
  if (lane < HUB_SLICES) {
    const int64_t p = (int64_t)hidx * HUB_SLICES + lane;
    best = Best{p_gain[p], p_gid[p], p_dense[p]};
  }
  // lane = record (2 * slice + {first, last}), i.e. records in slice order
  const int64_t r = (int64_t)hidx * 2 * HUB_SLICES + lane;
  const int32_t key = r_key[r];
  const double sum = key >= 0 ? r_sum[r] : 0.0;
  double total = 0.0;
  bool leader = key >= 0;  // lowest lane of its key evaluates the run
#pragma unroll 4
  for (int j = 0; j < 64; j++) {
    const int32_t kj = __shfl(key, j, 64);
    const double sj = __shfl(sum, j, 64);
    if (kj == key) {
      total += sj;
      if (j < lane) leader = false;
    }
  }
  if (leader && key != cc && (!REFINE || cand_bound[key] == mb)) {
    const double eiy = (double)(W)total;
    const double ay = (double)comm_degree[key];
    const double g = move_gain(eiy, eix, vdeg, ay, ax, constant);
    best_combine(best, g, gid_of(comm_gid, gid_base, n_local, key), key);
  }
  best_reduce<64>(best);
  if (lane == 0) {
    int32_t tgt = best.dense;
    // singleton-swap guard (louvain.cpp:2238-2239)
    if (!REFINE && comm_size[tgt] == 1 && comm_size[cc] == 1 &&
        best.gid > gid_cc)
      tgt = cc;
    target_hub[hidx] = tgt;
    cw_hub[hidx] = wcc;
    if (!REFINE) account_target(next_size, next_degree, n_next, tgt, vdeg_w);
  }
}

// ------------------------------- launchers ---------------------------------

static int grid_for(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  // >> 2048 workgroups keeps all 8 XCDs fed; cap to bound tail latency
  return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

// One row of CLASS_TABLE. The sub and the block kernel take the same
// parameters; they differ in the vertices a block serves (GROUPS).
template <typename W, int C, bool REFINE>
static auto class_kernel() {
  constexpr ClassGeometry g = CLASS_TABLE[C];
  if constexpr (g.lanes != 0)
    return lv_move_sub<W, g.lanes, g.cap, CLASS_BLOCK, REFINE>;
  else
    return lv_move_block<W, g.cap, CLASS_BLOCK, REFINE>;
}

// Walks CLASS_TABLE at compile time down to row c and launches its kernel.
template <typename W, bool REFINE, int C = 0>
static void launch_class_row(int c, const int32_t* vlist, int nlist,
                             const MoveArgs<W>& a, hipStream_t stream) {
  if constexpr (C < NUM_CLASSES) {
    if (c != C)
      return launch_class_row<W, REFINE, C + 1>(c, vlist, nlist, a, stream);
    constexpr ClassGeometry g = CLASS_TABLE[C];
    constexpr int GROUPS = g.lanes != 0 ? CLASS_BLOCK / g.lanes : 1;
    const int grid = (nlist + GROUPS - 1) / GROUPS;
    const size_t shmem =
        (size_t)GROUPS * g.cap * (sizeof(W) + sizeof(int32_t));
    auto kern = class_kernel<W, C, REFINE>();
    if (shmem > 65536)
      (void)hipFuncSetAttribute((const void*)kern,
                                hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)shmem);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(CLASS_BLOCK), shmem, stream,
                       vlist, nlist, a.rowptr, a.tails, a.weights,
                       a.curr_comm, a.v_degree, a.comm_size, a.comm_degree,
                       a.comm_gid, a.constant, a.target, a.cluster_weight,
                       a.gid_base, a.n_local, a.next_size, a.next_degree,
                       a.n_next, a.mover_bound, a.cand_bound);
  }
}

// REFINE = false: the plain kernels (the bound arrays are null and not
// read); REFINE = true: the refine kernels, same grids and tables. A class
// outside the table launches nothing.
template <typename W>
void launch_class(int c, const int32_t* vlist, int nlist,
                  const MoveArgs<W>& args, hipStream_t stream) {
  if (args.mover_bound != nullptr)
    launch_class_row<W, true>(c, vlist, nlist, args, stream);
  else
    launch_class_row<W, false>(c, vlist, nlist, args, stream);
}
template void launch_class<float>(int, const int32_t*, int,
                                  const MoveArgs<float>&, hipStream_t);
template void launch_class<double>(int, const int32_t*, int,
                                   const MoveArgs<double>&, hipStream_t);

template <typename W>
void launch_modularity(const W* cw, const W* cd, int64_t nv, double* out,
                       hipStream_t stream) {
  constexpr int BLOCK = 256;
  int grid = (int)((nv + BLOCK - 1) / BLOCK);
  if (grid > 2048) grid = 2048;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL((modularity_reduce<W, BLOCK>), dim3(grid), dim3(BLOCK), 0,
                     stream, cw, cd, nv, out);
}

template void launch_modularity<float>(const float*, const float*, int64_t,
                                       double*, hipStream_t);
template void launch_modularity<double>(const double*, const double*, int64_t,
                                        double*, hipStream_t);

template <typename W>
void launch_scatter_add(W* out, const int64_t* idx, const W* val, int64_t n,
                        hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL((scatter_add_kernel<W>), dim3(grid_for(n, 256)),
                     dim3(256), 0, stream, out, idx, val, n);
}
template void launch_scatter_add<float>(float*, const int64_t*, const float*,
                                        int64_t, hipStream_t);
template void launch_scatter_add<double>(double*, const int64_t*,
                                         const double*, int64_t, hipStream_t);

// Fresh recount of the community aggregates from scratch: one pass, two
// atomics per vertex. At world=1 in a heavy-move regime this beats the
// delta update (4 atomics per MOVED vertex; rocprof: 25 ms vs ~12 at s26
// where most vertices move every oscillating sweep). The distributed path
// keeps deltas (owners need only the cross-rank changes).
template <typename W>
__global__ void recount_kernel(const int64_t* __restrict__ labels,
                               const W* __restrict__ v_degree, int64_t nv,
                               int64_t base, int64_t ncomm,
                               int64_t* __restrict__ size,
                               W* __restrict__ degree) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv;
       i += stride) {
    const int64_t c = labels[i] - base;
    // world-1 labels are local by construction; the bounds check is a
    // memory-safety guard (an OOB label must not corrupt memory)
    if (c < 0 || c >= ncomm) continue;
    atomicAdd((unsigned long long*)&size[c], 1ull);
    unsafeAtomicAdd(&degree[c], v_degree[i]);
  }
}

template <typename W>
void launch_recount(const int64_t* labels, const W* v_degree, int64_t nv,
                    int64_t base, int64_t ncomm, int64_t* size, W* degree,
                    hipStream_t stream) {
  if (nv == 0) return;
  hipLaunchKernelGGL((recount_kernel<W>), dim3(grid_for(nv, 256)), dim3(256),
                     0, stream, labels, v_degree, nv, base, ncomm, size,
                     degree);
}
template void launch_recount<float>(const int64_t*, const float*, int64_t,
                                    int64_t, int64_t, int64_t*, float*,
                                    hipStream_t);
template void launch_recount<double>(const int64_t*, const double*, int64_t,
                                     int64_t, int64_t, int64_t*, double*,
                                     hipStream_t);

template <typename W>
void launch_apply_deltas(const int64_t* target, const int64_t* curr,
                         const W* v_degree, int64_t nv, int64_t base,
                         int64_t bound, int64_t* local_size, W* local_degree,
                         hipStream_t stream) {
  if (nv == 0) return;
  hipLaunchKernelGGL((apply_deltas_kernel<W>), dim3(grid_for(nv, 256)),
                     dim3(256), 0, stream, target, curr, v_degree, nv, base,
                     bound, local_size, local_degree);
}
template void launch_apply_deltas<float>(const int64_t*, const int64_t*,
                                         const float*, int64_t, int64_t,
                                         int64_t, int64_t*, float*,
                                         hipStream_t);
template void launch_apply_deltas<double>(const int64_t*, const int64_t*,
                                          const double*, int64_t, int64_t,
                                          int64_t, int64_t*, double*,
                                          hipStream_t);

void launch_degree_count(const int64_t* src, int64_t n, int64_t base,
                         int32_t* cnt, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(degree_count_kernel, dim3(grid_for(n, 256)), dim3(256), 0,
                     stream, src, n, base, cnt);
}

template <typename W>
void launch_csr_place(const int64_t* src, const int64_t* dst, const W* w,
                      int64_t n, int64_t base, const int64_t* rowptr,
                      int32_t* cursor, int64_t* tails_out, W* w_out,
                      hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL((csr_place_kernel<W>), dim3(grid_for(n, 256)), dim3(256),
                     0, stream, src, dst, w, n, base, rowptr, cursor,
                     tails_out, w_out);
}
template void launch_csr_place<float>(const int64_t*, const int64_t*,
                                      const float*, int64_t, int64_t,
                                      const int64_t*, int32_t*, int64_t*,
                                      float*, hipStream_t);
template void launch_csr_place<double>(const int64_t*, const int64_t*,
                                       const double*, int64_t, int64_t,
                                       const int64_t*, int32_t*, int64_t*,
                                       double*, hipStream_t);

void launch_gather_comm(const int32_t* tails_flat, const int32_t* curr_comm,
                        int64_t n, int32_t* keys, hipStream_t stream) {
  if (n == 0) return;
  hipLaunchKernelGGL(gather_comm_kernel, dim3(grid_for(n, 256)), dim3(256), 0,
                     stream, tails_flat, curr_comm, n, keys);
}

// The own-weight kernel is shared; the slice and final kernels are plain or
// REFINE instantiations, chosen like the class kernels'.
template <typename W, bool REFINE>
static void launch_hub_argmax_impl(const HubArgs<W>& h, hipStream_t stream) {
  constexpr int BLOCK = 256;
  constexpr int WAVES = BLOCK / 64;
  static_assert(HUB_SLICES % WAVES == 0, "whole blocks per hub");
  const dim3 slice_grid((uint32_t)h.nhub * (HUB_SLICES / WAVES));
  hipLaunchKernelGGL((hub_own_weight_kernel<W, BLOCK>), slice_grid,
                     dim3(BLOCK), 0, stream, h.keys, h.vals, h.eoffs, h.hubs,
                     h.nhub, h.curr_comm, h.p_wcc);
  hipLaunchKernelGGL((hub_slice_kernel<W, BLOCK, REFINE>), slice_grid,
                     dim3(BLOCK), 0, stream, h.keys, h.vals, h.eoffs, h.hubs,
                     h.nhub, h.hub_self, h.p_wcc, h.curr_comm, h.v_degree,
                     h.comm_degree, h.comm_gid, h.gid_base, h.n_local,
                     h.constant, h.p_gain, h.p_gid, h.p_dense, h.r_key,
                     h.r_sum, h.mover_bound, h.cand_bound);
  hipLaunchKernelGGL((hub_final_kernel<W, BLOCK, REFINE>),
                     dim3((h.nhub + WAVES - 1) / WAVES), dim3(BLOCK), 0,
                     stream, h.hubs, h.nhub, h.hub_self, h.p_wcc, h.curr_comm,
                     h.v_degree, h.comm_size, h.comm_degree, h.comm_gid,
                     h.gid_base, h.n_local, h.constant, h.p_gain, h.p_gid,
                     h.p_dense, h.r_key, h.r_sum, h.target_hub, h.cw_hub,
                     h.next_size, h.next_degree, h.n_next, h.mover_bound,
                     h.cand_bound);
}

template <typename W>
void launch_hub_argmax(const HubArgs<W>& args, hipStream_t stream) {
  if (args.nhub == 0) return;
  if (args.mover_bound != nullptr)
    launch_hub_argmax_impl<W, true>(args, stream);
  else
    launch_hub_argmax_impl<W, false>(args, stream);
}
template void launch_hub_argmax<float>(const HubArgs<float>&, hipStream_t);
template void launch_hub_argmax<double>(const HubArgs<double>&, hipStream_t);

int hub_slices() { return HUB_SLICES; }

template <typename W>
void launch_row_sum(const int64_t* rowptr, const W* weights, int64_t nv,
                    W* out, hipStream_t stream) {
  if (nv == 0) return;
  constexpr int BLOCK = 256;
  constexpr int WAVES = BLOCK / 64;
  int64_t grid = (nv + WAVES - 1) / WAVES;
  if (grid > 1048576) grid = 1048576;  // stay under 2^32-1 workitems
  hipLaunchKernelGGL((row_sum_kernel<W, BLOCK>), dim3((uint32_t)grid),
                     dim3(BLOCK), 0, stream, rowptr, weights, nv, out);
}
template void launch_row_sum<float>(const int64_t*, const float*, int64_t,
                                    float*, hipStream_t);
template void launch_row_sum<double>(const int64_t*, const double*, int64_t,
                                     double*, hipStream_t);

// `out` must be zero-initialised by the caller (rows cut by a span boundary
// are accumulated with atomics; edgeless rows are never written).
template <typename W, typename L>
void launch_intra_weight(const int64_t* rowptr, const int32_t* tails,
                         const W* weights, const L* labels, int64_t nv,
                         int64_t ne, int64_t nl, W* out, hipStream_t stream) {
  if (nv == 0 || ne == 0) return;
  constexpr int BLOCK = 256;
  const int64_t nspan = (ne + IW_SPAN - 1) / IW_SPAN;
  hipLaunchKernelGGL((intra_weight_kernel<W, L, BLOCK, false>),
                     dim3(grid_for(nspan * 64, BLOCK)), dim3(BLOCK), 0, stream,
                     rowptr, tails, weights, labels, nv, ne, nl, out,
                     (uint8_t*)nullptr);
}

// intra_weight plus the boundary mask (MARK): `out` and `mask` (uint8 [nv])
// must both be zero-initialised by the caller.
template <typename W, typename L>
void launch_intra_boundary(const int64_t* rowptr, const int32_t* tails,
                           const W* weights, const L* labels, int64_t nv,
                           int64_t ne, int64_t nl, W* out, uint8_t* mask,
                           hipStream_t stream) {
  if (nv == 0 || ne == 0) return;
  constexpr int BLOCK = 256;
  const int64_t nspan = (ne + IW_SPAN - 1) / IW_SPAN;
  hipLaunchKernelGGL((intra_weight_kernel<W, L, BLOCK, true>),
                     dim3(grid_for(nspan * 64, BLOCK)), dim3(BLOCK), 0, stream,
                     rowptr, tails, weights, labels, nv, ne, nl, out, mask);
}
#define INSTANTIATE_IW(W, L)                                                  \
  template void launch_intra_weight<W, L>(const int64_t*, const int32_t*,    \
                                          const W*, const L*, int64_t,       \
                                          int64_t, int64_t, W*, hipStream_t); \
  template void launch_intra_boundary<W, L>(const int64_t*, const int32_t*,  \
                                            const W*, const L*, int64_t,     \
                                            int64_t, int64_t, W*, uint8_t*,  \
                                            hipStream_t);
INSTANTIATE_IW(float, int32_t)
INSTANTIATE_IW(float, int64_t)
INSTANTIATE_IW(double, int32_t)
INSTANTIATE_IW(double, int64_t)

int intra_weight_span() { return IW_SPAN; }

// One hook pass of the label-restricted connected components (see
// cc_hook_kernel). The caller zeroes `changed` first and checks nv, ne > 0.
template <typename L>
void launch_cc_hook(const int64_t* rowptr, const int32_t* tails,
                    const L* labels, int64_t nv, int64_t ne, int64_t nl,
                    int32_t* comp, int32_t* changed, hipStream_t stream) {
  if (nv == 0 || ne == 0) return;
  constexpr int BLOCK = 256;
  const int64_t nspan = (ne + IW_SPAN - 1) / IW_SPAN;
  hipLaunchKernelGGL((cc_hook_kernel<L, BLOCK>),
                     dim3(grid_for(nspan * 64, BLOCK)), dim3(BLOCK), 0, stream,
                     rowptr, tails, labels, nv, ne, nl, comp, changed);
}
template void launch_cc_hook<int32_t>(const int64_t*, const int32_t*,
                                      const int32_t*, int64_t, int64_t,
                                      int64_t, int32_t*, int32_t*,
                                      hipStream_t);
template void launch_cc_hook<int64_t>(const int64_t*, const int32_t*,
                                      const int64_t*, int64_t, int64_t,
                                      int64_t, int32_t*, int32_t*,
                                      hipStream_t);

void launch_cc_compress(int32_t* comp, int64_t nl, hipStream_t stream) {
  if (nl == 0) return;
  hipLaunchKernelGGL(cc_compress_kernel, dim3(grid_for(nl, 256)), dim3(256),
                     0, stream, comp, nl);
}

// Degrees of the changed rows into deg_out; marks the changed locals.
void launch_frontier_degrees(const FrontierArgs& a, int64_t* deg_out,
                             hipStream_t stream) {
  if (a.nc == 0) return;
  hipLaunchKernelGGL(frontier_degrees_kernel, dim3(grid_for(a.nc, 256)),
                     dim3(256), 0, stream, a.changed, a.nc, a.rowptr, a.nv,
                     a.g_rowptr, a.ng, deg_out, a.active);
}

// The edge total offs[nc] stays on the device: the grid is sized by the
// host-side bound `edge_bound` on it (capped; the waves stride over spans).
void launch_frontier_expand(const FrontierArgs& a, const int64_t* offs,
                            int64_t edge_bound, hipStream_t stream) {
  if (a.nc == 0 || edge_bound <= 0) return;
  constexpr int BLOCK = 256;
  const int64_t nspan = (edge_bound + FX_SPAN - 1) / FX_SPAN;
  int grid = grid_for(nspan * 64, BLOCK);
  if (grid > 2048) grid = 2048;
  hipLaunchKernelGGL((frontier_expand_kernel<BLOCK>), dim3(grid), dim3(BLOCK),
                     0, stream, a.changed, a.nc, offs, a.rowptr, a.tails, a.nv,
                     a.ne, a.g_rowptr, a.g_heads, a.ng, a.neg, a.active);
}

int frontier_span() { return FX_SPAN; }
int frontier_classes() { return FC_CLASSES; }
int64_t frontier_units(int64_t nv) { return (nv + FC_UNIT - 1) / FC_UNIT; }

void launch_frontier_compact(const uint8_t* active, const uint8_t* cls,
                             int64_t nv, int32_t* unit_cnt,
                             const int32_t* unit_off,
                             const int32_t* class_base, int32_t* lists,
                             bool write, hipStream_t stream) {
  const int64_t nunit = frontier_units(nv);
  if (nunit == 0) return;
  const int grid = (int)((nunit + 3) / 4);  // 4 waves per 256-thread block
  if (write)
    hipLaunchKernelGGL(frontier_compact_kernel<true>, dim3(grid), dim3(256), 0,
                       stream, active, cls, nv, nunit, unit_cnt, unit_off,
                       class_base, lists);
  else
    hipLaunchKernelGGL(frontier_compact_kernel<false>, dim3(grid), dim3(256),
                       0, stream, active, cls, nv, nunit, unit_cnt, unit_off,
                       class_base, lists);
}

int batch_span() { return BA_SPAN; }
int64_t batch_spans(int64_t n_touched) {
  return (n_touched + BA_SPAN - 1) / BA_SPAN;
}

void launch_batch_mark(const BatchMarkArgs& a, hipStream_t stream) {
  const BatchRows& r = a.rows;
  if (r.nt == 0 || r.n_touched <= 0) return;
  constexpr int BLOCK = 256;
  hipLaunchKernelGGL((batch_mark_kernel<BLOCK>),
                     dim3(grid_for(batch_spans(r.n_touched) * 64, BLOCK)),
                     dim3(BLOCK), 0, stream, r.rowptr, r.tails, r.ne, r.t_rows,
                     r.t_offs, r.nt, r.n_touched, a.d_offs, a.d_dst, a.nd,
                     a.d_matched, a.keep, a.span_cnt, a.row_kept);
}

template <typename W>
void launch_batch_copy(const BatchWriteArgs<W>& a, hipStream_t stream) {
  const BatchRows& r = a.rows;
  if (r.nv == 0 || r.ne == 0) return;
  constexpr int BLOCK = 256;
  const int64_t nspan = (r.ne + BA_COPY_SPAN - 1) / BA_COPY_SPAN;
  hipLaunchKernelGGL((batch_copy_kernel<W, BLOCK>),
                     dim3(grid_for(nspan * 64, BLOCK)), dim3(BLOCK), 0, stream,
                     r.rowptr, r.tails, a.weights, r.nv, r.ne, a.touched,
                     a.new_rowptr, a.new_ne, a.new_tails, a.new_weights);
}

// Kept entries of the touched rows, then their insertions.
template <typename W>
void launch_batch_compact(const BatchWriteArgs<W>& a, hipStream_t stream) {
  const BatchRows& r = a.rows;
  constexpr int BLOCK = 256;
  if (r.nt > 0 && r.n_touched > 0)
    hipLaunchKernelGGL((batch_compact_kernel<W, BLOCK>),
                       dim3(grid_for(batch_spans(r.n_touched) * 64, BLOCK)),
                       dim3(BLOCK), 0, stream, r.rowptr, r.tails, a.weights,
                       r.ne, r.t_rows, r.t_offs, r.nt, r.n_touched, a.keep,
                       a.span_offs, a.kept_offs, a.new_rowptr, a.new_ne,
                       a.new_tails, a.new_weights);
  if (r.nt > 0 && a.ni > 0)
    hipLaunchKernelGGL((batch_insert_kernel<W>), dim3(grid_for(a.ni, BLOCK)),
                       dim3(BLOCK), 0, stream, r.t_rows, r.nt, a.i_offs,
                       a.i_dst, a.i_w, a.ni, a.row_kept, a.new_rowptr,
                       a.new_ne, a.new_tails, a.new_weights);
}

#define INSTANTIATE_BATCH(W)                                                  \
  template void launch_batch_copy<W>(const BatchWriteArgs<W>&, hipStream_t); \
  template void launch_batch_compact<W>(const BatchWriteArgs<W>&,            \
                                        hipStream_t);
INSTANTIATE_BATCH(float)
INSTANTIATE_BATCH(double)
#undef INSTANTIATE_BATCH

// rocPRIM wrappers (two-phase: bytes query with temp==nullptr, then run).
template <typename W>
void segsort_pairs(void* temp, size_t* bytes, const int32_t* keys_in,
                   int32_t* keys_out, const W* vals_in, W* vals_out,
                   int64_t n, int nseg, const int64_t* offs, int end_bit,
                   hipStream_t stream) {
  (void)rocprim::segmented_radix_sort_pairs(
      temp, *bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n,
      (unsigned)nseg, offs, offs + 1, 0u, (unsigned)end_bit, stream);
}
template void segsort_pairs<float>(void*, size_t*, const int32_t*, int32_t*,
                                   const float*, float*, int64_t, int,
                                   const int64_t*, int, hipStream_t);
template void segsort_pairs<double>(void*, size_t*, const int32_t*, int32_t*,
                                    const double*, double*, int64_t, int,
                                    const int64_t*, int, hipStream_t);

// Narrow-bit global radix sort of packed (src, dst) coarse-edge keys with
// their weights (coarsening aggregate; end_bit = bits of gnc^2, ~50 at s26
// vs the 64 bits a generic int64 sort pays).
template <typename W>
void sort_pairs64(void* temp, size_t* bytes, const int64_t* keys_in,
                  int64_t* keys_out, const W* vals_in, W* vals_out,
                  int64_t n, int end_bit, hipStream_t stream) {
  (void)rocprim::radix_sort_pairs(temp, *bytes, keys_in, keys_out, vals_in,
                                  vals_out, (size_t)n, 0u,
                                  (unsigned)end_bit, stream);
}
template void sort_pairs64<float>(void*, size_t*, const int64_t*, int64_t*,
                                  const float*, float*, int64_t, int,
                                  hipStream_t);
template void sort_pairs64<double>(void*, size_t*, const int64_t*, int64_t*,
                                   const double*, double*, int64_t, int,
                                   hipStream_t);

// Sums of equal adjacent keys (coarsening aggregate, after sort_pairs64).
template <typename W>
void reduce_by_key64(void* temp, size_t* bytes, const int64_t* keys,
                     const W* vals, int64_t n, int64_t* uniq_out, W* sums_out,
                     unsigned int* count_out, hipStream_t stream) {
  (void)rocprim::reduce_by_key(temp, *bytes, keys, vals, (size_t)n, uniq_out,
                               sums_out, count_out, rocprim::plus<W>(),
                               rocprim::equal_to<int64_t>(), stream);
}
template void reduce_by_key64<float>(void*, size_t*, const int64_t*,
                                     const float*, int64_t, int64_t*, float*,
                                     unsigned int*, hipStream_t);
template void reduce_by_key64<double>(void*, size_t*, const int64_t*,
                                      const double*, int64_t, int64_t*,
                                      double*, unsigned int*, hipStream_t);

}  // namespace cuvite
