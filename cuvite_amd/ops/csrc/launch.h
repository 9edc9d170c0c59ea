// Host-side launch interface of the cuvite_amd HIP kernels: the argument
// structs and the declaration of every launcher that louvain_kernels.hip
// defines and bindings.cpp calls. Plain C++ (no torch), included by both.
//
// The structs exist on the host only. The kernels keep positional
// `__restrict__` parameters and the launchers unpack a struct at the launch.
// All pointers are device pointers; W is the weight dtype (float or double).

#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

namespace cuvite {

// Arguments of the degree-class move kernels (lv_move_sub, lv_move_block).
// mover_bound and cand_bound both null: plain local move. Both set: one
// Leiden refine round.
template <typename W>
struct MoveArgs {
  const int64_t* rowptr;
  const int32_t* tails;
  const W* weights;
  const int32_t* curr_comm;
  const W* v_degree;
  const int64_t* comm_size;  // null in a refine round, not read
  const W* comm_degree;
  const int64_t* comm_gid;
  double constant;
  int32_t* target;
  W* cluster_weight;
  int64_t gid_base;     // gid(y) = gid_base + y for y < n_local (gid_of)
  int32_t n_local;      // 0: every gid is read from comm_gid
  int64_t* next_size;   // fused aggregates (account_target); null = off;
                        // null in a refine round, not read
  W* next_degree;       // null in a refine round, not read
  int64_t n_next;       // length of next_size / next_degree
  const int32_t* mover_bound;  // int32 [>= nv]: bound id of a mover, else -1
  const int32_t* cand_bound;   // int32 [nc]: bound id of a candidate, else -1
};

// Arguments of the hub argmax (hub_own_weight_kernel, hub_slice_kernel,
// hub_final_kernel). n = eoffs[nhub] sorted pairs, nc dense communities,
// S = hub_slices(). The bound arrays select plain move or refine round as
// in MoveArgs.
template <typename W>
struct HubArgs {
  const int32_t* keys;        // int32 [n]: communities, ascending per hub
  const W* vals;              // W [n]: edge weights, permuted with keys
  const int64_t* eoffs;       // int64 [nhub + 1]: segment offsets into keys
  const int32_t* hubs;        // int32 [nhub]: dense vertex id of each hub
  int nhub;
  const double* hub_self;     // double [nhub]: self-loop weight of each hub
  const int32_t* curr_comm;   // int32 [nv + ng]: dense community per vertex
  const W* v_degree;          // W [nv]: weighted vertex degrees
  const int64_t* comm_size;   // int64 [nc]; null in a refine round, not read
  const W* comm_degree;       // W [nc]
  const int64_t* comm_gid;    // int64 [nc]: global id per dense community
  int64_t gid_base;           // as in MoveArgs
  int32_t n_local;            // as in MoveArgs
  double constant;
  double* p_wcc;              // scratch double [nhub * S]: own-weight partials
  double* p_gain;             // scratch double [nhub * S]: best gain per slice
  int64_t* p_gid;             // scratch int64 [nhub * S]: its global id
  int32_t* p_dense;           // scratch int32 [nhub * S]: its dense id
  int32_t* r_key;             // scratch int32 [2 * nhub * S]: open-run keys
  double* r_sum;              // scratch double [2 * nhub * S]: open-run sums
  int32_t* target_hub;        // out int32 [nhub]: target dense community
  W* cw_hub;                  // out W [nhub]: weight into the own community
  int64_t* next_size;         // int64 [n_next]; null = off, null in a refine
                              // round, not read
  W* next_degree;             // W [n_next]; null with next_size
  int64_t n_next;             // length of next_size / next_degree
  const int32_t* mover_bound; // int32 [>= nv], indexed by hubs[] entries
  const int32_t* cand_bound;  // int32 [nc]
};

// Degree class c in [0, 7) over the vertex list vlist[0, nlist); the classes
// are CLASS_TABLE in louvain_kernels.hip. A sub class list (c < 4) may be
// padded with -1.
template <typename W>
void launch_class(int c, const int32_t* vlist, int nlist,
                  const MoveArgs<W>& args, hipStream_t stream);

// Own weight, sliced argmax and per-hub stitch over the sorted pairs.
template <typename W>
void launch_hub_argmax(const HubArgs<W>& args, hipStream_t stream);
int hub_slices();

template <typename W>
void launch_modularity(const W* cluster_weight, const W* comm_degree,
                       int64_t nv, double* out, hipStream_t stream);
template <typename W>
void launch_scatter_add(W* out, const int64_t* idx, const W* val, int64_t n,
                        hipStream_t stream);
void launch_degree_count(const int64_t* src, int64_t n, int64_t base,
                         int32_t* cnt, hipStream_t stream);
template <typename W>
void launch_csr_place(const int64_t* src, const int64_t* dst, const W* w,
                      int64_t n, int64_t base, const int64_t* rowptr,
                      int32_t* cursor, int64_t* tails_out, W* w_out,
                      hipStream_t stream);
template <typename W>
void launch_row_sum(const int64_t* rowptr, const W* weights, int64_t nv,
                    W* out, hipStream_t stream);
void launch_gather_comm(const int32_t* tails_flat, const int32_t* curr_comm,
                        int64_t n, int32_t* keys, hipStream_t stream);
template <typename W>
void launch_apply_deltas(const int64_t* target, const int64_t* curr,
                         const W* v_degree, int64_t nv, int64_t base,
                         int64_t bound, int64_t* local_size, W* local_degree,
                         hipStream_t stream);
template <typename W>
void launch_recount(const int64_t* labels, const W* v_degree, int64_t nv,
                    int64_t base, int64_t ncomm, int64_t* size, W* degree,
                    hipStream_t stream);
void launch_coloring_minmax(const int64_t* rowptr, const int32_t* tails,
                            const int64_t* gid_all, const bool* uncolored,
                            const int64_t* colors, int64_t nv, int64_t base,
                            const int64_t* seeds, int n_hash, int64_t* mn_out,
                            int64_t* mx_out, hipStream_t stream);
// `out` must be zero-initialised by the caller.
template <typename W, typename L>
void launch_intra_weight(const int64_t* rowptr, const int32_t* tails,
                         const W* weights, const L* labels, int64_t nv,
                         int64_t ne, int64_t nl, W* out, hipStream_t stream);
// intra_weight plus mask[v] = 1 for every row with an in-range tail of
// another label; `out` and `mask` (uint8 [nv]) zero-initialised by the caller.
template <typename W, typename L>
void launch_intra_boundary(const int64_t* rowptr, const int32_t* tails,
                           const W* weights, const L* labels, int64_t nv,
                           int64_t ne, int64_t nl, W* out, uint8_t* mask,
                           hipStream_t stream);
int intra_weight_span();
// The caller zeroes `changed` first.
template <typename L>
void launch_cc_hook(const int64_t* rowptr, const int32_t* tails,
                    const L* labels, int64_t nv, int64_t ne, int64_t nl,
                    int32_t* comp, int32_t* changed, hipStream_t stream);
void launch_cc_compress(int32_t* comp, int64_t nl, hipStream_t stream);

// Arguments of the frontier expansion (frontier_degrees_kernel,
// frontier_expand_kernel): the changed dense ids and the two CSRs their
// neighbours are read from.
struct FrontierArgs {
  const int32_t* changed;   // int32 [nc]: dense ids in [0, nv + ng)
  int64_t nc;
  const int64_t* rowptr;    // int64 [nv + 1]: level CSR, local rows
  const int32_t* tails;     // int32 [ne]: dense tails (ghosts >= nv skipped)
  int64_t nv, ne;
  const int64_t* g_rowptr;  // int64 [ng + 1]: ghost -> local reverse CSR
  const int32_t* g_heads;   // int32 [neg]: local heads of each ghost
  int64_t ng, neg;
  uint8_t* active;          // out uint8 [nv]: 1 is stored, nothing cleared
};

void launch_frontier_degrees(const FrontierArgs& args, int64_t* deg_out,
                             hipStream_t stream);
// offs: int64 [nc + 1], exclusive prefix sums of deg_out; edge_bound: any
// host-side upper estimate of offs[nc] (sizes the grid only).
void launch_frontier_expand(const FrontierArgs& args, const int64_t* offs,
                            int64_t edge_bound, hipStream_t stream);
int frontier_span();
// Class lists of the active vertices. cls: uint8 [nv] class id per vertex in
// [0, frontier_classes()). write == false: per-wave class counts into
// unit_cnt [frontier_units(nv) * frontier_classes()]. write == true: ids into
// lists [nv] at class_base[c] + unit_off[unit][c] + rank, ascending.
void launch_frontier_compact(const uint8_t* active, const uint8_t* cls,
                             int64_t nv, int32_t* unit_cnt,
                             const int32_t* unit_off,
                             const int32_t* class_base, int32_t* lists,
                             bool write, hipStream_t stream);
int frontier_classes();
int64_t frontier_units(int64_t nv);

// Arguments of the edge-batch kernels (batch_mark_kernel, batch_copy_kernel,
// batch_compact_kernel, batch_insert_kernel). BatchRows: the old CSR with
// global int64 tails and the nt touched rows, whose old entries form one
// concatenated edge space of t_offs[nt] = n_touched entries.
struct BatchRows {
  const int64_t* rowptr;     // int64 [nv + 1]: old CSR
  const int64_t* tails;      // int64 [ne]: global ids
  int64_t nv, ne;
  const int64_t* t_rows;     // int64 [nt]: touched local rows, ascending
  const int64_t* t_offs;     // int64 [nt + 1]: prefix sums of their degrees
  int64_t nt, n_touched;
};

// Mark: the touched rows' slices of the sorted deletion list and what the
// pass stores. No weights are read.
struct BatchMarkArgs {
  BatchRows rows;
  const int64_t* d_offs;     // int64 [nt + 1]: deletion slice of each row
  const int64_t* d_dst;      // int64 [nd]: tails to delete, ascending per row
  int64_t nd;
  uint8_t* d_matched;        // uint8 [nd]: 1 is stored where an entry matched
  uint8_t* keep;             // uint8 [n_touched]: 1 = the entry stays
  int64_t* span_cnt;         // int64 [batch_spans(n_touched)]: kept per span
  int64_t* row_kept;         // int64 [nt]: kept per row; zeroed by the caller
};

// Copy, compact and insert: mark's results, their scans and the new CSR.
template <typename W>
struct BatchWriteArgs {
  BatchRows rows;
  const W* weights;          // W [ne]
  const uint8_t* keep;       // uint8 [n_touched]
  const int64_t* row_kept;   // int64 [nt]
  const uint8_t* touched;    // uint8 [nv]: 1 for a touched row
  const int64_t* span_offs;  // int64 [spans]: exclusive scan of span_cnt
  const int64_t* kept_offs;  // int64 [nt]: exclusive scan of row_kept
  const int64_t* new_rowptr; // int64 [nv + 1]
  int64_t new_ne;
  int64_t* new_tails;        // int64 [new_ne]
  W* new_weights;            // W [new_ne]
  const int64_t* i_offs;     // int64 [nt + 1]: insertion slice of each row
  const int64_t* i_dst;      // int64 [ni]: inserted tails, list order per row
  const W* i_w;              // W [ni]
  int64_t ni;
};

// Keep flags, per-span and per-row kept counts, matched deletions.
void launch_batch_mark(const BatchMarkArgs& args, hipStream_t stream);
// Untouched rows, moved to their new offset.
template <typename W>
void launch_batch_copy(const BatchWriteArgs<W>& args, hipStream_t stream);
// Touched rows: kept entries in their old order, then the insertions.
template <typename W>
void launch_batch_compact(const BatchWriteArgs<W>& args, hipStream_t stream);
int batch_span();
int64_t batch_spans(int64_t n_touched);

// rocPRIM wrappers, two-phase: temp == nullptr only stores the scratch size
// in *bytes, a second call with that much scratch at temp does the work.
template <typename W>
void segsort_pairs(void* temp, size_t* bytes, const int32_t* keys_in,
                   int32_t* keys_out, const W* vals_in, W* vals_out,
                   int64_t n, int nseg, const int64_t* offs, int end_bit,
                   hipStream_t stream);
template <typename W>
void sort_pairs64(void* temp, size_t* bytes, const int64_t* keys_in,
                  int64_t* keys_out, const W* vals_in, W* vals_out,
                  int64_t n, int end_bit, hipStream_t stream);
template <typename W>
void reduce_by_key64(void* temp, size_t* bytes, const int64_t* keys,
                     const W* vals, int64_t n, int64_t* uniq_out, W* sums_out,
                     unsigned int* count_out, hipStream_t stream);

}  // namespace cuvite
