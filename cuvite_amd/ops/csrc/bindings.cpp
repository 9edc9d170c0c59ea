// Python bindings for the cuvite_amd HIP kernels (torch extension).

#include <torch/extension.h>
#include <hip/hip_runtime.h>
#include <c10/hip/HIPStream.h>

#include "launch.h"

#include <cstdint>
#include <tuple>
#include <vector>

namespace {

// A tensor a kernel reads or writes: on the device and contiguous.
#define CHECK_INPUT(t)                                            \
  do {                                                            \
    TORCH_CHECK((t).is_cuda(), #t " must be on GPU");             \
    TORCH_CHECK((t).is_contiguous(), #t " must be contiguous");   \
  } while (0)

// Two-phase rocPRIM call: run(nullptr, bytes) stores the scratch size in
// `bytes`, then run(temp, bytes) works with that much scratch, allocated as
// a byte tensor beside `like`.
template <typename F>
void with_scratch(const at::Tensor& like, F run) {
  size_t bytes = 0;
  run(nullptr, bytes);
  auto temp = at::empty({(int64_t)bytes}, like.options().dtype(at::kByte));
  run(temp.data_ptr(), bytes);
}

// Optional second aggregate pair the move kernels account their targets in
// (see account_target): both or neither, int64 sizes, degrees in the weight
// dtype, equal lengths.
void check_next(const c10::optional<at::Tensor>& next_size,
                const c10::optional<at::Tensor>& next_degree,
                const at::Tensor& weights) {
  TORCH_CHECK(next_size.has_value() == next_degree.has_value(),
              "next_size and next_degree go together");
  if (!next_size.has_value()) return;
  CHECK_INPUT(*next_size);
  CHECK_INPUT(*next_degree);
  TORCH_CHECK(next_size->scalar_type() == at::kLong,
              "next_size must be int64");
  TORCH_CHECK(next_degree->scalar_type() == weights.scalar_type(),
              "next_degree must have the weight dtype");
  TORCH_CHECK(next_size->numel() == next_degree->numel(),
              "next_size/next_degree length mismatch");
}

void check_local_gids(int64_t n_local, const at::Tensor& comm_gid) {
  TORCH_CHECK(n_local >= 0 && n_local <= comm_gid.numel() &&
              n_local <= (int64_t)INT32_MAX,
              "n_local must lie in [0, number of communities]");
}

// comm_size, the next_* pair and the bound arrays may be absent (null in
// MoveArgs): see launch.h for who reads what.
template <typename W>
cuvite::MoveArgs<W> make_args(const at::Tensor& rowptr, const at::Tensor& tails,
                              const at::Tensor& weights,
                              const at::Tensor& curr_comm,
                              const at::Tensor& v_degree,
                              const c10::optional<at::Tensor>& comm_size,
                              const at::Tensor& comm_degree,
                              const at::Tensor& comm_gid, double constant,
                              at::Tensor& target, at::Tensor& cw,
                              int64_t gid_base, int64_t n_local,
                              const c10::optional<at::Tensor>& next_size,
                              const c10::optional<at::Tensor>& next_degree,
                              const int32_t* mover_bound,
                              const int32_t* cand_bound) {
  cuvite::MoveArgs<W> a{};
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.tails = tails.data_ptr<int32_t>();
  a.weights = weights.data_ptr<W>();
  a.curr_comm = curr_comm.data_ptr<int32_t>();
  a.v_degree = v_degree.data_ptr<W>();
  a.comm_size = comm_size ? comm_size->data_ptr<int64_t>() : nullptr;
  a.comm_degree = comm_degree.data_ptr<W>();
  a.comm_gid = comm_gid.data_ptr<int64_t>();
  a.constant = constant;
  a.target = target.data_ptr<int32_t>();
  a.cluster_weight = cw.data_ptr<W>();
  a.gid_base = gid_base;
  a.n_local = (int32_t)n_local;
  a.next_size = next_size ? next_size->data_ptr<int64_t>() : nullptr;
  a.next_degree = next_degree ? next_degree->data_ptr<W>() : nullptr;
  a.n_next = next_size ? next_size->numel() : 0;
  a.mover_bound = mover_bound;
  a.cand_bound = cand_bound;
  return a;
}

// Auxiliary stream and fork/join events of local_move, made once per device
// and kept for the life of the process (a stream pool would hand out a
// different stream on every call). The events carry no timing. An event may
// be recorded again by a later call: a wait binds to the record before it.
struct ClassStream {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};

ClassStream& class_stream(int device) {
  static std::vector<ClassStream> per_device(64);
  TORCH_CHECK(device >= 0 && device < (int)per_device.size(),
              "device index out of range");
  ClassStream& cs = per_device[device];
  if (cs.stream == nullptr) {
    C10_HIP_CHECK(hipStreamCreateWithFlags(&cs.stream, hipStreamNonBlocking));
    C10_HIP_CHECK(hipEventCreateWithFlags(&cs.fork, hipEventDisableTiming));
    C10_HIP_CHECK(hipEventCreateWithFlags(&cs.join, hipEventDisableTiming));
  }
  return cs;
}

// vlists: the 7 LDS degree-class vertex lists (hubs excluded), int32; a sub
// class list may be padded with -1 (the sub kernels skip those entries).
//
// Schedule. The sub classes 0-3 (6 KB of LDS per block, all 32 wave slots
// of a CU) run on the calling stream. The block classes 4-6 (24-96 KB
// tables, 24 down to 4 resident waves per CU) want the opposite resource,
// so with `class_streams` they run beside the sub classes on an auxiliary
// stream, largest class first, instead of behind them. The auxiliary
// stream forks from the calling stream after the outputs are initialised
// and is joined into it before this returns: the outputs (allocated on the
// calling stream) carry no work pending elsewhere, and the call is correct
// from any stream. `class_streams = false` is the serial schedule: all
// seven kernels on the calling stream.
//
// With `mover_bound` / `cand_bound` (both or neither) the refine kernels run
// instead and `comm_size` is absent: see refine_move below.
std::vector<at::Tensor> local_move_impl(
    at::Tensor rowptr, at::Tensor tails, at::Tensor weights,
    at::Tensor curr_comm, at::Tensor v_degree,
    c10::optional<at::Tensor> comm_size, at::Tensor comm_degree,
    at::Tensor comm_gid, double constant, std::vector<at::Tensor> vlists,
    int64_t gid_base, int64_t n_local, c10::optional<at::Tensor> next_size,
    c10::optional<at::Tensor> next_degree, bool class_streams,
    const int32_t* mover_bound, const int32_t* cand_bound,
    c10::optional<at::Tensor> out_target = c10::nullopt,
    c10::optional<at::Tensor> out_cw = c10::nullopt, bool keep_cw = false) {
  CHECK_INPUT(rowptr);
  CHECK_INPUT(tails);
  CHECK_INPUT(weights);
  CHECK_INPUT(curr_comm);
  TORCH_CHECK(tails.scalar_type() == at::kInt, "tails must be int32");
  TORCH_CHECK(curr_comm.scalar_type() == at::kInt, "curr_comm must be int32");
  TORCH_CHECK(vlists.size() == 7, "expected 7 degree-class vertex lists"
              " (hub vertices go through the hub_moves pipeline)");
  check_local_gids(n_local, comm_gid);
  check_next(next_size, next_degree, weights);

  const int64_t nv = rowptr.numel() - 1;
  TORCH_CHECK(out_target.has_value() == out_cw.has_value(),
              "out_target and out_cw go together");
  at::Tensor target, cw;
  if (out_target.has_value()) {
    // caller's buffers: int32 [nv] and weight dtype [nv], contiguous
    CHECK_INPUT(*out_target);
    CHECK_INPUT(*out_cw);
    TORCH_CHECK(out_target->scalar_type() == at::kInt &&
                out_target->numel() == nv &&
                out_cw->scalar_type() == weights.scalar_type() &&
                out_cw->numel() == nv,
                "out_target must be int32 [nv], out_cw weight dtype [nv]");
    target = *out_target;
    cw = *out_cw;
    target.copy_(curr_comm.narrow(0, 0, nv));
    // keep_cw: a vertex in no list keeps the caller's value (frontier sweep)
    if (!keep_cw) cw.zero_();
  } else {
    TORCH_CHECK(!keep_cw, "keep_cw needs out_cw");
    target = curr_comm.narrow(0, 0, nv).clone();
    cw = at::zeros({nv}, weights.options());
  }
  auto stream = at::hip::getCurrentHIPStream().stream();

  const bool fork = class_streams && (vlists[4].numel() ||
                                      vlists[5].numel() || vlists[6].numel());
  ClassStream* cs = nullptr;
  hipStream_t block_stream = stream;
  if (fork) {
    cs = &class_stream(rowptr.get_device());
    C10_HIP_CHECK(hipEventRecord(cs->fork, stream));
    C10_HIP_CHECK(hipStreamWaitEvent(cs->stream, cs->fork, 0));
    block_stream = cs->stream;
  }

  AT_DISPATCH_FLOATING_TYPES(weights.scalar_type(), "local_move", [&] {
    using W = scalar_t;
    auto args = make_args<W>(rowptr, tails, weights, curr_comm, v_degree,
                             comm_size, comm_degree, comm_gid, constant,
                             target, cw, gid_base, n_local, next_size,
                             next_degree, mover_bound, cand_bound);
    auto run_class = [&](int c, hipStream_t st) {
      if (!vlists[c].numel()) return;
      cuvite::launch_class<W>(c, vlists[c].data_ptr<int32_t>(),
                              (int)vlists[c].numel(), args, st);
    };
    if (fork)
      for (int c : {6, 5, 4}) run_class(c, block_stream);
    for (int c : {0, 1, 2, 3}) run_class(c, stream);
    if (!fork)
      for (int c : {4, 5, 6}) run_class(c, stream);
  });
  if (fork) {
    C10_HIP_CHECK(hipEventRecord(cs->join, cs->stream));
    C10_HIP_CHECK(hipStreamWaitEvent(stream, cs->join, 0));
  }
  C10_HIP_CHECK(hipGetLastError());
  return {target, cw};
}

std::vector<at::Tensor> local_move(
    at::Tensor rowptr, at::Tensor tails, at::Tensor weights,
    at::Tensor curr_comm, at::Tensor v_degree, at::Tensor comm_size,
    at::Tensor comm_degree, at::Tensor comm_gid, double constant,
    std::vector<at::Tensor> vlists, int64_t gid_base, int64_t n_local,
    c10::optional<at::Tensor> next_size,
    c10::optional<at::Tensor> next_degree, bool class_streams,
    c10::optional<at::Tensor> out_target, c10::optional<at::Tensor> out_cw,
    bool keep_cw) {
  return local_move_impl(rowptr, tails, weights, curr_comm, v_degree,
                         comm_size, comm_degree, comm_gid, constant, vlists,
                         gid_base, n_local, next_size, next_degree,
                         class_streams, nullptr, nullptr, out_target, out_cw,
                         keep_cw);
}

// The two bound arrays of a refine round: mover_bound int32 [>= nv] (bound
// id of a vertex that moves this round, else -1), cand_bound int32 [nc]
// (bound id of a dense community that may be joined this round, else -1).
void check_bounds(const at::Tensor& mover_bound, const at::Tensor& cand_bound,
                  int64_t nv, const at::Tensor& comm_degree) {
  CHECK_INPUT(mover_bound);
  CHECK_INPUT(cand_bound);
  TORCH_CHECK(mover_bound.scalar_type() == at::kInt &&
              cand_bound.scalar_type() == at::kInt,
              "mover_bound / cand_bound must be int32");
  TORCH_CHECK(mover_bound.numel() >= nv,
              "mover_bound must cover all local vertices");
  TORCH_CHECK(cand_bound.numel() == comm_degree.numel(),
              "cand_bound must have one entry per dense community");
}

// One Leiden refine round over the LDS classes: local_move's kernels and
// schedule with the candidate filter cand_bound[y] == mover_bound[v] in the
// argmax fold, no singleton guard and no aggregate accounting. A vertex
// with mover_bound[v] < 0 keeps its label (cw 0). out_target / out_cw:
// optional caller-owned result buffers (both or neither).
std::vector<at::Tensor> refine_move(
    at::Tensor rowptr, at::Tensor tails, at::Tensor weights,
    at::Tensor curr_comm, at::Tensor v_degree, at::Tensor comm_degree,
    at::Tensor comm_gid, double constant, std::vector<at::Tensor> vlists,
    at::Tensor mover_bound, at::Tensor cand_bound, int64_t gid_base,
    int64_t n_local, bool class_streams,
    c10::optional<at::Tensor> out_target, c10::optional<at::Tensor> out_cw) {
  check_bounds(mover_bound, cand_bound, rowptr.numel() - 1, comm_degree);
  // comm_size is not read by the refine kernels
  return local_move_impl(rowptr, tails, weights, curr_comm, v_degree,
                         c10::nullopt, comm_degree, comm_gid, constant, vlists,
                         gid_base, n_local, c10::nullopt, c10::nullopt,
                         class_streams, mover_bound.data_ptr<int32_t>(),
                         cand_bound.data_ptr<int32_t>(), out_target, out_cw);
}

at::Tensor modularity_parts(at::Tensor cluster_weight, at::Tensor comm_degree) {
  CHECK_INPUT(cluster_weight);
  CHECK_INPUT(comm_degree);
  TORCH_CHECK(cluster_weight.numel() == comm_degree.numel());
  auto out = at::zeros({2}, cluster_weight.options().dtype(at::kDouble));
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(cluster_weight.scalar_type(), "modularity", [&] {
    cuvite::launch_modularity<scalar_t>(cluster_weight.data_ptr<scalar_t>(),
                                        comm_degree.data_ptr<scalar_t>(),
                                        cluster_weight.numel(),
                                        out.data_ptr<double>(), stream);
  });
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

void scatter_add_(at::Tensor out, at::Tensor idx, at::Tensor val) {
  CHECK_INPUT(out);
  CHECK_INPUT(idx);
  CHECK_INPUT(val);
  TORCH_CHECK(idx.scalar_type() == at::kLong, "idx must be int64");
  TORCH_CHECK(idx.numel() == val.numel(), "idx/val length mismatch");
  TORCH_CHECK(out.scalar_type() == val.scalar_type(), "dtype mismatch");
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(out.scalar_type(), "scatter_add", [&] {
    cuvite::launch_scatter_add<scalar_t>(out.data_ptr<scalar_t>(),
                                         idx.data_ptr<int64_t>(),
                                         val.data_ptr<scalar_t>(),
                                         idx.numel(), stream);
  });
  C10_HIP_CHECK(hipGetLastError());
}

std::vector<at::Tensor> csr_from_edges(int64_t nv, int64_t base,
                                       at::Tensor src, at::Tensor dst,
                                       at::Tensor w) {
  CHECK_INPUT(src);
  CHECK_INPUT(dst);
  CHECK_INPUT(w);
  TORCH_CHECK(src.scalar_type() == at::kLong && dst.scalar_type() == at::kLong,
              "src/dst must be int64");
  const int64_t ne = src.numel();
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto cnt = at::zeros({nv}, src.options().dtype(at::kInt));
  cuvite::launch_degree_count(src.data_ptr<int64_t>(), ne, base,
                              cnt.data_ptr<int32_t>(), stream);
  auto rowptr = at::zeros({nv + 1}, src.options());
  // int64 accumulation: an int32 cumsum overflows past 2^31 total edges
  rowptr.narrow(0, 1, nv).copy_(at::cumsum(cnt, 0, at::kLong));
  auto tails = at::empty({ne}, src.options());
  auto weights = at::empty({ne}, w.options());
  cnt.zero_();  // reuse as the per-row placement cursor
  AT_DISPATCH_FLOATING_TYPES(w.scalar_type(), "csr_place", [&] {
    cuvite::launch_csr_place<scalar_t>(
        src.data_ptr<int64_t>(), dst.data_ptr<int64_t>(),
        w.data_ptr<scalar_t>(), ne, base, rowptr.data_ptr<int64_t>(),
        cnt.data_ptr<int32_t>(), tails.data_ptr<int64_t>(),
        weights.data_ptr<scalar_t>(), stream);
  });
  C10_HIP_CHECK(hipGetLastError());
  return {rowptr, tails, weights};
}

// Full hub move, all device-side (no host sync): gather the neighbours'
// communities -> segmented sort (community, weight) per hub -> one pass over
// the sorted pairs in hub_slices() element slices per hub (own-community
// weight, run sums, gains, partial argmax) -> per-hub stitch of the slice
// records, guard and store. Scratch beyond the sort's is O(nhub * slices).
// eoffs: int64 [nhub + 1] segment offsets into tails_flat / weights_flat.
// Returns per-hub (target, wcc); with next_size / next_degree the hubs are
// also accounted in that aggregate pair.
// With mover_bound / cand_bound the refine argmax kernels run and comm_size
// is absent (hub_refine_moves).
std::vector<at::Tensor> hub_moves_impl(
    at::Tensor tails_flat, at::Tensor weights_flat, at::Tensor eoffs,
    at::Tensor hubs_i32, at::Tensor hub_self, at::Tensor curr_comm,
    at::Tensor v_degree, c10::optional<at::Tensor> comm_size,
    at::Tensor comm_degree, at::Tensor comm_gid, double constant,
    int64_t gid_base, int64_t n_local, c10::optional<at::Tensor> next_size,
    c10::optional<at::Tensor> next_degree, const int32_t* mover_bound,
    const int32_t* cand_bound) {
  CHECK_INPUT(tails_flat);
  CHECK_INPUT(weights_flat);
  CHECK_INPUT(eoffs);
  CHECK_INPUT(hubs_i32);
  check_local_gids(n_local, comm_gid);
  check_next(next_size, next_degree, weights_flat);
  TORCH_CHECK(tails_flat.scalar_type() == at::kInt);
  TORCH_CHECK(hubs_i32.scalar_type() == at::kInt);
  TORCH_CHECK(hub_self.scalar_type() == at::kDouble);
  TORCH_CHECK(eoffs.scalar_type() == at::kLong);
  const int64_t n = tails_flat.numel();
  TORCH_CHECK(weights_flat.numel() == n, "tails/weights length mismatch");
  TORCH_CHECK(n < (int64_t)INT32_MAX,
              "hub candidate batch exceeds int32 count range; chunk the hubs");
  const int nhub = (int)hubs_i32.numel();
  TORCH_CHECK(eoffs.numel() == (int64_t)nhub + 1 &&
              hub_self.numel() == (int64_t)nhub,
              "eoffs / hub_self do not match the hub list");
  const int64_t C = comm_degree.numel();
  TORCH_CHECK(C < (int64_t)INT32_MAX, "community count exceeds int32");
  auto stream = at::hip::getCurrentHIPStream().stream();
  int end_bit = 1;
  while ((int64_t(1) << end_bit) < C) end_bit++;
  auto target_hub = at::empty({nhub}, hubs_i32.options());
  auto cw_hub = at::empty({nhub}, weights_flat.options());
  AT_DISPATCH_FLOATING_TYPES(weights_flat.scalar_type(), "hub_moves", [&] {
    using W = scalar_t;
    auto keys = at::empty({n}, tails_flat.options());
    cuvite::launch_gather_comm(tails_flat.data_ptr<int32_t>(),
                               curr_comm.data_ptr<int32_t>(), n,
                               keys.data_ptr<int32_t>(), stream);
    auto keys2 = at::empty({n}, tails_flat.options());
    auto vals2 = at::empty({n}, weights_flat.options());
    with_scratch(tails_flat, [&](void* temp, size_t& bytes) {
      cuvite::segsort_pairs<W>(temp, &bytes, keys.data_ptr<int32_t>(),
                               keys2.data_ptr<int32_t>(),
                               weights_flat.data_ptr<W>(),
                               vals2.data_ptr<W>(), n, nhub,
                               eoffs.data_ptr<int64_t>(), end_bit, stream);
    });
    const int64_t nslice = (int64_t)nhub * cuvite::hub_slices();
    auto f64 = eoffs.options().dtype(at::kDouble);
    auto p_wcc = at::empty({nslice}, f64);
    auto p_gain = at::empty({nslice}, f64);
    auto p_gid = at::empty({nslice}, eoffs.options().dtype(at::kLong));
    auto p_dense = at::empty({nslice}, tails_flat.options());
    auto r_key = at::empty({2 * nslice}, tails_flat.options());
    auto r_sum = at::empty({2 * nslice}, f64);
    cuvite::HubArgs<W> h{};
    h.keys = keys2.data_ptr<int32_t>();
    h.vals = vals2.data_ptr<W>();
    h.eoffs = eoffs.data_ptr<int64_t>();
    h.hubs = hubs_i32.data_ptr<int32_t>();
    h.nhub = nhub;
    h.hub_self = hub_self.data_ptr<double>();
    h.curr_comm = curr_comm.data_ptr<int32_t>();
    h.v_degree = v_degree.data_ptr<W>();
    h.comm_size = comm_size ? comm_size->data_ptr<int64_t>() : nullptr;
    h.comm_degree = comm_degree.data_ptr<W>();
    h.comm_gid = comm_gid.data_ptr<int64_t>();
    h.gid_base = gid_base;
    h.n_local = (int32_t)n_local;
    h.constant = constant;
    h.p_wcc = p_wcc.data_ptr<double>();
    h.p_gain = p_gain.data_ptr<double>();
    h.p_gid = p_gid.data_ptr<int64_t>();
    h.p_dense = p_dense.data_ptr<int32_t>();
    h.r_key = r_key.data_ptr<int32_t>();
    h.r_sum = r_sum.data_ptr<double>();
    h.target_hub = target_hub.data_ptr<int32_t>();
    h.cw_hub = cw_hub.data_ptr<W>();
    h.next_size = next_size ? next_size->data_ptr<int64_t>() : nullptr;
    h.next_degree = next_degree ? next_degree->data_ptr<W>() : nullptr;
    h.n_next = next_size ? next_size->numel() : 0;
    h.mover_bound = mover_bound;
    h.cand_bound = cand_bound;
    cuvite::launch_hub_argmax<W>(h, stream);
  });
  C10_HIP_CHECK(hipGetLastError());
  return {target_hub, cw_hub};
}

std::vector<at::Tensor> hub_moves(
    at::Tensor tails_flat, at::Tensor weights_flat, at::Tensor eoffs,
    at::Tensor hubs_i32, at::Tensor hub_self, at::Tensor curr_comm,
    at::Tensor v_degree, at::Tensor comm_size, at::Tensor comm_degree,
    at::Tensor comm_gid, double constant, int64_t gid_base, int64_t n_local,
    c10::optional<at::Tensor> next_size,
    c10::optional<at::Tensor> next_degree) {
  return hub_moves_impl(tails_flat, weights_flat, eoffs, hubs_i32, hub_self,
                        curr_comm, v_degree, comm_size, comm_degree, comm_gid,
                        constant, gid_base, n_local, next_size, next_degree,
                        nullptr, nullptr);
}

// One refine round for hub vertices: hub_moves with the refine argmax
// kernels. mover_bound is indexed by the dense vertex id (hubs_i32 entries).
std::vector<at::Tensor> hub_refine_moves(
    at::Tensor tails_flat, at::Tensor weights_flat, at::Tensor eoffs,
    at::Tensor hubs_i32, at::Tensor hub_self, at::Tensor curr_comm,
    at::Tensor v_degree, at::Tensor comm_degree, at::Tensor comm_gid,
    double constant, at::Tensor mover_bound, at::Tensor cand_bound,
    int64_t gid_base, int64_t n_local) {
  check_bounds(mover_bound, cand_bound, v_degree.numel(), comm_degree);
  return hub_moves_impl(tails_flat, weights_flat, eoffs, hubs_i32, hub_self,
                        curr_comm, v_degree, c10::nullopt, comm_degree,
                        comm_gid, constant, gid_base, n_local, c10::nullopt,
                        c10::nullopt, mover_bound.data_ptr<int32_t>(),
                        cand_bound.data_ptr<int32_t>());
}

// Fresh world-1 recount of the community aggregates (see recount_kernel).
void recount_(at::Tensor labels, at::Tensor v_degree, int64_t base,
              at::Tensor size, at::Tensor degree) {
  CHECK_INPUT(labels);
  CHECK_INPUT(v_degree);
  CHECK_INPUT(size);
  CHECK_INPUT(degree);
  TORCH_CHECK(labels.scalar_type() == at::kLong);
  TORCH_CHECK(size.scalar_type() == at::kLong);
  TORCH_CHECK(labels.numel() == v_degree.numel());
  size.zero_();
  degree.zero_();
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(degree.scalar_type(), "recount", [&] {
    cuvite::launch_recount<scalar_t>(
        labels.data_ptr<int64_t>(), v_degree.data_ptr<scalar_t>(),
        labels.numel(), base, size.numel(), size.data_ptr<int64_t>(),
        degree.data_ptr<scalar_t>(), stream);
  });
  C10_HIP_CHECK(hipGetLastError());
}

// Coarsening aggregate: sort packed (src,dst) keys with weights (narrow-bit
// radix) and sum duplicate keys. Returns (uniq int64 [n], sums W [n],
// count int32[1]) — caller trims to count (ref fill_newEdgesMap +
// duplicate-edge merge, rebuild.cpp:244-279, 379-411, done with nested
// std::maps on the host there).
std::vector<at::Tensor> sort_reduce_pairs(at::Tensor key, at::Tensor val,
                                          int64_t end_bit) {
  CHECK_INPUT(key);
  CHECK_INPUT(val);
  TORCH_CHECK(key.scalar_type() == at::kLong, "key must be int64");
  TORCH_CHECK(key.numel() == val.numel());
  const int64_t n = key.numel();
  TORCH_CHECK(n < (int64_t)INT32_MAX, "chunk exceeds int32 count range");
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto uniq = at::empty({std::max<int64_t>(n, 1)}, key.options());
  auto sums = at::empty({std::max<int64_t>(n, 1)}, val.options());
  auto cnt = at::zeros({1}, key.options().dtype(at::kInt));
  if (n == 0) return {uniq.narrow(0, 0, 0), sums.narrow(0, 0, 0), cnt};
  AT_DISPATCH_FLOATING_TYPES(val.scalar_type(), "sort_reduce_pairs", [&] {
    using W = scalar_t;
    auto keys2 = at::empty({n}, key.options());
    auto vals2 = at::empty({n}, val.options());
    with_scratch(key, [&](void* temp, size_t& bytes) {
      cuvite::sort_pairs64<W>(temp, &bytes, key.data_ptr<int64_t>(),
                              keys2.data_ptr<int64_t>(), val.data_ptr<W>(),
                              vals2.data_ptr<W>(), n, (int)end_bit, stream);
    });
    with_scratch(key, [&](void* temp, size_t& bytes) {
      cuvite::reduce_by_key64<W>(temp, &bytes, keys2.data_ptr<int64_t>(),
                                 vals2.data_ptr<W>(), n,
                                 uniq.data_ptr<int64_t>(), sums.data_ptr<W>(),
                                 (unsigned int*)cnt.data_ptr<int32_t>(),
                                 stream);
    });
  });
  C10_HIP_CHECK(hipGetLastError());
  return {uniq, sums, cnt};
}

void apply_deltas_(at::Tensor target, at::Tensor curr, at::Tensor v_degree,
                   int64_t base, int64_t bound, at::Tensor local_size,
                   at::Tensor local_degree) {
  CHECK_INPUT(target);
  CHECK_INPUT(curr);
  CHECK_INPUT(v_degree);
  CHECK_INPUT(local_size);
  CHECK_INPUT(local_degree);
  TORCH_CHECK(target.scalar_type() == at::kLong &&
              curr.scalar_type() == at::kLong, "labels must be int64");
  TORCH_CHECK(local_size.scalar_type() == at::kLong);
  TORCH_CHECK(target.numel() == curr.numel() &&
              target.numel() == v_degree.numel());
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(local_degree.scalar_type(), "apply_deltas", [&] {
    cuvite::launch_apply_deltas<scalar_t>(
        target.data_ptr<int64_t>(), curr.data_ptr<int64_t>(),
        v_degree.data_ptr<scalar_t>(), target.numel(), base, bound,
        local_size.data_ptr<int64_t>(), local_degree.data_ptr<scalar_t>(),
        stream);
  });
  C10_HIP_CHECK(hipGetLastError());
}

// One coloring round's strict min/max of each hash over competing
// neighbors, per vertex (ref distColoringIteration, coloring.cpp:87-202).
std::vector<at::Tensor> coloring_minmax(at::Tensor rowptr, at::Tensor tails,
                                        at::Tensor gid_all,
                                        at::Tensor uncolored,
                                        at::Tensor colors, int64_t base,
                                        at::Tensor seeds) {
  CHECK_INPUT(rowptr);
  CHECK_INPUT(tails);
  CHECK_INPUT(gid_all);
  CHECK_INPUT(uncolored);
  CHECK_INPUT(colors);
  TORCH_CHECK(tails.scalar_type() == at::kInt);
  TORCH_CHECK(uncolored.scalar_type() == at::kBool);
  TORCH_CHECK(seeds.scalar_type() == at::kLong && seeds.is_cuda());
  const int n_hash = (int)seeds.numel();
  TORCH_CHECK(1 <= n_hash && n_hash <= 8, "n_hash must be in [1,8]");
  const int64_t nv = rowptr.numel() - 1;
  auto mn = at::empty({nv, n_hash}, rowptr.options());
  auto mx = at::empty({nv, n_hash}, rowptr.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  cuvite::launch_coloring_minmax(
      rowptr.data_ptr<int64_t>(), tails.data_ptr<int32_t>(),
      gid_all.data_ptr<int64_t>(), uncolored.data_ptr<bool>(),
      colors.data_ptr<int64_t>(), nv, base, seeds.data_ptr<int64_t>(),
      n_hash, mn.data_ptr<int64_t>(), mx.data_ptr<int64_t>(), stream);
  C10_HIP_CHECK(hipGetLastError());
  return {mn, mx};
}

at::Tensor row_sum(at::Tensor rowptr, at::Tensor weights) {
  CHECK_INPUT(rowptr);
  CHECK_INPUT(weights);
  const int64_t nv = rowptr.numel() - 1;
  auto out = at::empty({nv}, weights.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(weights.scalar_type(), "row_sum", [&] {
    cuvite::launch_row_sum<scalar_t>(rowptr.data_ptr<int64_t>(),
                                     weights.data_ptr<scalar_t>(), nv,
                                     out.data_ptr<scalar_t>(), stream);
  });
  C10_HIP_CHECK(hipGetLastError());
  return out;
}

// Per-vertex weight into the vertex's own community for arbitrary labels
// (see intra_weight_kernel). labels: int32 or int64, [nv + ng]. With `mark`
// the same pass also fills the boundary mask (uint8 [nv], second result);
// without it the second result is undefined.
static std::tuple<at::Tensor, at::Tensor> intra_weight_impl(
    at::Tensor rowptr, at::Tensor tails, at::Tensor weights,
    at::Tensor labels, bool mark) {
  CHECK_INPUT(rowptr);
  CHECK_INPUT(tails);
  CHECK_INPUT(weights);
  CHECK_INPUT(labels);
  TORCH_CHECK(rowptr.scalar_type() == at::kLong, "rowptr must be int64");
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must have nv + 1 entries");
  TORCH_CHECK(tails.scalar_type() == at::kInt, "tails must be int32");
  TORCH_CHECK(labels.scalar_type() == at::kInt ||
              labels.scalar_type() == at::kLong,
              "labels must be int32 or int64");
  TORCH_CHECK(tails.numel() == weights.numel(), "tails/weights mismatch");
  const int64_t nv = rowptr.numel() - 1;
  TORCH_CHECK(nv < (int64_t)INT32_MAX, "nv exceeds the int32 dense id range");
  TORCH_CHECK(labels.numel() >= nv, "labels must cover all local vertices");
  auto out = at::zeros({nv}, weights.options());
  at::Tensor mask;
  if (mark) mask = at::zeros({nv}, rowptr.options().dtype(at::kByte));
  auto stream = at::hip::getCurrentHIPStream().stream();
  AT_DISPATCH_FLOATING_TYPES(weights.scalar_type(), "intra_weight", [&] {
    using W = scalar_t;
    auto run = [&](auto* lab) {
      using L = std::remove_const_t<std::remove_pointer_t<decltype(lab)>>;
      if (mark)
        cuvite::launch_intra_boundary<W, L>(
            rowptr.data_ptr<int64_t>(), tails.data_ptr<int32_t>(),
            weights.data_ptr<W>(), lab, nv, tails.numel(), labels.numel(),
            out.data_ptr<W>(), mask.data_ptr<uint8_t>(), stream);
      else
        cuvite::launch_intra_weight<W, L>(
            rowptr.data_ptr<int64_t>(), tails.data_ptr<int32_t>(),
            weights.data_ptr<W>(), lab, nv, tails.numel(), labels.numel(),
            out.data_ptr<W>(), stream);
    };
    if (labels.scalar_type() == at::kInt)
      run(labels.data_ptr<int32_t>());
    else
      run(labels.data_ptr<int64_t>());
  });
  C10_HIP_CHECK(hipGetLastError());
  return {out, mask};
}

at::Tensor intra_weight(at::Tensor rowptr, at::Tensor tails,
                        at::Tensor weights, at::Tensor labels) {
  return std::get<0>(intra_weight_impl(rowptr, tails, weights, labels, false));
}

// intra_weight and, from the same edge pass, the boundary mask: mask[v] = 1
// iff row v holds an edge whose tail lies inside `labels` and carries another
// label than v. Returns (cw [nv], mask uint8 [nv]).
std::tuple<at::Tensor, at::Tensor> intra_boundary(at::Tensor rowptr,
                                                  at::Tensor tails,
                                                  at::Tensor weights,
                                                  at::Tensor labels) {
  return intra_weight_impl(rowptr, tails, weights, labels, true);
}

// Connected components of the graph restricted to edges whose endpoints
// carry the same label (see cc_hook_kernel): hook, compress and one read of
// the flag per round, until a hook pass sees no edge between two roots.
// labels: int32 or int64, [nv + ng]. Returns (comp int32 [nv + ng], rounds).
std::tuple<at::Tensor, int64_t> cc_components(at::Tensor rowptr,
                                              at::Tensor tails,
                                              at::Tensor labels) {
  CHECK_INPUT(rowptr);
  CHECK_INPUT(tails);
  CHECK_INPUT(labels);
  TORCH_CHECK(rowptr.scalar_type() == at::kLong, "rowptr must be int64");
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must have nv + 1 entries");
  TORCH_CHECK(tails.scalar_type() == at::kInt, "tails must be int32");
  TORCH_CHECK(labels.scalar_type() == at::kInt ||
              labels.scalar_type() == at::kLong,
              "labels must be int32 or int64");
  const int64_t nv = rowptr.numel() - 1;
  const int64_t ne = tails.numel();
  const int64_t nl = labels.numel();
  TORCH_CHECK(nl >= nv, "labels must cover all local vertices");
  TORCH_CHECK(nl < (int64_t)INT32_MAX,
              "nv + ng exceeds the int32 dense id range");
  auto comp = at::arange(nl, tails.options());
  if (nv == 0 || ne == 0) return {comp, 0};
  auto changed = at::zeros({1}, tails.options());
  auto stream = at::hip::getCurrentHIPStream().stream();
  int64_t rounds = 0;
  while (true) {
    TORCH_CHECK(rounds <= nl, "cc_components: no fixed point after ", rounds,
                " rounds (every changing round removes a root)");
    rounds++;
    changed.zero_();
    if (labels.scalar_type() == at::kInt)
      cuvite::launch_cc_hook<int32_t>(
          rowptr.data_ptr<int64_t>(), tails.data_ptr<int32_t>(),
          labels.data_ptr<int32_t>(), nv, ne, nl, comp.data_ptr<int32_t>(),
          changed.data_ptr<int32_t>(), stream);
    else
      cuvite::launch_cc_hook<int64_t>(
          rowptr.data_ptr<int64_t>(), tails.data_ptr<int32_t>(),
          labels.data_ptr<int64_t>(), nv, ne, nl, comp.data_ptr<int32_t>(),
          changed.data_ptr<int32_t>(), stream);
    cuvite::launch_cc_compress(comp.data_ptr<int32_t>(), nl, stream);
    C10_HIP_CHECK(hipGetLastError());
    if (changed.item<int32_t>() == 0) break;  // the round's one host sync
  }
  return {comp, rounds};
}

// Frontier expansion (see frontier_expand_kernel): active[u] = 1 for every
// changed local id and every local neighbour u of a changed dense id.
// changed: int32 [nc] dense ids in [0, nv + ng); rowptr / tails: the level
// CSR with dense tails; g_rowptr / g_heads: ghost -> local reverse CSR
// (g_rowptr int64 [ng + 1]); active: uint8 [nv], written in place. No host
// sync: the prefix sums over the changed rows' degrees stay on the device.
void frontier_expand(at::Tensor changed, at::Tensor rowptr, at::Tensor tails,
                     at::Tensor g_rowptr, at::Tensor g_heads,
                     at::Tensor active) {
  CHECK_INPUT(changed);
  CHECK_INPUT(rowptr);
  CHECK_INPUT(tails);
  CHECK_INPUT(g_rowptr);
  CHECK_INPUT(g_heads);
  CHECK_INPUT(active);
  TORCH_CHECK(changed.scalar_type() == at::kInt, "changed must be int32");
  TORCH_CHECK(rowptr.scalar_type() == at::kLong &&
              g_rowptr.scalar_type() == at::kLong,
              "rowptr / g_rowptr must be int64");
  TORCH_CHECK(tails.scalar_type() == at::kInt &&
              g_heads.scalar_type() == at::kInt,
              "tails / g_heads must be int32");
  TORCH_CHECK(active.scalar_type() == at::kByte, "active must be uint8");
  TORCH_CHECK(rowptr.numel() >= 1 && g_rowptr.numel() >= 1,
              "rowptr / g_rowptr must have n + 1 entries");
  const int64_t nv = rowptr.numel() - 1;
  const int64_t ng = g_rowptr.numel() - 1;
  TORCH_CHECK(active.numel() == nv, "active must have one entry per vertex");
  TORCH_CHECK(nv + ng < (int64_t)INT32_MAX,
              "nv + ng exceeds the int32 dense id range");
  const int64_t nc = changed.numel();
  if (nc == 0 || nv == 0) return;
  auto stream = at::hip::getCurrentHIPStream().stream();
  cuvite::FrontierArgs a{};
  a.changed = changed.data_ptr<int32_t>();
  a.nc = nc;
  a.rowptr = rowptr.data_ptr<int64_t>();
  a.tails = tails.data_ptr<int32_t>();
  a.nv = nv;
  a.ne = tails.numel();
  a.g_rowptr = g_rowptr.data_ptr<int64_t>();
  a.g_heads = g_heads.data_ptr<int32_t>();
  a.ng = ng;
  a.neg = g_heads.numel();
  a.active = active.data_ptr<uint8_t>();
  auto offs = at::zeros({nc + 1}, rowptr.options());
  auto deg = at::empty({nc}, rowptr.options());
  cuvite::launch_frontier_degrees(a, deg.data_ptr<int64_t>(), stream);
  offs.narrow(0, 1, nc).copy_(at::cumsum(deg, 0));
  // a row is at most as long as its CSR, so this bounds offs[nc] for a
  // duplicate-free list; a longer total is covered by the span stride
  const int64_t edge_bound = a.ne + a.neg;
  cuvite::launch_frontier_expand(a, offs.data_ptr<int64_t>(), edge_bound,
                                 stream);
  C10_HIP_CHECK(hipGetLastError());
}

// Class lists of the active vertices (see frontier_compact_kernel). active:
// uint8 [nv]; cls: uint8 [nv], class id per vertex in [0, frontier_classes()).
// Returns (lists int32 [nv], counts int32 [frontier_classes()]): class c's
// ascending vertex ids sit at lists[sum(counts[:c]) : sum(counts[:c + 1])].
// Both stay on the device; the caller reads counts with one copy.
std::vector<at::Tensor> frontier_compact(at::Tensor active, at::Tensor cls) {
  CHECK_INPUT(active);
  CHECK_INPUT(cls);
  TORCH_CHECK(active.scalar_type() == at::kByte &&
              cls.scalar_type() == at::kByte, "active / cls must be uint8");
  const int64_t nv = active.numel();
  TORCH_CHECK(cls.numel() == nv, "active / cls length mismatch");
  TORCH_CHECK(nv < (int64_t)INT32_MAX, "nv exceeds the int32 dense id range");
  const int C = cuvite::frontier_classes();
  auto i32 = active.options().dtype(at::kInt);
  auto lists = at::empty({nv}, i32);
  if (nv == 0) return {lists, at::zeros({C}, i32)};
  const int64_t nunit = cuvite::frontier_units(nv);
  auto stream = at::hip::getCurrentHIPStream().stream();
  auto unit_cnt = at::empty({nunit, C}, i32);
  cuvite::launch_frontier_compact(
      active.data_ptr<uint8_t>(), cls.data_ptr<uint8_t>(), nv,
      unit_cnt.data_ptr<int32_t>(), nullptr, nullptr, nullptr, false, stream);
  auto incl = at::cumsum(unit_cnt, 0, at::kInt);
  auto counts = incl.select(0, nunit - 1).contiguous();
  auto unit_off = (incl - unit_cnt).contiguous();
  auto class_base = (at::cumsum(counts, 0, at::kInt) - counts).contiguous();
  cuvite::launch_frontier_compact(
      active.data_ptr<uint8_t>(), cls.data_ptr<uint8_t>(), nv, nullptr,
      unit_off.data_ptr<int32_t>(), class_base.data_ptr<int32_t>(),
      lists.data_ptr<int32_t>(), true, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {lists, counts};
}

void check_i64(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), name,
              " must be a contiguous GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kLong, name, " must be int64");
}

// The part of the batch arguments that both bindings fill: the old CSR and
// the touched rows.
cuvite::BatchRows batch_rows(const at::Tensor& rowptr, const at::Tensor& tails,
                             const at::Tensor& t_rows,
                             const at::Tensor& t_offs, int64_t n_touched) {
  check_i64(rowptr, "rowptr");
  check_i64(tails, "tails");
  check_i64(t_rows, "t_rows");
  check_i64(t_offs, "t_offs");
  TORCH_CHECK(rowptr.numel() >= 1, "rowptr must have nv + 1 entries");
  TORCH_CHECK(t_offs.numel() == t_rows.numel() + 1,
              "t_offs must have one entry more than t_rows");
  TORCH_CHECK(n_touched >= 0 && n_touched <= tails.numel(),
              "n_touched must lie in [0, ne]");
  cuvite::BatchRows r{};
  r.rowptr = rowptr.data_ptr<int64_t>();
  r.tails = tails.data_ptr<int64_t>();
  r.nv = rowptr.numel() - 1;
  r.ne = tails.numel();
  r.t_rows = t_rows.data_ptr<int64_t>();
  r.t_offs = t_offs.data_ptr<int64_t>();
  r.nt = t_rows.numel();
  r.n_touched = n_touched;
  return r;
}

// Edge batch, first half (see batch_mark_kernel). t_rows: the touched local
// rows, ascending, each in [0, nv); t_offs: prefix sums of their old degrees,
// n_touched = t_offs[nt] as the host knows it; d_offs / d_dst: per-row slices
// of the deduplicated deletions, tails ascending inside a row. Returns (keep
// uint8 [n_touched], span_cnt int64 [spans], row_kept int64 [nt], matched
// uint8 [nd]). No host sync.
std::vector<at::Tensor> batch_mark(at::Tensor rowptr, at::Tensor tails,
                                   at::Tensor t_rows, at::Tensor t_offs,
                                   int64_t n_touched, at::Tensor d_offs,
                                   at::Tensor d_dst) {
  cuvite::BatchMarkArgs a{};
  a.rows = batch_rows(rowptr, tails, t_rows, t_offs, n_touched);
  check_i64(d_offs, "d_offs");
  check_i64(d_dst, "d_dst");
  TORCH_CHECK(d_offs.numel() == a.rows.nt + 1,
              "d_offs must have one entry more than t_rows");
  auto u8 = rowptr.options().dtype(at::kByte);
  auto keep = at::empty({n_touched}, u8);
  auto span_cnt = at::zeros({cuvite::batch_spans(n_touched)},
                            rowptr.options());
  auto row_kept = at::zeros({a.rows.nt}, rowptr.options());
  auto matched = at::zeros({d_dst.numel()}, u8);
  a.d_offs = d_offs.data_ptr<int64_t>();
  a.d_dst = d_dst.data_ptr<int64_t>();
  a.nd = d_dst.numel();
  a.d_matched = matched.data_ptr<uint8_t>();
  a.keep = keep.data_ptr<uint8_t>();
  a.span_cnt = span_cnt.data_ptr<int64_t>();
  a.row_kept = row_kept.data_ptr<int64_t>();
  auto stream = at::hip::getCurrentHIPStream().stream();
  cuvite::launch_batch_mark(a, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {keep, span_cnt, row_kept, matched};
}

template <typename W>
std::vector<at::Tensor> batch_write_impl(
    const at::Tensor& rowptr, const at::Tensor& tails,
    const at::Tensor& weights, const at::Tensor& t_rows,
    const at::Tensor& t_offs, int64_t n_touched, const at::Tensor& keep,
    const at::Tensor& span_offs, const at::Tensor& kept_offs,
    const at::Tensor& row_kept, const at::Tensor& touched,
    const at::Tensor& new_rowptr, int64_t new_ne, const at::Tensor& i_offs,
    const at::Tensor& i_dst, const at::Tensor& i_w) {
  cuvite::BatchWriteArgs<W> a{};
  a.rows = batch_rows(rowptr, tails, t_rows, t_offs, n_touched);
  auto new_tails = at::empty({new_ne}, tails.options());
  auto new_weights = at::empty({new_ne}, weights.options());
  a.weights = weights.data_ptr<W>();
  a.keep = keep.data_ptr<uint8_t>();
  a.row_kept = row_kept.data_ptr<int64_t>();
  a.touched = touched.data_ptr<uint8_t>();
  a.span_offs = span_offs.data_ptr<int64_t>();
  a.kept_offs = kept_offs.data_ptr<int64_t>();
  a.new_rowptr = new_rowptr.data_ptr<int64_t>();
  a.new_ne = new_ne;
  a.new_tails = new_tails.data_ptr<int64_t>();
  a.new_weights = new_weights.data_ptr<W>();
  a.i_offs = i_offs.data_ptr<int64_t>();
  a.i_dst = i_dst.data_ptr<int64_t>();
  a.i_w = i_w.data_ptr<W>();
  a.ni = i_dst.numel();
  auto stream = at::hip::getCurrentHIPStream().stream();
  cuvite::launch_batch_copy(a, stream);
  cuvite::launch_batch_compact(a, stream);
  C10_HIP_CHECK(hipGetLastError());
  return {new_tails, new_weights};
}

// Edge batch, second half (batch_copy_kernel, batch_compact_kernel,
// batch_insert_kernel): fills the new CSR's tails and weights. keep /
// row_kept: batch_mark's results; span_offs / kept_offs: exclusive scans of
// its span_cnt / row_kept; touched: uint8 [nv], 1 for every row of t_rows;
// new_rowptr / new_ne: the new CSR's offsets and its edge count as the host
// knows it; i_offs / i_dst / i_w: per-row slices of the insertions in list
// order. Returns (new_tails int64 [new_ne], new_weights [new_ne]).
std::vector<at::Tensor> batch_write(
    at::Tensor rowptr, at::Tensor tails, at::Tensor weights, at::Tensor t_rows,
    at::Tensor t_offs, int64_t n_touched, at::Tensor keep,
    at::Tensor span_offs, at::Tensor kept_offs, at::Tensor row_kept,
    at::Tensor touched, at::Tensor new_rowptr, int64_t new_ne,
    at::Tensor i_offs, at::Tensor i_dst, at::Tensor i_w) {
  CHECK_INPUT(weights);
  CHECK_INPUT(keep);
  CHECK_INPUT(touched);
  CHECK_INPUT(i_w);
  check_i64(span_offs, "span_offs");
  check_i64(kept_offs, "kept_offs");
  check_i64(row_kept, "row_kept");
  check_i64(new_rowptr, "new_rowptr");
  check_i64(i_offs, "i_offs");
  check_i64(i_dst, "i_dst");
  TORCH_CHECK(keep.scalar_type() == at::kByte &&
              touched.scalar_type() == at::kByte,
              "keep / touched must be uint8");
  const int64_t nv = rowptr.numel() - 1;
  const int64_t nt = t_rows.numel();
  TORCH_CHECK(weights.numel() == tails.numel(), "tails / weights mismatch");
  TORCH_CHECK(keep.numel() == n_touched, "keep must have n_touched entries");
  TORCH_CHECK(span_offs.numel() == cuvite::batch_spans(n_touched),
              "span_offs must have one entry per span");
  TORCH_CHECK(kept_offs.numel() == nt && row_kept.numel() == nt &&
              i_offs.numel() == nt + 1,
              "kept_offs / row_kept / i_offs do not match t_rows");
  TORCH_CHECK(touched.numel() == nv && new_rowptr.numel() == nv + 1,
              "touched / new_rowptr do not match rowptr");
  TORCH_CHECK(new_ne >= 0, "new_ne must not be negative");
  TORCH_CHECK(i_w.numel() == i_dst.numel() &&
              i_w.scalar_type() == weights.scalar_type(),
              "i_w must match i_dst and the weight dtype");
  if (weights.scalar_type() == at::kFloat)
    return batch_write_impl<float>(rowptr, tails, weights, t_rows, t_offs,
                                   n_touched, keep, span_offs, kept_offs,
                                   row_kept, touched, new_rowptr, new_ne,
                                   i_offs, i_dst, i_w);
  TORCH_CHECK(weights.scalar_type() == at::kDouble,
              "weights must be fp32 or fp64");
  return batch_write_impl<double>(rowptr, tails, weights, t_rows, t_offs,
                                  n_touched, keep, span_offs, kept_offs,
                                  row_kept, touched, new_rowptr, new_ne,
                                  i_offs, i_dst, i_w);
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("batch_mark", &batch_mark,
        "edge batch: keep flags, kept counts and matched deletions over the "
        "touched rows (HIP); returns (keep, span_cnt, row_kept, matched)",
        py::arg("rowptr"), py::arg("tails"), py::arg("t_rows"),
        py::arg("t_offs"), py::arg("n_touched"), py::arg("d_offs"),
        py::arg("d_dst"));
  m.def("batch_write", &batch_write,
        "edge batch: the new CSR's tails and weights, untouched rows copied, "
        "touched rows compacted and appended to (HIP)",
        py::arg("rowptr"), py::arg("tails"), py::arg("weights"),
        py::arg("t_rows"), py::arg("t_offs"), py::arg("n_touched"),
        py::arg("keep"), py::arg("span_offs"), py::arg("kept_offs"),
        py::arg("row_kept"), py::arg("touched"), py::arg("new_rowptr"),
        py::arg("new_ne"), py::arg("i_offs"), py::arg("i_dst"),
        py::arg("i_w"));
  m.def("batch_span", &cuvite::batch_span,
        "touched entries per wave span of the edge-batch kernels");
  m.def("local_move_bucketed", &local_move,
        "Louvain local-move iteration (HIP, degree-class routed)",
        py::arg("rowptr"), py::arg("tails"), py::arg("weights"),
        py::arg("curr_comm"), py::arg("v_degree"), py::arg("comm_size"),
        py::arg("comm_degree"), py::arg("comm_gid"), py::arg("constant"),
        py::arg("vlists"), py::arg("gid_base") = 0, py::arg("n_local") = 0,
        py::arg("next_size") = py::none(),
        py::arg("next_degree") = py::none(), py::arg("class_streams") = true,
        py::arg("out_target") = py::none(), py::arg("out_cw") = py::none(),
        py::arg("keep_cw") = false);
  m.def("refine_move_bucketed", &refine_move,
        "Leiden refine round (HIP, degree-class routed, bound-filtered)",
        py::arg("rowptr"), py::arg("tails"), py::arg("weights"),
        py::arg("curr_comm"), py::arg("v_degree"), py::arg("comm_degree"),
        py::arg("comm_gid"), py::arg("constant"), py::arg("vlists"),
        py::arg("mover_bound"), py::arg("cand_bound"),
        py::arg("gid_base") = 0, py::arg("n_local") = 0,
        py::arg("class_streams") = true,
        py::arg("out_target") = py::none(), py::arg("out_cw") = py::none());
  m.def("hub_refine_moves", &hub_refine_moves,
        "Leiden refine round for hub vertices: segsort + bound-filtered "
        "sliced argmax",
        py::arg("tails_flat"), py::arg("weights_flat"), py::arg("eoffs"),
        py::arg("hubs_i32"), py::arg("hub_self"), py::arg("curr_comm"),
        py::arg("v_degree"), py::arg("comm_degree"), py::arg("comm_gid"),
        py::arg("constant"), py::arg("mover_bound"), py::arg("cand_bound"),
        py::arg("gid_base") = 0, py::arg("n_local") = 0);
  m.def("modularity_parts", &modularity_parts,
        "fp64 (sum cw, sum degree^2) reduction (HIP)");
  m.def("scatter_add_", &scatter_add_,
        "out[idx[i]] += val[i] with native fp atomics (HIP)");
  m.def("csr_from_edges", &csr_from_edges,
        "sort-free CSR assembly on device (HIP)");
  m.def("row_sum", &row_sum, "per-row CSR weight sum (HIP)");
  m.def("apply_deltas_", &apply_deltas_,
        "fused community size/degree delta update for moved vertices (HIP)");
  m.def("sort_reduce_pairs", &sort_reduce_pairs,
        "narrow-bit radix sort + reduce_by_key coarse-edge aggregate "
        "(rocPRIM)");
  m.def("coloring_minmax", &coloring_minmax,
        "per-vertex multi-hash min/max over competing neighbors (HIP)");
  m.def("recount_", &recount_,
        "fresh community size/degree recount from labels (HIP)");
  m.def("intra_weight", &intra_weight,
        "per-vertex weight into the own community, edge-balanced (HIP)");
  m.def("intra_boundary", &intra_boundary,
        "intra_weight plus the uint8 boundary mask, in one edge pass");
  m.def("intra_weight_span", &cuvite::intra_weight_span,
        "edges per wave span of the intra_weight kernel");
  m.def("cc_components", &cc_components,
        "connected components over same-label edges, hook + compress rounds "
        "(HIP); returns (comp, rounds)");
  m.def("frontier_expand", &frontier_expand,
        "mark the changed locals and the local neighbours of the changed "
        "dense ids, span-balanced (HIP)",
        py::arg("changed"), py::arg("rowptr"), py::arg("tails"),
        py::arg("g_rowptr"), py::arg("g_heads"), py::arg("active"));
  m.def("frontier_span", &cuvite::frontier_span,
        "edges per wave span of the frontier_expand kernel");
  m.def("frontier_compact", &frontier_compact,
        "ascending per-class lists of the active vertices and their counts "
        "(HIP); returns (lists, counts)",
        py::arg("active"), py::arg("cls"));
  m.def("frontier_classes", &cuvite::frontier_classes,
        "number of class ids frontier_compact sorts into");
  m.def("hub_slices", &cuvite::hub_slices,
        "element slices per hub segment in the hub argmax kernels");
  m.def("hub_moves", &hub_moves,
        "full device-side hub move: segsort + sliced run-sum argmax",
        py::arg("tails_flat"), py::arg("weights_flat"), py::arg("eoffs"), py::arg("hubs_i32"), py::arg("hub_self"),
        py::arg("curr_comm"), py::arg("v_degree"), py::arg("comm_size"),
        py::arg("comm_degree"), py::arg("comm_gid"), py::arg("constant"),
        py::arg("gid_base") = 0, py::arg("n_local") = 0,
        py::arg("next_size") = py::none(),
        py::arg("next_degree") = py::none());
}
