// torch_ops.cpp -- torch.ops.isplib.* for device tensors, on top of the C ABI.
//
// Mirrors the reference's operator + autograd layer (csrc/fusedmm.cpp:206-570):
// same op names and argument lists, same saved-for-backward operands, same
// backward formulas -- with the launcher (csrc/fusedmm.cpp:113-203) replaced by
// fusedMM_csr_hip and the ATen scatter chain of max/min backward replaced by
// one fused kernel.  Host-side only: no kernels here, torch is used for memory,
// the current stream and autograd bookkeeping.
//
// Deliberate differences from the reference (each is a defect there):
//   * tensors must live on the GPU; there is NO CPU path (a CPU tensor raises).
//   * value == None means unit weights and the value stream is never read (the
//     reference substitutes ones_like(col), an int64 tensor, :241,:329).
//   * the cached transpose operands (value_index_select / row_index_select /
//     new_row / new_rowcount) may be None: they are then built on the device
//     when backward needs them (the reference dereferences them blindly,
//     :246-247,:333).
//   * grad_value of sum/mean is computed (SDDMM); the reference returns an
//     undefined tensor (:268-272,:349-353).
//   * outputs are torch::empty: the kernel writes every element, including the
//     0 / nnz the reference gets from zeros()/full_like() fills (:147-152,171).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/library.h>

#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <limits>
#include <mutex>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/isplib_hip.h"

namespace {

using at::Tensor;
using c10::optional;
using torch::autograd::AutogradContext;
using torch::autograd::Variable;
using torch::autograd::variable_list;

enum Reduction { R_SUM = 0, R_MAX = 1, R_MIN = 2, R_MEAN = 3 };   // codes of csrc/fusedmm.cpp:168-186

void check_status(int st, const char *what) {
   TORCH_CHECK(st == ISPLIB_SUCCESS, what, " failed with status ", st, ": ", isplib_hip_last_error());
}

void check_index(const Tensor &t, const char *name) {
   TORCH_CHECK(t.defined(), "isplib: `", name, "` is missing");
   TORCH_CHECK(t.is_cuda(), "isplib: `", name, "` must be a GPU tensor -- isplib_amd has no CPU path");
   TORCH_CHECK(t.scalar_type() == at::kLong, "isplib: `", name, "` must be int64 (csrc/fusedmm.cpp:43)");
}

void check_float(const Tensor &t, const char *name) {
   TORCH_CHECK(t.defined(), "isplib: `", name, "` is missing");
   TORCH_CHECK(t.is_cuda(), "isplib: `", name, "` must be a GPU tensor -- isplib_amd has no CPU path");
   TORCH_CHECK(t.scalar_type() == at::kFloat, "isplib: `", name, "` must be float32 (csrc/fusedmm.cpp:44)");
}

// 16-bit features (bf16 / fp16) of the SpMM operators: products, sums and the mean's division in fp32, the finished row rounded
// once to the operand's type (include/isplib_hip.h: fusedMM_csr_stream16_hip).  Everything the native entry does not serve takes
// the CONVERSION ROUTE -- the operand to fp32, the fp32 path unchanged, the result to the operand's type -- which has the same
// semantics by construction.  Edge weights are fp32 everywhere: a 16-bit `value` is brought to fp32 (exact).
bool is_half(const Tensor &t) { return t.defined() && (t.scalar_type() == at::kBFloat16 || t.scalar_type() == at::kHalf); }

void check_feature(const Tensor &t, const char *name) {
   TORCH_CHECK(t.defined(), "isplib: `", name, "` is missing");
   TORCH_CHECK(t.is_cuda(), "isplib: `", name, "` must be a GPU tensor -- isplib_amd has no CPU path");
   TORCH_CHECK(t.scalar_type() == at::kFloat || is_half(t), "isplib: `", name, "` must be float32, bfloat16 or float16");
}

Tensor as_float(const Tensor &t) { return t.defined() && t.scalar_type() != at::kFloat ? t.to(at::kFloat) : t; }

void *current_stream(const Tensor &t) { return (void *)c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// ISPLIB_DEBUG=1: per-operator device time on stderr under the reference's own labels (the commented-out timers
// of csrc/fusedmm.cpp:52-53,252-253,288-289,...: FUSEDMM_SPMM_<RED>_{FW,BW}).  Synchronises per op: debugging only.
struct OpTimer {
   const char *name;
   bool on;
   hipStream_t st = nullptr;
   hipEvent_t a = nullptr, b = nullptr;
   OpTimer(const char *n, const Tensor &t) : name(n) {
      static const bool enabled = [] { const char *e = std::getenv("ISPLIB_DEBUG"); return e && *e && *e != '0'; }();
      on = enabled && t.defined() && t.is_cuda();
      if (!on) return;
      st = (hipStream_t)current_stream(t);
      on = hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess && hipEventRecord(a, st) == hipSuccess;
   }
   ~OpTimer() {
      if (on && hipEventRecord(b, st) == hipSuccess && hipEventSynchronize(b) == hipSuccess) {
         float ms = 0.0f;
         if (hipEventElapsedTime(&ms, a, b) == hipSuccess) std::fprintf(stderr, "%s: %.3f ms\n", name, ms);
      }
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
   }
};

// fusedmm_spmm_fw, csrc/fusedmm.cpp:113-203
// `plan`: per-graph schedule operands (isplib_amd/plan.py, include/isplib_hip.h):
//   {}                                                   plain row kernel
//   {sliceptr}                                           column-sliced kernel
//   {task_row, task_b, task_len, seg_off, lane_off_cpu}  task-list kernel
using Plan = std::vector<Tensor>;
// task plan = {task_row, task_b, task_len, seg_off, lane_off (host)} + optionally the 32-bit copy of col
static inline bool is_task_plan(const Plan &p) { return p.size() == 5 || p.size() == 6; }
// stream plan (sum / mean; isplib_stream_plan) = {words, vals (empty = unit weights), wave_step_off, wave_row, wave_part,
// hub_row, hub_off, meta (host int64: rows, cols, slices, gens, waves_per_gen, rows_per_wave, streams, n_steps, n_parts, n_hub)}
static inline bool is_stream_plan(const Plan &p) { return p.size() == 8 || p.size() == 9; }   // 9: + perm (max / min)
// what the reference-schema operators pass: "no plan was given, choose for me" (one undefined tensor), as opposed
// to the empty plan of the *_planned operators, which means "the plain kernel, please"
static inline Plan auto_plan() { return Plan{Tensor()}; }
static inline bool is_auto_plan(const Plan &p) { return p.size() == 1 && !p[0].defined(); }
// 16-bit row plan (a 16-bit `mat`; sum / mean: fusedMM_csr_rows16_hip, max / min: fusedMM_csr_rows16_minmax_hip) = {row order (device int32 [M], or EMPTY int32 = index order),
// marker (host int32 [1] = 16)}: the plug-in's decision (rows16_route, rows16_minmax_route) handed over with the call -- nothing is re-read from the
// environment here.  For an fp32 `mat` (e.g. the conversion route of an operand the entry does not serve) it means what its first
// tensor means alone: the plain kernel, in that row order
static inline bool is_rows16_plan(const Plan &p) {
   return p.size() == 2 && p[0].defined() && p[0].scalar_type() == at::kInt && p[1].defined() && !p[1].is_cuda() &&
          p[1].scalar_type() == at::kInt && p[1].numel() == 1 && p[1].data_ptr<int32_t>()[0] == 16;
}
// the three-element form a mean's plan_t may take: a 16-bit row plan + the fp32 device table 1 / max(deg, 1) of A's rows (the
// plug-in's rows16_mean_bw_route said "rows16").  SpmmMean::backward reads it; everywhere else it means its first two tensors
static inline bool is_rows16_colscale_plan(const Plan &p) {
   return p.size() == 3 && is_rows16_plan(Plan{p[0], p[1]}) && p[2].defined() && p[2].is_cuda() && p[2].scalar_type() == at::kFloat &&
          p[2].dim() == 1;
}
// the three-element form the forward `plan` of a sum / mean may take: a 16-bit row plan + a second marker (host int32 [1] = 0xDA) --
// the plug-in's rows16_da_route said "rows16": the value gradient of this call runs on isplib_sddmm_csr_rows16_hip.  The forward
// strips it (forward_plan) before it reads the plan; SpmmSum::backward / SpmmMean::backward read it (value_grad), nobody else does
static inline bool is_rows16_da_plan(const Plan &p) {
   return p.size() == 3 && is_rows16_plan(Plan{p[0], p[1]}) && p[2].defined() && !p[2].is_cuda() && p[2].scalar_type() == at::kInt &&
          p[2].numel() == 1 && p[2].data_ptr<int32_t>()[0] == 0xDA;
}
static inline Plan forward_plan(const Plan &p) { return is_rows16_da_plan(p) ? Plan{p[0], p[1]} : p; }
static inline const int32_t *plan_col32(const Plan &p, const Tensor &col) {
   if (p.size() != 6) return nullptr;
   TORCH_CHECK(p[5].scalar_type() == at::kInt && p[5].numel() == col.numel() && p[5].device() == col.device(),
               "isplib: the plan's packed column ids do not match col");
   return p[5].data_ptr<int32_t>();
}
// the C struct of a stream plan handed over as a tensor list (is_stream_plan), checked against its own meta
static isplib_stream_plan stream_plan_of(const Plan &plan) {
   const Tensor &words = plan[0], &vals = plan[1], &step_off = plan[2], &wave_row = plan[3], &wave_part = plan[4],
                &hub_row = plan[5], &hub_off = plan[6], &meta = plan[7];
   TORCH_CHECK(!meta.is_cuda() && meta.scalar_type() == at::kLong && meta.numel() == 11, "isplib: stream plan meta must be 11 host int64");
   TORCH_CHECK(words.is_cuda() && words.scalar_type() == at::kInt && step_off.scalar_type() == at::kLong &&
                   wave_row.scalar_type() == at::kInt && wave_part.scalar_type() == at::kInt &&
                   hub_row.scalar_type() == at::kInt && hub_off.scalar_type() == at::kInt &&
                   (vals.numel() == 0 || (vals.scalar_type() == at::kFloat && vals.numel() == words.numel())),
               "isplib: malformed stream plan");
   const int64_t *mt = meta.data_ptr<int64_t>();
   isplib_stream_plan sp;
   sp.rows = mt[0]; sp.cols = mt[1]; sp.slices = (int32_t)mt[2]; sp.gens = (int32_t)mt[3]; sp.waves_per_gen = (int32_t)mt[4];
   sp.rows_per_wave = (int32_t)mt[5]; sp.streams = (int32_t)mt[6]; sp.n_steps = mt[7]; sp.n_parts = mt[8]; sp.n_hub = mt[9]; sp.chunk = (int32_t)mt[10];
   TORCH_CHECK(words.numel() == sp.n_steps * sp.streams && step_off.numel() == (int64_t)sp.gens * sp.waves_per_gen + 1 &&
                   wave_row.numel() == (int64_t)sp.gens * sp.waves_per_gen * sp.rows_per_wave && wave_part.numel() == wave_row.numel() &&
                   hub_row.numel() == sp.n_hub && hub_off.numel() == sp.n_hub + 1,
               "isplib: stream plan arrays do not match its meta");
   sp.words = words.data_ptr<int32_t>();
   sp.vals = vals.numel() ? vals.data_ptr<float>() : nullptr;
   sp.wave_step_off = step_off.data_ptr<int64_t>();
   sp.wave_row = wave_row.data_ptr<int32_t>();
   sp.wave_part = wave_part.data_ptr<int32_t>();
   sp.hub_row = sp.n_hub ? hub_row.data_ptr<int32_t>() : nullptr;
   sp.hub_off = hub_off.data_ptr<int32_t>();
   sp.perm = nullptr;
   sp.packed = nullptr; sp.has_packed = 0;      // a tensor-list plan carries no packed word stream: these calls read `words`
   if (plan.size() == 9) {
      TORCH_CHECK(plan[8].is_cuda() && plan[8].scalar_type() == at::kInt && plan[8].numel() == words.numel(), "isplib: stream plan perm must be int32, one per word");
      sp.perm = plan[8].data_ptr<int32_t>();
   }
   return sp;
}

// ---- per-graph handles for callers that pass no plan (the reference-schema operators) --------------------------
// iSpLib's Python keeps its per-graph operands in dicts keyed by raw data pointers (isplib/__init__.py:35-40,50) and
// calls the operators with just (rowptr, col, value, mat).  To give that caller the fast schedules, the operator
// library keeps one isplib_graph per STRUCTURE (rowptr, col, dense rows) it has seen -- keyed by the same pointers,
// but every hit is checked against weak references to the very tensors (and their version counters), so a
// freed-and-reused address can never serve a stale plan.  The weights are an argument of the call, not part of the
// key: another `value` tensor, or the same one stepped in place by an optimiser (its version counter moves), keeps
// the plans, the packed column ids and the CSC structure and only tells the handle that its copies of the weights
// are stale (isplib_graph_set_values: no synchronisation, nothing freed).  Small graphs never get here.
struct GraphCacheEntry {
   c10::weak_intrusive_ptr<c10::TensorImpl> rowptr, col, value;
   uint32_t v_rowptr = 0, v_col = 0, v_value = 0;
   bool has_value = false;
   isplib_graph *handle = nullptr;
   GraphCacheEntry(const Tensor &r, const Tensor &c, const Tensor &v)
       : rowptr(r.getIntrusivePtr()), col(c.getIntrusivePtr()), value(v.defined() ? v.getIntrusivePtr() : c.getIntrusivePtr()),
         v_rowptr(r._version()), v_col(c._version()), v_value(v.defined() ? v._version() : 0), has_value(v.defined()) {}
   bool alive() const { return !rowptr.expired() && !col.expired(); }
   bool same_structure(const Tensor &r, const Tensor &c) const {
      return rowptr.lock() == r.getIntrusivePtr() && col.lock() == c.getIntrusivePtr() && v_rowptr == r._version() && v_col == c._version();
   }
   bool same_values(const Tensor &v) const {
      return has_value == v.defined() && (!v.defined() || (value.lock() == v.getIntrusivePtr() && v_value == v._version()));
   }
   void remember_values(const Tensor &v, const Tensor &c) {
      value = c10::weak_intrusive_ptr<c10::TensorImpl>(v.defined() ? v.getIntrusivePtr() : c.getIntrusivePtr());
      v_value = v.defined() ? v._version() : 0;
      has_value = v.defined();
   }
};
struct GraphKey {
   const void *rowptr, *col;
   int64_t n;
   bool operator==(const GraphKey &o) const { return rowptr == o.rowptr && col == o.col && n == o.n; }
};
struct GraphKeyHash {
   size_t operator()(const GraphKey &k) const {
      return std::hash<const void *>()(k.rowptr) ^ (std::hash<const void *>()(k.col) << 1) ^ std::hash<int64_t>()(k.n);
   }
};
std::mutex g_graph_mutex;
std::unordered_map<GraphKey, GraphCacheEntry, GraphKeyHash> g_graphs;
// Handles whose graph is gone or has changed.  isplib_graph_destroy synchronises the device (nothing of the handle's may
// still be in flight when its memory goes), which must not happen inside somebody's forward call: retired handles wait
// here until the next NEW graph gets its handle -- a point where the call synchronises anyway (the plan builders do) and
// is about to allocate what the dead handles hold (plans of A and A^T, packed ids, CSC arrays, workspaces: several GB
// for a Reddit-sized graph): a job that cycles through large graphs never holds more than the graphs retired since the
// last one was created -- or until graph_cache_clear().  graph_cache_size() counts them in.
std::vector<isplib_graph *> g_retired;

void retire_handle_locked(isplib_graph *h) { g_retired.push_back(h); }

void destroy_retired_locked() {
   for (isplib_graph *r : g_retired) isplib_graph_destroy(r);
   g_retired.clear();
}

// the handle of the structure (rowptr, col) with N dense rows; g_graph_mutex must be held.  with_values: the call is
// going to read the weights (SpMM and its backward), so the handle must hold `value` as it is now; SDDMM does not
// read them and takes the handle as it finds it.
isplib_graph *graph_handle_locked(const Tensor &rowptr, const Tensor &col, const Tensor &value, int64_t N, bool with_values = true) {
   const int64_t M = rowptr.numel() - 1, nnz = col.numel();
   const GraphKey key{rowptr.data_ptr(), col.data_ptr(), N};
   auto it = g_graphs.find(key);
   if (it != g_graphs.end() && !it->second.same_structure(rowptr, col)) {
      retire_handle_locked(it->second.handle);
      g_graphs.erase(it);
      it = g_graphs.end();
   }
   if (it == g_graphs.end()) {
      for (auto dead = g_graphs.begin(); dead != g_graphs.end();) {      // graphs whose tensors are gone
         if (!dead->second.alive()) {
            retire_handle_locked(dead->second.handle);
            dead = g_graphs.erase(dead);
         } else {
            ++dead;
         }
      }
      destroy_retired_locked();
      const Tensor first = with_values ? value : Tensor();
      GraphCacheEntry e(rowptr, col, first);
      check_status(isplib_graph_create(M, N, nnz, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                       first.defined() ? first.data_ptr<float>() : nullptr, &e.handle),
                   "isplib_graph_create");
      it = g_graphs.emplace(key, std::move(e)).first;
   } else if (with_values && !it->second.same_values(value)) {
      check_status(isplib_graph_set_values(it->second.handle, value.defined() ? value.data_ptr<float>() : nullptr), "isplib_graph_set_values");
      it->second.remember_values(value, col);
   }
   return it->second.handle;
}

bool spmm_through_handle(int32_t msg, const Tensor &rowptr, const Tensor &col, const Tensor &value, const Tensor &mat,
                         Tensor &out, Tensor &arg) {
   const int64_t M = rowptr.numel() - 1, N = mat.size(0), K = mat.size(1), nnz = col.numel();
   if (isplib_suggest_slices(M, N, nnz, K, (msg & 0xF0000) != ISPLIB_AOP_ADD) <= 0) return false;
   std::lock_guard<std::mutex> lock(g_graph_mutex);        // also serialises the handle's shared workspace
   isplib_graph *handle = graph_handle_locked(rowptr, col, value, N);
   const int st = isplib_graph_spmm(handle, msg, K, mat.data_ptr<float>(), K, out.data_ptr<float>(), K,
                                    arg.defined() ? arg.data_ptr<int64_t>() : nullptr, current_stream(mat));
   if (st == ISPLIB_NOT_ENOUGH_MEM) return false;      // no room for the plan beside torch's pool: the plain kernel needs none
   check_status(st, "isplib_graph_spmm");
   return true;
}

// The pitch (floats per row) a gathered [N, K] operand of the stream schedule should be read at: 48 for 33..47 columns (the
// GCN's 41 classes) on large graphs, K otherwise.  What the address pipeline charges for is the 128-byte line a gather
// touches, and a 164-byte row at its packed pitch straddles 2.25 of them on average, at a 192-byte pitch exactly 2 -- Reddit
// shape K=41: 1.365 -> 1.285 ms, the copy 0.015 (scripts/exp_round4.py k41; 176 B: no gain, 256 B: 1.314).  The wider
// operand has to stay inside the max / min stream entry's 2 GiB.
static int64_t gather_pitch(int64_t N, int64_t K, bool stream) {
   return (stream && K > 32 && K < 48 && N >= (1 << 16) && isplib_rows_within(N, 48, ISPLIB_STREAM_MINMAX_BYTES_END - 1u)) ? 48 : K;
}

// a [N, K] matrix whose rows may sit at a wider pitch (a view of an [N, pitch] buffer): usable as it is by the stream entries
static bool row_strided(const Tensor &t) { return t.dim() == 2 && t.stride(1) == 1 && (t.size(0) <= 1 || t.stride(0) >= t.size(1)); }

std::tuple<Tensor, Tensor> spmm_fw(const Tensor &rowptr_, const Tensor &col_, const optional<Tensor> &value_,
                                   const Tensor &mat_, int reduction, const Plan &plan, bool want_arg);

// a 16-bit operand the native entries can read packed: contiguous AND on a 4-byte boundary.  A contiguous tensor may start 2 bytes
// past one (an odd-element slice of a flat buffer): `contiguous()` returns it as it is, so it is copied (16 bits, a fresh allocation)
static Tensor packed16(const Tensor &t) {
   const Tensor c = t.contiguous();
   return (reinterpret_cast<uintptr_t>(c.data_ptr()) & 3) == 0 ? c : c.clone(at::MemoryFormat::Contiguous);
}

// a row order (int32 [M], position -> row) as the entries read it
static Tensor row_order_of(const Tensor &order_, int64_t M) {
   const Tensor order = order_.contiguous();
   TORCH_CHECK(order.is_cuda() && order.numel() == M, "isplib: the row order must hold one int32 position per row");
   return order;
}

// One call of the 16-bit row family (fusedMM_csr_rows16{,_minmax,_colscale}_hip), prepared: the operand as it lies (a row-strided
// view keeps its pitch) or packed, whichever isplib_rows16_serves accepts, the graph's arrays contiguous, the weights (`per_edge`:
// one per edge, checked; else a table of the caller's length) and the plan's row order.  served = false: the family does not take
// this operand, nothing was copied.  The struct keeps the tensors its pointers point into
struct Rows16Call {
   bool served = false;
   Tensor mat, ptr_t, idx_t, weight_t, order_t;
   int dtype = 0;
   int64_t ldy = 0;
   const int64_t *ptr = nullptr, *idx = nullptr;
   const float *weight = nullptr;      // null = unit weights
   const int32_t *order = nullptr;     // null = index order
};

static Rows16Call rows16_call(const Tensor &ptr_, const Tensor &idx_, const Tensor &weight_, bool per_edge, const Tensor &mat_, const Plan &plan) {
   Rows16Call c;
   const int64_t M = ptr_.numel() - 1, N = mat_.size(0), K = mat_.size(1);
   const bool as_is = row_strided(mat_) && (reinterpret_cast<uintptr_t>(mat_.data_ptr()) & 3) == 0 &&
                      isplib_rows16_serves(N, K, N > 1 ? mat_.stride(0) : K, K);
   if (!as_is && !isplib_rows16_serves(N, K, K, K)) return c;
   c.served = true;
   c.mat = as_is ? mat_ : packed16(mat_);
   c.dtype = c.mat.scalar_type() == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
   c.ldy = N > 1 ? c.mat.stride(0) : K;
   c.ptr_t = ptr_.contiguous();
   c.idx_t = idx_.contiguous();
   c.ptr = c.ptr_t.data_ptr<int64_t>();
   c.idx = c.idx_t.data_ptr<int64_t>();
   if (weight_.defined()) {
      c.weight_t = weight_.contiguous();
      TORCH_CHECK(!per_edge || c.weight_t.numel() == idx_.numel(), "isplib: `value` and `col` differ in length");
      c.weight = c.weight_t.data_ptr<float>();
   }
   if (plan[0].numel() > 0) {
      c.order_t = row_order_of(plan[0], M);
      c.order = c.order_t.data_ptr<int32_t>();
   }
   return c;
}

// A 16-bit `mat`: the native entry when the reduction is sum / mean, the plan is a stream plan of the sum kernel's geometry and
// isplib_stream16_serves accepts the operand as it lies (a row-strided view keeps its pitch) or packed; the 16-bit row entry when
// the plan is a 16-bit row plan (is_rows16_plan) and isplib_rows16_serves accepts the operand the same way -- for sum / mean and, through
// its own entry, for max / min; else the conversion route.
std::tuple<Tensor, Tensor> spmm_fw_half(const Tensor &rowptr_, const Tensor &col_, const optional<Tensor> &value_,
                                        const Tensor &mat_, int reduction, const Plan &plan, bool want_arg) {
   TORCH_CHECK(mat_.dim() == 2, "isplib: `mat` must be 2-D [N, K] (csrc/fusedmm.cpp:121-122)");
   TORCH_CHECK(rowptr_.dim() == 1 && rowptr_.numel() >= 1, "isplib: `rowptr` must be 1-D with M+1 entries");
   const int64_t M = rowptr_.numel() - 1, N = mat_.size(0), K = mat_.size(1), nnz = col_.numel();
   const bool sum_op = reduction == R_SUM || reduction == R_MEAN;
   if (sum_op && is_stream_plan(plan) && plan.size() == 8 && M > 0 && K > 0 && rowptr_.device() == mat_.device()) {
      c10::DeviceGuard guard(mat_.device());
      const bool as_is = row_strided(mat_) && (reinterpret_cast<uintptr_t>(mat_.data_ptr()) & 3) == 0 &&
                         isplib_stream16_serves(N, K, N > 1 ? mat_.stride(0) : K, K, nnz);
      if (as_is || isplib_stream16_serves(N, K, K, K, nnz)) {
         const Tensor mat = as_is ? mat_ : packed16(mat_);
         const int64_t ldy = N > 1 ? mat.stride(0) : K;
         const Tensor rowptr = rowptr_.contiguous();
         const isplib_stream_plan sp = stream_plan_of(plan);
         Tensor out = at::empty({M, K}, mat.options());
         const size_t ws = isplib_spmm_stream_workspace_bytes(&sp);
         Tensor work = at::empty({(int64_t)ws}, mat.options().dtype(at::kByte));
         const int64_t *rp = rowptr.data_ptr<int64_t>();
         const int st = fusedMM_csr_stream16_hip(reduction == R_MEAN ? ISPLIB_MSG_SPMM_MEAN : ISPLIB_MSG_SPMM_SUM,
                                                 mat.scalar_type() == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16, M, N, K, nnz, rp, rp + 1,
                                                 &sp, mat.data_ptr(), ldy, out.data_ptr(), K, work.data_ptr(), ws, current_stream(mat));
         check_status(st, "fusedMM_csr_stream16_hip");
         return std::make_tuple(out, Tensor());
      }
   }
   // a 16-bit row plan: fusedMM_csr_rows16_hip for sum / mean; for max / min fusedMM_csr_rows16_minmax_hip -- values and positions
   // bit-equal to the conversion route below, without the fp32 copy; want_arg = false is its values-only launch (the second tensor
   // stays undefined)
   if (is_rows16_plan(plan) && M > 0 && K > 0 && rowptr_.device() == mat_.device() && col_.device() == mat_.device()) {
      c10::DeviceGuard guard(mat_.device());
      const Tensor value = value_.has_value() && value_->defined() ? *value_ : Tensor();
      const Rows16Call c = rows16_call(rowptr_, col_, value, true, mat_, plan);
      if (c.served) {
         Tensor out = at::empty({M, K}, c.mat.options());
         Tensor arg;
         int st;
         if (sum_op) {
            st = fusedMM_csr_rows16_hip(reduction == R_MEAN ? ISPLIB_MSG_SPMM_MEAN : ISPLIB_MSG_SPMM_SUM, c.dtype, M, N, K, nnz, c.weight, c.idx, c.ptr,
                                        c.ptr + 1, c.order, c.mat.data_ptr(), c.ldy, out.data_ptr(), K, current_stream(c.mat));
         } else {
            if (want_arg) arg = at::empty({M, K}, rowptr_.options());
            st = fusedMM_csr_rows16_minmax_hip(reduction == R_MAX ? ISPLIB_MSG_SPMM_MAX : ISPLIB_MSG_SPMM_MIN, c.dtype, M, N, K, nnz, c.weight, c.idx,
                                               c.ptr, c.ptr + 1, c.order, c.mat.data_ptr(), c.ldy, out.data_ptr(), K,
                                               arg.defined() ? arg.data_ptr<int64_t>() : nullptr, K, current_stream(c.mat));
         }
         check_status(st, sum_op ? "fusedMM_csr_rows16_hip" : "fusedMM_csr_rows16_minmax_hip");
         return std::make_tuple(out, arg);
      }
   }
   auto r = spmm_fw(rowptr_, col_, value_, mat_.to(at::kFloat), reduction, plan, want_arg);
   return std::make_tuple(std::get<0>(r).to(mat_.scalar_type()), std::get<1>(r));
}

// The unit-weight mean backward of a 16-bit dY on the column-scaled row kernel (fusedMM_csr_rows16_colscale_hip):
// dX = A^T (diag(scale) dY) on (colptr, row_t, dY) with scale = 1 / max(deg, 1) applied per gathered row inside the kernel -- no fp32
// dY / deg, no conversion of the result.  Undefined when the call is not served (spmm_fw_half's conditions): the caller then takes
// the route it always took.
static Tensor mean_bw_colscale(const Tensor &colptr_, const Tensor &row_t_, const Tensor &grad_out, const Plan &row_plan, const Tensor &scale_,
                               int64_t rows_of_a) {
   if (!is_half(grad_out) || !is_rows16_plan(row_plan) || grad_out.dim() != 2 || colptr_.dim() != 1 || colptr_.numel() < 1) return Tensor();
   const int64_t M = colptr_.numel() - 1, N = grad_out.size(0), K = grad_out.size(1), nnz = row_t_.numel();
   if (N != rows_of_a || scale_.numel() != N || M <= 0 || K <= 0 || !grad_out.is_cuda() || colptr_.device() != grad_out.device() ||
       row_t_.device() != grad_out.device() || scale_.device() != grad_out.device() || colptr_.scalar_type() != at::kLong ||
       row_t_.scalar_type() != at::kLong)
      return Tensor();
   c10::DeviceGuard guard(grad_out.device());
   const Rows16Call c = rows16_call(colptr_, row_t_, scale_, false, grad_out, row_plan);
   if (!c.served) return Tensor();
   Tensor out = at::empty({M, K}, c.mat.options());
   const int st = fusedMM_csr_rows16_colscale_hip(ISPLIB_MSG_SPMM_SUM, c.dtype, M, N, K, nnz, c.weight, c.idx, c.ptr, c.ptr + 1, c.order,
                                                  c.mat.data_ptr(), c.ldy, out.data_ptr(), K, current_stream(c.mat));
   check_status(st, "fusedMM_csr_rows16_colscale_hip");
   return out;
}

// want_arg = false (max / min through the *_values operators: nobody will ask which edge won): on a stream plan the
// launch then leaves the positions out altogether (isplib_hip.h: fusedMM_csr_stream_minmax_hip with z_arg = NULL) and the
// second tensor of the result is undefined; every other schedule computes them as always
std::tuple<Tensor, Tensor> spmm_fw(const Tensor &rowptr_, const Tensor &col_, const optional<Tensor> &value_,
                                   const Tensor &mat_, int reduction, const Plan &plan = Plan(), bool want_arg = true) {
   check_index(rowptr_, "rowptr");
   check_index(col_, "col");
   check_feature(mat_, "mat");
   if (value_.has_value() && value_->defined() && is_half(*value_)) {         // the weights are fp32 everywhere
      check_feature(*value_, "value");
      return spmm_fw(rowptr_, col_, optional<Tensor>(value_->to(at::kFloat)), mat_, reduction, plan, want_arg);
   }
   if (is_half(mat_)) {
      if (value_.has_value() && value_->defined()) check_float(*value_, "value");
      return spmm_fw_half(rowptr_, col_, value_, mat_, reduction, plan, want_arg);
   }
   if (is_rows16_plan(plan))      // an fp32 operand on a 16-bit row plan: the plain kernel in the plan's row order
      return spmm_fw(rowptr_, col_, value_, mat_, reduction, plan[0].numel() > 0 ? Plan{plan[0]} : Plan(), want_arg);
   TORCH_CHECK(mat_.dim() == 2, "isplib: `mat` must be 2-D [N, K] (csrc/fusedmm.cpp:121-122)");
   TORCH_CHECK(rowptr_.dim() == 1 && rowptr_.numel() >= 1, "isplib: `rowptr` must be 1-D with M+1 entries");
   c10::DeviceGuard guard(mat_.device());
   const Tensor rowptr = rowptr_.contiguous(), col = col_.contiguous(), mat = mat_.contiguous();   // :140
   Tensor value;
   if (value_.has_value() && value_->defined()) {
      check_float(*value_, "value");
      value = value_->contiguous();
      TORCH_CHECK(value.numel() == col.numel(), "isplib: `value` and `col` differ in length");
   }
   TORCH_CHECK(rowptr.device() == mat.device() && col.device() == mat.device(), "isplib: operands on different devices");
   const int64_t M = rowptr.numel() - 1, N = mat.size(0), K = mat.size(1), nnz = col.numel();
   Tensor out = at::empty({M, K}, mat.options());
   Tensor arg;
   int32_t msg = ISPLIB_MSG_SPMM_SUM;
   if (reduction == R_MAX) msg = ISPLIB_MSG_SPMM_MAX;
   if (reduction == R_MIN) msg = ISPLIB_MSG_SPMM_MIN;
   if (reduction == R_MEAN) msg = ISPLIB_MSG_SPMM_MEAN;
   const int64_t *rp = rowptr.data_ptr<int64_t>();
   const bool tasks_fit = isplib_tasks_serve(N, K, K);
   // (a stream plan for a shape outside the stream entry's domain -- dense operand over 3.5 GiB, k < 4 -- is not an error:
   // the graph is served by the kernels below, which read `col` / `value`)
   const bool minmax_op = reduction == R_MAX || reduction == R_MIN;      // (the max / min stream entry serves dense operands under 2 GiB)
   const bool on_stream = is_stream_plan(plan) && M > 0 && isplib_stream_serves(N, K, K, nnz, minmax_op);
   if (minmax_op && (want_arg || !on_stream)) arg = at::empty({M, K}, rowptr.options());
   if (on_stream) {
      // the plan carries the edges (and the weights) in its own order: `col` / `value` are not read
      const isplib_stream_plan sp = stream_plan_of(plan);
      // a line-friendly pitch for 33..47 columns: only the gathered operand is copied, the output stays packed
      const float *y = mat.data_ptr<float>();
      const int64_t ldy = gather_pitch(N, K, true);
      Tensor pitched;
      if (ldy != K) {
         pitched = at::empty({N, ldy}, mat.options());
         pitched.narrow(1, 0, K).copy_(mat);
         y = pitched.data_ptr<float>();
      }
      if (reduction == R_MAX || reduction == R_MIN) {
         TORCH_CHECK(sp.perm != nullptr, "isplib: max / min on a stream plan need its permutation (a 9-element plan)");
         const size_t ws = isplib_spmm_stream_minmax_workspace_bytes(&sp);
         Tensor work = at::empty({(int64_t)ws}, mat.options().dtype(at::kByte));
         const int st = fusedMM_csr_stream_minmax_hip(msg, M, N, K, nnz, rp, rp + 1, &sp, y, ldy, out.data_ptr<float>(), K,
                                                      arg.defined() ? arg.data_ptr<int64_t>() : nullptr, work.data_ptr(), ws, current_stream(mat));
         check_status(st, "fusedMM_csr_stream_minmax_hip");
         return std::make_tuple(out, arg);
      }
      const size_t ws = isplib_spmm_stream_workspace_bytes(&sp);
      Tensor work = at::empty({(int64_t)ws}, mat.options().dtype(at::kByte));
      const int st = fusedMM_csr_stream_hip(msg, M, N, K, nnz, rp, rp + 1, &sp, y, ldy, out.data_ptr<float>(), K,
                                            work.data_ptr(), ws, nullptr, current_stream(mat));
      check_status(st, "fusedMM_csr_stream_hip");
      return std::make_tuple(out, arg);
   }
   if (is_task_plan(plan) && tasks_fit && M > 0 && K > 0) {
      const Tensor &task_row = plan[0], &task_b = plan[1], &task_len = plan[2], &seg_off = plan[3], &lane = plan[4];
      TORCH_CHECK(task_row.is_cuda() && task_row.scalar_type() == at::kInt && task_len.scalar_type() == at::kInt &&
                      seg_off.scalar_type() == at::kInt && task_b.scalar_type() == at::kLong,
                  "isplib: malformed task plan");
      TORCH_CHECK(!lane.is_cuda() && lane.scalar_type() == at::kLong && lane.numel() == 9, "isplib: lane_off must be 9 host int64");
      TORCH_CHECK((seg_off.numel() - 1) % M == 0, "isplib: task plan does not match rowptr");
      const int nsl = (int)((seg_off.numel() - 1) / M);
      const int64_t n_tasks = task_row.numel();
      const size_t ws = isplib_spmm_tasks_workspace_bytes(msg, n_tasks, K);
      Tensor work = at::empty({(int64_t)ws}, mat.options().dtype(at::kByte));
      const int st = fusedMM_csr_tasks_hip(msg, M, N, K, nnz, value.defined() ? value.data_ptr<float>() : nullptr,
                                           col.data_ptr<int64_t>(), plan_col32(plan, col), rp, rp + 1, n_tasks, task_row.data_ptr<int32_t>(),
                                           task_b.data_ptr<int64_t>(), task_len.data_ptr<int32_t>(),
                                           seg_off.data_ptr<int32_t>(), nsl, lane.data_ptr<int64_t>(),
                                           mat.data_ptr<float>(), K, out.data_ptr<float>(), K,
                                           arg.defined() ? arg.data_ptr<int64_t>() : nullptr, work.data_ptr(), ws,
                                           current_stream(mat));
      check_status(st, "fusedMM_csr_tasks_hip");
      return std::make_tuple(out, arg);
   }
   if (plan.size() == 1 && plan[0].defined() && plan[0].scalar_type() == at::kInt && M > 0 && K > 0) {
      // a row order (int32 [M], position -> row): the plain kernel with the rows taken in that order (operands larger
      // than the Infinity Cache on graphs with community structure; fusedMM_csr_ordered_hip) -- the same bits as below
      const Tensor order = row_order_of(plan[0], M);
      const int st = fusedMM_csr_ordered_hip(msg, M, N, K, nnz, value.defined() ? value.data_ptr<float>() : nullptr,
                                             col.data_ptr<int64_t>(), rp, rp + 1, order.data_ptr<int32_t>(), mat.data_ptr<float>(), K,
                                             out.data_ptr<float>(), K, arg.defined() ? arg.data_ptr<int64_t>() : nullptr,
                                             current_stream(mat));
      check_status(st, "fusedMM_csr_ordered_hip");
      return std::make_tuple(out, arg);
   }
   if (plan.size() == 1 && plan[0].defined() && M > 0 && K > 0) {
      check_index(plan[0], "slices");
      const Tensor table = plan[0].contiguous();
      TORCH_CHECK(table.numel() % M == 0 && table.numel() / M >= 9, "isplib: slice table does not match rowptr");
      const int nsl = (int)(table.numel() / M - 1);
      const size_t ws = isplib_spmm_sliced_workspace_bytes(msg, M, K, nsl);
      Tensor work = at::empty({(int64_t)ws}, mat.options().dtype(at::kByte));
      const int st = fusedMM_csr_sliced_hip(msg, M, N, K, nnz, value.defined() ? value.data_ptr<float>() : nullptr,
                                            col.data_ptr<int64_t>(), rp, rp + 1, table.data_ptr<int64_t>(), nsl,
                                            mat.data_ptr<float>(), K, out.data_ptr<float>(), K,
                                            arg.defined() ? arg.data_ptr<int64_t>() : nullptr, work.data_ptr(), ws,
                                            current_stream(mat));
      check_status(st, "fusedMM_csr_sliced_hip");
      return std::make_tuple(out, arg);
   }
   // no plan given (the reference's own call pattern): large graphs go through a cached per-graph handle
   if (is_auto_plan(plan) && M > 0 && K > 0 && rowptr.is_same(rowptr_) && col.is_same(col_) &&
       (!value.defined() || value.is_same(*value_)) && spmm_through_handle(msg, rowptr, col, value, mat, out, arg))
      return std::make_tuple(out, arg);
   const int st = fusedMM_csr_hip(msg, M, N, K, 1.0f, nnz, M, N, value.defined() ? value.data_ptr<float>() : nullptr,
                                  col.data_ptr<int64_t>(), rp, rp + 1, nullptr, K, mat.data_ptr<float>(), K, 0.0f,
                                  out.data_ptr<float>(), K, arg.defined() ? arg.data_ptr<int64_t>() : nullptr,
                                  current_stream(mat));
   check_status(st, "fusedMM_csr_hip");
   return std::make_tuple(out, arg);
}

struct Transposed {
   Tensor colptr, row_t, val_t;
};

// A^T operands built on the device (isplib/__init__.py:79-80 / :86-99 equivalents)
Transposed build_transpose(const Tensor &rowptr, const Tensor &col, const Tensor &value_, int64_t ncols, bool mean) {
   c10::DeviceGuard guard(col.device());
   const Tensor value = as_float(value_);
   const int64_t M = rowptr.numel() - 1, nnz = col.numel();
   Transposed t;
   t.colptr = at::empty({ncols + 1}, rowptr.options());
   t.row_t = at::empty({nnz}, rowptr.options());
   t.val_t = at::empty({nnz}, col.options().dtype(at::kFloat));
   const size_t ws = isplib_csr2csc_workspace_bytes(M, ncols, nnz);
   TORCH_CHECK(ws > 0, "isplib_csr2csc_workspace_bytes failed: ", isplib_hip_last_error());
   Tensor work = at::empty({(int64_t)ws}, col.options().dtype(at::kByte));
   const int st = isplib_csr2csc_hip(M, ncols, nnz, rowptr.data_ptr<int64_t>(), col.data_ptr<int64_t>(),
                                     value.defined() ? value.data_ptr<float>() : nullptr, mean ? 1 : 0,
                                     t.colptr.data_ptr<int64_t>(), nullptr, t.row_t.data_ptr<int64_t>(),
                                     t.val_t.data_ptr<float>(), work.data_ptr(), ws, current_stream(col));
   check_status(st, "isplib_csr2csc_hip");
   return t;
}

Tensor sddmm(const Tensor &rowptr, const Tensor &col, const Tensor &mat, const Tensor &grad_out, bool mean,
             const std::vector<Tensor> &plan = {}, const Tensor &value = Tensor()) {
   c10::DeviceGuard guard(mat.device());
   const Tensor g = as_float(grad_out).contiguous(), y = as_float(mat).contiguous();      // 16-bit operands: dA is formed in fp32
   const int64_t M = rowptr.numel() - 1, N = y.size(0), K = y.size(1);
   Tensor dval = at::empty({col.numel()}, y.options());
   const int64_t *rp = rowptr.data_ptr<int64_t>();
   // The dot product needs whole rows of y, so the SpMM's plan (sized for 64-column panels) is the wrong one here:
   // large graphs go through the graph's handle, which keeps a plan sized for whole rows (Reddit K=128: 3.7 ms with
   // 16 slices, 4.6 ms on the SpMM's 8).  dA does not read the weights (and the weights tensor autograd hands back
   // here is a different object from the forward's): the structure's handle is used as it is.
   (void)value;
   if (K >= 4 && rowptr.is_contiguous() && col.is_contiguous() && isplib_suggest_slices_whole_rows(M, N, col.numel(), K) > 0) {
      std::lock_guard<std::mutex> lock(g_graph_mutex);
      isplib_graph *handle = graph_handle_locked(rowptr, col, Tensor(), N, /*with_values=*/false);
      const int st = isplib_graph_sddmm(handle, mean ? 1 : 0, K, y.data_ptr<float>(), K, g.data_ptr<float>(), K,
                                        dval.data_ptr<float>(), current_stream(y));
      if (st != ISPLIB_NOT_ENOUGH_MEM) {
         check_status(st, "isplib_graph_sddmm");
         return dval;
      }
   }
   if (is_task_plan(plan) && isplib_sddmm_tasks_serve(N, K, K)) {
      const int st = isplib_sddmm_csr_tasks_hip(M, N, K, col.data_ptr<int64_t>(), plan_col32(plan, col), rp, rp + 1, plan[0].numel(),
                                                plan[0].data_ptr<int32_t>(), plan[1].data_ptr<int64_t>(),
                                                plan[2].data_ptr<int32_t>(), plan[4].data_ptr<int64_t>(),
                                                y.data_ptr<float>(), K, g.data_ptr<float>(), K, mean ? 1 : 0,
                                                dval.data_ptr<float>(), current_stream(y));
      check_status(st, "isplib_sddmm_csr_tasks_hip");
      return dval;
   }
   const int st = isplib_sddmm_csr_hip(M, K, col.data_ptr<int64_t>(), rp, rp + 1, y.data_ptr<float>(), K,
                                       g.data_ptr<float>(), K, mean ? 1 : 0, dval.data_ptr<float>(), current_stream(y));
   check_status(st, "isplib_sddmm_csr_hip");
   return dval;
}

// The value gradient of a 16-bit sum / mean on the 16-bit SDDMM row kernel (isplib_sddmm_csr_rows16_hip): neither X nor dY is widened
// in memory, dval is fp32.  The operands are prepared as rows16_call prepares them -- `mat` as it lies if its pitch is served, else
// packed; dY contiguous; either copied in 16 bits if its base is 2 bytes off a 4-byte boundary.  Undefined when the call is not
// served (nothing was launched, nothing raises): the caller then takes the route it always took.
static Tensor sddmm_rows16(const Tensor &rowptr, const Tensor &col, const Tensor &mat, const Tensor &grad_out, bool mean, const Plan &row_plan) {
   if (!is_half(mat) || !is_half(grad_out) || mat.scalar_type() != grad_out.scalar_type() || mat.dim() != 2 || grad_out.dim() != 2 ||
       rowptr.dim() != 1 || rowptr.numel() < 1 || !is_rows16_plan(row_plan))
      return Tensor();
   const int64_t M = rowptr.numel() - 1, N = mat.size(0), K = mat.size(1), nnz = col.numel();
   if (M <= 0 || K <= 0 || K > ISPLIB_SDDMM_TASKS_K_MAX || grad_out.size(0) != M || grad_out.size(1) != K || !mat.is_cuda() ||
       rowptr.device() != mat.device() || col.device() != mat.device() || grad_out.device() != mat.device() ||
       rowptr.scalar_type() != at::kLong || col.scalar_type() != at::kLong)
      return Tensor();
   c10::DeviceGuard guard(mat.device());
   const Rows16Call c = rows16_call(rowptr, col, Tensor(), false, mat, row_plan);      // (served: isplib_rows16_serves at K <= 1024 is isplib_sddmm_rows16_serves)
   if (!c.served) return Tensor();
   const Tensor g = packed16(grad_out);
   Tensor dval = at::empty({nnz}, mat.options().dtype(at::kFloat));
   const int st = isplib_sddmm_csr_rows16_hip(c.dtype, M, N, K, nnz, c.idx, c.ptr, c.ptr + 1, c.order, c.mat.data_ptr(), c.ldy, g.data_ptr(), K,
                                              mean ? 1 : 0, dval.data_ptr<float>(), current_stream(c.mat));
   check_status(st, "isplib_sddmm_csr_rows16_hip");
   return dval;
}

// dA of SpmmSum / SpmmMean: the 16-bit kernel when the saved forward plan carries the marker and the call is served, else sddmm()
static Tensor value_grad(const Tensor &rowptr, const Tensor &col, const Tensor &mat, const Tensor &grad_out, bool mean, const Plan &plan,
                         const Tensor &value) {
   if (is_rows16_da_plan(plan)) {
      const Tensor dval = sddmm_rows16(rowptr, col, mat, grad_out, mean, Plan{plan[0], plan[1]});
      if (dval.defined()) return dval;
   }
   return sddmm(rowptr, col, mat, grad_out, mean, forward_plan(plan), value);
}

// sum-SpMM with unit weights and the fused epilogue out = act(row_scale * (A y + self) + bias); the fold kernel
// applies it when a task plan is given (isplib_epilogue), otherwise it is composed from ATen ops.
Tensor epilogue_spmm(const Tensor &rowptr, const Tensor &col, const Plan &plan, const Tensor &y_, const Tensor &self_,
                     const Tensor &row_scale, const Tensor &bias, bool relu) {
   const int64_t M = rowptr.numel() - 1, N = y_.size(0), K = y_.size(1), nnz = col.numel();
   const bool tasks_fit = is_task_plan(plan) && M > 0 && isplib_tasks_serve(N, K, K);
   if (is_stream_plan(plan) && M > 0 && K >= 4) {
      // the stream kernel applies the same epilogue when it writes a finished row (hub rows: in their fold)
      c10::DeviceGuard guard(y_.device());
      const Tensor y = row_strided(y_) ? y_ : y_.contiguous();          // the gather's own pitch is kept (GcnNormSpmm)
      const int64_t ldy = N > 1 ? y.stride(0) : K;
      TORCH_CHECK(isplib_dense_in_descriptor(N, ldy), "isplib: dense operand beyond one buffer descriptor");
      const Tensor self = self_.defined() ? (row_strided(self_) ? self_ : self_.contiguous()) : Tensor();
      const Tensor rs = row_scale.defined() ? row_scale.contiguous() : Tensor();
      const Tensor bs = bias.defined() ? bias.contiguous() : Tensor();
      if (self.defined()) TORCH_CHECK(self.size(0) == M && self.size(1) == K, "isplib: `self` must be [M, K]");
      if (rs.defined()) TORCH_CHECK(rs.numel() == M, "isplib: `row_scale` must have M entries");
      if (bs.defined()) TORCH_CHECK(bs.numel() == K, "isplib: `bias` must have K entries");
      const isplib_stream_plan sp = stream_plan_of(plan);
      TORCH_CHECK(sp.vals == nullptr, "isplib: the fused epilogue is defined for unit weights");
      const Tensor rp_c = rowptr.contiguous();
      Tensor out = at::empty({M, K}, y.options());
      const size_t ws = isplib_spmm_stream_workspace_bytes(&sp);
      Tensor work = at::empty({(int64_t)ws}, y.options().dtype(at::kByte));
      isplib_epilogue ep;
      ep.row_scale = rs.defined() ? rs.data_ptr<float>() : nullptr;
      ep.self = self.defined() ? self.data_ptr<float>() : nullptr;
      ep.ld_self = self.defined() && M > 1 ? self.stride(0) : K;
      ep.bias = bs.defined() ? bs.data_ptr<float>() : nullptr;
      ep.relu = relu ? 1 : 0;
      const int64_t *rp = rp_c.data_ptr<int64_t>();
      const int st = fusedMM_csr_stream_hip(ISPLIB_MSG_SPMM_SUM, M, N, K, nnz, rp, rp + 1, &sp, y.data_ptr<float>(), ldy, out.data_ptr<float>(), K,
                                            work.data_ptr(), ws, &ep, current_stream(y));
      check_status(st, "fusedMM_csr_stream_hip");
      return out;
   }
   const Tensor y = y_.contiguous();
   if (!tasks_fit) {
      Tensor out = std::get<0>(spmm_fw(rowptr, col, c10::nullopt, y, R_SUM, plan));
      if (self_.defined()) out = out + self_;
      if (row_scale.defined()) out = out * row_scale.unsqueeze(1);
      if (bias.defined()) out = out + bias;
      return relu ? at::relu(out) : out;
   }
   c10::DeviceGuard guard(y.device());
   const Tensor self = self_.defined() ? self_.contiguous() : Tensor();
   const Tensor rs = row_scale.defined() ? row_scale.contiguous() : Tensor();
   const Tensor bs = bias.defined() ? bias.contiguous() : Tensor();
   if (self.defined()) TORCH_CHECK(self.size(0) == M && self.size(1) == K, "isplib: `self` must be [M, K]");
   if (rs.defined()) TORCH_CHECK(rs.numel() == M, "isplib: `row_scale` must have M entries");
   if (bs.defined()) TORCH_CHECK(bs.numel() == K, "isplib: `bias` must have K entries");
   const Tensor rp_c = rowptr.contiguous(), col_c = col.contiguous();
   Tensor out = at::empty({M, K}, y.options());
   const int nsl = (int)((plan[3].numel() - 1) / M);
   const int64_t n_tasks = plan[0].numel();
   const size_t ws = isplib_spmm_tasks_workspace_bytes(ISPLIB_MSG_SPMM_SUM, n_tasks, K);
   Tensor work = at::empty({(int64_t)ws}, y.options().dtype(at::kByte));
   isplib_epilogue ep;
   ep.row_scale = rs.defined() ? rs.data_ptr<float>() : nullptr;
   ep.self = self.defined() ? self.data_ptr<float>() : nullptr;
   ep.ld_self = K;
   ep.bias = bs.defined() ? bs.data_ptr<float>() : nullptr;
   ep.relu = relu ? 1 : 0;
   const int64_t *rp = rp_c.data_ptr<int64_t>();
   const int st = fusedMM_csr_tasks_epilogue_hip(
       ISPLIB_MSG_SPMM_SUM, M, N, K, nnz, nullptr, col_c.data_ptr<int64_t>(), plan_col32(plan, col_c), rp, rp + 1, n_tasks,
       plan[0].data_ptr<int32_t>(), plan[1].data_ptr<int64_t>(), plan[2].data_ptr<int32_t>(), plan[3].data_ptr<int32_t>(), nsl,
       plan[4].data_ptr<int64_t>(), y.data_ptr<float>(), K, out.data_ptr<float>(), K, work.data_ptr(), ws, &ep,
       current_stream(y));
   check_status(st, "fusedMM_csr_tasks_epilogue_hip");
   return out;
}

Tensor or_undef(const optional<Tensor> &t) { return t.has_value() ? *t : Tensor(); }

// AutogradContext::needs_input_grad() is indexed by autograd EDGE, i.e. by position among
// the tensor arguments that are actually present -- absent optionals take no edge.
int64_t edge_of(std::initializer_list<bool> present_before) {
   int64_t e = 0;
   for (bool p : present_before) e += p ? 1 : 0;
   return e;
}
bool present(const optional<Tensor> &t) { return t.has_value() && t->defined(); }

// ---- sum: csrc/fusedmm.cpp:210-294 ---------------------------------------------------------
class SpmmSum : public torch::autograd::Function<SpmmSum> {
 public:
   static variable_list forward(AutogradContext *ctx, optional<Variable> opt_row, Variable rowptr, Variable col,
                                optional<Variable> opt_value, optional<Variable> opt_colptr,
                                optional<Variable> opt_csr2csc, Variable mat, optional<Variable> value_index_select,
                                optional<Variable> row_index_select, Plan plan, Plan plan_t) {
      const bool has_value = opt_value.has_value() && opt_value->defined();
      OpTimer timer("FUSEDMM_SPMM_SUM_FW", mat);
      auto out = std::get<0>(spmm_fw(rowptr, col, opt_value, mat, R_SUM, forward_plan(plan)));   // :244
      ctx->saved_data["plan_t"] = plan_t;
      ctx->saved_data["plan"] = plan;
      ctx->saved_data["has_value"] = has_value;
      ctx->saved_data["value_edge"] = edge_of({present(opt_row), true, true});
      ctx->saved_data["mat_edge"] =
          edge_of({present(opt_row), true, true, has_value, present(opt_colptr), present(opt_csr2csc)});
      ctx->save_for_backward({or_undef(opt_row), rowptr, col, or_undef(opt_value), or_undef(opt_colptr),
                              or_undef(opt_csr2csc), mat, or_undef(value_index_select), or_undef(row_index_select)});
      return {out};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_SPMM_SUM_BW", grad_outs[0]);
      const bool has_value = ctx->saved_data["has_value"].toBool();
      auto saved = ctx->get_saved_variables();
      auto rowptr = saved[1], col = saved[2], value = saved[3], colptr = saved[4], mat = saved[6],
           value_sel = saved[7], row_sel = saved[8];
      auto grad_out = grad_outs[0].to(mat.scalar_type());       // a gradient of another float type is brought to mat's

      auto grad_value = Variable();
      if (has_value && ctx->needs_input_grad(ctx->saved_data["value_edge"].toInt()))   // :269-272 (SDDMM, commented out there)
         grad_value = value_grad(rowptr, col, mat, grad_out, false, ctx->saved_data["plan"].toTensorVector(), value);

      auto grad_mat = Variable();
      if (ctx->needs_input_grad(ctx->saved_data["mat_edge"].toInt())) {
         // :285  grad_mat = fusedmm_spmm_fw(colptr, row_index_select, value_index_select, grad_out)
         if (colptr.defined() && row_sel.defined() && (value_sel.defined() || !has_value)) {
            optional<Tensor> v = has_value ? optional<Tensor>(value_sel) : c10::nullopt;
            grad_mat = std::get<0>(spmm_fw(colptr, row_sel, v, grad_out, R_SUM, ctx->saved_data["plan_t"].toTensorVector()));
         } else {
            auto t = build_transpose(rowptr, col, has_value ? value : Tensor(), mat.size(0), false);
            optional<Tensor> v = has_value ? optional<Tensor>(t.val_t) : c10::nullopt;
            grad_mat = std::get<0>(spmm_fw(t.colptr, t.row_t, v, grad_out, R_SUM));
         }
      }
      return {Variable(), Variable(), Variable(), grad_value, Variable(), Variable(),
              grad_mat,   Variable(), Variable(), Variable(),  Variable()};
   }
};

// ---- mean: csrc/fusedmm.cpp:296-384 --------------------------------------------------------
class SpmmMean : public torch::autograd::Function<SpmmMean> {
 public:
   static variable_list forward(AutogradContext *ctx, optional<Variable> opt_row, Variable rowptr, Variable col,
                                optional<Variable> opt_value, optional<Variable> opt_rowcount,
                                optional<Variable> opt_colptr, optional<Variable> opt_csr2csc, Variable mat,
                                optional<Variable> new_row, optional<Variable> new_rowcount, Plan plan, Plan plan_t) {
      const bool has_value = opt_value.has_value() && opt_value->defined();
      OpTimer timer("FUSEDMM_SPMM_MEAN_FW", mat);
      auto out = std::get<0>(spmm_fw(rowptr, col, opt_value, mat, R_MEAN, forward_plan(plan)));   // :331
      ctx->saved_data["plan_t"] = plan_t;
      ctx->saved_data["plan"] = plan;
      ctx->saved_data["has_value"] = has_value;
      ctx->saved_data["value_edge"] = edge_of({present(opt_row), true, true});
      ctx->saved_data["mat_edge"] = edge_of({present(opt_row), true, true, has_value, present(opt_rowcount),
                                             present(opt_colptr), present(opt_csr2csc)});
      ctx->save_for_backward({or_undef(opt_row), rowptr, col, or_undef(opt_value), or_undef(opt_rowcount),
                              or_undef(opt_colptr), or_undef(opt_csr2csc), mat, or_undef(new_row),
                              or_undef(new_rowcount)});
      return {out};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_SPMM_MEAN_BW", grad_outs[0]);
      const bool has_value = ctx->saved_data["has_value"].toBool();
      auto saved = ctx->get_saved_variables();
      auto rowptr = saved[1], col = saved[2], value = saved[3], colptr = saved[5], mat = saved[7], new_row = saved[8],
           new_rowcount = saved[9];
      auto grad_out = grad_outs[0].to(mat.scalar_type());

      auto grad_value = Variable();
      if (has_value && ctx->needs_input_grad(ctx->saved_data["value_edge"].toInt()))
         grad_value = value_grad(rowptr, col, mat, grad_out, true, ctx->saved_data["plan"].toTensorVector(), value);   // :350-353

      auto grad_mat = Variable();
      if (ctx->needs_input_grad(ctx->saved_data["mat_edge"].toInt())) {
         // :375  grad_mat = fusedmm_spmm_fw(colptr, new_row, new_rowcount, grad_out)   (a SUM on A^T)
         const bool cached = colptr.defined() && new_row.defined() && new_rowcount.defined() &&
                             new_row.numel() == col.numel() && new_rowcount.numel() == col.numel() &&
                             new_rowcount.scalar_type() == at::kFloat && new_row.is_cuda();
         // an unweighted graph needs no edge weights here either: (A^T diag(1/deg)) dY = A^T (diag(1/deg) dY) -- the rows
         // of dY are scaled once (M x K elementwise) and the SUM on A^T runs with unit weights, i.e. without a weight stream
         const bool unit_planned = !has_value && colptr.defined() && new_row.defined() && !new_rowcount.defined() &&
                                   new_row.numel() == col.numel() && new_row.is_cuda();
         // a plan_t of the three-element form (is_rows16_colscale_plan) is read by the unit_planned branch alone
         Plan plan_t = ctx->saved_data["plan_t"].toTensorVector();
         Tensor col_scale;
         if (is_rows16_colscale_plan(plan_t)) {
            col_scale = plan_t[2];
            plan_t.pop_back();
         }
         if (cached) {
            grad_mat = std::get<0>(spmm_fw(colptr, new_row, optional<Tensor>(new_rowcount), grad_out, R_SUM, plan_t));
         } else if (unit_planned) {
            // a 16-bit dY whose plan_t carries the table 1 / max(deg, 1): the column-scaled 16-bit row kernel applies it to the
            // gathered rows of dY in fp32, inside the sum -- no fp32 copy of dY, one rounding
            if (col_scale.defined())
               grad_mat = mean_bw_colscale(colptr, new_row, grad_out, plan_t, col_scale, rowptr.numel() - 1);
            if (!grad_mat.defined()) {
               // (a 16-bit dY otherwise: gy is formed and kept in fp32 -- rounding it here and the sum again would round twice --
               // so the SpMM on A^T takes the conversion route)
               const Tensor deg = (rowptr.slice(0, 1) - rowptr.slice(0, 0, -1)).clamp_min(1).to(at::kFloat);
               const Tensor gy = as_float(grad_out) / deg.unsqueeze(1);
               grad_mat = std::get<0>(spmm_fw(colptr, new_row, c10::nullopt, gy, R_SUM, plan_t)).to(mat.scalar_type());
            }
         } else {
            auto t = build_transpose(rowptr, col, has_value ? value : Tensor(), mat.size(0), true);
            grad_mat = std::get<0>(spmm_fw(t.colptr, t.row_t, optional<Tensor>(t.val_t), grad_out, R_SUM));
         }
      }
      return {Variable(), Variable(), Variable(), grad_value, Variable(), Variable(),
              Variable(), grad_mat,   Variable(), Variable(), Variable(),  Variable()};
   }
};

// ---- max / min: csrc/fusedmm.cpp:386-452, 454-518 ------------------------------------------
template <int RED>
class SpmmMinMax : public torch::autograd::Function<SpmmMinMax<RED>> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, optional<Variable> opt_value,
                                Variable mat, Plan plan) {
      const bool has_value = opt_value.has_value() && opt_value->defined();
      OpTimer timer(RED == R_MAX ? "FUSEDMM_SPMM_MAX_FW" : "FUSEDMM_SPMM_MIN_FW", mat);
      auto result = spmm_fw(rowptr, col, opt_value, mat, RED, plan);   // :397 / :465
      auto out = std::get<0>(result);
      auto arg_out = std::get<1>(result);
      ctx->saved_data["has_value"] = has_value;
      ctx->save_for_backward({col, or_undef(opt_value), mat, arg_out});
      ctx->mark_non_differentiable({arg_out});                    // :403 / :470
      return {out, arg_out};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer(RED == R_MAX ? "FUSEDMM_SPMM_MAX_BW" : "FUSEDMM_SPMM_MIN_BW", grad_outs[0]);
      const bool has_value = ctx->saved_data["has_value"].toBool();
      auto saved = ctx->get_saved_variables();
      auto col = saved[0], value = saved[1], mat = saved[2], arg_out = saved[3];
      const Tensor grad_out = as_float(grad_outs[0]).contiguous();      // 16-bit operands: the gradients are formed in fp32
      if (has_value) value = as_float(value);
      // edges: rowptr 0, col 1, value 2 (if present), mat last
      const bool need_val = has_value && ctx->needs_input_grad(2);
      const bool need_mat = ctx->needs_input_grad(has_value ? 3 : 2);
      auto grad_value = Variable(), grad_mat = Variable();
      if (need_val || need_mat) {
         c10::DeviceGuard guard(mat.device());
         const Tensor y = as_float(mat).contiguous();
         const int64_t M = arg_out.size(0), N = y.size(0), K = y.size(1), nnz = col.numel();
         if (need_val) grad_value = at::empty({nnz}, y.options());
         if (need_mat) grad_mat = at::empty({N, K}, y.options());
         // one fused pass for :417-446 (mask, gather, mul, masked_fill, scatter_add x2)
         // the atomic-free form (bitwise reproducible gradients) wherever its 32-bit keys reach; else the one-pass scatter
         const size_t ws = isplib_spmm_minmax_bw_workspace_bytes(M, N, K);
         if (ws > 0) {
            Tensor work = at::empty({(int64_t)ws}, y.options().dtype(at::kByte));
            const int st = isplib_spmm_minmax_bw_det_hip(
                M, N, K, nnz, col.data_ptr<int64_t>(), has_value ? value.data_ptr<float>() : nullptr, y.data_ptr<float>(),
                arg_out.data_ptr<int64_t>(), grad_out.data_ptr<float>(), need_mat ? grad_mat.data_ptr<float>() : nullptr,
                need_val ? grad_value.data_ptr<float>() : nullptr, work.data_ptr(), ws, current_stream(y));
            check_status(st, "isplib_spmm_minmax_bw_det_hip");
         } else {
            const int st = isplib_spmm_minmax_bw_hip(
                M, N, K, nnz, col.data_ptr<int64_t>(), has_value ? value.data_ptr<float>() : nullptr, y.data_ptr<float>(),
                arg_out.data_ptr<int64_t>(), grad_out.data_ptr<float>(), need_mat ? grad_mat.data_ptr<float>() : nullptr,
                need_val ? grad_value.data_ptr<float>() : nullptr, current_stream(y));
            check_status(st, "isplib_spmm_minmax_bw_hip");
         }
      }
      if (grad_mat.defined() && is_half(mat)) grad_mat = grad_mat.to(mat.scalar_type());      // rounded once
      return {Variable(), Variable(), grad_value, grad_mat, Variable()};
   }
};

// y = D^-1/2 X in one pass (isplib_row_scale_hip), written at the gather's pitch: a [N, K] view
static Tensor gcn_row_scale(const Tensor &mat_, const Tensor &dinv_, bool stream) {
   c10::DeviceGuard guard(mat_.device());
   const Tensor mat = row_strided(mat_) ? mat_ : mat_.contiguous();
   const Tensor dinv = dinv_.contiguous();
   const int64_t N = mat.size(0), K = mat.size(1);
   TORCH_CHECK(dinv.numel() == N, "isplib: `dinv` must have one entry per row of `mat`");
   const int64_t ld = gather_pitch(N, K, stream);
   Tensor buf = at::empty({N, ld}, mat.options());
   const int st = isplib_row_scale_hip(N, K, mat.data_ptr<float>(), N > 1 ? mat.stride(0) : K, dinv.data_ptr<float>(), buf.data_ptr<float>(),
                                       ld, current_stream(mat));
   check_status(st, "isplib_row_scale_hip");
   return buf.narrow(1, 0, K);
}

// ---- GCN's normalised aggregation, fused: relu(D^-1/2 (A + I) D^-1/2 X + b) with unit-weight A ----------
// (the `normalize=True` callers, tests/dist/gcn/pyg-sparse.py:61-62; not an operator of the reference)
class GcnNormSpmm : public torch::autograd::Function<GcnNormSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable mat, Variable dinv,
                                optional<Variable> opt_colptr, optional<Variable> opt_row_t, Plan plan, Plan plan_t,
                                optional<Variable> opt_bias, bool relu) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_float(mat, "mat"); check_float(dinv, "dinv");
      TORCH_CHECK(mat.dim() == 2 && rowptr.numel() - 1 == mat.size(0), "isplib: gcn_norm_spmm needs a square graph and [N, K] features");
      const Tensor bias = or_undef(opt_bias);
      const Tensor y = gcn_row_scale(mat, dinv, is_stream_plan(plan));      // D^-1/2 X, one pass, at the gather's pitch
      Tensor out = epilogue_spmm(rowptr, col, plan, y, y, dinv, bias, relu);
      ctx->saved_data["relu"] = relu;
      ctx->saved_data["plan_t"] = plan_t;
      ctx->saved_data["bias_edge"] = (int64_t)(4 + (present(opt_colptr) ? 1 : 0) + (present(opt_row_t) ? 1 : 0));
      ctx->saved_data["has_bias"] = bias.defined();
      ctx->save_for_backward({rowptr, col, dinv, or_undef(opt_colptr), or_undef(opt_row_t), relu ? out : Tensor()});
      return {out};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      auto saved = ctx->get_saved_variables();
      auto rowptr = saved[0], col = saved[1], dinv = saved[2], colptr = saved[3], row_t = saved[4], out = saved[5];
      const Tensor dz = grad_outs[0].contiguous();
      check_float(dz, "grad_out");
      auto grad_bias = Variable(), grad_mat = Variable();
      const bool need_bias = ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(ctx->saved_data["bias_edge"].toInt());
      const bool need_mat = ctx->needs_input_grad(2);
      if (need_bias || need_mat) {
         // ONE pass over dZ (and the saved output, for the ReLU mask): gY = (dZ . [out > 0]) D^-1/2 written at the pitch the
         // backward's gather wants, and the bias gradient as a tall-skinny column sum (per-block partials + one fold,
         // deterministic) -- the four ATen passes this replaces included a 1.2 ms reduce_kernel on a 38 MB matrix
         c10::DeviceGuard guard(dz.device());
         Plan plan_t = ctx->saved_data["plan_t"].toTensorVector();
         if (need_mat && (!colptr.defined() || !row_t.defined())) {
            auto t = build_transpose(rowptr, col, Tensor(), rowptr.numel() - 1, false);
            colptr = t.colptr; row_t = t.row_t; plan_t.clear();
         }
         const int64_t N = dz.size(0), K = dz.size(1);
         const int64_t ld = need_mat ? gather_pitch(N, K, is_stream_plan(plan_t)) : K;
         Tensor gy_buf = need_mat ? at::empty({N, ld}, dz.options()) : Tensor();
         if (need_bias) grad_bias = at::empty({K}, dz.options());
         const Tensor mask = ctx->saved_data["relu"].toBool() ? out.contiguous() : Tensor();
         const Tensor scale = dinv.contiguous();
         const size_t ws = isplib_masked_scale_colsum_workspace_bytes(N, K);
         Tensor work = at::empty({(int64_t)ws}, dz.options().dtype(at::kByte));
         const int st = isplib_masked_scale_colsum_hip(N, K, dz.data_ptr<float>(), K, mask.defined() ? mask.data_ptr<float>() : nullptr, K,
                                                       scale.data_ptr<float>(), need_mat ? gy_buf.data_ptr<float>() : nullptr, ld,
                                                       need_bias ? grad_bias.data_ptr<float>() : nullptr, work.data_ptr(), ws,
                                                       current_stream(dz));
         check_status(st, "isplib_masked_scale_colsum_hip");
         if (need_mat) {
            const Tensor gy = gy_buf.narrow(1, 0, K);
            grad_mat = epilogue_spmm(colptr, row_t, plan_t, gy, gy, dinv, Tensor(), false);   // D (A^T + I) D dZ
         }
      }
      return {Variable(), Variable(), grad_mat, Variable(), Variable(), Variable(), Variable(), Variable(), grad_bias, Variable()};
   }
};

// ---- the same layer for a 16-bit `mat` on the 16-bit row kernel (fusedMM_csr_rows16_epilogue_hip) ----------
// One call of the entry with col_scale = self_scale = row_scale = dinv on (ptr, idx): act(D^-1/2 (A + I) D^-1/2 mat + bias), mat as it
// lies (rows16_call's preparation), the finished fp32 row rounded once.  Undefined when the family does not take the operand.
static Tensor gcn_rows16(const Tensor &ptr, const Tensor &idx, const Tensor &mat, const Plan &row_plan, const Tensor &dinv, const Tensor &bias32,
                         bool relu) {
   const int64_t M = ptr.numel() - 1, N = mat.size(0), K = mat.size(1), nnz = idx.numel();
   TORCH_CHECK(M == N && dinv.numel() == N, "isplib: gcn_norm_spmm needs a square graph, [N, K] features and one `dinv` entry per row");
   TORCH_CHECK(ptr.device() == mat.device() && idx.device() == mat.device() && dinv.device() == mat.device(),
               "isplib: gcn_norm_spmm needs its operands on one device");
   c10::DeviceGuard guard(mat.device());
   const Rows16Call c = rows16_call(ptr, idx, dinv, false, mat, row_plan);
   if (!c.served) return Tensor();
   const Tensor bs = bias32.defined() ? bias32.contiguous() : Tensor();
   if (bs.defined()) TORCH_CHECK(bs.numel() == K && bs.scalar_type() == at::kFloat && bs.device() == mat.device(), "isplib: `bias` must have K entries");
   Tensor out = at::empty({M, K}, c.mat.options());
   isplib_epilogue16 ep;
   ep.row_scale = c.weight;
   ep.self_scale = c.weight;
   ep.bias = bs.defined() ? bs.data_ptr<float>() : nullptr;
   ep.relu = relu ? 1 : 0;
   const int st = fusedMM_csr_rows16_epilogue_hip(c.dtype, M, N, K, nnz, c.weight, c.idx, c.ptr, c.ptr + 1, c.order, c.mat.data_ptr(), c.ldy,
                                                  out.data_ptr(), K, &ep, current_stream(c.mat));
   check_status(st, "fusedMM_csr_rows16_epilogue_hip");
   return out;
}

// whether gcn_rows16 would serve `mat` (rows16_call's test, without preparing anything)
static bool gcn_rows16_serves(const Tensor &rowptr, const Tensor &mat) {
   if (!is_half(mat) || !mat.is_cuda() || mat.dim() != 2 || rowptr.dim() != 1 || rowptr.numel() - 1 != mat.size(0)) return false;
   const int64_t N = mat.size(0), K = mat.size(1);
   return N > 0 && K > 0 && isplib_rows16_serves(N, K, K, K);      // (packed is always possible: the pitch test of the view is rows16_call's)
}

static Plan index_order_rows16_plan(const Tensor &like) {
   return Plan{at::empty({0}, like.options().dtype(at::kInt)), at::full({1}, 16, at::TensorOptions().dtype(at::kInt))};
}

// No fp32 [N, K] tensor in either direction: the forward allocates `out`, the backward g = dZ . [out > 0] (a bit select on the saved
// 16-bit output, isplib_masked_colsum16_hip; without ReLU g is dZ itself) and dX.  The mask is taken from the ROUNDED output the caller
// saw -- what a separate 16-bit relu would do: a sum that is positive in fp32 but rounds to 0 is masked.
class GcnNormSpmm16 : public torch::autograd::Function<GcnNormSpmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable mat, Variable dinv,
                                optional<Variable> opt_colptr, optional<Variable> opt_row_t, Plan plan, Plan plan_t,
                                optional<Variable> opt_bias, bool relu) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_feature(mat, "mat"); check_float(dinv, "dinv");
      const Tensor bias = or_undef(opt_bias);
      if (bias.defined()) check_feature(bias, "bias");
      const Tensor bias32 = bias.defined() && is_half(bias) ? bias.to(at::kFloat) : bias;      // K elements
      Tensor out = gcn_rows16(rowptr, col, mat, plan, dinv, bias32, relu);
      TORCH_CHECK(out.defined(), "isplib: gcn_norm_spmm: the 16-bit row kernel does not serve this operand");
      ctx->saved_data["relu"] = relu;
      ctx->saved_data["plan_t"] = plan_t;
      ctx->saved_data["bias_edge"] = (int64_t)(4 + (present(opt_colptr) ? 1 : 0) + (present(opt_row_t) ? 1 : 0));
      ctx->saved_data["has_bias"] = bias.defined();
      ctx->saved_data["bias_half"] = bias.defined() && is_half(bias);
      ctx->save_for_backward({rowptr, col, dinv, or_undef(opt_colptr), or_undef(opt_row_t), relu ? out : Tensor()});
      return {out};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      auto saved = ctx->get_saved_variables();
      auto rowptr = saved[0], col = saved[1], dinv = saved[2], colptr = saved[3], row_t = saved[4], out = saved[5];
      auto grad_bias = Variable(), grad_mat = Variable();
      const bool need_bias = ctx->saved_data["has_bias"].toBool() && ctx->needs_input_grad(ctx->saved_data["bias_edge"].toInt());
      const bool need_mat = ctx->needs_input_grad(2);
      if (need_bias || need_mat) {
         TORCH_CHECK(is_half(grad_outs[0]) && grad_outs[0].dim() == 2, "isplib: gcn_norm_spmm: `grad_out` must have the output's 16-bit dtype");
         const Tensor dz = packed16(grad_outs[0]);
         c10::DeviceGuard guard(dz.device());
         Plan plan_t = ctx->saved_data["plan_t"].toTensorVector();
         if (need_mat && (!colptr.defined() || !row_t.defined())) {
            auto t = build_transpose(rowptr, col, Tensor(), rowptr.numel() - 1, false);
            colptr = t.colptr; row_t = t.row_t; plan_t.clear();
         }
         if (!is_rows16_plan(plan_t)) plan_t = index_order_rows16_plan(dz);
         const int64_t N = dz.size(0), K = dz.size(1);
         const Tensor mask = ctx->saved_data["relu"].toBool() ? packed16(out) : Tensor();
         Tensor g = dz, gb32;                                               // no ReLU: g is dZ itself, no pass writes it
         if (mask.defined() && need_mat) g = at::empty({N, K}, dz.options());
         if (need_bias) gb32 = at::empty({K}, dz.options().dtype(at::kFloat));
         if (need_bias || (mask.defined() && need_mat)) {
            const size_t ws = isplib_masked_colsum16_workspace_bytes(N, K);
            Tensor work = at::empty({(int64_t)ws}, dz.options().dtype(at::kByte));
            const int st = isplib_masked_colsum16_hip(dz.scalar_type() == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16, N, K, dz.data_ptr(), K,
                                                      mask.defined() ? mask.data_ptr() : nullptr, K,
                                                      mask.defined() && need_mat ? g.data_ptr() : nullptr, K,
                                                      need_bias ? gb32.data_ptr<float>() : nullptr, work.data_ptr(), ws, current_stream(dz));
            check_status(st, "isplib_masked_colsum16_hip");
         }
         if (need_bias) grad_bias = ctx->saved_data["bias_half"].toBool() ? gb32.to(dz.scalar_type()) : gb32;      // rounded once
         if (need_mat) {
            grad_mat = gcn_rows16(colptr, row_t, g, plan_t, dinv, Tensor(), false);      // D (A^T + I) D g
            TORCH_CHECK(grad_mat.defined(), "isplib: gcn_norm_spmm: the 16-bit row kernel does not serve this gradient");
         }
      }
      return {Variable(), Variable(), grad_mat, Variable(), Variable(), Variable(), Variable(), Variable(), grad_bias, Variable()};
   }
};

Tensor gcn_norm_spmm(Tensor rowptr, Tensor col, Tensor mat, Tensor dinv, optional<Tensor> colptr, optional<Tensor> row_t,
                     Plan plan, Plan plan_t, optional<Tensor> bias, bool relu) {
   // a 16-bit `mat` on a 16-bit row plan (the plug-in's rows16_gcn_route said "rows16"): the 16-bit kernel where it serves the operand,
   // else the conversion route -- nothing raises.  Any other plan with a 16-bit `mat` is refused as it always was (check_float)
   if (is_half(mat) && is_rows16_plan(plan)) {
      if (gcn_rows16_serves(rowptr, mat)) return GcnNormSpmm16::apply(rowptr, col, mat, dinv, colptr, row_t, plan, plan_t, bias, relu)[0];
      const optional<Tensor> bias32 = present(bias) && is_half(*bias) ? optional<Tensor>(bias->to(at::kFloat)) : bias;
      return GcnNormSpmm::apply(rowptr, col, mat.to(at::kFloat), dinv, colptr, row_t, plan, plan_t, bias32, relu)[0].to(mat.scalar_type());
   }
   return GcnNormSpmm::apply(rowptr, col, mat, dinv, colptr, row_t, plan, plan_t, bias, relu)[0];
}

// ---- op wrappers: csrc/fusedmm.cpp:520-563 -------------------------------------------------
Tensor fusedmm_spmm_add(optional<Tensor> opt_row, Tensor rowptr, Tensor col, optional<Tensor> opt_value,
                        optional<Tensor> opt_colptr, optional<Tensor> opt_csr2csc, Tensor mat,
                        optional<Tensor> value_index_select, optional<Tensor> row_index_select) {
   return SpmmSum::apply(opt_row, rowptr, col, opt_value, opt_colptr, opt_csr2csc, mat, value_index_select,
                         row_index_select, auto_plan(), auto_plan())[0];
}

// same operators fed with the per-graph schedule operands of A (forward) and A^T (backward)
Tensor fusedmm_spmm_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, optional<Tensor> opt_colptr,
                            Tensor mat, optional<Tensor> value_t, optional<Tensor> row_t, Plan plan, Plan plan_t) {
   return SpmmSum::apply(optional<Tensor>(), rowptr, col, opt_value, opt_colptr, optional<Tensor>(), mat, value_t,
                         row_t, plan, plan_t)[0];
}

Tensor fusedmm_spmm_mean_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, optional<Tensor> opt_colptr,
                                 Tensor mat, optional<Tensor> row_t, optional<Tensor> mean_value_t, Plan plan,
                                 Plan plan_t) {
   return SpmmMean::apply(optional<Tensor>(), rowptr, col, opt_value, optional<Tensor>(), opt_colptr,
                          optional<Tensor>(), mat, row_t, mean_value_t, plan, plan_t)[0];
}

std::tuple<Tensor, Tensor> fusedmm_spmm_max_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat,
                                                    Plan plan);
std::tuple<Tensor, Tensor> fusedmm_spmm_min_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat,
                                                    Plan plan);

Tensor fusedmm_spmm_mean(optional<Tensor> opt_row, Tensor rowptr, Tensor col, optional<Tensor> opt_value,
                         optional<Tensor> opt_rowcount, optional<Tensor> opt_colptr, optional<Tensor> opt_csr2csc,
                         Tensor mat, optional<Tensor> new_row, optional<Tensor> new_rowcount) {
   return SpmmMean::apply(opt_row, rowptr, col, opt_value, opt_rowcount, opt_colptr, opt_csr2csc, mat, new_row,
                          new_rowcount, auto_plan(), auto_plan())[0];
}

std::tuple<Tensor, Tensor> fusedmm_spmm_max(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat) {
   auto r = SpmmMinMax<R_MAX>::apply(rowptr, col, opt_value, mat, auto_plan());
   return std::make_tuple(r[0], r[1]);
}

std::tuple<Tensor, Tensor> fusedmm_spmm_max_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat,
                                                    Plan plan) {
   auto r = SpmmMinMax<R_MAX>::apply(rowptr, col, opt_value, mat, plan);
   return std::make_tuple(r[0], r[1]);
}

std::tuple<Tensor, Tensor> fusedmm_spmm_min_planned(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat,
                                                    Plan plan) {
   auto r = SpmmMinMax<R_MIN>::apply(rowptr, col, opt_value, mat, plan);
   return std::make_tuple(r[0], r[1]);
}

// values only, no autograd node: what the plug-in calls for max / min when no gradient can be asked for (the patched matmul
// returns the tensor alone, isplib/__init__.py:143,145 + SURVEY 8a P1, so the positions would be computed and dropped)
Tensor fusedmm_spmm_max_values(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat, Plan plan) {
   OpTimer timer("FUSEDMM_SPMM_MAX_VALUES", mat);
   return std::get<0>(spmm_fw(rowptr, col, opt_value, mat, R_MAX, plan, /* want_arg = */ false));
}

Tensor fusedmm_spmm_min_values(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat, Plan plan) {
   OpTimer timer("FUSEDMM_SPMM_MIN_VALUES", mat);
   return std::get<0>(spmm_fw(rowptr, col, opt_value, mat, R_MIN, plan, /* want_arg = */ false));
}

std::tuple<Tensor, Tensor> fusedmm_spmm_min(Tensor rowptr, Tensor col, optional<Tensor> opt_value, Tensor mat) {
   auto r = SpmmMinMax<R_MIN>::apply(rowptr, col, opt_value, mat, auto_plan());
   return std::make_tuple(r[0], r[1]);
}

// ---- row-softmax attention aggregation (isplib_attention_*_hip; not an operator of the reference) ----------
// z_i = sum_e softmax_e(scale <x_i, y_j>) y_j over the stored entries of the CSR structure.  Saved for backward: x, y, z and ONE scalar
// per row (lse) -- the weights are recomputed, nothing of length nnz is kept.  Operands go in as they lie: a row-strided view (a head
// of one [N, H*d] tensor) keeps its pitch; only an operand without unit inner stride is copied.
struct AttnOperand {
   Tensor t;
   int64_t ld;
};
static AttnOperand attn_operand(const Tensor &src, const char *name, int64_t rows, int64_t k) {
   check_float(src, name);
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: attention_spmm: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   const bool as_is = src.size(0) == 0 || src.size(1) == 0 || (src.stride(1) == 1 && (src.size(0) == 1 || src.stride(0) >= k));
   const Tensor t = as_is ? src : src.contiguous();
   return {t, t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(k, 1)};
}

class AttentionSpmm : public torch::autograd::Function<AttentionSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable x, Variable y,
                                double scale) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(x.defined() && x.dim() == 2 && y.defined() && y.dim() == 2, "isplib: attention_spmm needs 2-D `x` [M, K] and `y` [N, K]");
      OpTimer timer("FUSEDMM_ATTENTION_FW", x);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = x.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: attention_spmm: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      const AttnOperand xo = attn_operand(x, "x", M, K), yo = attn_operand(y, "y", N, K);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &y})
         TORCH_CHECK(t->device() == x.device(), "isplib: attention_spmm: every operand must be on x's device");
      TORCH_CHECK(K == 0 || isplib_attention_serves(N, K, yo.ld), "isplib: attention_spmm: outside isplib_attention_serves (1 <= K <= ",
                  ISPLIB_ATTENTION_K_MAX, ", N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", K = ", K, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(x.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, x.options()), lse = at::empty({M}, x.options());
      if (M > 0 && K > 0) {
         const int st = isplib_attention_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                 xo.t.data_ptr<float>(), xo.ld, nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld, (float)scale,
                                                 z.data_ptr<float>(), K, lse.data_ptr<float>(), current_stream(x));
         check_status(st, "isplib_attention_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["scale"] = scale;
      ctx->save_for_backward({rp, cl, colptr, row_t, x, y, z, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_ATTENTION_BW", grad_outs[0]);
      const bool need_x = ctx->needs_input_grad(4), need_y = ctx->needs_input_grad(5);
      auto grad_x = Variable(), grad_y = Variable();
      if (need_x || need_y) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), x = saved[4], y = saved[5], z = saved[6],
              lse = saved[7];
         const float scale = (float)ctx->saved_data["scale"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = x.size(1), nnz = cl.numel();
         const AttnOperand xo = attn_operand(x, "x", M, K), yo = attn_operand(y, "y", N, K);
         const AttnOperand go = attn_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(x.device());
         // the rows kernel always runs: its D_i = <g_i, z_i> feeds the columns kernel; the columns kernel only when y asks
         Tensor dx = at::empty({M, K}, x.options()), dsum = at::empty({M}, x.options());
         if (M > 0 && K > 0) {
            const int st = isplib_attention_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                        xo.t.data_ptr<float>(), xo.ld, nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld, scale,
                                                        go.t.data_ptr<float>(), go.ld, z.data_ptr<float>(), K, lse.data_ptr<float>(),
                                                        dx.data_ptr<float>(), K, dsum.data_ptr<float>(), current_stream(x));
            check_status(st, "isplib_attention_bw_rows_hip");
         }
         if (need_x) grad_x = dx;
         if (need_y) {
            TORCH_CHECK(K == 0 || (isplib_attention_serves(M, K, xo.ld) && isplib_attention_serves(M, K, go.ld)),
                        "isplib: attention_spmm backward: outside isplib_attention_serves for the gathered rows of x: M = ", M, ", K = ", K);
            grad_y = at::empty({N, K}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_attention_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                           colptr.data_ptr<int64_t>() + 1, nnz > 0 ? xo.t.data_ptr<float>() : nullptr, xo.ld,
                                                           yo.t.data_ptr<float>(), yo.ld, scale, nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld,
                                                           lse.data_ptr<float>(), dsum.data_ptr<float>(), grad_y.data_ptr<float>(), K,
                                                           current_stream(x));
               check_status(st, "isplib_attention_bw_cols_hip");
            }
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_x, grad_y, Variable()};
   }
};

Tensor attention_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, double scale) {
   return AttentionSpmm::apply(rowptr, col, colptr, row_t, x, y, scale)[0];
}

// ---- GAT attention aggregation, all heads in one launch (isplib_gat_*_hip; not an operator of the reference) ----------
// z_i[head h] = sum_e softmax_e(leaky_relu(a_dst[i,h] + a_src[j,h])) y_j[head h].  Saved for backward: y, a_dst, a_src, z and lse [M, H]
// -- nothing of length nnz.  Every shape is checked before a launch: a mis-shaped dense operand must raise, never launch.
static Tensor gat_table(const Tensor &src, const char *name, int64_t rows, int64_t heads) {
   check_float(src, name);
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == heads, "isplib: gat_spmm: `", name, "` must be [", rows, ", ", heads,
               "] (one entry per row and head), got ", src.sizes());
   return src.contiguous();
}

static AttnOperand gat_operand(const Tensor &src, const char *name, int64_t rows, int64_t k) {
   check_float(src, name);
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: gat_spmm: `", name, "` must be [", rows, ", ", k, "], got ",
               src.sizes());
   const bool as_is = src.size(0) == 0 || src.size(1) == 0 || (src.stride(1) == 1 && (src.size(0) == 1 || src.stride(0) >= k));
   const Tensor t = as_is ? src : src.contiguous();
   return {t, t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(k, 1)};
}

class GatSpmm : public torch::autograd::Function<GatSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable y, Variable a_dst,
                                Variable a_src, int64_t heads, double negative_slope) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(y.defined() && y.dim() == 2, "isplib: gat_spmm needs a 2-D `y` [N, heads * d]");
      OpTimer timer("FUSEDMM_GAT_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: gat_spmm: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gat_spmm: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const AttnOperand yo = gat_operand(y, "y", N, K);
      TORCH_CHECK(a_dst.defined() && a_src.defined(), "isplib: gat_spmm needs `a_dst` [M, heads] and `a_src` [N, heads]");
      const Tensor ad = gat_table(a_dst, "a_dst", M, heads), as = gat_table(a_src, "a_src", N, heads);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &a_dst, &a_src})
         TORCH_CHECK(t->device() == y.device(), "isplib: gat_spmm: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gat_serves(N, heads, K / heads, yo.ld), "isplib: gat_spmm: outside isplib_gat_serves (heads * d <= ",
                  ISPLIB_GAT_K_MAX, ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(y.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options());
      if (M > 0 && K > 0) {
         const int st = isplib_gat_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                           ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                           nnz > 0 ? as.data_ptr<float>() : nullptr, heads, (float)negative_slope, z.data_ptr<float>(), K,
                                           lse.data_ptr<float>(), current_stream(y));
         check_status(st, "isplib_gat_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->save_for_backward({rp, cl, colptr, row_t, y, a_dst, a_src, z, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GAT_BW", grad_outs[0]);
      const bool need_y = ctx->needs_input_grad(4), need_dst = ctx->needs_input_grad(5), need_src = ctx->needs_input_grad(6);
      auto grad_y = Variable(), grad_dst = Variable(), grad_src = Variable();
      if (need_y || need_dst || need_src) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), y = saved[4], z = saved[7], lse = saved[8];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const AttnOperand yo = gat_operand(y, "y", N, K);
         const Tensor ad = gat_table(saved[5], "a_dst", M, heads), as = gat_table(saved[6], "a_src", N, heads);
         const AttnOperand go = gat_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(y.device());
         // the rows kernel always runs: its D[i,h] = <g_i, z_i>_h feeds the columns kernel; the columns kernel only when y or a_src asks
         Tensor dadst = at::empty({M, heads}, y.options()), dsum = at::empty({M, heads}, y.options());
         if (M > 0 && K > 0) {
            const int st = isplib_gat_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                  ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                  nnz > 0 ? as.data_ptr<float>() : nullptr, heads, ns, go.t.data_ptr<float>(), go.ld,
                                                  z.data_ptr<float>(), K, lse.data_ptr<float>(), dadst.data_ptr<float>(), dsum.data_ptr<float>(),
                                                  current_stream(y));
            check_status(st, "isplib_gat_bw_rows_hip");
         } else if (M > 0) {
            dadst.zero_();
         }
         if (need_dst) grad_dst = dadst;
         if (need_y || need_src) {
            TORCH_CHECK(K == 0 || isplib_gat_serves(M, heads, K / heads, go.ld),
                        "isplib: gat_spmm backward: outside isplib_gat_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options()), dasrc = at::empty({N, heads}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gat_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                     colptr.data_ptr<int64_t>() + 1, nnz > 0 ? ad.data_ptr<float>() : nullptr,
                                                     yo.t.data_ptr<float>(), yo.ld, as.data_ptr<float>(), heads, ns,
                                                     nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld, lse.data_ptr<float>(),
                                                     dsum.data_ptr<float>(), dy.data_ptr<float>(), K, dasrc.data_ptr<float>(), current_stream(y));
               check_status(st, "isplib_gat_bw_cols_hip");
            } else if (N > 0) {
               dasrc.zero_();
            }
            if (need_y) grad_y = dy;
            if (need_src) grad_src = dasrc;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_y, grad_dst, grad_src, Variable(), Variable()};
   }
};

Tensor gat_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor y, Tensor a_dst, Tensor a_src, int64_t heads,
                double negative_slope) {
   return GatSpmm::apply(rowptr, col, colptr, row_t, y, a_dst, a_src, heads, negative_slope)[0];
}

// ---- the GAT aggregation with a per-edge score term (isplib_gat_edge_*_hip) ----------
// u_e = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h], a_edge [nnz, heads] in CSR position order.  Saved for backward: what GatSpmm saves, plus
// a_edge and csr2csc (the columns kernel gathers a_edge by CSR position).  d a_edge [nnz, heads] is allocated, and written by the rows
// kernel, only when a_edge asks for a gradient.  The domain of everything the backward needs is checked in the forward.
class GatEdgeSpmm : public torch::autograd::Function<GatEdgeSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable csr2csc,
                                Variable y, Variable a_dst, Variable a_src, Variable a_edge, int64_t heads, double negative_slope) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      check_index(csr2csc, "csr2csc");
      TORCH_CHECK(y.defined() && y.dim() == 2, "isplib: gat_edge_spmm needs a 2-D `y` [N, heads * d]");
      OpTimer timer("FUSEDMM_GAT_EDGE_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz && csr2csc.numel() == nnz,
                  "isplib: gat_edge_spmm: `rowptr` / `colptr` need one entry more than rows / columns, `row_t` and `csr2csc` one entry per "
                  "stored entry (", nnz, "), got ", row_t.numel(), " and ", csr2csc.numel());
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gat_edge_spmm: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const AttnOperand yo = gat_operand(y, "y", N, K);
      TORCH_CHECK(a_dst.defined() && a_src.defined() && a_edge.defined(),
                  "isplib: gat_edge_spmm needs `a_dst` [M, heads], `a_src` [N, heads] and `a_edge` [nnz, heads]");
      const Tensor ad = gat_table(a_dst, "a_dst", M, heads), as = gat_table(a_src, "a_src", N, heads);
      check_float(a_edge, "a_edge");
      TORCH_CHECK(a_edge.dim() == 2 && a_edge.size(0) == nnz && a_edge.size(1) == heads, "isplib: gat_edge_spmm: `a_edge` must be [", nnz, ", ",
                  heads, "] (one row per stored entry, in the order of `col`), got ", a_edge.sizes());
      const Tensor ae = a_edge.contiguous();
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &csr2csc, &a_dst, &a_src, &a_edge})
         TORCH_CHECK(t->device() == y.device(), "isplib: gat_edge_spmm: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gat_serves(N, heads, K / heads, yo.ld), "isplib: gat_edge_spmm: outside isplib_gat_serves (heads * d <= ",
                  ISPLIB_GAT_K_MAX, ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitch = ", yo.ld);
      TORCH_CHECK(K == 0 || isplib_gat_serves(M, heads, K / heads, K),
                  "isplib: gat_edge_spmm: outside isplib_gat_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
      TORCH_CHECK(isplib_gat_edge_serves(nnz, heads), "isplib: gat_edge_spmm: outside isplib_gat_edge_serves (nnz < 2^31, nnz * heads * 4 <= "
                  "3.5 GiB, `a_edge` behind one buffer descriptor): nnz = ", nnz, ", heads = ", heads,
                  " -- pass fewer heads per call, on column views of `y`");
      c10::DeviceGuard guard(y.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options());
      if (M > 0 && K > 0) {
         const int st = isplib_gat_edge_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                nnz > 0 ? as.data_ptr<float>() : nullptr, nnz > 0 ? ae.data_ptr<float>() : nullptr, heads,
                                                (float)negative_slope, z.data_ptr<float>(), K, lse.data_ptr<float>(), current_stream(y));
         check_status(st, "isplib_gat_edge_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->save_for_backward({rp, cl, colptr, row_t, y, a_dst, a_src, z, lse, a_edge, csr2csc});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GAT_EDGE_BW", grad_outs[0]);
      const bool need_y = ctx->needs_input_grad(5), need_dst = ctx->needs_input_grad(6), need_src = ctx->needs_input_grad(7),
                 need_edge = ctx->needs_input_grad(8);
      auto grad_y = Variable(), grad_dst = Variable(), grad_src = Variable(), grad_edge = Variable();
      if (need_y || need_dst || need_src || need_edge) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), y = saved[4], z = saved[7], lse = saved[8];
         const Tensor csr2csc = saved[10].contiguous();
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const AttnOperand yo = gat_operand(y, "y", N, K);
         const Tensor ad = gat_table(saved[5], "a_dst", M, heads), as = gat_table(saved[6], "a_src", N, heads), ae = saved[9].contiguous();
         const AttnOperand go = gat_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(y.device());
         // the rows kernel always runs (D feeds the columns kernel); it gets d a_edge only when a_edge asks -- no [nnz, H] tensor otherwise
         Tensor dadst = at::empty({M, heads}, y.options()), dsum = at::empty({M, heads}, y.options());
         Tensor dedge = need_edge ? at::empty({nnz, heads}, y.options()) : Tensor();
         if (M > 0 && K > 0) {
            const int st = isplib_gat_edge_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                       ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                       nnz > 0 ? as.data_ptr<float>() : nullptr, nnz > 0 ? ae.data_ptr<float>() : nullptr, heads,
                                                       ns, go.t.data_ptr<float>(), go.ld, z.data_ptr<float>(), K, lse.data_ptr<float>(),
                                                       dadst.data_ptr<float>(), dsum.data_ptr<float>(), current_stream(y),
                                                       need_edge && nnz > 0 ? dedge.data_ptr<float>() : nullptr);
            check_status(st, "isplib_gat_edge_bw_rows_hip");
         } else if (M > 0) {
            dadst.zero_();
            if (need_edge) dedge.zero_();                // K == 0: heads * d with d == 0 -- every du_e is 0
         }
         if (need_dst) grad_dst = dadst;
         if (need_edge) grad_edge = dedge;
         if (need_y || need_src) {
            TORCH_CHECK(K == 0 || isplib_gat_serves(M, heads, K / heads, go.ld),
                        "isplib: gat_edge_spmm backward: outside isplib_gat_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options()), dasrc = at::empty({N, heads}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gat_edge_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                          colptr.data_ptr<int64_t>() + 1, nnz > 0 ? csr2csc.data_ptr<int64_t>() : nullptr,
                                                          nnz > 0 ? ad.data_ptr<float>() : nullptr, yo.t.data_ptr<float>(), yo.ld,
                                                          as.data_ptr<float>(), nnz > 0 ? ae.data_ptr<float>() : nullptr, heads, ns,
                                                          nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld, lse.data_ptr<float>(),
                                                          dsum.data_ptr<float>(), dy.data_ptr<float>(), K, dasrc.data_ptr<float>(),
                                                          current_stream(y));
               check_status(st, "isplib_gat_edge_bw_cols_hip");
            } else if (N > 0) {
               dasrc.zero_();
            }
            if (need_y) grad_y = dy;
            if (need_src) grad_src = dasrc;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), Variable(), grad_y, grad_dst, grad_src, grad_edge, Variable(), Variable()};
   }
};

Tensor gat_edge_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor y, Tensor a_dst, Tensor a_src,
                     Tensor a_edge, int64_t heads, double negative_slope) {
   return GatEdgeSpmm::apply(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, a_edge, heads, negative_slope)[0];
}

// ---- the GAT aggregation with attention dropout (isplib_gat_drop_*_hip) ----------
// The coefficients are dropped after the softmax, per stored entry and head; the keep bit is a pure function of (seed, CSR position,
// head), so the backward regenerates the mask from the seed.  a_edge is optional (`edge` false: no per-edge term).  Saved for backward: what
// GatEdgeSpmm saves, plus the two scalars p and seed.  Only the kernels whose gradients are asked for run.
class GatDropSpmm : public torch::autograd::Function<GatDropSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable csr2csc,
                                Variable y, Variable a_dst, Variable a_src, Variable a_edge, bool edge, int64_t heads, double negative_slope,
                                double p, int64_t seed) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      check_index(csr2csc, "csr2csc");
      TORCH_CHECK(y.defined() && y.dim() == 2, "isplib: gat_drop_spmm needs a 2-D `y` [N, heads * d]");
      TORCH_CHECK(p > 0.0 && p < 1.0, "isplib: gat_drop_spmm: `p` must lie in (0, 1), got ", p, " (p == 0: gat_spmm / gat_edge_spmm)");
      TORCH_CHECK(seed >= 0, "isplib: gat_drop_spmm: `seed` must be a non-negative int64, got ", seed);
      OpTimer timer("FUSEDMM_GAT_DROP_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz && csr2csc.numel() == nnz,
                  "isplib: gat_drop_spmm: `rowptr` / `colptr` need one entry more than rows / columns, `row_t` and `csr2csc` one entry per "
                  "stored entry (", nnz, "), got ", row_t.numel(), " and ", csr2csc.numel());
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gat_drop_spmm: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const AttnOperand yo = gat_operand(y, "y", N, K);
      TORCH_CHECK(a_dst.defined() && a_src.defined(), "isplib: gat_drop_spmm needs `a_dst` [M, heads] and `a_src` [N, heads]");
      const Tensor ad = gat_table(a_dst, "a_dst", M, heads), as = gat_table(a_src, "a_src", N, heads);
      Tensor ae;
      if (edge) {
         check_float(a_edge, "a_edge");
         TORCH_CHECK(a_edge.dim() == 2 && a_edge.size(0) == nnz && a_edge.size(1) == heads, "isplib: gat_drop_spmm: `a_edge` must be [", nnz,
                     ", ", heads, "] (one row per stored entry, in the order of `col`), got ", a_edge.sizes());
         TORCH_CHECK(a_edge.device() == y.device(), "isplib: gat_drop_spmm: every operand must be on y's device");
         ae = a_edge.contiguous();
      }
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &csr2csc, &a_dst, &a_src})
         TORCH_CHECK(t->device() == y.device(), "isplib: gat_drop_spmm: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gat_serves(N, heads, K / heads, yo.ld), "isplib: gat_drop_spmm: outside isplib_gat_serves (heads * d <= ",
                  ISPLIB_GAT_K_MAX, ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitch = ", yo.ld);
      TORCH_CHECK(K == 0 || isplib_gat_serves(M, heads, K / heads, K),
                  "isplib: gat_drop_spmm: outside isplib_gat_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
      TORCH_CHECK(nnz < (1LL << 31), "isplib: gat_drop_spmm: the keep bit is defined for CSR positions below 2^31, got nnz = ", nnz);
      TORCH_CHECK(!edge || isplib_gat_edge_serves(nnz, heads), "isplib: gat_drop_spmm: outside isplib_gat_edge_serves (nnz < 2^31, nnz * heads "
                  "* 4 <= 3.5 GiB, `a_edge` behind one buffer descriptor): nnz = ", nnz, ", heads = ", heads,
                  " -- pass fewer heads per call, on column views of `y`");
      c10::DeviceGuard guard(y.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options());
      if (M > 0 && K > 0) {
         const int st = isplib_gat_drop_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                nnz > 0 ? as.data_ptr<float>() : nullptr, edge && nnz > 0 ? ae.data_ptr<float>() : nullptr,
                                                heads, (float)negative_slope, z.data_ptr<float>(), K, lse.data_ptr<float>(), current_stream(y),
                                                isplib_gat_drop_threshold(p), (float)(1.0 / (1.0 - p)), (uint64_t)seed);
         check_status(st, "isplib_gat_drop_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->saved_data["p"] = p;
      ctx->saved_data["seed"] = seed;
      ctx->saved_data["edge"] = edge;
      ctx->save_for_backward({rp, cl, colptr, row_t, y, a_dst, a_src, z, lse, a_edge, csr2csc});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GAT_DROP_BW", grad_outs[0]);
      const bool edge = ctx->saved_data["edge"].toBool();
      const bool need_y = ctx->needs_input_grad(5), need_dst = ctx->needs_input_grad(6), need_src = ctx->needs_input_grad(7),
                 need_edge = edge && ctx->needs_input_grad(8);
      auto grad_y = Variable(), grad_dst = Variable(), grad_src = Variable(), grad_edge = Variable();
      if (need_y || need_dst || need_src || need_edge) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), y = saved[4], z = saved[7], lse = saved[8];
         const Tensor csr2csc = saved[10].contiguous();
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const double p = ctx->saved_data["p"].toDouble();
         const uint32_t threshold = isplib_gat_drop_threshold(p);
         const float scale = (float)(1.0 / (1.0 - p));
         const uint64_t seed = (uint64_t)ctx->saved_data["seed"].toInt();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const AttnOperand yo = gat_operand(y, "y", N, K);
         const Tensor ad = gat_table(saved[5], "a_dst", M, heads), as = gat_table(saved[6], "a_src", N, heads);
         const Tensor ae = edge ? saved[9].contiguous() : Tensor();
         const float *aep = edge && nnz > 0 ? ae.data_ptr<float>() : nullptr;
         const AttnOperand go = gat_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(y.device());
         // the rows kernel always runs (D feeds the columns kernel); it gets d a_edge only when a_edge asks -- no [nnz, H] tensor otherwise
         Tensor dadst = at::empty({M, heads}, y.options()), dsum = at::empty({M, heads}, y.options());
         Tensor dedge = need_edge ? at::empty({nnz, heads}, y.options()) : Tensor();
         if (M > 0 && K > 0) {
            const int st = isplib_gat_drop_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                       ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                       nnz > 0 ? as.data_ptr<float>() : nullptr, aep, heads, ns, go.t.data_ptr<float>(), go.ld,
                                                       z.data_ptr<float>(), K, lse.data_ptr<float>(), dadst.data_ptr<float>(),
                                                       dsum.data_ptr<float>(), current_stream(y),
                                                       need_edge && nnz > 0 ? dedge.data_ptr<float>() : nullptr, threshold, scale, seed);
            check_status(st, "isplib_gat_drop_bw_rows_hip");
         } else if (M > 0) {
            dadst.zero_();
            if (need_edge) dedge.zero_();
         }
         if (need_dst) grad_dst = dadst;
         if (need_edge) grad_edge = dedge;
         if (need_y || need_src) {
            TORCH_CHECK(K == 0 || isplib_gat_serves(M, heads, K / heads, go.ld),
                        "isplib: gat_drop_spmm backward: outside isplib_gat_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options()), dasrc = at::empty({N, heads}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gat_drop_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                          colptr.data_ptr<int64_t>() + 1, nnz > 0 ? csr2csc.data_ptr<int64_t>() : nullptr,
                                                          nnz > 0 ? ad.data_ptr<float>() : nullptr, yo.t.data_ptr<float>(), yo.ld,
                                                          as.data_ptr<float>(), aep, heads, ns, nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld,
                                                          lse.data_ptr<float>(), dsum.data_ptr<float>(), dy.data_ptr<float>(), K,
                                                          dasrc.data_ptr<float>(), current_stream(y), threshold, scale, seed);
               check_status(st, "isplib_gat_drop_bw_cols_hip");
            } else if (N > 0) {
               dasrc.zero_();
            }
            if (need_y) grad_y = dy;
            if (need_src) grad_src = dasrc;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), Variable(), grad_y, grad_dst, grad_src, grad_edge, Variable(), Variable(),
              Variable(), Variable(), Variable()};
   }
};

Tensor gat_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor y, Tensor a_dst, Tensor a_src,
                     c10::optional<Tensor> a_edge, int64_t heads, double negative_slope, double p, int64_t seed) {
   // without the per-edge term the slot holds an empty placeholder (an autograd function takes defined tensors)
   const bool edge = a_edge.has_value() && a_edge->defined();
   return GatDropSpmm::apply(rowptr, col, colptr, row_t, csr2csc, y, a_dst, a_src, edge ? *a_edge : at::empty({0}, y.options()), edge, heads,
                             negative_slope, p, seed)[0];
}

// ---- the same aggregation for bf16 / fp16 operands (isplib_attention16_*_hip) ----------
// x and y go in as they lie, z / dx / dy come back in their dtype, lse and D stay fp32: no fp32 [*, K] tensor in either direction.  Saved
// for backward: the structure, x, y and lse -- NOT z: the rows kernel forms D_i from the row's edges (the rounded z would cost every
// ds_e an error of u * sum |g z|).  An operand is copied only without unit inner stride, or where the domain admits it packed but not at
// its pitch or alignment.
static AttnOperand attn16_operand(const Tensor &src, const char *name, int64_t rows, int64_t k, at::ScalarType dtype) {
   TORCH_CHECK(src.defined() && src.scalar_type() == dtype, "isplib: attention_spmm16: `", name, "` must be ", dtype, " (x and y both bfloat16 or both "
               "float16), got ", src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: attention_spmm16: `", name, "` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: attention_spmm16: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   if (rows == 0 || k == 0) return {src, std::max<int64_t>(k, 1)};
   const int64_t ld = rows > 1 ? src.stride(0) : k;
   const bool as_is = src.stride(1) == 1 && ld >= k && ((uintptr_t)src.data_ptr() & 3) == 0 && isplib_attention16_serves(rows, k, ld);
   if (as_is) return {src, ld};
   return {src.clone(at::MemoryFormat::Contiguous), k};
}

class AttentionSpmm16 : public torch::autograd::Function<AttentionSpmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable x, Variable y,
                                double scale) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(x.defined() && x.dim() == 2 && y.defined() && y.dim() == 2, "isplib: attention_spmm16 needs 2-D `x` [M, K] and `y` [N, K]");
      TORCH_CHECK(is_half(x), "isplib: attention_spmm16: `x` and `y` must both be bfloat16 or both float16, got ", x.scalar_type(), " and ",
                  y.scalar_type(), " (float32: attention_spmm)");
      OpTimer timer("FUSEDMM_ATTENTION_FW", x);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = x.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: attention_spmm16: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      const at::ScalarType dt = x.scalar_type();
      const AttnOperand xo = attn16_operand(x, "x", M, K, dt), yo = attn16_operand(y, "y", N, K, dt);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &y})
         TORCH_CHECK(t->device() == x.device(), "isplib: attention_spmm16: every operand must be on x's device");
      TORCH_CHECK(K == 0 || (isplib_attention16_serves(N, K, yo.ld) && xo.ld % 2 == 0),
                  "isplib: attention_spmm16: outside isplib_attention16_serves (", ISPLIB_ATTENTION16_K_MIN, " <= K <= ", ISPLIB_ATTENTION16_K_MAX,
                  ", K even, N < 2^31, N * pitch * 2 <= 3.5 GiB): N = ", N, ", K = ", K, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(x.device());
      const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, x.options()), lse = at::empty({M}, x.options().dtype(at::kFloat));
      if (M > 0 && K > 0) {
         const int st = isplib_attention16_csr_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                   xo.t.data_ptr(), xo.ld, nnz > 0 ? yo.t.data_ptr() : nullptr, yo.ld, (float)scale, z.data_ptr(), K,
                                                   lse.data_ptr<float>(), current_stream(x));
         check_status(st, "isplib_attention16_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["scale"] = scale;
      ctx->save_for_backward({rp, cl, colptr, row_t, x, y, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_ATTENTION_BW", grad_outs[0]);
      const bool need_x = ctx->needs_input_grad(4), need_y = ctx->needs_input_grad(5);
      auto grad_x = Variable(), grad_y = Variable();
      if (need_x || need_y) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), x = saved[4], y = saved[5], lse = saved[6];
         const float scale = (float)ctx->saved_data["scale"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = x.size(1), nnz = cl.numel();
         const at::ScalarType dt = x.scalar_type();
         const AttnOperand xo = attn16_operand(x, "x", M, K, dt), yo = attn16_operand(y, "y", N, K, dt);
         const AttnOperand go = attn16_operand(grad_outs[0].to(dt), "grad_out", M, K, dt);      // a grad of another dtype is cast to the operands'
         c10::DeviceGuard guard(x.device());
         const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
         // the rows kernel always runs: its D_i feeds the columns kernel; the columns kernel only when y asks
         Tensor dx = at::empty({M, K}, x.options()), dsum = at::empty({M}, x.options().dtype(at::kFloat));
         if (M > 0 && K > 0) {
            const int st = isplib_attention16_bw_rows_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                          rp.data_ptr<int64_t>() + 1, xo.t.data_ptr(), xo.ld, nnz > 0 ? yo.t.data_ptr() : nullptr,
                                                          yo.ld, scale, go.t.data_ptr(), go.ld, lse.data_ptr<float>(), dx.data_ptr(), K,
                                                          dsum.data_ptr<float>(), current_stream(x));
            check_status(st, "isplib_attention16_bw_rows_hip");
         }
         if (need_x) grad_x = dx;
         if (need_y) {
            TORCH_CHECK(K == 0 || (isplib_attention16_serves(M, K, xo.ld) && isplib_attention16_serves(M, K, go.ld)),
                        "isplib: attention_spmm16 backward: outside isplib_attention16_serves for the gathered rows of x: M = ", M, ", K = ", K);
            grad_y = at::empty({N, K}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_attention16_bw_cols_hip(code, M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                             colptr.data_ptr<int64_t>() + 1, nnz > 0 ? xo.t.data_ptr() : nullptr, xo.ld,
                                                             yo.t.data_ptr(), yo.ld, scale, nnz > 0 ? go.t.data_ptr() : nullptr, go.ld,
                                                             lse.data_ptr<float>(), dsum.data_ptr<float>(), grad_y.data_ptr(), K,
                                                             current_stream(x));
               check_status(st, "isplib_attention16_bw_cols_hip");
            }
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_x, grad_y, Variable()};
   }
};

Tensor attention_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, double scale) {
   return AttentionSpmm16::apply(rowptr, col, colptr, row_t, x, y, scale)[0];
}

// ---- the GAT aggregation for a bf16 / fp16 `y` (isplib_gat16_*_hip) ----------
// y goes in as it lies, z and dy come back in its dtype; the two score tables, lse, D and the score gradients stay fp32: no fp32 [*, K]
// tensor in either direction.  Saved for backward: the structure, y, a_dst, a_src and lse -- NOT z: the rows kernel forms D[i,h] from the
// row's edges.  y (or the gradient) is copied only without unit inner stride, or where the domain admits it packed but not at its pitch
// or alignment.
static AttnOperand gat16_operand(const Tensor &src, const char *name, int64_t rows, int64_t k, int64_t heads, at::ScalarType dtype) {
   TORCH_CHECK(src.defined() && src.scalar_type() == dtype, "isplib: gat_spmm16: `", name, "` must be ", dtype, ", got ",
               src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: gat_spmm16: `", name, "` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: gat_spmm16: `", name, "` must be [", rows, ", ", k, "], got ",
               src.sizes());
   if (rows == 0 || k == 0) return {src, std::max<int64_t>(k, 1)};
   const int64_t ld = rows > 1 ? src.stride(0) : k;
   const bool as_is = src.stride(1) == 1 && ld >= k && ((uintptr_t)src.data_ptr() & 3) == 0 && isplib_gat16_serves(rows, heads, k / heads, ld);
   if (as_is) return {src, ld};
   return {src.clone(at::MemoryFormat::Contiguous), k};
}

static Tensor gat16_table(const Tensor &src, const char *name, int64_t rows, int64_t heads) {
   TORCH_CHECK(src.defined() && src.scalar_type() == at::kFloat, "isplib: gat_spmm16: `", name, "` must be float32 (the score tables stay fp32), got ",
               src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: gat_spmm16: `", name, "` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == heads, "isplib: gat_spmm16: `", name, "` must be [", rows, ", ", heads,
               "] (one entry per row and head), got ", src.sizes());
   return src.contiguous();
}

class GatSpmm16 : public torch::autograd::Function<GatSpmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable y, Variable a_dst,
                                Variable a_src, int64_t heads, double negative_slope) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(y.defined() && y.dim() == 2, "isplib: gat_spmm16 needs a 2-D `y` [N, heads * d]");
      TORCH_CHECK(is_half(y), "isplib: gat_spmm16: `y` must be bfloat16 or float16, got ", y.scalar_type(), " (float32: gat_spmm)");
      OpTimer timer("FUSEDMM_GAT_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: gat_spmm16: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gat_spmm16: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const at::ScalarType dt = y.scalar_type();
      const AttnOperand yo = gat16_operand(y, "y", N, K, heads, dt);
      const Tensor ad = gat16_table(a_dst, "a_dst", M, heads), as = gat16_table(a_src, "a_src", N, heads);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &a_dst, &a_src})
         TORCH_CHECK(t->device() == y.device(), "isplib: gat_spmm16: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gat16_serves(N, heads, K / heads, yo.ld), "isplib: gat_spmm16: outside isplib_gat16_serves (",
                  ISPLIB_GAT16_K_MIN, " <= heads * d <= ", ISPLIB_GAT16_K_MAX, ", heads == 1 with d even or d a power of two >= 8, N < 2^31, "
                  "N * pitch * 2 <= 3.5 GiB): N = ", N, ", heads = ", heads, ", d = ", K / heads, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(y.device());
      const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options().dtype(at::kFloat));
      if (M > 0 && K > 0) {
         const int st = isplib_gat16_csr_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                             ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr() : nullptr, yo.ld,
                                             nnz > 0 ? as.data_ptr<float>() : nullptr, heads, (float)negative_slope, z.data_ptr(), K,
                                             lse.data_ptr<float>(), current_stream(y));
         check_status(st, "isplib_gat16_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->save_for_backward({rp, cl, colptr, row_t, y, a_dst, a_src, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GAT_BW", grad_outs[0]);
      const bool need_y = ctx->needs_input_grad(4), need_dst = ctx->needs_input_grad(5), need_src = ctx->needs_input_grad(6);
      auto grad_y = Variable(), grad_dst = Variable(), grad_src = Variable();
      if (need_y || need_dst || need_src) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), y = saved[4], lse = saved[7];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const at::ScalarType dt = y.scalar_type();
         const AttnOperand yo = gat16_operand(y, "y", N, K, heads, dt);
         const Tensor ad = gat16_table(saved[5], "a_dst", M, heads), as = gat16_table(saved[6], "a_src", N, heads);
         const AttnOperand go = gat16_operand(grad_outs[0].to(dt), "grad_out", M, K, heads, dt);      // a grad of another dtype is cast to y's
         c10::DeviceGuard guard(y.device());
         const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
         const auto f32 = y.options().dtype(at::kFloat);
         // the rows kernel always runs: its D[i,h] feeds the columns kernel; the columns kernel only when y or a_src asks
         Tensor dadst = at::empty({M, heads}, f32), dsum = at::empty({M, heads}, f32);
         if (M > 0 && K > 0) {
            const int st = isplib_gat16_bw_rows_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                    ad.data_ptr<float>(), nnz > 0 ? yo.t.data_ptr() : nullptr, yo.ld,
                                                    nnz > 0 ? as.data_ptr<float>() : nullptr, heads, ns, go.t.data_ptr(), go.ld,
                                                    lse.data_ptr<float>(), dadst.data_ptr<float>(), dsum.data_ptr<float>(), current_stream(y));
            check_status(st, "isplib_gat16_bw_rows_hip");
         } else if (M > 0) {
            dadst.zero_();
         }
         if (need_dst) grad_dst = dadst;
         if (need_y || need_src) {
            TORCH_CHECK(K == 0 || isplib_gat16_serves(M, heads, K / heads, go.ld),
                        "isplib: gat_spmm16 backward: outside isplib_gat16_serves for the gathered rows of the gradient: M = ", M, ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options()), dasrc = at::empty({N, heads}, f32);
            if (N > 0 && K > 0) {
               const int st = isplib_gat16_bw_cols_hip(code, M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                       colptr.data_ptr<int64_t>() + 1, nnz > 0 ? ad.data_ptr<float>() : nullptr, yo.t.data_ptr(),
                                                       yo.ld, as.data_ptr<float>(), heads, ns, nnz > 0 ? go.t.data_ptr() : nullptr, go.ld,
                                                       lse.data_ptr<float>(), dsum.data_ptr<float>(), dy.data_ptr(), K, dasrc.data_ptr<float>(),
                                                       current_stream(y));
               check_status(st, "isplib_gat16_bw_cols_hip");
            } else if (N > 0) {
               dasrc.zero_();
            }
            if (need_y) grad_y = dy;
            if (need_src) grad_src = dasrc;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_y, grad_dst, grad_src, Variable(), Variable()};
   }
};

Tensor gat_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor y, Tensor a_dst, Tensor a_src, int64_t heads,
                  double negative_slope) {
   return GatSpmm16::apply(rowptr, col, colptr, row_t, y, a_dst, a_src, heads, negative_slope)[0];
}

// ---- GATv2 attention aggregation, all heads in one launch (isplib_gatv2_*_hip; not an operator of the reference) ----------
// z_i[head h] = sum_e softmax_e(sum_c att_c leaky_relu(x_ic + y_jc)) y_j[head h].  Saved for backward: the structure, x, y, att, z and lse
// [M, H] -- nothing of length nnz.  Every shape is checked before a launch: a mis-shaped dense operand must raise, never launch.
static AttnOperand gatv2_operand(const Tensor &src, const char *name, int64_t rows, int64_t k) {
   check_float(src, name);
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: gatv2_spmm: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   const bool as_is = src.size(0) == 0 || src.size(1) == 0 || (src.stride(1) == 1 && (src.size(0) == 1 || src.stride(0) >= k));
   const Tensor t = as_is ? src : src.contiguous();
   return {t, t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(k, 1)};
}

static Tensor gatv2_att(const Tensor &src, int64_t heads, int64_t d) {
   check_float(src, "att");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == heads && src.size(1) == d, "isplib: gatv2_spmm: `att` must be [", heads, ", ", d,
               "] (heads x d), got ", src.sizes());
   return src.contiguous();
}

class Gatv2Spmm : public torch::autograd::Function<Gatv2Spmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable x, Variable y,
                                Variable att, int64_t heads, double negative_slope) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(x.defined() && x.dim() == 2 && y.defined() && y.dim() == 2, "isplib: gatv2_spmm needs 2-D `x` [M, heads * d] and `y` "
                                                                              "[N, heads * d]");
      OpTimer timer("FUSEDMM_GATV2_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: gatv2_spmm: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gatv2_spmm: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const AttnOperand xo = gatv2_operand(x, "x", M, K), yo = gatv2_operand(y, "y", N, K);
      TORCH_CHECK(att.defined(), "isplib: gatv2_spmm needs `att` [heads, d]");
      const Tensor av = gatv2_att(att, heads, K / heads);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &x, &att})
         TORCH_CHECK(t->device() == y.device(), "isplib: gatv2_spmm: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gatv2_serves(N, heads, K / heads, yo.ld), "isplib: gatv2_spmm: outside isplib_gatv2_serves (heads * d <= ",
                  ISPLIB_GAT_K_MAX, ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(y.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options());
      if (M > 0 && K > 0) {
         const int st = isplib_gatv2_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                             xo.t.data_ptr<float>(), xo.ld, nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                             av.data_ptr<float>(), heads, (float)negative_slope, z.data_ptr<float>(), K, lse.data_ptr<float>(),
                                             current_stream(y));
         check_status(st, "isplib_gatv2_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->save_for_backward({rp, cl, colptr, row_t, x, y, att, z, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GATV2_BW", grad_outs[0]);
      const bool need_x = ctx->needs_input_grad(4), need_y = ctx->needs_input_grad(5), need_att = ctx->needs_input_grad(6);
      auto grad_x = Variable(), grad_y = Variable(), grad_att = Variable();
      if (need_x || need_y || need_att) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), x = saved[4], y = saved[5], z = saved[7],
              lse = saved[8];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const AttnOperand xo = gatv2_operand(x, "x", M, K), yo = gatv2_operand(y, "y", N, K);
         const Tensor av = gatv2_att(saved[6], heads, K / heads);
         const AttnOperand go = gatv2_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(y.device());
         // the rows kernel always runs: its D[i,h] = <g_i, z_i>_h feeds the columns kernel; its datt instantiation only when att asks; the
         // columns kernel only when y asks
         Tensor dx = at::empty({M, K}, y.options()), dsum = at::empty({M, heads}, y.options());
         Tensor datt = need_att ? at::empty({heads, K / heads}, y.options()) : Tensor();
         if (M > 0 && K > 0) {
            const size_t ws = need_att ? isplib_gatv2_bw_rows_workspace_bytes(M, K) : 0;
            Tensor work = need_att ? at::empty({(int64_t)ws}, y.options().dtype(at::kByte)) : Tensor();
            const int st = isplib_gatv2_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                    xo.t.data_ptr<float>(), xo.ld, nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                    av.data_ptr<float>(), heads, ns, go.t.data_ptr<float>(), go.ld, z.data_ptr<float>(), K,
                                                    lse.data_ptr<float>(), dx.data_ptr<float>(), K, dsum.data_ptr<float>(),
                                                    need_att ? datt.data_ptr<float>() : nullptr, need_att ? work.data_ptr() : nullptr, ws,
                                                    current_stream(y));
            check_status(st, "isplib_gatv2_bw_rows_hip");
         } else if (need_att) {
            datt.zero_();
         }
         if (need_x) grad_x = dx;
         if (need_att) grad_att = datt;
         if (need_y) {
            TORCH_CHECK(K == 0 || (isplib_gatv2_serves(M, heads, K / heads, xo.ld) && isplib_gatv2_serves(M, heads, K / heads, go.ld)),
                        "isplib: gatv2_spmm backward: outside isplib_gatv2_serves for the gathered rows of x and of the gradient: M = ", M,
                        ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gatv2_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                       colptr.data_ptr<int64_t>() + 1, nnz > 0 ? xo.t.data_ptr<float>() : nullptr, xo.ld,
                                                       yo.t.data_ptr<float>(), yo.ld, av.data_ptr<float>(), heads, ns,
                                                       nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld, lse.data_ptr<float>(),
                                                       dsum.data_ptr<float>(), dy.data_ptr<float>(), K, current_stream(y));
               check_status(st, "isplib_gatv2_bw_cols_hip");
            }
            grad_y = dy;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_x, grad_y, grad_att, Variable(), Variable()};
   }
};

Tensor gatv2_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, Tensor att, int64_t heads,
                  double negative_slope) {
   return Gatv2Spmm::apply(rowptr, col, colptr, row_t, x, y, att, heads, negative_slope)[0];
}

// ---- sparse multi-head dot-product attention with separate keys and values (isplib_mha_*_hip; not an operator of the
// reference) ----------
// z_i[head h] = sum_e softmax_e(scale <q_i, k_j>_h) v_j[head h].  Saved for backward: the structure, q, k, v, z and lse [M, H] -- nothing of
// length nnz.  Operands with unit column stride and a row pitch >= K go in as they lie (column views of one fused [rows, 3K] projection
// are not copied); anything else is made contiguous.  Every shape is checked before a launch.
static AttnOperand mha_operand(const Tensor &src, const char *name, int64_t rows, int64_t k) {
   check_float(src, name);
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: mha_spmm: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   const bool as_is = src.size(0) == 0 || src.size(1) == 0 || (src.stride(1) == 1 && (src.size(0) == 1 || src.stride(0) >= k));
   const Tensor t = as_is ? src : src.contiguous();
   return {t, t.size(0) > 1 ? t.stride(0) : std::max<int64_t>(k, 1)};
}

class MhaSpmm : public torch::autograd::Function<MhaSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable q, Variable k,
                                Variable v, int64_t heads, double scale) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(q.defined() && q.dim() == 2 && k.defined() && k.dim() == 2 && v.defined() && v.dim() == 2,
                  "isplib: mha_spmm needs 2-D `q` [M, heads * d], `k` and `v` [N, heads * d]");
      OpTimer timer("FUSEDMM_MHA_FW", q);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: mha_spmm: `rowptr` / `colptr` need one entry more than rows / columns, "
                                                             "`row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: mha_spmm: the width of `q` (", K, ") must be heads * d, got heads = ", heads);
      TORCH_CHECK(std::isfinite(scale), "isplib: mha_spmm: `scale` must be a finite number, got ", scale);
      const AttnOperand qo = mha_operand(q, "q", M, K), ko = mha_operand(k, "k", N, K), vo = mha_operand(v, "v", N, K);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &k, &v})
         TORCH_CHECK(t->device() == q.device(), "isplib: mha_spmm: every operand must be on q's device");
      TORCH_CHECK(K == 0 || (isplib_mha_serves(N, heads, K / heads, ko.ld) && isplib_mha_serves(N, heads, K / heads, vo.ld)),
                  "isplib: mha_spmm: outside isplib_mha_serves (heads * d <= ", ISPLIB_GAT_K_MAX,
                  ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads, ", d = ",
                  K / heads, ", pitches = ", ko.ld, ", ", vo.ld);
      c10::DeviceGuard guard(q.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, q.options()), lse = at::empty({M, heads}, q.options());
      if (M > 0 && K > 0) {
         const int st = isplib_mha_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1, heads,
                                           (float)scale, qo.t.data_ptr<float>(), qo.ld, nnz > 0 ? ko.t.data_ptr<float>() : nullptr, ko.ld,
                                           nnz > 0 ? vo.t.data_ptr<float>() : nullptr, vo.ld, z.data_ptr<float>(), K, lse.data_ptr<float>(),
                                           current_stream(q));
         check_status(st, "isplib_mha_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["scale"] = scale;
      ctx->save_for_backward({rp, cl, colptr, row_t, q, k, v, z, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_MHA_BW", grad_outs[0]);
      const bool need_q = ctx->needs_input_grad(4), need_k = ctx->needs_input_grad(5), need_v = ctx->needs_input_grad(6);
      auto grad_q = Variable(), grad_k = Variable(), grad_v = Variable();
      if (need_q || need_k || need_v) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), q = saved[4], k = saved[5], v = saved[6],
              z = saved[7], lse = saved[8];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float p = (float)ctx->saved_data["scale"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = cl.numel();
         const AttnOperand qo = mha_operand(q, "q", M, K), ko = mha_operand(k, "k", N, K), vo = mha_operand(v, "v", N, K);
         const AttnOperand go = mha_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(q.device());
         // the rows kernel always runs: its D[i,h] = <g_i, z_i>_h feeds the columns kernel; the columns kernel only when k or v asks
         Tensor dq = at::empty({M, K}, q.options()), dsum = at::empty({M, heads}, q.options());
         if (M > 0 && K > 0) {
            const int st = isplib_mha_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1, heads,
                                                  p, qo.t.data_ptr<float>(), qo.ld, nnz > 0 ? ko.t.data_ptr<float>() : nullptr, ko.ld,
                                                  nnz > 0 ? vo.t.data_ptr<float>() : nullptr, vo.ld, go.t.data_ptr<float>(), go.ld,
                                                  z.data_ptr<float>(), K, lse.data_ptr<float>(), dq.data_ptr<float>(), K,
                                                  dsum.data_ptr<float>(), current_stream(q));
            check_status(st, "isplib_mha_bw_rows_hip");
         }
         if (need_q) grad_q = dq;
         if (need_k || need_v) {
            TORCH_CHECK(K == 0 || (isplib_mha_serves(M, heads, K / heads, qo.ld) && isplib_mha_serves(M, heads, K / heads, go.ld)),
                        "isplib: mha_spmm backward: outside isplib_mha_serves for the gathered rows of q and of the gradient: M = ", M,
                        ", K = ", K);
            Tensor dk = at::empty({N, K}, q.options()), dv = at::empty({N, K}, q.options());
            if (N > 0 && K > 0) {
               const int st = isplib_mha_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                     colptr.data_ptr<int64_t>() + 1, heads, p, nnz > 0 ? qo.t.data_ptr<float>() : nullptr, qo.ld,
                                                     nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld, lse.data_ptr<float>(),
                                                     dsum.data_ptr<float>(), ko.t.data_ptr<float>(), ko.ld, vo.t.data_ptr<float>(), vo.ld,
                                                     dk.data_ptr<float>(), K, dv.data_ptr<float>(), K, current_stream(q));
               check_status(st, "isplib_mha_bw_cols_hip");
            }
            if (need_k) grad_k = dk;
            if (need_v) grad_v = dv;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_q, grad_k, grad_v, Variable(), Variable()};
   }
};

Tensor mha_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int64_t heads, double scale) {
   return MhaSpmm::apply(rowptr, col, colptr, row_t, q, k, v, heads, scale)[0];
}

// ---- the same attention with attention dropout (isplib_qkv_drop_*_hip) ----------
// The coefficients are dropped after the softmax, per stored entry and head; the keep bit is the pure function of (seed, CSR position,
// head) of gat_drop_spmm, so the backward regenerates the mask from the seed.  Saved for backward: what MhaSpmm saves, plus the three
// scalars (threshold, keep scale, seed) and csr2csc (the columns kernel walks the transposed structure) -- nothing of length nnz that
// the call did not receive.  The columns kernel runs only when k or v asks for a gradient.
class MhaDropSpmm : public torch::autograd::Function<MhaDropSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable csr2csc,
                                Variable q, Variable k, Variable v, int64_t heads, double scale, double p, int64_t seed) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      check_index(csr2csc, "csr2csc");
      TORCH_CHECK(q.defined() && q.dim() == 2 && k.defined() && k.dim() == 2 && v.defined() && v.dim() == 2,
                  "isplib: mha_drop_spmm needs 2-D `q` [M, heads * d], `k` and `v` [N, heads * d]");
      TORCH_CHECK(p > 0.0 && p < 1.0, "isplib: mha_drop_spmm: `p` must lie in (0, 1), got ", p, " (p == 0: mha_spmm)");
      TORCH_CHECK(seed >= 0, "isplib: mha_drop_spmm: `seed` must be a non-negative int64, got ", seed);
      OpTimer timer("FUSEDMM_MHA_DROP_FW", q);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz && csr2csc.numel() == nnz,
                  "isplib: mha_drop_spmm: `rowptr` / `colptr` need one entry more than rows / columns, `row_t` and `csr2csc` one entry per "
                  "stored entry (", nnz, "), got ", row_t.numel(), " and ", csr2csc.numel());
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: mha_drop_spmm: the width of `q` (", K, ") must be heads * d, got heads = ", heads);
      TORCH_CHECK(std::isfinite(scale), "isplib: mha_drop_spmm: `scale` must be a finite number, got ", scale);
      const AttnOperand qo = mha_operand(q, "q", M, K), ko = mha_operand(k, "k", N, K), vo = mha_operand(v, "v", N, K);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &csr2csc, &k, &v})
         TORCH_CHECK(t->device() == q.device(), "isplib: mha_drop_spmm: every operand must be on q's device");
      TORCH_CHECK(K == 0 || (isplib_mha_serves(N, heads, K / heads, ko.ld) && isplib_mha_serves(N, heads, K / heads, vo.ld)),
                  "isplib: mha_drop_spmm: outside isplib_mha_serves (heads * d <= ", ISPLIB_GAT_K_MAX,
                  ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ", heads, ", d = ",
                  K / heads, ", pitches = ", ko.ld, ", ", vo.ld);
      TORCH_CHECK(nnz < (1LL << 31), "isplib: mha_drop_spmm: the keep bit is defined for CSR positions below 2^31, got nnz = ", nnz);
      const uint32_t threshold = isplib_gat_drop_threshold(p);
      const float keep_scale = (float)(1.0 / (1.0 - p));
      c10::DeviceGuard guard(q.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, q.options()), lse = at::empty({M, heads}, q.options());
      if (M > 0 && K > 0) {
         const int st = isplib_qkv_drop_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                heads, (float)scale, qo.t.data_ptr<float>(), qo.ld,
                                                nnz > 0 ? ko.t.data_ptr<float>() : nullptr, ko.ld,
                                                nnz > 0 ? vo.t.data_ptr<float>() : nullptr, vo.ld, z.data_ptr<float>(), K,
                                                lse.data_ptr<float>(), current_stream(q), threshold, keep_scale, (uint64_t)seed);
         check_status(st, "isplib_qkv_drop_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["scale"] = scale;
      ctx->saved_data["threshold"] = (int64_t)threshold;
      ctx->saved_data["keep_scale"] = (double)keep_scale;
      ctx->saved_data["seed"] = seed;
      ctx->save_for_backward({rp, cl, colptr, row_t, q, k, v, z, lse, csr2csc});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_MHA_DROP_BW", grad_outs[0]);
      const bool need_q = ctx->needs_input_grad(5), need_k = ctx->needs_input_grad(6), need_v = ctx->needs_input_grad(7);
      auto grad_q = Variable(), grad_k = Variable(), grad_v = Variable();
      if (need_q || need_k || need_v) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), q = saved[4], k = saved[5], v = saved[6],
              z = saved[7], lse = saved[8];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ps = (float)ctx->saved_data["scale"].toDouble();
         const uint32_t threshold = (uint32_t)ctx->saved_data["threshold"].toInt();
         const float keep_scale = (float)ctx->saved_data["keep_scale"].toDouble();
         const uint64_t seed = (uint64_t)ctx->saved_data["seed"].toInt();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = cl.numel();
         const AttnOperand qo = mha_operand(q, "q", M, K), ko = mha_operand(k, "k", N, K), vo = mha_operand(v, "v", N, K);
         const AttnOperand go = mha_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(q.device());
         // as in MhaSpmm: the rows kernel always runs (D feeds the columns kernel), the columns kernel only when k or v asks
         Tensor dq = at::empty({M, K}, q.options()), dsum = at::empty({M, heads}, q.options());
         if (M > 0 && K > 0) {
            const int st = isplib_qkv_drop_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                       rp.data_ptr<int64_t>() + 1, heads, ps, qo.t.data_ptr<float>(), qo.ld,
                                                       nnz > 0 ? ko.t.data_ptr<float>() : nullptr, ko.ld,
                                                       nnz > 0 ? vo.t.data_ptr<float>() : nullptr, vo.ld, go.t.data_ptr<float>(), go.ld,
                                                       z.data_ptr<float>(), K, lse.data_ptr<float>(), dq.data_ptr<float>(), K,
                                                       dsum.data_ptr<float>(), current_stream(q), threshold, keep_scale, seed);
            check_status(st, "isplib_qkv_drop_bw_rows_hip");
         }
         if (need_q) grad_q = dq;
         if (need_k || need_v) {
            TORCH_CHECK(K == 0 || (isplib_mha_serves(M, heads, K / heads, qo.ld) && isplib_mha_serves(M, heads, K / heads, go.ld)),
                        "isplib: mha_drop_spmm backward: outside isplib_mha_serves for the gathered rows of q and of the gradient: M = ", M,
                        ", K = ", K);
            const Tensor pos = saved[9].contiguous();
            Tensor dk = at::empty({N, K}, q.options()), dv = at::empty({N, K}, q.options());
            if (N > 0 && K > 0) {
               const int st = isplib_qkv_drop_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                          colptr.data_ptr<int64_t>() + 1, nnz > 0 ? pos.data_ptr<int64_t>() : nullptr, heads,
                                                          ps, nnz > 0 ? qo.t.data_ptr<float>() : nullptr, qo.ld,
                                                          nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld, lse.data_ptr<float>(),
                                                          dsum.data_ptr<float>(), ko.t.data_ptr<float>(), ko.ld, vo.t.data_ptr<float>(), vo.ld,
                                                          dk.data_ptr<float>(), K, dv.data_ptr<float>(), K, current_stream(q), threshold,
                                                          keep_scale, seed);
               check_status(st, "isplib_qkv_drop_bw_cols_hip");
            }
            if (need_k) grad_k = dk;
            if (need_v) grad_v = dv;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), Variable(), grad_q, grad_k, grad_v, Variable(), Variable(), Variable(),
              Variable()};
   }
};

Tensor mha_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, int64_t heads,
                     double scale, double p, int64_t seed) {
   return MhaDropSpmm::apply(rowptr, col, colptr, row_t, csr2csc, q, k, v, heads, scale, p, seed)[0];
}

// ---- the GATv2 aggregation with attention dropout (isplib_gatv2_drop_*_hip) ----------
// The coefficients are dropped after the softmax, per stored entry and head; the keep bit is the pure function of (seed, CSR position,
// head) of gat_drop_spmm, so the backward regenerates the mask from the seed.  Saved for backward: what Gatv2Spmm saves, plus the two
// scalars p and seed and csr2csc (the columns kernel walks the transposed structure).  Only the kernels whose gradients are asked for run.
class Gatv2DropSpmm : public torch::autograd::Function<Gatv2DropSpmm> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable csr2csc,
                                Variable x, Variable y, Variable att, int64_t heads, double negative_slope, double p, int64_t seed) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      check_index(csr2csc, "csr2csc");
      TORCH_CHECK(x.defined() && x.dim() == 2 && y.defined() && y.dim() == 2, "isplib: gatv2_drop_spmm needs 2-D `x` [M, heads * d] and "
                                                                              "`y` [N, heads * d]");
      TORCH_CHECK(p > 0.0 && p < 1.0, "isplib: gatv2_drop_spmm: `p` must lie in (0, 1), got ", p, " (p == 0: gatv2_spmm)");
      TORCH_CHECK(seed >= 0, "isplib: gatv2_drop_spmm: `seed` must be a non-negative int64, got ", seed);
      OpTimer timer("FUSEDMM_GATV2_DROP_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz && csr2csc.numel() == nnz,
                  "isplib: gatv2_drop_spmm: `rowptr` / `colptr` need one entry more than rows / columns, `row_t` and `csr2csc` one entry per "
                  "stored entry (", nnz, "), got ", row_t.numel(), " and ", csr2csc.numel());
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gatv2_drop_spmm: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const AttnOperand xo = gatv2_operand(x, "x", M, K), yo = gatv2_operand(y, "y", N, K);
      TORCH_CHECK(att.defined(), "isplib: gatv2_drop_spmm needs `att` [heads, d]");
      const Tensor av = gatv2_att(att, heads, K / heads);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &csr2csc, &x, &att})
         TORCH_CHECK(t->device() == y.device(), "isplib: gatv2_drop_spmm: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gatv2_serves(N, heads, K / heads, yo.ld), "isplib: gatv2_drop_spmm: outside isplib_gatv2_serves (heads * d "
                  "<= ", ISPLIB_GAT_K_MAX, ", heads == 1 or d a power of two >= 4, N < 2^31, N * pitch * 4 <= 3.5 GiB): N = ", N, ", heads = ",
                  heads, ", d = ", K / heads, ", pitch = ", yo.ld);
      TORCH_CHECK(nnz < (1LL << 31), "isplib: gatv2_drop_spmm: the keep bit is defined for CSR positions below 2^31, got nnz = ", nnz);
      c10::DeviceGuard guard(y.device());
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options());
      if (M > 0 && K > 0) {
         const int st = isplib_gatv2_drop_csr_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                  xo.t.data_ptr<float>(), xo.ld, nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld,
                                                  av.data_ptr<float>(), heads, (float)negative_slope, z.data_ptr<float>(), K,
                                                  lse.data_ptr<float>(), current_stream(y), isplib_gat_drop_threshold(p),
                                                  (float)(1.0 / (1.0 - p)), (uint64_t)seed);
         check_status(st, "isplib_gatv2_drop_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->saved_data["p"] = p;
      ctx->saved_data["seed"] = seed;
      ctx->save_for_backward({rp, cl, colptr, row_t, x, y, att, z, lse, csr2csc});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GATV2_DROP_BW", grad_outs[0]);
      const bool need_x = ctx->needs_input_grad(5), need_y = ctx->needs_input_grad(6), need_att = ctx->needs_input_grad(7);
      auto grad_x = Variable(), grad_y = Variable(), grad_att = Variable();
      if (need_x || need_y || need_att) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), x = saved[4], y = saved[5], z = saved[7],
              lse = saved[8];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const double p = ctx->saved_data["p"].toDouble();
         const uint32_t threshold = isplib_gat_drop_threshold(p);
         const float scale = (float)(1.0 / (1.0 - p));
         const uint64_t seed = (uint64_t)ctx->saved_data["seed"].toInt();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const AttnOperand xo = gatv2_operand(x, "x", M, K), yo = gatv2_operand(y, "y", N, K);
         const Tensor av = gatv2_att(saved[6], heads, K / heads);
         const AttnOperand go = gatv2_operand(grad_outs[0].to(at::kFloat), "grad_out", M, K);
         c10::DeviceGuard guard(y.device());
         // as in Gatv2Spmm: the rows kernel always runs (D feeds the columns kernel), its datt instantiation only when att asks, the
         // columns kernel only when y asks
         Tensor dx = at::empty({M, K}, y.options()), dsum = at::empty({M, heads}, y.options());
         Tensor datt = need_att ? at::empty({heads, K / heads}, y.options()) : Tensor();
         if (M > 0 && K > 0) {
            const size_t ws = need_att ? isplib_gatv2_bw_rows_workspace_bytes(M, K) : 0;
            Tensor work = need_att ? at::empty({(int64_t)ws}, y.options().dtype(at::kByte)) : Tensor();
            const int st = isplib_gatv2_drop_bw_rows_hip(M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                         rp.data_ptr<int64_t>() + 1, xo.t.data_ptr<float>(), xo.ld,
                                                         nnz > 0 ? yo.t.data_ptr<float>() : nullptr, yo.ld, av.data_ptr<float>(), heads, ns,
                                                         go.t.data_ptr<float>(), go.ld, z.data_ptr<float>(), K, lse.data_ptr<float>(),
                                                         dx.data_ptr<float>(), K, dsum.data_ptr<float>(),
                                                         need_att ? datt.data_ptr<float>() : nullptr, need_att ? work.data_ptr() : nullptr, ws,
                                                         current_stream(y), threshold, scale, seed);
            check_status(st, "isplib_gatv2_drop_bw_rows_hip");
         } else if (need_att) {
            datt.zero_();
         }
         if (need_x) grad_x = dx;
         if (need_att) grad_att = datt;
         if (need_y) {
            TORCH_CHECK(K == 0 || (isplib_gatv2_serves(M, heads, K / heads, xo.ld) && isplib_gatv2_serves(M, heads, K / heads, go.ld)),
                        "isplib: gatv2_drop_spmm backward: outside isplib_gatv2_serves for the gathered rows of x and of the gradient: M = ",
                        M, ", K = ", K);
            const Tensor pos = saved[9].contiguous();
            Tensor dy = at::empty({N, K}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gatv2_drop_bw_cols_hip(M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                            colptr.data_ptr<int64_t>() + 1, nnz > 0 ? pos.data_ptr<int64_t>() : nullptr,
                                                            nnz > 0 ? xo.t.data_ptr<float>() : nullptr, xo.ld, yo.t.data_ptr<float>(), yo.ld,
                                                            av.data_ptr<float>(), heads, ns, nnz > 0 ? go.t.data_ptr<float>() : nullptr, go.ld,
                                                            lse.data_ptr<float>(), dsum.data_ptr<float>(), dy.data_ptr<float>(), K,
                                                            current_stream(y), threshold, scale, seed);
               check_status(st, "isplib_gatv2_drop_bw_cols_hip");
            }
            grad_y = dy;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), Variable(), grad_x, grad_y, grad_att, Variable(), Variable(), Variable(),
              Variable()};
   }
};

Tensor gatv2_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor x, Tensor y, Tensor att, int64_t heads,
                       double negative_slope, double p, int64_t seed) {
   return Gatv2DropSpmm::apply(rowptr, col, colptr, row_t, csr2csc, x, y, att, heads, negative_slope, p, seed)[0];
}

// ---- the GATv2 aggregation for bf16 / fp16 `x` and `y` (isplib_gatv2_16_*_hip) ----------
// x and y go in as they lie, z, dx and dy come back in their dtype; att, lse, D and datt stay fp32: no fp32 [*, K] tensor in either
// direction.  Saved for backward: the structure, x, y, att and lse -- NOT z: the rows kernel forms D[i,h] from the row's edges.  A wide
// operand is copied only without unit inner stride, or where the domain admits it packed but not at its pitch or alignment.
static AttnOperand gatv2_16_operand(const Tensor &src, const char *name, int64_t rows, int64_t k, int64_t heads, at::ScalarType dtype) {
   TORCH_CHECK(src.defined() && src.scalar_type() == dtype, "isplib: gatv2_spmm16: `", name, "` must be ", dtype, ", got ",
               src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: gatv2_spmm16: `", name, "` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: gatv2_spmm16: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   if (rows == 0 || k == 0) return {src, std::max<int64_t>(k, 1)};
   const int64_t ld = rows > 1 ? src.stride(0) : k;
   const bool as_is = src.stride(1) == 1 && ld >= k && ((uintptr_t)src.data_ptr() & 3) == 0 && isplib_gatv2_16_serves(rows, heads, k / heads, ld);
   if (as_is) return {src, ld};
   return {src.clone(at::MemoryFormat::Contiguous), k};
}

static Tensor gatv2_16_att(const Tensor &src, int64_t heads, int64_t d) {
   TORCH_CHECK(src.defined() && src.scalar_type() == at::kFloat, "isplib: gatv2_spmm16: `att` must be float32 (att stays fp32), got ",
               src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: gatv2_spmm16: `att` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == heads && src.size(1) == d, "isplib: gatv2_spmm16: `att` must be [", heads, ", ", d,
               "] (heads x d), got ", src.sizes());
   return src.contiguous();
}

class Gatv2Spmm16 : public torch::autograd::Function<Gatv2Spmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable x, Variable y,
                                Variable att, int64_t heads, double negative_slope) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(x.defined() && x.dim() == 2 && y.defined() && y.dim() == 2, "isplib: gatv2_spmm16 needs 2-D `x` [M, heads * d] and `y` "
                                                                              "[N, heads * d]");
      TORCH_CHECK(is_half(y), "isplib: gatv2_spmm16: `y` must be bfloat16 or float16, got ", y.scalar_type(), " (float32: gatv2_spmm)");
      OpTimer timer("FUSEDMM_GATV2_FW", y);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: gatv2_spmm16: `rowptr` / `colptr` need one entry more than rows / "
                                                             "columns, `row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: gatv2_spmm16: the width of `y` (", K, ") must be heads * d, got heads = ", heads);
      const at::ScalarType dt = y.scalar_type();
      const AttnOperand yo = gatv2_16_operand(y, "y", N, K, heads, dt), xo = gatv2_16_operand(x, "x", M, K, heads, dt);
      TORCH_CHECK(att.defined(), "isplib: gatv2_spmm16 needs `att` [heads, d]");
      const Tensor av = gatv2_16_att(att, heads, K / heads);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &x, &att})
         TORCH_CHECK(t->device() == y.device(), "isplib: gatv2_spmm16: every operand must be on y's device");
      TORCH_CHECK(K == 0 || isplib_gatv2_16_serves(N, heads, K / heads, yo.ld), "isplib: gatv2_spmm16: outside isplib_gatv2_16_serves (",
                  ISPLIB_GAT16_K_MIN, " <= heads * d <= ", ISPLIB_GAT16_K_MAX, ", heads == 1 with d even or d a power of two >= 8, N < 2^31, "
                  "N * pitch * 2 <= 3.5 GiB): N = ", N, ", heads = ", heads, ", d = ", K / heads, ", pitch = ", yo.ld);
      c10::DeviceGuard guard(y.device());
      const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, y.options()), lse = at::empty({M, heads}, y.options().dtype(at::kFloat));
      if (M > 0 && K > 0) {
         const int st = isplib_gatv2_16_csr_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                                xo.t.data_ptr(), xo.ld, nnz > 0 ? yo.t.data_ptr() : nullptr, yo.ld, av.data_ptr<float>(), heads,
                                                (float)negative_slope, z.data_ptr(), K, lse.data_ptr<float>(), current_stream(y));
         check_status(st, "isplib_gatv2_16_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["negative_slope"] = negative_slope;
      ctx->save_for_backward({rp, cl, colptr, row_t, x, y, att, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_GATV2_BW", grad_outs[0]);
      const bool need_x = ctx->needs_input_grad(4), need_y = ctx->needs_input_grad(5), need_att = ctx->needs_input_grad(6);
      auto grad_x = Variable(), grad_y = Variable(), grad_att = Variable();
      if (need_x || need_y || need_att) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), x = saved[4], y = saved[5], lse = saved[7];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ns = (float)ctx->saved_data["negative_slope"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = y.size(1), nnz = cl.numel();
         const at::ScalarType dt = y.scalar_type();
         const AttnOperand yo = gatv2_16_operand(y, "y", N, K, heads, dt), xo = gatv2_16_operand(x, "x", M, K, heads, dt);
         const Tensor av = gatv2_16_att(saved[6], heads, K / heads);
         const AttnOperand go = gatv2_16_operand(grad_outs[0].to(dt), "grad_out", M, K, heads, dt);   // a grad of another dtype is cast to y's
         c10::DeviceGuard guard(y.device());
         const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
         const auto f32 = y.options().dtype(at::kFloat);
         // the rows kernel always runs: its D[i,h] feeds the columns kernel; its datt instantiation and workspace only when att asks; the
         // columns kernel only when y asks
         Tensor dx = at::empty({M, K}, y.options()), dsum = at::empty({M, heads}, f32);
         Tensor datt = need_att ? at::empty({heads, K / heads}, f32) : Tensor();
         if (M > 0 && K > 0) {
            const size_t ws = need_att ? isplib_gatv2_16_bw_rows_workspace_bytes(M, K) : 0;
            Tensor work = need_att ? at::empty({(int64_t)ws}, y.options().dtype(at::kByte)) : Tensor();
            const int st = isplib_gatv2_16_bw_rows_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                       rp.data_ptr<int64_t>() + 1, xo.t.data_ptr(), xo.ld, nnz > 0 ? yo.t.data_ptr() : nullptr, yo.ld,
                                                       av.data_ptr<float>(), heads, ns, go.t.data_ptr(), go.ld, lse.data_ptr<float>(), dx.data_ptr(), K,
                                                       dsum.data_ptr<float>(), need_att ? datt.data_ptr<float>() : nullptr,
                                                       need_att ? work.data_ptr() : nullptr, ws, current_stream(y));
            check_status(st, "isplib_gatv2_16_bw_rows_hip");
         } else if (need_att) {
            datt.zero_();
         }
         if (need_x) grad_x = dx;
         if (need_att) grad_att = datt;
         if (need_y) {
            TORCH_CHECK(K == 0 || (isplib_gatv2_16_serves(M, heads, K / heads, xo.ld) && isplib_gatv2_16_serves(M, heads, K / heads, go.ld)),
                        "isplib: gatv2_spmm16 backward: outside isplib_gatv2_16_serves for the gathered rows of x and of the gradient: M = ", M,
                        ", K = ", K);
            Tensor dy = at::empty({N, K}, y.options());
            if (N > 0 && K > 0) {
               const int st = isplib_gatv2_16_bw_cols_hip(code, M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                          colptr.data_ptr<int64_t>() + 1, nnz > 0 ? xo.t.data_ptr() : nullptr, xo.ld, yo.t.data_ptr(),
                                                          yo.ld, av.data_ptr<float>(), heads, ns, nnz > 0 ? go.t.data_ptr() : nullptr, go.ld,
                                                          lse.data_ptr<float>(), dsum.data_ptr<float>(), dy.data_ptr(), K, current_stream(y));
               check_status(st, "isplib_gatv2_16_bw_cols_hip");
            }
            grad_y = dy;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_x, grad_y, grad_att, Variable(), Variable()};
   }
};

Tensor gatv2_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, Tensor att, int64_t heads,
                    double negative_slope) {
   return Gatv2Spmm16::apply(rowptr, col, colptr, row_t, x, y, att, heads, negative_slope)[0];
}

// ---- sparse multi-head attention (q, k, v) for bf16 / fp16 operands (isplib_qkv16_*_hip) ----------
// q, k and v go in as they lie, z, dq, dk and dv come back in their dtype; lse and D stay fp32: no fp32 [*, K] tensor in either
// direction.  Saved for backward: the structure, q, k, v and lse -- NOT z: the rows kernel forms D[i,h] from the row's edges -- and
// nothing of length nnz.  Operands with unit column stride go in at their own even pitch (the three column blocks of one fused 16-bit
// [rows, 3K] projection are not copied); anything else is made contiguous.  Every shape, dtype, device and domain check comes before
// a launch.
static AttnOperand mha16_operand(const Tensor &src, const char *name, int64_t rows, int64_t k, int64_t heads, at::ScalarType dtype) {
   TORCH_CHECK(src.defined() && src.scalar_type() == dtype, "isplib: mha_spmm16: `", name, "` must be ", dtype, " (q, k and v of one "
               "16-bit dtype), got ", src.defined() ? src.scalar_type() : at::ScalarType::Undefined);
   TORCH_CHECK(src.is_cuda(), "isplib: mha_spmm16: `", name, "` must be a GPU tensor -- there is no CPU path");
   TORCH_CHECK(src.dim() == 2 && src.size(0) == rows && src.size(1) == k, "isplib: mha_spmm16: `", name, "` must be [", rows, ", ", k,
               "], got ", src.sizes());
   if (rows == 0 || k == 0) return {src, std::max<int64_t>(k, 1)};
   const int64_t ld = rows > 1 ? src.stride(0) : k;
   const bool as_is = src.stride(1) == 1 && ld >= k && ((uintptr_t)src.data_ptr() & 3) == 0 && isplib_qkv16_serves(rows, heads, k / heads, ld);
   if (as_is) return {src, ld};
   return {src.clone(at::MemoryFormat::Contiguous), k};
}

class MhaSpmm16 : public torch::autograd::Function<MhaSpmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable q, Variable k,
                                Variable v, int64_t heads, double scale) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      TORCH_CHECK(q.defined() && q.dim() == 2 && k.defined() && k.dim() == 2 && v.defined() && v.dim() == 2,
                  "isplib: mha_spmm16 needs 2-D `q` [M, heads * d], `k` and `v` [N, heads * d]");
      TORCH_CHECK(is_half(q), "isplib: mha_spmm16: `q` must be bfloat16 or float16, got ", q.scalar_type(), " (float32: mha_spmm)");
      OpTimer timer("FUSEDMM_MHA_FW", q);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz, "isplib: mha_spmm16: `rowptr` / `colptr` need one entry more than rows / "
                                                             "columns, `row_t` one entry per stored entry");
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: mha_spmm16: the width of `q` (", K, ") must be heads * d, got heads = ", heads);
      TORCH_CHECK(std::isfinite(scale), "isplib: mha_spmm16: `scale` must be a finite number, got ", scale);
      const at::ScalarType dt = q.scalar_type();
      const AttnOperand qo = mha16_operand(q, "q", M, K, heads, dt), ko = mha16_operand(k, "k", N, K, heads, dt),
                        vo = mha16_operand(v, "v", N, K, heads, dt);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &k, &v})
         TORCH_CHECK(t->device() == q.device(), "isplib: mha_spmm16: every operand must be on q's device");
      TORCH_CHECK(K == 0 || (isplib_qkv16_serves(N, heads, K / heads, ko.ld) && isplib_qkv16_serves(N, heads, K / heads, vo.ld) &&
                             qo.ld % 2 == 0),
                  "isplib: mha_spmm16: outside isplib_qkv16_serves (", ISPLIB_GAT16_K_MIN, " <= heads * d <= ", ISPLIB_GAT16_K_MAX,
                  ", heads == 1 with d even or d a power of two >= 8, N < 2^31, N * pitch * 2 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitches = ", ko.ld, ", ", vo.ld);
      c10::DeviceGuard guard(q.device());
      const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, q.options()), lse = at::empty({M, heads}, q.options().dtype(at::kFloat));
      if (M > 0 && K > 0) {
         const int st = isplib_qkv16_csr_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(), rp.data_ptr<int64_t>() + 1,
                                             heads, (float)scale, qo.t.data_ptr(), qo.ld, nnz > 0 ? ko.t.data_ptr() : nullptr, ko.ld,
                                             nnz > 0 ? vo.t.data_ptr() : nullptr, vo.ld, z.data_ptr(), K, lse.data_ptr<float>(),
                                             current_stream(q));
         check_status(st, "isplib_qkv16_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["scale"] = scale;
      ctx->save_for_backward({rp, cl, colptr, row_t, q, k, v, lse});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_MHA_BW", grad_outs[0]);
      const bool need_q = ctx->needs_input_grad(4), need_k = ctx->needs_input_grad(5), need_v = ctx->needs_input_grad(6);
      auto grad_q = Variable(), grad_k = Variable(), grad_v = Variable();
      if (need_q || need_k || need_v) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), q = saved[4], k = saved[5], v = saved[6],
              lse = saved[7];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float p = (float)ctx->saved_data["scale"].toDouble();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = cl.numel();
         const at::ScalarType dt = q.scalar_type();
         const AttnOperand qo = mha16_operand(q, "q", M, K, heads, dt), ko = mha16_operand(k, "k", N, K, heads, dt),
                           vo = mha16_operand(v, "v", N, K, heads, dt);
         const AttnOperand go = mha16_operand(grad_outs[0].to(dt), "grad_out", M, K, heads, dt);   // a grad of another dtype is cast to q's
         c10::DeviceGuard guard(q.device());
         const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
         // the rows kernel always runs: its D[i,h] feeds the columns kernel; the columns kernel only when k or v asks
         Tensor dq = at::empty({M, K}, q.options()), dsum = at::empty({M, heads}, q.options().dtype(at::kFloat));
         if (M > 0 && K > 0) {
            const int st = isplib_qkv16_bw_rows_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                    rp.data_ptr<int64_t>() + 1, heads, p, qo.t.data_ptr(), qo.ld,
                                                    nnz > 0 ? ko.t.data_ptr() : nullptr, ko.ld, nnz > 0 ? vo.t.data_ptr() : nullptr, vo.ld,
                                                    go.t.data_ptr(), go.ld, lse.data_ptr<float>(), dq.data_ptr(), K, dsum.data_ptr<float>(),
                                                    current_stream(q));
            check_status(st, "isplib_qkv16_bw_rows_hip");
         }
         if (need_q) grad_q = dq;
         if (need_k || need_v) {
            TORCH_CHECK(K == 0 || (isplib_qkv16_serves(M, heads, K / heads, qo.ld) && isplib_qkv16_serves(M, heads, K / heads, go.ld)),
                        "isplib: mha_spmm16 backward: outside isplib_qkv16_serves for the gathered rows of q and of the gradient: M = ", M,
                        ", K = ", K);
            Tensor dk = at::empty({N, K}, q.options()), dv = at::empty({N, K}, q.options());
            if (N > 0 && K > 0) {
               const int st = isplib_qkv16_bw_cols_hip(code, M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                       colptr.data_ptr<int64_t>() + 1, heads, p, nnz > 0 ? qo.t.data_ptr() : nullptr, qo.ld,
                                                       nnz > 0 ? go.t.data_ptr() : nullptr, go.ld, lse.data_ptr<float>(),
                                                       dsum.data_ptr<float>(), ko.t.data_ptr(), ko.ld, vo.t.data_ptr(), vo.ld, dk.data_ptr(), K,
                                                       dv.data_ptr(), K, current_stream(q));
               check_status(st, "isplib_qkv16_bw_cols_hip");
            }
            if (need_k) grad_k = dk;
            if (need_v) grad_v = dv;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), grad_q, grad_k, grad_v, Variable(), Variable()};
   }
};

Tensor mha_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int64_t heads, double scale) {
   return MhaSpmm16::apply(rowptr, col, colptr, row_t, q, k, v, heads, scale)[0];
}

// ---- the same 16-bit attention with attention dropout (isplib_qkv_half_drop_*_hip) ----------
// MhaSpmm16 with the keep bit of MhaDropSpmm: the checks of both, the operands as they lie (mha16_operand), z, dq, dk and dv in their
// dtype, lse and D fp32.  Saved for backward: the structure, q, k, v, lse, csr2csc and the three scalars (threshold, keep scale, seed)
// -- NOT z, and nothing of length nnz that the call did not receive.  The columns kernel runs only when k or v asks for a gradient.
class MhaDropSpmm16 : public torch::autograd::Function<MhaDropSpmm16> {
 public:
   static variable_list forward(AutogradContext *ctx, Variable rowptr, Variable col, Variable colptr, Variable row_t, Variable csr2csc,
                                Variable q, Variable k, Variable v, int64_t heads, double scale, double p, int64_t seed) {
      check_index(rowptr, "rowptr"); check_index(col, "col"); check_index(colptr, "colptr"); check_index(row_t, "row_t");
      check_index(csr2csc, "csr2csc");
      TORCH_CHECK(q.defined() && q.dim() == 2 && k.defined() && k.dim() == 2 && v.defined() && v.dim() == 2,
                  "isplib: mha_drop_spmm16 needs 2-D `q` [M, heads * d], `k` and `v` [N, heads * d]");
      TORCH_CHECK(is_half(q), "isplib: mha_drop_spmm16: `q` must be bfloat16 or float16, got ", q.scalar_type(), " (float32: mha_drop_spmm)");
      TORCH_CHECK(p > 0.0 && p < 1.0, "isplib: mha_drop_spmm16: `p` must lie in (0, 1), got ", p, " (p == 0: mha_spmm16)");
      TORCH_CHECK(seed >= 0, "isplib: mha_drop_spmm16: `seed` must be a non-negative int64, got ", seed);
      OpTimer timer("FUSEDMM_MHA_DROP_FW", q);
      const int64_t M = rowptr.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = col.numel();
      TORCH_CHECK(M >= 0 && N >= 0 && row_t.numel() == nnz && csr2csc.numel() == nnz,
                  "isplib: mha_drop_spmm16: `rowptr` / `colptr` need one entry more than rows / columns, `row_t` and `csr2csc` one entry per "
                  "stored entry (", nnz, "), got ", row_t.numel(), " and ", csr2csc.numel());
      TORCH_CHECK(heads >= 1 && K % heads == 0, "isplib: mha_drop_spmm16: the width of `q` (", K, ") must be heads * d, got heads = ", heads);
      TORCH_CHECK(std::isfinite(scale), "isplib: mha_drop_spmm16: `scale` must be a finite number, got ", scale);
      const at::ScalarType dt = q.scalar_type();
      const AttnOperand qo = mha16_operand(q, "q", M, K, heads, dt), ko = mha16_operand(k, "k", N, K, heads, dt),
                        vo = mha16_operand(v, "v", N, K, heads, dt);
      for (const Tensor *t : {&rowptr, &col, &colptr, &row_t, &csr2csc, &k, &v})
         TORCH_CHECK(t->device() == q.device(), "isplib: mha_drop_spmm16: every operand must be on q's device");
      TORCH_CHECK(K == 0 || (isplib_qkv16_serves(N, heads, K / heads, ko.ld) && isplib_qkv16_serves(N, heads, K / heads, vo.ld) &&
                             qo.ld % 2 == 0),
                  "isplib: mha_drop_spmm16: outside isplib_qkv16_serves (", ISPLIB_GAT16_K_MIN, " <= heads * d <= ", ISPLIB_GAT16_K_MAX,
                  ", heads == 1 with d even or d a power of two >= 8, N < 2^31, N * pitch * 2 <= 3.5 GiB): N = ", N, ", heads = ", heads,
                  ", d = ", K / heads, ", pitches = ", ko.ld, ", ", vo.ld);
      TORCH_CHECK(nnz < (1LL << 31), "isplib: mha_drop_spmm16: the keep bit is defined for CSR positions below 2^31, got nnz = ", nnz);
      const uint32_t threshold = isplib_gat_drop_threshold(p);
      const float keep_scale = (float)(1.0 / (1.0 - p));
      c10::DeviceGuard guard(q.device());
      const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
      const Tensor rp = rowptr.contiguous(), cl = col.contiguous();
      Tensor z = at::empty({M, K}, q.options()), lse = at::empty({M, heads}, q.options().dtype(at::kFloat));
      if (M > 0 && K > 0) {
         const int st = isplib_qkv_half_drop_csr_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                     rp.data_ptr<int64_t>() + 1, heads, (float)scale, qo.t.data_ptr(), qo.ld,
                                                     nnz > 0 ? ko.t.data_ptr() : nullptr, ko.ld, nnz > 0 ? vo.t.data_ptr() : nullptr, vo.ld,
                                                     z.data_ptr(), K, lse.data_ptr<float>(), current_stream(q), threshold, keep_scale,
                                                     (uint64_t)seed);
         check_status(st, "isplib_qkv_half_drop_csr_hip");
      } else if (M > 0) {
         lse.fill_(-std::numeric_limits<float>::infinity());
      }
      ctx->saved_data["heads"] = heads;
      ctx->saved_data["scale"] = scale;
      ctx->saved_data["threshold"] = (int64_t)threshold;
      ctx->saved_data["keep_scale"] = (double)keep_scale;
      ctx->saved_data["seed"] = seed;
      ctx->save_for_backward({rp, cl, colptr, row_t, q, k, v, lse, csr2csc});
      return {z};
   }

   static variable_list backward(AutogradContext *ctx, variable_list grad_outs) {
      OpTimer timer("FUSEDMM_MHA_DROP_BW", grad_outs[0]);
      const bool need_q = ctx->needs_input_grad(5), need_k = ctx->needs_input_grad(6), need_v = ctx->needs_input_grad(7);
      auto grad_q = Variable(), grad_k = Variable(), grad_v = Variable();
      if (need_q || need_k || need_v) {
         auto saved = ctx->get_saved_variables();
         auto rp = saved[0], cl = saved[1], colptr = saved[2].contiguous(), row_t = saved[3].contiguous(), q = saved[4], k = saved[5], v = saved[6],
              lse = saved[7];
         const int64_t heads = ctx->saved_data["heads"].toInt();
         const float ps = (float)ctx->saved_data["scale"].toDouble();
         const uint32_t threshold = (uint32_t)ctx->saved_data["threshold"].toInt();
         const float keep_scale = (float)ctx->saved_data["keep_scale"].toDouble();
         const uint64_t seed = (uint64_t)ctx->saved_data["seed"].toInt();
         const int64_t M = rp.numel() - 1, N = colptr.numel() - 1, K = q.size(1), nnz = cl.numel();
         const at::ScalarType dt = q.scalar_type();
         const AttnOperand qo = mha16_operand(q, "q", M, K, heads, dt), ko = mha16_operand(k, "k", N, K, heads, dt),
                           vo = mha16_operand(v, "v", N, K, heads, dt);
         const AttnOperand go = mha16_operand(grad_outs[0].to(dt), "grad_out", M, K, heads, dt);   // a grad of another dtype is cast to q's
         c10::DeviceGuard guard(q.device());
         const int code = dt == at::kBFloat16 ? ISPLIB_DTYPE_BF16 : ISPLIB_DTYPE_F16;
         // as in MhaSpmm16: the rows kernel always runs (D feeds the columns kernel), the columns kernel only when k or v asks
         Tensor dq = at::empty({M, K}, q.options()), dsum = at::empty({M, heads}, q.options().dtype(at::kFloat));
         if (M > 0 && K > 0) {
            const int st = isplib_qkv_half_drop_bw_rows_hip(code, M, N, K, nnz, cl.data_ptr<int64_t>(), rp.data_ptr<int64_t>(),
                                                            rp.data_ptr<int64_t>() + 1, heads, ps, qo.t.data_ptr(), qo.ld,
                                                            nnz > 0 ? ko.t.data_ptr() : nullptr, ko.ld,
                                                            nnz > 0 ? vo.t.data_ptr() : nullptr, vo.ld, go.t.data_ptr(), go.ld,
                                                            lse.data_ptr<float>(), dq.data_ptr(), K, dsum.data_ptr<float>(),
                                                            current_stream(q), threshold, keep_scale, seed);
            check_status(st, "isplib_qkv_half_drop_bw_rows_hip");
         }
         if (need_q) grad_q = dq;
         if (need_k || need_v) {
            TORCH_CHECK(K == 0 || (isplib_qkv16_serves(M, heads, K / heads, qo.ld) && isplib_qkv16_serves(M, heads, K / heads, go.ld)),
                        "isplib: mha_drop_spmm16 backward: outside isplib_qkv16_serves for the gathered rows of q and of the gradient: M = ",
                        M, ", K = ", K);
            const Tensor pos = saved[8].contiguous();
            Tensor dk = at::empty({N, K}, q.options()), dv = at::empty({N, K}, q.options());
            if (N > 0 && K > 0) {
               const int st = isplib_qkv_half_drop_bw_cols_hip(code, M, N, K, nnz, row_t.data_ptr<int64_t>(), colptr.data_ptr<int64_t>(),
                                                               colptr.data_ptr<int64_t>() + 1, nnz > 0 ? pos.data_ptr<int64_t>() : nullptr,
                                                               heads, ps, nnz > 0 ? qo.t.data_ptr() : nullptr, qo.ld,
                                                               nnz > 0 ? go.t.data_ptr() : nullptr, go.ld, lse.data_ptr<float>(),
                                                               dsum.data_ptr<float>(), ko.t.data_ptr(), ko.ld, vo.t.data_ptr(), vo.ld,
                                                               dk.data_ptr(), K, dv.data_ptr(), K, current_stream(q), threshold, keep_scale,
                                                               seed);
               check_status(st, "isplib_qkv_half_drop_bw_cols_hip");
            }
            if (need_k) grad_k = dk;
            if (need_v) grad_v = dv;
         }
      }
      return {Variable(), Variable(), Variable(), Variable(), Variable(), grad_q, grad_k, grad_v, Variable(), Variable(), Variable(),
              Variable()};
   }
};

Tensor mha_drop_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, int64_t heads,
                       double scale, double p, int64_t seed) {
   return MhaDropSpmm16::apply(rowptr, col, colptr, row_t, csr2csc, q, k, v, heads, scale, p, seed)[0];
}

// introspection / housekeeping of the per-graph handle cache of the reference-schema operators
int64_t graph_cache_size() {
   std::lock_guard<std::mutex> lock(g_graph_mutex);
   return (int64_t)(g_graphs.size() + g_retired.size());
}
void graph_cache_clear() {
   std::lock_guard<std::mutex> lock(g_graph_mutex);
   for (auto &kv : g_graphs) isplib_graph_destroy(kv.second.handle);
   g_graphs.clear();
   destroy_retired_locked();
}

void performDummySpMM(int64_t flag) { performDummySpMM_hip(flag, (void *)c10::hip::getCurrentHIPStream().stream()); }

}  // namespace

// schemas as registered at csrc/fusedmm.cpp:565-570
TORCH_LIBRARY(isplib, m) {
   m.def("fusedmm_spmm(Tensor? row, Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor? csr2csc, "
         "Tensor mat, Tensor? value_index_select, Tensor? row_index_select) -> Tensor",
         &fusedmm_spmm_add);
   m.def("fusedmm_spmm_mean(Tensor? row, Tensor rowptr, Tensor col, Tensor? value, Tensor? rowcount, Tensor? colptr, "
         "Tensor? csr2csc, Tensor mat, Tensor? new_row, Tensor? new_rowcount) -> Tensor",
         &fusedmm_spmm_mean);
   m.def("fusedmm_spmm_max(Tensor rowptr, Tensor col, Tensor? value, Tensor mat) -> (Tensor, Tensor)",
         &fusedmm_spmm_max);
   m.def("fusedmm_spmm_min(Tensor rowptr, Tensor col, Tensor? value, Tensor mat) -> (Tensor, Tensor)",
         &fusedmm_spmm_min);
   m.def("performDummySpMM(int flag) -> ()", &performDummySpMM);
   m.def("graph_cache_size() -> int", &graph_cache_size);
   m.def("graph_cache_clear() -> ()", &graph_cache_clear);
   // additions (not in the reference): the same operators fed with per-graph schedule operands
   // (plan = [] | [sliceptr] | [task_row, task_b, task_len, seg_off, lane_off_cpu]; plan_t: the same for A^T)
   m.def("fusedmm_spmm_planned(Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor mat, Tensor? value_t, "
         "Tensor? row_t, Tensor[] plan, Tensor[] plan_t) -> Tensor",
         &fusedmm_spmm_planned);
   m.def("fusedmm_spmm_mean_planned(Tensor rowptr, Tensor col, Tensor? value, Tensor? colptr, Tensor mat, Tensor? row_t, "
         "Tensor? mean_value_t, Tensor[] plan, Tensor[] plan_t) -> Tensor",
         &fusedmm_spmm_mean_planned);
   m.def("fusedmm_spmm_max_planned(Tensor rowptr, Tensor col, Tensor? value, Tensor mat, Tensor[] plan) -> (Tensor, Tensor)",
         &fusedmm_spmm_max_planned);
   m.def("fusedmm_spmm_min_planned(Tensor rowptr, Tensor col, Tensor? value, Tensor mat, Tensor[] plan) -> (Tensor, Tensor)",
         &fusedmm_spmm_min_planned);
   m.def("fusedmm_spmm_max_values(Tensor rowptr, Tensor col, Tensor? value, Tensor mat, Tensor[] plan) -> Tensor", &fusedmm_spmm_max_values);
   m.def("fusedmm_spmm_min_values(Tensor rowptr, Tensor col, Tensor? value, Tensor mat, Tensor[] plan) -> Tensor", &fusedmm_spmm_min_values);
   m.def("gcn_norm_spmm(Tensor rowptr, Tensor col, Tensor mat, Tensor dinv, Tensor? colptr, Tensor? row_t, Tensor[] plan, "
         "Tensor[] plan_t, Tensor? bias, bool relu) -> Tensor",
         &gcn_norm_spmm);
   m.def("attention_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, float scale) -> Tensor", &attention_spmm);
   m.def("gat_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor y, Tensor a_dst, Tensor a_src, int heads, float negative_slope) -> Tensor",
         &gat_spmm);
   m.def("gat_edge_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor y, Tensor a_dst, Tensor a_src, Tensor a_edge, int heads, float negative_slope) -> Tensor",
         &gat_edge_spmm);
   m.def("gat_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor y, Tensor a_dst, Tensor a_src, Tensor? a_edge, int heads, float negative_slope, float p, int seed) -> Tensor",
         &gat_drop_spmm);
   m.def("attention_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, float scale) -> Tensor", &attention_spmm16);
   m.def("gat_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor y, Tensor a_dst, Tensor a_src, int heads, float negative_slope) -> Tensor",
         &gat_spmm16);
   m.def("gatv2_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, Tensor att, int heads, float negative_slope) -> Tensor",
         &gatv2_spmm);
   m.def("gatv2_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor x, Tensor y, Tensor att, int heads, float negative_slope, float p, int seed) -> Tensor",
         &gatv2_drop_spmm);
   m.def("gatv2_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor x, Tensor y, Tensor att, int heads, float negative_slope) -> Tensor",
         &gatv2_spmm16);
   m.def("mha_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int heads, float scale) -> Tensor", &mha_spmm);
   m.def("mha_drop_spmm(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, int heads, float scale, float p, int seed) -> Tensor",
         &mha_drop_spmm);
   m.def("mha_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor q, Tensor k, Tensor v, int heads, float scale) -> Tensor", &mha_spmm16);
   m.def("mha_drop_spmm16(Tensor rowptr, Tensor col, Tensor colptr, Tensor row_t, Tensor csr2csc, Tensor q, Tensor k, Tensor v, int heads, float scale, float p, int seed) -> Tensor",
         &mha_drop_spmm16);
}
