/*
 * isplib_hip.h -- C ABI of the MI355X (gfx950) SpMM aggregation backend.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch types.
 * Every pointer marked [dev] is a DEVICE pointer (HBM); every entry point is
 * asynchronous on `stream` (a hipStream_t passed as void*; NULL = the default
 * stream) and returns a FusedMM status code.  The compute entries neither
 * allocate, free nor synchronise, so they are hipGraph-capturable; those that
 * need scratch take a caller-owned workspace whose size a *_workspace_bytes
 * query reports.  The two exceptions say so where they are declared: the plan
 * builder isplib_spmm_tasks_count_hip (one stream synchronisation, once per
 * graph) and the isplib_graph_* handle, which owns device memory on the
 * caller's behalf.
 *
 * Reference interfaces replaced (paths relative to the iSpLib tree):
 *   fusedMM_csr_hip            <- fusedMM_csr, csrc/fusedMM.h:77-99, called at
 *                                 csrc/fusedmm.cpp:198; it takes the place of
 *                                 the never-linked fusedmm_cuda() stub at
 *                                 csrc/fusedmm.cpp:89-110,191-196 and of the
 *                                 thread-per-row prototype gpu/fusedmm.cu:18-51.
 *   performDummySpMM_hip       <- performDummySpMM, csrc/fusedmm.cpp:61,570.
 *   isplib_spmm_minmax_bw_hip  <- the ATen gather/mul/masked_fill/scatter_add_
 *                                 chain of FusedMM_SPMMMax/Min::backward,
 *                                 csrc/fusedmm.cpp:410-451 and 477-517.
 *   isplib_sddmm_csr_hip       <- the commented-out spmm_value_bw call,
 *                                 csrc/fusedmm.cpp:270,351 (dA for sum/mean).
 *   isplib_csr_* (graph prep)  <- torch_sparse storage getters the wrapper
 *                                 forces at isplib/__init__.py:67-73 and the two
 *                                 nnz-sized gathers it caches at :79-80,:86-99.
 *   isplib_graph_*             <- the per-graph caches of isplib/__init__.py:35-40,
 *                                 50,76-106 (class-level dicts keyed by data pointers).
 *   isplib_suggest_slices*     <- autotuner/findbestk.py, gpu/kernels/codegen.py
 *                                 (sweep a parameter, keep the fastest).
 *   fusedMM_csr_udef*_hip      <- the other message words of csrc/fusedMM.h:18-74
 *                                 (defined there, never sent by iSpLib).
 */
#ifndef ISPLIB_HIP_H
#define ISPLIB_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISPLIB_HIP_ABI_VERSION 1
#define ISPLIB_MAX_SLICES 4096       /* column-slice counts accepted by the sliced / task-list entries: 1..4096 */

/* ---- FusedMM op message (values fixed by csrc/fusedMM.h:18-74) ---------- */
#define ISPLIB_VOP_COPY_RHS 0x2
#define ISPLIB_ROP_NOOP     0x00
#define ISPLIB_SOP_COPY     0x100
#define ISPLIB_VSC_MUL      0x1000
#define ISPLIB_VSC_MEAN     0x3000
#define ISPLIB_AOP_ADD      0x10000
#define ISPLIB_AOP_MAX      0x20000
#define ISPLIB_AOP_MIN      0x30000
/* the four messages the reference sends, csrc/fusedmm.cpp:168-186 */
#define ISPLIB_MSG_SPMM_SUM  (ISPLIB_VOP_COPY_RHS | ISPLIB_ROP_NOOP | ISPLIB_SOP_COPY | ISPLIB_VSC_MUL  | ISPLIB_AOP_ADD)
#define ISPLIB_MSG_SPMM_MEAN (ISPLIB_VOP_COPY_RHS | ISPLIB_ROP_NOOP | ISPLIB_SOP_COPY | ISPLIB_VSC_MEAN | ISPLIB_AOP_ADD)
#define ISPLIB_MSG_SPMM_MAX  (ISPLIB_VOP_COPY_RHS | ISPLIB_ROP_NOOP | ISPLIB_SOP_COPY | ISPLIB_VSC_MUL  | ISPLIB_AOP_MAX)
#define ISPLIB_MSG_SPMM_MIN  (ISPLIB_VOP_COPY_RHS | ISPLIB_ROP_NOOP | ISPLIB_SOP_COPY | ISPLIB_VSC_MUL  | ISPLIB_AOP_MIN)

/* ---- status codes (csrc/fusedMM.h:105-114) + one for HIP runtime errors -- */
#define ISPLIB_SUCCESS         0
#define ISPLIB_FAIL            1    /* bad argument                            */
#define ISPLIB_NOT_ENOUGH_MEM (-1)  /* workspace too small                      */
#define ISPLIB_UNDEFINED_USER_FUNCTION 64 /* a *_UDEF stage without a built-in function (csrc/fusedMM.h:113) */
#define ISPLIB_NO_OPT_IMPL     128  /* message outside the implemented set      */
#define ISPLIB_HIP_ERROR       256  /* a HIP call failed; see isplib_hip_last_error */

int         isplib_hip_abi_version(void);
const char *isplib_hip_last_error(void);   /* thread-local, "" if none */

/* ---- address domains of the kernel families ------------------------------------------------------------------------
 * Every schedule has a hard domain set by how its kernel forms addresses.  This is its ONE statement: the entries below
 * refuse a call outside their domain (ISPLIB_FAIL; the generic pipeline ISPLIB_NO_OPT_IMPL), and every layer that picks a
 * schedule for a call -- the isplib_suggest_stream* rules, the isplib_graph_* handle, the torch op layer, the Python
 * layers through the mirror in isplib_amd/cabi.py -- asks the same predicates with the leading dimension the call will really use, so a
 * shape is never offered a schedule whose entry then refuses it.  _MAX: the largest value served; _END: the first refused. */
#define ISPLIB_DENSE_BYTES_MAX         0xE0000000u  /* 3.5 GiB: n*ldy*4 of a dense operand read through one buffer descriptor */
#define ISPLIB_DENSE_OOB_OFFSET        0xF0000000u  /* a byte offset such a descriptor answers with 0 (masked lanes carry it);
                                                       + any column offset (< 2^24) stays < 2^32: never wraps */
#define ISPLIB_STREAM_N_END            (1 << 24)    /* stream words are (local row << 24) | column, multiplied in 24 bits */
#define ISPLIB_STREAM_LDY_END          (1 << 22)    /* ... by a row pitch in BYTES that has to fit 24 bits too */
#define ISPLIB_STREAM_NNZ_END          (1LL << 31)  /* 32-bit CSR positions in a stream plan */
#define ISPLIB_STREAM_MINMAX_BYTES_END 0x80000000u  /* 2 GiB: lanes past column k of the max / min stream kernel carry 2^31 */
#define ISPLIB_K_MIN                   4            /* every entry that takes a plan; narrower operands: fusedMM_csr_hip */
#define ISPLIB_SDDMM_TASKS_K_MAX       1024         /* isplib_sddmm_csr_tasks_hip holds g[row, :] in registers */
#define ISPLIB_ATTENTION_K_MAX         512          /* the attention entries hold a row in registers, two chunks per lane */

/* n rows of ldy floats take at most `bytes` bytes (exact for any operands: no product is formed) */
static inline int isplib_rows_within(int64_t n, int64_t ldy, uint64_t bytes) { return n <= 0 || ldy <= (int64_t)(bytes / 4 / (uint64_t)n); }
/* the dense operand fits one buffer descriptor: what every entry but the plain kernel's needs */
static inline int isplib_dense_in_descriptor(int64_t n, int64_t ldy) { return isplib_rows_within(n, ldy, ISPLIB_DENSE_BYTES_MAX); }
/* the task-list entries (fusedMM_csr_tasks_hip, _epilogue_hip) serve an n x k operand at leading dimension ldy */
static inline int isplib_tasks_serve(int64_t n, int64_t k, int64_t ldy) { return k >= ISPLIB_K_MIN && isplib_dense_in_descriptor(n, ldy); }
/* isplib_sddmm_csr_tasks_hip does */
static inline int isplib_sddmm_tasks_serve(int64_t n, int64_t k, int64_t ldy) { return k <= ISPLIB_SDDMM_TASKS_K_MAX && isplib_tasks_serve(n, k, ldy); }
/* the stream entries (fusedMM_csr_stream_hip; minmax != 0: fusedMM_csr_stream_minmax_hip) and the builders of their plans do */
static inline int isplib_stream_serves(int64_t n, int64_t k, int64_t ldy, int64_t nnz, int minmax) {
   return isplib_tasks_serve(n, k, ldy) && n < ISPLIB_STREAM_N_END && ldy < ISPLIB_STREAM_LDY_END && nnz < ISPLIB_STREAM_NNZ_END &&
          (!minmax || isplib_rows_within(n, ldy, ISPLIB_STREAM_MINMAX_BYTES_END - 1u));
}
/* the 16-bit stream entry (fusedMM_csr_stream16_hip: bf16 / fp16 dense operands, sum / mean) does: the stream entry's domain with
 * the byte sizes at 2 bytes per element, and k, ldy, ldz all even -- every 8-byte gather and store is then 4-byte aligned, the
 * last vector of a ragged panel (shifted back to end at column k) included.  The entry also refuses a y or z base that is not
 * 4-byte aligned.  What this refuses is served by converting the operand to fp32 (the layers above do that; nothing raises). */
static inline int isplib_stream16_serves(int64_t n, int64_t k, int64_t ldy, int64_t ldz, int64_t nnz) {
   return k >= ISPLIB_K_MIN && n < ISPLIB_STREAM_N_END && ldy < ISPLIB_STREAM_LDY_END && nnz < ISPLIB_STREAM_NNZ_END &&
          isplib_rows_within(n, ldy, 2ull * ISPLIB_DENSE_BYTES_MAX) && (k % 2) == 0 && (ldy % 2) == 0 && (ldz % 2) == 0;
}
/* the 16-bit row entry (fusedMM_csr_rows16_hip: bf16 / fp16 dense operands on the plain row-per-wave schedule, sum / mean) does:
 * a lane's 16-byte gather holds eight columns, so k >= ISPLIB_ROWS16_K_MIN; k, ldy, ldz all even -- every 16-byte gather and store
 * is then 4-byte aligned, the last vector of a ragged row (shifted back to end at column k) included; ONE descriptor with 32-bit
 * byte offsets at 2 bytes per element, n*ldy*2 <= ISPLIB_DENSE_BYTES_MAX; n < 2^31 (32-bit column ids times the pitch); and
 * k < ISPLIB_ROWS16_K_END, so that a masked lane's offset (ISPLIB_DENSE_OOB_OFFSET + its column's bytes) cannot wrap.  With a row
 * order the entry also needs m < 2^31, and it refuses a y or z base that is not 4-byte aligned.  What this refuses is served by
 * converting the operand to fp32 (the layers above do that; nothing raises). */
#define ISPLIB_ROWS16_K_MIN            8
#define ISPLIB_ROWS16_K_END            (1 << 24)
static inline int isplib_rows16_serves(int64_t n, int64_t k, int64_t ldy, int64_t ldz) {
   return k >= ISPLIB_ROWS16_K_MIN && k < ISPLIB_ROWS16_K_END && n < (1LL << 31) && isplib_rows_within(n, ldy, 2ull * ISPLIB_DENSE_BYTES_MAX) &&
          (k % 2) == 0 && (ldy % 2) == 0 && (ldz % 2) == 0;
}
#define ISPLIB_MINMAX_BW_PAIRS_END     0xFFFFFFFEu  /* the sort-based max / min backward: m*k (row, feature) pairs < this */
#define ISPLIB_MINMAX_BW_KEYS_MAX      0xFFFFFFFEu  /* 32-bit sort keys: n*k destinations and one key behind them, n*k + 1 < 2^32 */
#define ISPLIB_OWNER_WORLD_MAX         64           /* ranks of the owner-bucketed exchange: their row cuts travel as a kernel argument */
/* rows * k is at most `most` (exact: no product is formed) */
static inline int isplib_product_within(int64_t rows, int64_t k, uint64_t most) {
   return rows <= 0 || k <= 0 || (uint64_t)k <= most / (uint64_t)rows;
}
/* the owner-bucketed exchange of the partitioned max / min backward (isplib_minmax_bw_bucket_hip) serves m x k winners cut for
 * `world` owners at the ascending row boundaries cuts[0..world]: every owner's keys (cuts[p+1] - cuts[p]) * k + 1 < 2^32.
 * isplib_scatter_keys_det_hip serves the same two bounds (total pairs in place of m*k, its n x k block as the one owner). */
static inline int isplib_owner_exchange_serves(int64_t m, int64_t k, int world, const int64_t *cuts) {
   if (world < 1 || world > ISPLIB_OWNER_WORLD_MAX || m < 0 || k < 0 || !isplib_product_within(m, k, ISPLIB_MINMAX_BW_PAIRS_END - 1u)) return 0;
   for (int p = 0; p < world; p++)
      if (cuts[p + 1] < cuts[p] || !isplib_product_within(cuts[p + 1] - cuts[p], k, ISPLIB_MINMAX_BW_KEYS_MAX)) return 0;
   return 1;
}

/*
 * The one convention of this path that nothing in the reference tree pins: what an EMPTY row of a max / min SpMM holds.
 * The reference launcher pre-fills the output with lowest() / max() and the positions with nnz (csrc/fusedmm.cpp:147-150,
 * 171,177) and hands them to fusedMM_csr, whose body is not in the tree (configure:2-7).
 *   0 "zero" (default)  the row is 0 -- torch_sparse's CPU kernel, the one the iSpLib authors compared against
 *                       (isplib/__init__.py:120-128), and what oracle/ restates
 *   1 "init"            the row keeps the launcher's pre-fill, -FLT_MAX (max) / +FLT_MAX (min) -- what a body returns
 *                       that only visits stored entries
 * The positions are nnz either way; sum / mean are 0 either way.  Process-wide, every schedule; read once from the
 * environment (ISPLIB_EMPTY_ROW=init|zero) unless set here first.  A maintainer who holds the real fusedmm_cpu.a picks
 * whichever it does.
 */
int isplib_hip_set_empty_row(int init);
int isplib_hip_get_empty_row(void);

/*
 * SpMM with the reference's 20-argument FusedMM signature, device pointers.
 *
 *   z[i,:] = REDUCE_{j in [pntrb[i], pntre[i])}  val[j] * y[indx[j], :]
 *
 * REDUCE/scale from `imessage` (one of ISPLIB_MSG_SPMM_*).  Differences from
 * the host ABI, all consequences of running on the device:
 *   - z and z_arg are WRITE-ONLY: the kernel writes the value the reference
 *     gets by pre-filling z with 0 / -FLT_MAX / +FLT_MAX (csrc/fusedmm.cpp:
 *     147-152) and z_arg with nnz (:171,177) and then accumulating.  beta must
 *     be 0 (the only value the reference passes, :117).  This folds two
 *     M*K-sized fill passes into the kernel's write-back.
 *   - val may be NULL = unit weights (what isplib/__init__.py:51-57
 *     materialises as a ones vector); the stream is then never read.
 *   - MAX/MIN: strict compare in CSR order (lowest CSR position wins ties, NaN
 *     never wins); empty row -> value 0 (or the launcher's init value: isplib_hip_set_empty_row), z_arg = nnz.  z_arg (int64, same
 *     leading dimension as z) holds ABSOLUTE CSR positions; may be NULL.
 *   - x/ldx/alpha/rows/cols are accepted and ignored, as in the reference.
 * Requirements: n < 2^31, every row's degree < 2^31, ldy >= k, ldz >= k.
 * Any other message word is handed to the generic pipeline below
 * (fusedMM_csr_udef_hip with no user function).
 */
int fusedMM_csr_hip(int32_t imessage, int64_t m, int64_t n, int64_t k,
                    float alpha, int64_t nnz, int64_t rows, int64_t cols,
                    const float *val /*[dev] nnz | NULL*/,
                    const int64_t *indx /*[dev] nnz*/,
                    const int64_t *pntrb /*[dev] m*/,
                    const int64_t *pntre /*[dev] m*/,
                    const float *x /*[dev] m x ldx; only read by non-SpMM messages*/, int64_t ldx,
                    const float *y /*[dev] n x ldy*/, int64_t ldy, float beta,
                    float *z /*[dev] m x ldz*/, int64_t ldz,
                    int64_t *z_arg /*[dev] m x ldz | NULL*/, void *stream);

/*
 * The generic five-stage FusedMM pipeline (csrc/fusedMM.h:18-74) for message words other than
 * the four SpMM ones -- the SDDMM-fused patterns of the FusedMM paper (graph embedding with a
 * sigmoid or t-distribution kernel, score-then-aggregate attention).  The reference never sends
 * them (csrc/fusedmm.cpp:168-186) and the library that defines them is absent from its tree, so
 * the semantics are restated here and in oracle/fusedmm_oracle.c; nothing pins them.
 * For row i and stored entry e = (i, j), a = val[e] (1 if val is NULL), per column c:
 *   VOP  T[c] = COPY_LHS x[i,c] | COPY_RHS y[j,c] | ADD x+y | SUBL x-y | SUBR y-x | MAX | MIN
 *   ROP  s    = NOOP 1 | DOT sum x[i,c]*T[c] | ADD_LHS sum x | ADD_RHS sum T | NORML sum x^2 | NORMR sum T^2
 *   SOP  s'   = NOOP s | COPY a | UDEF f(s): C function pointers cannot cross to the device, so the
 *               user function is chosen from a built-in menu (`sop_udef`, `sop_param`)
 *   VSC  T'[c]= NOOP T[c] | MUL s'*T[c] | ADD s'+T[c] | MEAN (MUL, the row divided by max(deg,1))
 *   AOP  z[i,c] ADD += | MAX | MIN (z_arg as in fusedMM_csr_hip) T'[c]
 * VOP/ROP/VSC/AOP_UDEF and SOP_UDEF without a menu entry return ISPLIB_UNDEFINED_USER_FUNCTION,
 * flag values the header does not define ISPLIB_NO_OPT_IMPL.  k <= 1024; same write-only z,
 * beta == 0 and tie rules as fusedMM_csr_hip.  One wave per row, no atomics.
 */
enum isplib_sop_udef {
   ISPLIB_SOP_NONE = 0,
   ISPLIB_SOP_SIGMOID = 1,            /* 1 / (1 + exp(-s))                                  */
   ISPLIB_SOP_ONE_MINUS_SIGMOID = 2,  /* 1 - sigmoid(s): the gradient scale of sigmoid embedding */
   ISPLIB_SOP_TDIST = 3,              /* 1 / (1 + s): t-distribution kernel on s = |y_j - x_i|^2 */
   ISPLIB_SOP_SCALE = 4,              /* sop_param * s                                       */
   ISPLIB_SOP_EXP = 5,                /* exp(s)                                              */
   ISPLIB_SOP_LEAKY_EXP = 6           /* exp(s > 0 ? s : sop_param * s): un-normalised GAT score */
};
int fusedMM_csr_udef_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, float alpha, int64_t nnz,
                         int64_t rows, int64_t cols, const float *val /*[dev] nnz | NULL*/,
                         const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                         const float *x /*[dev] m x ldx | NULL if unused*/, int64_t ldx,
                         const float *y /*[dev] n x ldy*/, int64_t ldy, float beta,
                         float *z /*[dev] m x ldz*/, int64_t ldz, int64_t *z_arg /*[dev] | NULL*/,
                         int sop_udef /*enum isplib_sop_udef*/, float sop_param, void *stream);

/* The same pipeline over the task plan of the SpMM (isplib_spmm_tasks_*; one wave per task, partial rows in
 * `workspace` = isplib_spmm_tasks_workspace_bytes(AOP word, n_tasks, k), folded like the SpMM's): the gathers of y
 * get the L2 affinity of the column slices.  ROP needs whole rows, so there are no column panels: choose the
 * slice count for the full width (about n*k*4 / 7 MB).  4 <= k <= 1024. */
int fusedMM_csr_udef_tasks_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                               const float *val, const int64_t *indx, const int32_t *indx32 /*optional*/,
                               const int64_t *pntrb, const int64_t *pntre,
                               const float *x, int64_t ldx, int64_t n_tasks, const int32_t *task_row,
                               const int64_t *task_b, const int32_t *task_len, const int32_t *seg_off,
                               int slices, const int64_t *lane_off_host /*9, host*/,
                               const float *y, int64_t ldy, float *z, int64_t ldz, int64_t *z_arg,
                               int sop_udef, float sop_param, void *workspace, size_t workspace_bytes,
                               void *stream);

/*
 * Column-sliced SpMM: same result as fusedMM_csr_hip, faster when y does not fit an
 * XCD's 4 MiB L2 and rows are long (Reddit-like graphs).  The columns of A (= rows of
 * y) are cut into `slices` (1..ISPLIB_MAX_SLICES) equal ranges; every XCD of the MI355X
 * walks all rows of its own share of the slices, so its L2 holds 1/slices of y instead of all of
 * it; the per-slice partials (workspace) are folded in slice order by a second kernel.
 * No atomics: bitwise reproducible; max/min still resolve ties to the lowest CSR
 * position.  Requires column indices sorted within each row (torch_sparse order; the
 * CSC operands of csrc/fusedmm.cpp:285 are sorted too).
 *
 *   isplib_spmm_slices_build_hip: sliceptr[i*(slices+1)+s] = first CSR position of row
 *     i with column >= s*ceil(n/slices); once per graph, independent of k.  If
 *     unsorted_flag != NULL it receives 1 when some row is not sorted (the table must
 *     then not be used) -- the one-per-graph replacement for the per-graph caches of
 *     isplib/__init__.py:76-106.
 *   workspace: isplib_spmm_sliced_workspace_bytes(imessage, m, k, slices) bytes,
 *     256-byte aligned.
 */
size_t isplib_spmm_slices_bytes(int64_t m, int slices);
int    isplib_spmm_slices_build_hip(int64_t m, int64_t n, int64_t nnz,
                                    const int64_t *pntrb, const int64_t *pntre,
                                    const int64_t *indx, int slices,
                                    int64_t *sliceptr /*[dev] m*(slices+1)*/,
                                    int32_t *unsorted_flag /*[dev] 1 | NULL*/,
                                    void *stream);
size_t isplib_spmm_sliced_workspace_bytes(int32_t imessage, int64_t m, int64_t k, int slices);
int    fusedMM_csr_sliced_hip(int32_t imessage, int64_t m, int64_t n, int64_t k,
                              int64_t nnz, const float *val, const int64_t *indx,
                              const int64_t *pntrb, const int64_t *pntre,
                              const int64_t *sliceptr, int slices,
                              const float *y, int64_t ldy, float *z, int64_t ldz,
                              int64_t *z_arg, void *workspace,
                              size_t workspace_bytes, void *stream);

/*
 * The same computation in phases, for overlapping a collective with compute (1-D row
 * partition: the slices that fall in this rank's own shard of y need no remote data).
 * Runs the partial kernel over the slice_count slices slice_first, slice_first + 1, ... taken
 * modulo `slices` (so "every slice but mine" is one call; count may be 0) and, when `combine`
 * != 0, the fold over ALL `slices` planes afterwards.  Every
 * slice must have been covered by some phase, with the same workspace, before the
 * combining call.  `y` may differ between phases as long as y[indx[j]] addresses the right
 * row for every column of the phase's slices (e.g. a base pointer shifted onto a shard).
 */
int    fusedMM_csr_sliced_phase_hip(int32_t imessage, int64_t m, int64_t n, int64_t k,
                                    int64_t nnz, const float *val, const int64_t *indx,
                                    const int64_t *pntrb, const int64_t *pntre,
                                    const int64_t *sliceptr, int slices,
                                    int slice_first, int slice_count, int combine,
                                    const float *y, int64_t ldy, float *z, int64_t ldz,
                                    int64_t *z_arg, void *workspace,
                                    size_t workspace_bytes, void *stream);

/*
 * Task-list schedule: the most robust form of the sliced SpMM (hub rows, empty segments, short
 * rows).  The caller supplies a per-graph plan (isplib_spmm_tasks_count_hip / _fill_hip below):
 *   task t = edges [task_b[t], task_b[t] + task_len[t]) of row task_row[t], at most a few hundred
 *   edges, all in one column slice; tasks are grouped by XCD lane: lane x (blocks with
 *   blockIdx % 8 == x) runs tasks [lane_off[x], lane_off[x+1]) (lane_off: 9 HOST int64);
 *   seg_off[(s' * m) + i] = first task of row i in plan slice position s'
 *   (s' = (s % 8) * (slices / 8) + s / 8), slices*m + 1 entries.
 * Each task writes one partial row into the workspace (isplib_spmm_tasks_workspace_bytes);
 * a second kernel folds a row's partials in ascending CSR order.  Same results and conventions
 * as fusedMM_csr_hip; domain: isplib_tasks_serve(n, k, ldy) -- k >= ISPLIB_K_MIN, n*ldy*4 <= ISPLIB_DENSE_BYTES_MAX.
 */
typedef struct isplib_task_plan_info {
   int64_t n_tasks;
   int64_t lane_off[9];     /* tasks of XCD lane x: [lane_off[x], lane_off[x+1]) */
   int32_t slices, chunk, short_row, reserved;
} isplib_task_plan_info;

/*
 * Plan builder, two calls, once per graph (independent of k):
 *   count: from the slice table (isplib_spmm_slices_build_hip) derives the number of tasks of every
 *          (slice position, row) segment -- ceil(len / chunk), rows with fewer than short_row edges
 *          kept whole on slice row % slices -- and its exclusive prefix seg_off[slices*m + 1].
 *          Fills *info (HOST) and synchronises `stream` ONCE to do so; info->lane_off cuts the task
 *          list into eight contiguous runs of equal EDGE mass (one per XCD lane).
 *   fill : writes task_row / task_b / task_len (info->n_tasks entries each).
 */
size_t isplib_spmm_tasks_plan_workspace_bytes(int64_t m, int slices);
int    isplib_spmm_tasks_count_hip(int64_t m, const int64_t *pntrb, const int64_t *pntre,
                                   const int64_t *sliceptr, int slices, int chunk, int short_row,
                                   int32_t *seg_off /*[dev] slices*m+1*/, void *workspace,
                                   size_t workspace_bytes, isplib_task_plan_info *info /*host*/,
                                   void *stream);
int    isplib_spmm_tasks_fill_hip(int64_t m, const int64_t *pntrb, const int64_t *pntre,
                                  const int64_t *sliceptr, const isplib_task_plan_info *info,
                                  const int32_t *seg_off, int32_t *task_row, int64_t *task_b,
                                  int32_t *task_len, void *stream);
size_t isplib_spmm_tasks_workspace_bytes(int32_t imessage, int64_t n_tasks, int64_t k);
/* indx32 (optional, may be NULL): the column ids of indx packed to 32 bits, once per graph, by
 * isplib_pack_indices_hip.  The task kernels then stream 4 instead of 8 bytes per stored entry -- the index
 * stream is the one operand that always comes from HBM (Reddit: 917 MB per pass; -12 % time at k=32, -4 % at
 * k=128).  indx stays the reference's int64 array and is what NULL falls back to. */
int    isplib_pack_indices_hip(int64_t nnz, const int64_t *indx, int32_t *indx32, void *stream);
int    fusedMM_csr_tasks_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                             const float *val, const int64_t *indx, const int32_t *indx32,
                             const int64_t *pntrb, const int64_t *pntre,
                             int64_t n_tasks, const int32_t *task_row,
                             const int64_t *task_b, const int32_t *task_len,
                             const int32_t *seg_off, int slices,
                             const int64_t *lane_off_host /*9, host*/,
                             const float *y, int64_t ldy, float *z, int64_t ldz,
                             int64_t *z_arg, void *workspace, size_t workspace_bytes,
                             void *stream);

/*
 * The same with an epilogue fused into the fold (sum / mean only): the step right after the path in a GNN
 * layer -- GCN's D^-1/2 (A + I) D^-1/2 X without materialising edge weights (y = D^-1/2 X, self = y,
 * row_scale = D^-1/2), bias and ReLU (callers: tests/dist/gcn/pyg-sparse.py:61-62, normalize=True).
 *     out[i,c] = act( row_scale[i] * (reduce[i,c] + self[i,c]) + bias[c] )        every member optional
 */
typedef struct isplib_epilogue {
   const float *row_scale;   /* [dev] m, or NULL */
   const float *self;        /* [dev] m x ld_self, or NULL */
   int64_t      ld_self;
   const float *bias;        /* [dev] k, or NULL */
   int          relu;        /* nonzero: max(., 0) */
} isplib_epilogue;
int    fusedMM_csr_tasks_epilogue_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                      const float *val, const int64_t *indx, const int32_t *indx32,
                                      const int64_t *pntrb, const int64_t *pntre,
                                      int64_t n_tasks, const int32_t *task_row,
                                      const int64_t *task_b, const int32_t *task_len,
                                      const int32_t *seg_off, int slices,
                                      const int64_t *lane_off_host /*9, host*/,
                                      const float *y, int64_t ldy, float *z, int64_t ldz,
                                      void *workspace, size_t workspace_bytes,
                                      const isplib_epilogue *epilogue /*host, may be NULL*/,
                                      void *stream);

/*
 * The dense passes either side of the fused GCN aggregation (epilogue above with self = y, row_scale = D^-1/2), one launch each,
 * no atomics (the column sums are per-block partials folded in block order: bitwise reproducible):
 *   isplib_row_scale_hip            y[i,c] = scale[i] * x[i,c], c < k; columns k..ldy-1 of y are written 0 -- y = D^-1/2 X at
 *                                   whatever pitch the gather wants (a 33..47-column operand at 48 floats touches 2 lines
 *                                   per row instead of 2.25)
 *   isplib_masked_scale_colsum_hip  the backward's prologue, reading dz (and out) once:
 *                                   g[i,c] = out ? (out[i,c] > 0 ? dz[i,c] : 0) : dz[i,c]      (ReLU mask; out may be NULL)
 *                                   gy[i,c] = g[i,c] * (scale ? scale[i] : 1)                  (gy may be NULL; pitch as above)
 *                                   grad_bias[c] = sum_i g[i,c]                                (may be NULL; else workspace of
 *                                   isplib_masked_scale_colsum_workspace_bytes(n, k) bytes, 256-byte aligned)
 */
int    isplib_row_scale_hip(int64_t n, int64_t k, const float *x /*[dev] n x ldx*/, int64_t ldx, const float *scale /*[dev] n*/,
                            float *y /*[dev] n x ldy*/, int64_t ldy, void *stream);
size_t isplib_masked_scale_colsum_workspace_bytes(int64_t n, int64_t k);
int    isplib_masked_scale_colsum_hip(int64_t n, int64_t k, const float *dz, int64_t lddz, const float *out /*NULL: no mask*/,
                                      int64_t ldo, const float *scale /*[dev] n | NULL*/, float *gy /*[dev] n x ldgy | NULL*/,
                                      int64_t ldgy, float *grad_bias /*[dev] k | NULL*/, void *workspace, size_t workspace_bytes,
                                      void *stream);

/*
 * Stream schedule (sum / mean) -- the default on graphs with work for the whole chip.  A launch ("generation") holds only
 * waves that are resident together; every wave owns a fixed set of (virtual) rows whose running sums live in LDS, and all
 * waves walk the column slices of their own rows in step, so an XCD's L2 serves one or two slices at a time.  The plan owns
 * a COPY of the edges in the order the waves walk them, so a wave never sees a row or slice boundary.  Each of the `streams` (= 64 / lanes per row slot)
 * slots of a wave owns rows_per_wave / streams rows and a stream of 4-byte words, (local row << 24) | column, that
 * lists those rows' edges slice by slice; step i of a wave gathers word i of each of its streams in ONE full 1-KiB
 * buffer load, and every lane adds what arrives to the running sum of the row its slot is on (registers), which
 * moves to and from the slot's LDS row when the stream changes rows.  16 or 32 gathers are in flight per wave at all
 * times; there are no per-segment latency chains, no masked tails, no cross-lane reduction, no partial rows, no fold.
 * The slots of a wave own disjoint rows and a wave's LDS operations execute in order: every sum is formed in one
 * fixed order (bitwise reproducible).  The panel width is 256 / streams columns (streams = 4: 64 columns); k is
 * swept in such panels.  Weights are part of the plan (`vals`, in stream order; NULL = unit weights): a caller whose
 * weights change refreshes them through the plan's permutation.  A launch holds few, deep waves (2 or 3 per SIMD):
 * isplib_spmm_stream_geometry reports the rows per wave the kernel of a slot width is built for and the waves the
 * device holds at once (what waves_per_gen should be: persistent waves only stay on the same slices -- and the slices
 * in the L2 -- when they all start together).
 * Domain: isplib_stream_serves(n, k, ldy, nnz, 0) -- k >= ISPLIB_K_MIN (any k: a last vector that would reach past column
 * k is shifted back to end there; rows need only 4-byte alignment), n < ISPLIB_STREAM_N_END and ldy < ISPLIB_STREAM_LDY_END
 * (24-bit address arithmetic per edge), n*ldy*4 <= ISPLIB_DENSE_BYTES_MAX; the plan builders need nnz < ISPLIB_STREAM_NNZ_END.
 */
typedef struct isplib_stream_plan {
   int64_t rows, cols;              /* m, n of the graph the plan was built for */
   int32_t slices, gens, waves_per_gen, rows_per_wave, streams /* 2, 4 or 8 */, chunk /* rows over this many entries were dealt to virtual rows */;
   int64_t n_steps, n_parts, n_hub;
   const int32_t *words;            /* [dev] n_steps*streams: (local row << 24) | column; padding = (own row << 24) | n */
   const float   *vals;             /* [dev] n_steps*streams weights in the same order, or NULL */
   const int64_t *wave_step_off;    /* [dev] gens*waves_per_gen + 1: first step of a wave */
   const int32_t *wave_row;         /* [dev] gens*waves_per_gen*rows_per_wave: row of the local row, -1 = unused */
   const int32_t *wave_part;        /* [dev] same shape: -1 = whole row, else partial row id */
   const int32_t *hub_row;          /* [dev] n_hub */
   const int32_t *hub_off;          /* [dev] n_hub + 1 */
   const int32_t *perm;             /* [dev] n_steps*streams: CSR position of every word, -1 = padding (for re-gathering
                                       weights; the arg candidates of max / min); NULL in plans that do not carry it -- the
                                       sum / mean kernel never reads it */
   const uint32_t *packed;          /* [dev] the PACKED WORD STREAM (below): isplib_stream_packed_dwords(plan) dwords, or NULL */
   int32_t has_packed;              /* nonzero: `packed` holds every batch of `words`; 0: the plan has no packed stream (not
                                       representable, not a 4-stream sum / mean plan, no room) and every call reads `words` */
} isplib_stream_plan;
/* PACKED WORD STREAM (profiles/stream_packed_words.txt).  A launch reads the plan's words from beyond the L2 once per
 * 64-column panel, 4 bytes per entry; a word carries 4 bits of local row inside its slot and a column that, relative to its column
 * slice, needs 13 bits.  4-stream sum / mean plans therefore carry a second, bit-packed copy of `words`, built from them by one device
 * pass at plan build, which the sum / mean kernel decodes once per batch into the registers it loaded from `words` before -- the loop
 * that consumes them, `words`, `vals`, `perm` and every other kernel are unchanged, and the decoded values ARE the words, padding
 * included, so every sum has the bits it had.
 * A BATCH is the 128 consecutive words of one wave that the kernel holds in its two batch registers: entry e of batch b of a wave is
 * word b * 128 + e of the wave's stream = (step b * 32 + e / 4, slot e % 4); words past the end of the wave are padding.  A batch
 * takes ISPLIB_STREAM_PACK_DWORDS = 76 dwords (304 bytes instead of 512), and batch b of wave w (w counted through the whole plan,
 * its first step s0 = wave_step_off[w]) starts at dword ((s0 * 4) / 128 + w + b) * 76: the place follows from the wave's position
 * alone, no table (a wave's ceil(nwords / 128) batches never reach the next wave's first; up to one batch per wave stays unused).
 *   dwords 0..63   dword i: bits 0..12 the column of entry i, bits 13..25 the column of entry 64 + i, each relative to the first
 *                  column of its DECODED slice (below); bits 26..29 the local row of entry i inside its slot (word >> 24 minus
 *                  slot * 16); bit 30 / bit 31: the slice-advance flag of entry i / of entry 64 + i
 *   dwords 64..71  the local rows of entries 64..127, 4 bits each: entry 64 + i, i = 4 t + slot, is nibble t % 8 of dword
 *                  64 + slot * 2 + t / 8
 *   dwords 72..75  one header per slot: bits 0..11 the slot's base slice (the true slice of its first entry of the batch), bits 12..17 the
 *                  number of its entries (0..32, in step order) that are NOT padding -- a slot's padding words are the tail of its
 *                  stream, they decode to the kernel's own padding word ((slot * 16) << 24 | n) and their other bits are 0
 * The decoded slice of an entry is the header's slice plus the number of advance flags of its slot's entries up to and including
 * itself; its column is slice * W + the 13-bit field, W = ceil(cols / slices) the plan's slice width.  The packer sets a flag
 * whenever the entry's true slice is ahead of the decoded one, so the decoded slice follows the true one by at most one step per
 * entry: where a slot's stream skips slices (rows with no entry in them) the decoded slice may lag, and the entry is representable
 * while its column is still within 8,191 of the lagging slice's first column (narrow slices absorb any skip; with slices wider
 * than 4,096 columns a skip inside a batch is not representable -- a batch's first entry always is, the header is free).
 * Representable plans: streams == 4, rows_per_wave == 64 (16 rows per slot), W <= 8,192, slices <= 4,096, and every entry as above;
 * any other plan gets packed == NULL, has_packed == 0 and runs as before.  isplib_stream_pack_hip is the packing pass for callers
 * that build the plan's arrays themselves: `out` [dev] of isplib_stream_packed_dwords(plan) dwords (0: the geometry is not
 * representable); *representable (host, out) = 0 where an entry is not, and then `out` must not be attached to the plan.  It
 * synchronises `stream`.  The native builders call it themselves; isplib_stream_plan_free releases the array they attached.
 * fusedMM_csr_stream_hip reads the packed stream when the plan carries one and ISPLIB_STREAM_PACK (auto | 0 | 1, read once)
 * allows it: 0 never (the launch of a plan without one, exactly), 1 whenever the plan has one, auto (unset) from
 * ISPLIB_STREAM_PACK_MIN_WORDS stored entries on (where the stream schedule is offered at all).  Staged panels and the levelled
 * deal compose with it unchanged; the 16-bit-feature entry, max / min, FusedMM and the SDDMM over stream plans read `words`. */
#define ISPLIB_STREAM_PACK_DWORDS 76
#define ISPLIB_STREAM_PACK_COL_BITS 13
#define ISPLIB_STREAM_PACK_MIN_WORDS (4 * 1048576)
size_t isplib_stream_packed_dwords(const isplib_stream_plan *plan /*host*/);
int  isplib_stream_pack_hip(const isplib_stream_plan *plan /*host*/, uint32_t *out /*[dev]*/, int64_t out_dwords,
                            int *representable /*host, out*/, void *stream);
/* Native plan builder (the same construction as isplib_amd/plan.py, on the device with rocPRIM sorts): allocates the
 * plan's device arrays -- release them with isplib_stream_plan_free -- and synchronises `stream` (twice: the sizes of
 * the plan are data dependent).  streams / slices / chunk: from isplib_suggest_stream; waves_per_gen <= 0: what
 * isplib_spmm_stream_geometry reports.  val may be NULL (unit weights).  isplib_stream_plan_set_values_hip re-gathers
 * the weights (NULL: back to unit weights) when they change. */
int  isplib_stream_plan_build_hip(int64_t m, int64_t n, int64_t nnz, const int64_t *rowptr, const int64_t *col,
                                  const float *val, int streams, int slices, int chunk, int waves_per_gen,
                                  isplib_stream_plan *out /*host*/, void *stream);
/* LEVELLED DEAL (profiles/stream_level.txt).  The workgroups of a dispatch do not all gather at the same speed:
 * the eight XCDs differ by 1-2 %, a CU's second workgroup runs ~4 % behind its first, both persistently, and a dispatch ends
 * with its slowest wave.  Step 2 of the construction therefore
 * gives every stream a CAPACITY (fixed point, ISPLIB_STREAM_CAP_ONE = nominal) and orders the streams of a round by
 * load * ISPLIB_STREAM_CAP_ONE / capacity (integer division, saturated at 2^32 - 1) instead of by load: a slow XCD's streams get
 * fewer edges.  The deal only decides WHICH wave holds a row: every row's words and their order are unchanged; equal capacities
 * give today's plan arrays exactly.  A row's sum has the unlevelled plan's bits wherever the row is flushed at every column-slice
 * boundary in both plans -- the kernel adds a running sum to the row's LDS line when its stream turns to ANOTHER row, so a row
 * with no other row of its stream between its words of two slices is summed straight through, and which rows share a stream is
 * what the deal changes.  Streams of many rows with entries in every slice carry nothing (the headline: the whole output bitwise
 * equal); a plan of two or three short rows per stream may differ in the last bits of such rows, as it does between two slice
 * counts.  For a given plan every sum is formed in one fixed order, as before.
 * A capacity belongs to a wave of the generation (all its streams, in every generation): caps[w], w < waves_per_gen.
 * isplib_stream_capacities_hip fills caps for the sum / mean kernel of `streams` slots on `device` (< 0: the current one): a
 * calibration made once per (device, streams, waves_per_gen) and process -- one generation of the stream kernel itself, timed
 * per wave, on a synthetic plan (~11 ms; 2.7 GB of device memory at its peak, measured, released before it returns; no room: equal
 * capacities, *levelled = 0, no error, and the next plan build asks again), averaged per
 * XCD (workgroup index modulo 8) and residency order (the first or a later workgroup of its CU): speed assumptions only -- or
 * equal capacities where levelling does not apply: ISPLIB_STREAM_LEVEL=0, a waves_per_gen other than the resident waves
 * isplib_spmm_stream_geometry reports (<= 0 means those), and under auto (unset) nnz < 4 Mi, where the stream schedule is not
 * offered either.  *levelled (may be NULL) tells which.  ISPLIB_STREAM_LEVEL=auto|0|1 is read once; 1 levels at any nnz.
 * Max / min and FusedMM plans are never levelled.  The calibration never runs inside a call.
 * isplib_stream_plan_build_hip asks it itself; isplib_stream_plan_build_caps_hip takes the capacities from the caller
 * (host array of waves_per_gen entries in [ISPLIB_STREAM_CAP_ONE / 16, ISPLIB_STREAM_CAP_ONE * 16]; NULL: equal). */
#define ISPLIB_STREAM_CAP_ONE 4096u
int  isplib_stream_capacities_hip(int device, int streams, int waves_per_gen, int64_t nnz, uint32_t *caps /*host, out*/,
                                  int *levelled /*out*/, void *stream);
int  isplib_stream_plan_build_caps_hip(int64_t m, int64_t n, int64_t nnz, const int64_t *rowptr, const int64_t *col,
                                       const float *val, int streams, int slices, int chunk, int waves_per_gen,
                                       const uint32_t *caps /*host*/, isplib_stream_plan *out /*host*/, void *stream);
int  isplib_stream_plan_set_values_hip(isplib_stream_plan *plan, const float *val /*[dev] nnz | NULL*/, void *stream);
void isplib_stream_plan_free(isplib_stream_plan *plan);
int    isplib_spmm_stream_geometry(int streams, int *rows_per_wave /*out*/, int *waves_resident /*out*/);
/* the measured rule: nonzero when the stream schedule is expected to beat the task list for an m x n, nnz-entry SpMM
 * over k columns (sum / mean), with the plan parameters to build it with (streams, column slices, hub-row chunk) */
int    isplib_suggest_stream(int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk);
/* the same rule told whether the plan will carry edge weights (a weighted launch reads the plan's weight stream once per
 * column panel: whole multiples of 128 columns then run on 128-column slots, streams = 2); isplib_suggest_stream is this
 * with weighted = 0 */
int    isplib_suggest_stream_weighted(int64_t m, int64_t n, int64_t nnz, int64_t k, int weighted, int *streams, int *slices, int *chunk);
/* max / min on the stream schedule, for graphs whose rows are column-sorted (ascending, duplicates allowed).  The
 * running sum becomes the best value so far and the WORD INDEX at which it was met; a second LDS plane keeps those
 * indices beside the values, and only a strictly better candidate replaces the one held.  The plan walks a row's edges
 * slice by slice and, inside a slice, in CSR order -- for a column-sorted row that IS its CSR order, so the candidate
 * that stays among equals is the one at the lowest CSR position, the reference's tie rule (csrc/fusedmm.cpp:170-178 +
 * SURVEY.md row K3).  No position travels with the gathers: only the M x K winners are translated to CSR positions,
 * through the plan's `perm` (required), when a row is written out; hub rows cut into virtual rows carry (value, CSR
 * position) pairs into their fold.  Slots of 64 columns (streams = 4) or, for k <= 32, of 32 columns (streams = 8), with
 * half the rows per wave of the sum kernel, so max / min plans are built for isplib_spmm_stream_minmax_geometry -- isplib_stream_plan_build_minmax_hip
 * does that and returns ISPLIB_FAIL for a graph with an unsorted row (use the task list) -- and are not interchangeable
 * with sum plans.  Domain: isplib_stream_serves(n, k, ldy, nnz, 1) -- the sum entry's and n*ldy*4 < ISPLIB_STREAM_MINMAX_BYTES_END.  z_arg (may be NULL): [m][ldz] int64 CSR positions, nnz = empty row.  With z_arg = NULL the
 * launch is a values-only one: no position is tracked at all (a quarter of the loop's vector instructions), same plan,
 * same values bit for bit. */
int    isplib_spmm_stream_minmax_geometry(int streams /* 4 | 8 */, int *rows_per_wave /*out*/, int *waves_resident /*out*/);
int    isplib_suggest_stream_minmax(int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk);
int    isplib_stream_plan_build_minmax_hip(int64_t m, int64_t n, int64_t nnz, const int64_t *rowptr, const int64_t *col,
                                           const float *val, int streams, int slices, int chunk, int waves_per_gen,
                                           isplib_stream_plan *out /*host*/, void *stream);
size_t isplib_spmm_stream_minmax_workspace_bytes(const isplib_stream_plan *plan);
int    fusedMM_csr_stream_minmax_hip(int32_t imessage /* ISPLIB_MSG_SPMM_MAX | _MIN */, int64_t m, int64_t n, int64_t k,
                                     int64_t nnz, const int64_t *pntrb, const int64_t *pntre,
                                     const isplib_stream_plan *plan /*host*/,
                                     const float *y, int64_t ldy, float *z, int64_t ldz, int64_t *z_arg,
                                     void *workspace, size_t workspace_bytes, void *stream);
size_t isplib_spmm_stream_workspace_bytes(const isplib_stream_plan *plan);
int    fusedMM_csr_stream_hip(int32_t imessage /* ISPLIB_MSG_SPMM_SUM | _MEAN */, int64_t m, int64_t n, int64_t k,
                              int64_t nnz, const int64_t *pntrb, const int64_t *pntre,
                              const isplib_stream_plan *plan /*host*/,
                              const float *y, int64_t ldy, float *z, int64_t ldz,
                              void *workspace, size_t workspace_bytes,
                              const isplib_epilogue *epilogue /*host, may be NULL*/, void *stream);
/*
 * The stream schedule for a dense operand of 16-bit elements (dtype: ISPLIB_DTYPE_BF16 | ISPLIB_DTYPE_F16), sum / mean.  The
 * SAME plans as fusedMM_csr_stream_hip (sum plans of 2, 4 or 8 streams; the weights stay the plan's fp32 `vals`), the same
 * geometry; a lane's gather is 8 bytes instead of 16, so a 64-column panel row is one 128-byte line instead of two.  Products,
 * sums and the mean's division are formed in fp32; a finished row is rounded ONCE, to nearest even, to `dtype` (hub rows keep
 * fp32 partial rows in the workspace and round in their fold): the result is the fp32 entry's on the widened operand, rounded
 * -- NaN stays NaN, bf16 keeps subnormals, fp16 overflows to +-Inf.  y: n x ldy and z: m x ldz elements of `dtype`.
 * Domain: isplib_stream16_serves(n, k, ldy, ldz, nnz), and y, z 4-byte aligned; anything outside returns ISPLIB_FAIL before any
 * launch.  No epilogue and no staged panels.  workspace: the partial rows only (a workspace of
 * isplib_spmm_stream_workspace_bytes(plan) bytes is accepted: the staging area it includes is not used).
 * isplib_stream16_native_pays is the measured rule of the layers above (profiles/stream16_ab.txt): nonzero for the classes of
 * calls (slot width x weighted plan) where EVERY run of this entry was faster than EVERY run of "convert to fp32, run the fp32
 * entry, convert back"; a class that does not meet that keeps converting by default.  As measured NO class meets it: the 8-byte
 * gather costs the address pipeline what the 16-byte one does (the loop is charged per gather instruction, not per line), the
 * loop carries 17.4 vector instructions per step against 13.4, and the two conversion passes it saves cost 0.035 ms at K = 64
 * -- so the entry is a capability (half the footprint of X, no fp32 copy), not a speed-up, and `auto` converts everywhere.
 */
#define ISPLIB_DTYPE_BF16 1
#define ISPLIB_DTYPE_F16  2
int    fusedMM_csr_stream16_hip(int32_t imessage /* ISPLIB_MSG_SPMM_SUM | _MEAN */, int dtype, int64_t m, int64_t n, int64_t k,
                                int64_t nnz, const int64_t *pntrb, const int64_t *pntre,
                                const isplib_stream_plan *plan /*host*/,
                                const void *y, int64_t ldy, void *z, int64_t ldz,
                                void *workspace, size_t workspace_bytes, void *stream);
static inline int isplib_stream16_native_pays(int streams, int weighted) {
   (void)streams; (void)weighted;
   return 0;      /* measured (Reddit shape, bf16, K = 64 / 128): (4, unit), (4, weighted), (2, weighted) lose or tie; the rest unmeasured */
}
int    isplib_stream16_auto(int streams, int weighted);      /* the same rule as a symbol (for hosts that cannot include this header) */
/*
 * The plain schedule (one CSR row per wavefront, fusedMM_csr_hip / fusedMM_csr_ordered_hip) for a dense operand of 16-bit
 * elements, sum / mean: a lane's 16-byte gather holds EIGHT columns, so a row of k columns takes half the gather instructions and
 * half the cache lines of the fp32 kernel -- and no fp32 copy of the operand is made.  Weights are fp32 (`val`, may be NULL: unit
 * weights); `row_order` (device, m int32, position -> row; NULL = index order) is fusedMM_csr_ordered_hip's.  The contract is
 * fusedMM_csr_stream16_hip's: products, sums and the mean's division in fp32, the finished row rounded ONCE to nearest even -- NaN
 * stays NaN, bf16 keeps subnormals, fp16 overflows to +-Inf; an empty row is 0.  No atomics: two launches give equal bits and any
 * row order gives the bits of index order.  Bit equality with "convert, run fusedMM_csr_hip, convert back" is NOT promised on
 * real-valued data: the two kernels cut a row into edge slots differently, so the fp32 value before rounding may differ in its
 * last bits (where the fp32 sums are exact in any order, e.g. small integers, the bits are equal).
 * Domain: isplib_rows16_serves(n, k, ldy, ldz); with a row order m < 2^31.  Refused before any launch: another message word
 * (max / min included: ISPLIB_NO_OPT_IMPL), and with ISPLIB_FAIL another dtype, a shape outside the domain, ldy < k or ldz < k, a
 * null operand, a y or z base that is not 4-byte aligned.  m == 0 or k == 0 succeeds without a launch.
 * isplib_rows16_native_pays is the measured rule of the layers above (profiles/rows16_ab.txt): a class of calls is
 * (operand beyond 256 MiB at 2 bytes per element or not) x (rows in a community order or not) x (weighted or not), and it is
 * nonzero for a class only where EVERY run of this entry was faster than EVERY run of the conversion route on every measured
 * shape of that class.
 */
int    fusedMM_csr_rows16_hip(int32_t imessage /* ISPLIB_MSG_SPMM_SUM | _MEAN */, int dtype /* ISPLIB_DTYPE_BF16 | _F16 */,
                              int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val /* fp32, may be NULL */,
                              const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                              const int32_t *row_order /* optional */, const void *y, int64_t ldy, void *z, int64_t ldz, void *stream);
static inline int isplib_rows16_native_pays(int64_t n, int64_t ldy, int ordered, int weighted) {
   /* measured (profiles/rows16_ab.txt: ogbn-products shape, Chung-Lu and SBM twin, bf16, K = 128 / 256; inside the Infinity Cache
    * the shape at a quarter and at a fiftieth of its size and a Cora-shaped graph, K = 16 ... 128): every class measured pays,
    * unit and weighted alike -- beyond 256 MiB in index order 0.46-0.48 of the conversion route's time, in a community order
    * 0.49-0.61, inside 256 MiB in index order 0.45-0.92 (the narrow, launch-bound end saves the two conversion launches).  The one
    * class not measured (inside 256 MiB AND a community order: the layers above never look for an order there) stays on convert. */
   const int beyond = n > 0 && ldy > 0 && (double)n * (double)ldy * 2.0 > 256.0 * 1048576.0;
   (void)weighted;
   return (beyond || !ordered) ? 1 : 0;
}
int    isplib_rows16_auto(int64_t n, int64_t ldy, int ordered, int weighted);      /* the same rule as a symbol */
int    isplib_rows16_domain(int64_t n, int64_t k, int64_t ldy, int64_t ldz);       /* isplib_rows16_serves as a symbol */
/*
 * fusedMM_csr_rows16_hip with one fp32 factor per COLUMN of the sparse operand instead of one weight per edge:
 *   z[i,:] = round16( sum over the edges e of row i of col_scale[indx[e]] * y[indx[e],:] ),   MEAN: divided by max(deg, 1).
 * col_scale: n fp32 values in device memory.  The kernel is fusedMM_csr_rows16_hip's weighted kernel, and only the place a lane
 * takes its edge's factor from differs (the table at the edge's column instead of val at the edge), so the result has, bit for bit,
 * the bits of fusedMM_csr_rows16_hip given val[e] = col_scale[indx[e]] -- without an nnz-long weight stream.  The use it was built
 * for: the backward of `mean` on an unweighted graph, A^T (diag(1 / max(deg, 1)) dY), with col_scale = 1 / max(deg, 1) of A's rows
 * and a 16-bit dY that is never widened or scaled in memory.  Contract, determinism and row order: fusedMM_csr_rows16_hip's.
 * Domain and refusals: fusedMM_csr_rows16_hip's, and col_scale == NULL with nnz > 0 is refused (ISPLIB_FAIL) before any launch.
 * isplib_rows16_colscale_native_pays is the measured rule of the layers above for the unit-weight mean backward
 * (profiles/rows16_colscale_ab.txt), over the classes (operand beyond 256 MiB at 2 bytes per element or not) x
 * (rows in a community order or not): nonzero only where EVERY run of the backward on this entry was faster than EVERY run of the
 * conversion route (widen dY, divide, the fp32 row kernel, narrow dX) on every measured shape of the class.
 */
int    fusedMM_csr_rows16_colscale_hip(int32_t imessage /* ISPLIB_MSG_SPMM_SUM | _MEAN */, int dtype /* ISPLIB_DTYPE_BF16 | _F16 */,
                                       int64_t m, int64_t n, int64_t k, int64_t nnz, const float *col_scale /* [dev] n */,
                                       const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                       const int32_t *row_order /* optional */, const void *y, int64_t ldy, void *z, int64_t ldz, void *stream);
static inline int isplib_rows16_colscale_native_pays(int64_t n, int64_t ldy, int ordered) {
   /* measured (profiles/rows16_colscale_ab.txt: rows16_ab's shapes, bf16, the backward of mean on an unweighted graph): every class
    * measured pays -- beyond 256 MiB in index order 0.54-0.65 of the conversion route's time, in a community order 0.52-0.64, inside
    * 256 MiB in index order 0.41-0.88 (a quarter of the products shape 0.57, the launch-bound end saves three launches).  The one class
    * not measured (inside 256 MiB AND a community order: the layers above never look for an order there) stays on convert. */
   const int beyond = n > 0 && ldy > 0 && (double)n * (double)ldy * 2.0 > 256.0 * 1048576.0;
   return (beyond || !ordered) ? 1 : 0;
}
int    isplib_rows16_colscale_auto(int64_t n, int64_t ldy, int ordered);           /* the same rule as a symbol */
/*
 * fusedMM_csr_rows16_colscale_hip's sum (col_scale == NULL: fusedMM_csr_rows16_hip's unit-weight sum) with an epilogue applied in fp32
 * to the finished row before it is rounded ONCE:
 *   z[i,c] = round16( act( rs_i * ( sum over the edges e of row i of cs[indx[e]] * y[indx[e],c] + ss_i * y[i,c] ) + bias[c] ) )
 * in this order: the sum (the bits of the entries above), one fmaf(ss_i, y[i,c], sum), * rs_i, + bias[c], act(v) = v > 0 ? v : 0 when
 * relu is nonzero (the fp32 epilogue's: -0.0 and NaN give +0.0).  Every member of the epilogue is optional; ep == NULL is all of them
 * absent.  The use it was built for: the fused GCN layer relu(D^-1/2 (A + I) D^-1/2 X + b) of a 16-bit X, cs = ss = rs = D^-1/2 -- no
 * pre-scaled copy of X in either width -- and its backward on A^T.  Sum only, no per-edge weights.  No atomics: two
 * launches give equal bits, any row order the bits of index order.  An empty row gets its epilogue too (nnz == 0 launches).
 * Domain and refusals: fusedMM_csr_rows16_hip's, and self_scale != NULL with m != n (the self row of i is y[i,:]); refused before any
 * launch, z untouched.  m == 0 or k == 0 succeeds without a launch.
 * isplib_rows16_gcn_native_pays is the measured rule of the layers above for the fused GCN layer (forward + backward,
 * profiles/rows16_gcn_ab.txt), over the classes (operand beyond 256 MiB at 2 bytes per element or not) x (rows in a community order
 * or not): nonzero only where EVERY native run was faster than EVERY run of the conversion route on every measured shape of the class.
 */
typedef struct isplib_epilogue16 {
   const float *row_scale;   /* [dev] m fp32, or NULL (= 1) */
   const float *self_scale;  /* [dev] m fp32, or NULL = no self term; non-NULL needs m == n: the self row of i is y[i,:] */
   const float *bias;        /* [dev] k fp32, or NULL */
   int          relu;        /* nonzero: v > 0 ? v : 0 */
} isplib_epilogue16;
int    fusedMM_csr_rows16_epilogue_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                       const float *col_scale /* [dev] n, or NULL = unit */, const int64_t *indx, const int64_t *pntrb,
                                       const int64_t *pntre, const int32_t *row_order /* optional */, const void *y, int64_t ldy, void *z,
                                       int64_t ldz, const isplib_epilogue16 *epilogue /* host, may be NULL */, void *stream);
static inline int isplib_rows16_gcn_native_pays(int64_t n, int64_t ldy, int ordered) {
   /* measured (profiles/rows16_gcn_ab.txt: rows16_ab's shapes and the Reddit shape, bf16, forward + backward with bias and ReLU): beyond
    * 256 MiB every native run is below every convert run -- in index order 0.48-0.57 of the conversion route's time, in a community order
    * 0.28-0.37.  Inside 256 MiB in index order five shapes win (0.49-0.89) but the Reddit shape loses at K = 32 and 48 (1.9-2.2 x: the
    * conversion route's fp32 layer runs there on the stream schedule), so the class loses; inside 256 MiB in a community order is not
    * produced by the layers above and was not measured.  Both stay on convert. */
   (void)ordered;
   return (n > 0 && ldy > 0 && (double)n * (double)ldy * 2.0 > 256.0 * 1048576.0) ? 1 : 0;
}
int    isplib_rows16_gcn_auto(int64_t n, int64_t ldy, int ordered);                /* the same rule as a symbol */
/*
 * The backward's dense prologue of the fused GCN layer in 16 bits (dtype: ISPLIB_DTYPE_BF16 | _F16; dz, out, g: n x k elements of 2
 * bytes at their pitches), one pass over dz (and out):
 *   g[i,c] = out ? (out[i,c] > 0 ? dz[i,c] : +0) : dz[i,c]          a bit copy or +0: nothing is rounded (g may be NULL)
 *   grad_bias[c] = sum_i widen(g[i,c])                              fp32 (may be NULL; else a workspace of
 *                                                                   isplib_masked_colsum16_workspace_bytes(n, k) bytes, 256-byte aligned)
 * No atomics: per-block partials folded in block order, bitwise reproducible.  With neither g nor grad_bias nothing runs.
 */
size_t isplib_masked_colsum16_workspace_bytes(int64_t n, int64_t k);
int    isplib_masked_colsum16_hip(int dtype, int64_t n, int64_t k, const void *dz, int64_t lddz, const void *out /*NULL: no mask*/, int64_t ldo,
                                  void *g /*[dev] n x ldg | NULL*/, int64_t ldg, float *grad_bias /*[dev] k fp32 | NULL*/, void *workspace,
                                  size_t workspace_bytes, void *stream);
/*
 * fusedMM_csr_rows16_hip's schedule for max / min of a 16-bit dense operand: one CSR row per wavefront, 16-byte gathers of eight
 * columns, the optional row order, no fp32 copy of the operand.  The halves are widened in registers and every comparison is fp32:
 * the candidate of an edge is val * y (ONE fp32 multiply; val = NULL: y itself) and replaces the running value only if strictly
 * better, so the first edge wins a tie (+0 and -0 tie) and NaN never wins -- the comparator of fusedMM_csr_hip, whose result does
 * not depend on how a row's edges are cut into slots.  The finished fp32 winner is rounded ONCE, to nearest even.  Widening is exact,
 * so values AND positions are BIT-EQUAL to "convert the operand, run fusedMM_csr_hip, convert back", on any data.  z: m x ldz
 * elements of `dtype`; z_arg (may be NULL): int64 at pitch ldarg, the CSR position of the winner, nnz where nothing won.  An empty
 * row is 0 (under isplib_hip_set_empty_row(1): the identity -+FLT_MAX, which rounds to -+Inf in both types), its position nnz; a
 * non-empty row in which nothing wins (all NaN, or all -Inf under max / +Inf under min) keeps -+FLT_MAX -> -+Inf, position nnz.
 * z_arg = NULL is a values-only launch: no position is tracked at all, the same value bits.  No atomics: two launches give equal
 * bits and any row order gives the bits of index order.
 * Domain: isplib_rows16_serves(n, k, ldy, ldz); with a row order m < 2^31.  Refused before any launch, outputs untouched: a message
 * word other than max / min (ISPLIB_NO_OPT_IMPL), and with ISPLIB_FAIL another dtype, a negative dimension, ldy, ldz or ldarg < k,
 * a shape outside the domain, a null operand, a y or z base that is not 4-byte aligned.  m == 0 or k == 0 succeeds without a launch.
 * isplib_rows16_minmax_native_pays is the measured rule of the layers above (profiles/rows16_minmax_ab.txt), over
 * the classes of isplib_rows16_native_pays x (positions wanted or not): nonzero only where EVERY run of this entry was faster than
 * EVERY run of the conversion route on every measured shape of the class.
 */
int    fusedMM_csr_rows16_minmax_hip(int32_t imessage /* ISPLIB_MSG_SPMM_MAX | _MIN */, int dtype /* ISPLIB_DTYPE_BF16 | _F16 */,
                                     int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val /* fp32, may be NULL */,
                                     const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                     const int32_t *row_order /* optional */, const void *y, int64_t ldy, void *z, int64_t ldz,
                                     int64_t *z_arg /* may be NULL */, int64_t ldarg, void *stream);
static inline int isplib_rows16_minmax_native_pays(int64_t n, int64_t ldy, int ordered, int weighted, int want_arg) {
   /* measured (profiles/rows16_minmax_ab.txt: rows16_ab's shapes, bf16, forward max, values only and with positions): beyond 256 MiB
    * every class pays, unit and weighted, with and without positions -- in index order 0.45-0.51 of the conversion route's time, in a
    * community order 0.45-0.73.  Inside 256 MiB in index order the class does NOT pay: a quarter of the products shape at K = 128
    * (0.46-0.51), a Cora-shaped graph (0.65-0.69) and a fiftieth of the shape at K = 64 (0.71-0.89) win every run, but the fiftieth
    * at K = 16 loses every run (1.03-1.20: two of a slot's eight lanes hold columns), so the whole class stays on convert; inside
    * 256 MiB in a community order was not measured. */
   const int beyond = n > 0 && ldy > 0 && (double)n * (double)ldy * 2.0 > 256.0 * 1048576.0;
   (void)ordered; (void)weighted; (void)want_arg;
   return beyond ? 1 : 0;
}
int    isplib_rows16_minmax_auto(int64_t n, int64_t ldy, int ordered, int weighted, int want_arg);   /* the same rule as a symbol */
/*
 * The value gradient of SpMM-sum / SpMM-mean (isplib_sddmm_csr_hip) for dense operands of 16-bit elements, on the schedule of
 * fusedMM_csr_rows16_hip: for the edges j of row i
 *   dval[j] = <y[indx[j], :], g[i, :]> * (mean ? 1 / max(deg_i, 1) : 1).
 * y: n x ldy and g: m x ldg elements of `dtype`, neither widened in memory (a gathered row of y is half the bytes of the fp32
 * kernel's); dval: nnz fp32 values in CSR order -- the weights of a 16-bit call are fp32, so nothing is rounded to 16 bits.
 * Widening is exact, products and sums are fp32, the mean multiplies the finished dot by the fp32 1.0f / deg as isplib_sddmm_csr_hip
 * does; nothing is flushed (bf16 operands whose products are fp32 subnormals keep them).  A lane sums at most 16 products and the
 * slot reduction adds at most 6 levels: every result lies within 1e-5 * <|y|, |g|> of the exact one (about 1.4e-6 in the worst
 * case), and where the fp32 sums are exact in any order (small integers) it is exact.  `row_order` (device, m int32, position ->
 * row; NULL = index order) is fusedMM_csr_ordered_hip's.  No atomics: two launches give equal bits and any row order gives the
 * bits of index order.  Bit equality with "widen both operands, run isplib_sddmm_csr_hip" is NOT promised on real-valued data: the
 * fp32 kernel cuts a row's columns into other slots.
 * Domain: isplib_sddmm_rows16_serves(n, k, ldy, ldg) -- isplib_rows16_serves with ldg in the output pitch's place, and
 * k <= ISPLIB_SDDMM_TASKS_K_MAX: a dot product cannot be cut into column panels, so g[row, :] in two chunks per lane is the widest
 * form.  With a row order m < 2^31.  Refused before any launch with ISPLIB_FAIL, dval untouched: another dtype, a negative
 * dimension, ldy < k or ldg < k, a shape outside the domain, a null operand, a y or g base that is not 4-byte aligned.  m == 0,
 * k == 0 or nnz == 0 succeeds without a launch.
 * isplib_sddmm_rows16_native_pays is the measured rule of the layers above (profiles/sddmm_rows16_ab.txt), over the
 * classes (y beyond 256 MiB at 2 bytes per element or not) x (rows in a community order or not): nonzero only where EVERY run of
 * this entry was faster than EVERY run of the conversion route (widen y and g, isplib_sddmm_csr_hip) on every measured shape of the
 * class.
 */
int    isplib_sddmm_csr_rows16_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                   const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                   const int32_t *row_order /* optional */, const void *y, int64_t ldy,
                                   const void *g, int64_t ldg, int mean, float *dval, void *stream);
static inline int isplib_sddmm_rows16_serves(int64_t n, int64_t k, int64_t ldy, int64_t ldg) {
   return k <= ISPLIB_SDDMM_TASKS_K_MAX && isplib_rows16_serves(n, k, ldy, ldg);
}
static inline int isplib_sddmm_rows16_native_pays(int64_t n, int64_t ldy, int ordered) {
   /* measured (profiles/sddmm_rows16_ab.txt: rows16_ab's shapes, bf16, the backward of sum and of mean with only the weights requiring
    * grad): beyond 256 MiB every run of both classes pays -- in index order 0.36-0.43 of the conversion route's time (0.39-0.46 of the
    * fp32 kernel alone on operands widened beforehand), in a community order 0.21-0.25.  Inside 256 MiB in index order a quarter of
    * the products shape at K = 128 (0.39-0.41), a fiftieth at K = 16 / 64 (0.51 / 0.29) and a Cora-shaped graph at K = 64 (0.69) win
    * every run, but on the Cora shape at K = 16 one native run (0.038 ms, the first) lies above the fastest conversion run (0.028 ms):
    * the class does NOT pay and stays on convert; inside 256 MiB in a community order was not measured. */
   const int beyond = n > 0 && ldy > 0 && (double)n * (double)ldy * 2.0 > 256.0 * 1048576.0;
   (void)ordered;
   return beyond ? 1 : 0;
}
int    isplib_sddmm_rows16_auto(int64_t n, int64_t ldy, int ordered);             /* the same rule as a symbol */
/*
 * Row-softmax attention aggregation over the stored entries e = (i, j) of a CSR matrix A [m, n], forward and backward, fp32.
 * With x: m x ldx, y: n x ldy (k columns each) and a scalar `scale` = p:
 *   s_e  = p <x_i, y_j>       a_e = exp(s_e - lse_i),  lse_i = log sum_{e in row i} exp(s_e)       z_i = sum_e a_e y_j
 * and, for g = dL/dz (m x ldg),
 *   D_i  = <g_i, z_i>         t_e = <g_i, y_j>         ds_e = a_e (t_e - D_i)
 *   dx_i = p sum_e ds_e y_j   dy_j = sum_{e -> j} (a_e g_i + p ds_e x_i).
 * Stored values of A are not read (attention replaces them); every stored entry is its own edge, so a duplicate counts twice; the
 * column order inside a row is free.  An empty row has z_i = 0, lse_i = -inf, dx_i = 0 and D_i = 0; a column no entry points at has
 * dy_j = 0.  The softmax is computed relative to a running row maximum, so no score overflows: a row of one entry returns y_j bit
 * for bit whatever its score.  A +inf score, or a NaN anywhere in a row's operands, makes that row NaN and no other.
 *   isplib_attention_csr_hip      writes z (m x ldz) and lse (m).
 *   isplib_attention_bw_rows_hip  reads x, y, g, z and lse, writes dx (m x lddx) and dsum (m: D_i, which the next entry reads).
 *   isplib_attention_bw_cols_hip  runs on the transposed structure (colb / cole: n column ranges into row_t, the row ids of the
 *                                 entries in column-major order -- no permutation is needed, nothing per edge was stored); reads
 *                                 x, y, g, lse and dsum, writes dy (n x lddy).
 * Nothing is kept per edge: the backward recomputes a_e from lse_i.  Outputs are write-only and every element of every row is
 * written (empty rows included), nothing between the rows of a pitched output.  One wave per row (per column), no atomics, a fixed
 * order of operations: two launches give equal bits.  The entries neither allocate nor synchronise.
 * Domain: isplib_attention_serves(rows_gathered, k, ld) for every GATHERED operand (y with n rows in the first two entries; x and
 * g with m rows in the third): 1 <= k <= 512 (a row sits in registers, two 16-byte chunks per lane), ld >= k, rows_gathered < 2^31
 * (32-bit row ids times the pitch) and the operand inside one buffer descriptor.  Outside the domain: ISPLIB_NO_OPT_IMPL.  A
 * negative dimension, a null operand or a pitch of a row-resident operand or output below k: ISPLIB_FAIL.  All refusals come before
 * any launch.  m == 0 or k == 0 (n == 0 or k == 0 in the third entry) succeeds without a launch.
 */
static inline int isplib_attention_serves(int64_t rows_gathered, int64_t k, int64_t ld) {
   return k >= 1 && k <= ISPLIB_ATTENTION_K_MAX && ld >= k && rows_gathered < (1LL << 31) && isplib_dense_in_descriptor(rows_gathered, ld);
}
int    isplib_attention_domain(int64_t rows_gathered, int64_t k, int64_t ld);     /* isplib_attention_serves as a symbol */
int    isplib_attention_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                float *z, int64_t ldz, float *lse /* m */, void *stream);
int    isplib_attention_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                    const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                    const float *g, int64_t ldg, const float *z, int64_t ldz, const float *lse, float *dx,
                                    int64_t lddx, float *dsum /* m */, void *stream);
int    isplib_attention_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                    const int64_t *cole, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                    const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy,
                                    void *stream);
/*
 * GAT attention aggregation over the stored entries e = (i, j) of a CSR matrix A [m, n], all heads in one launch, forward and
 * backward, fp32.  With y: n x ldy of k = heads * d columns (head h owns the columns [h*d, (h+1)*d)), the per-node scores
 * a_dst [m, heads] and a_src [n, heads] (dense: a row pitch of `heads`) and a slope `negative_slope` = ns, for every head h:
 *   u_e  = a_dst[i,h] + a_src[j,h]      s_e = u_e > 0 ? u_e : ns u_e
 *   a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_{e in row i} exp(s_e)          z_i[head h] = sum_e a_e y_j[head h]
 * and, for g = dL/dz (m x ldg),
 *   D[i,h] = <g_i, z_i>_h       t_e = <g_i, y_j>_h       du_e = a_e (t_e - D[i,h]) (u_e > 0 ? 1 : ns)
 *   d a_dst[i,h] = sum_e du_e   d a_src[j,h] = sum_{e -> j} du_e                   dy_j[head h] = sum_{e -> j} a_e g_i[head h].
 * This is the aggregation of GATConv (GATv2 is not: its nonlinearity sits inside the dot product).  Stored values of A are not read;
 * every stored entry is its own edge, so a duplicate counts twice; the column order inside a row is free.  u_e is one fp32 add, so
 * the slope branch is decided by the sign of the exact sum.  An empty row has z_i = 0, lse = -inf, D = 0 and d a_dst = 0; a column
 * no entry points at has dy_j = 0 and d a_src = 0.  The softmax is computed relative to a running maximum, so no score overflows: a
 * row of one entry returns y_j bit for bit and lse = s_e.  A NaN in y_j reaches the rows that reference j, a NaN in a_src[j,h] head h
 * of those rows, and nothing else.
 *   isplib_gat_csr_hip      writes z (m x ldz) and lse (m x heads).
 *   isplib_gat_bw_rows_hip  reads a_dst, y, a_src, g, z and lse, writes d_a_dst (m x heads) and dsum (m x heads: D, which the next
 *                           entry reads).
 *   isplib_gat_bw_cols_hip  runs on the transposed structure (colb / cole: n column ranges into row_t); reads a_dst, y, a_src, g,
 *                           lse and dsum, writes dy (n x lddy) and d_a_src (n x heads).
 * Nothing is kept per edge: the backward recomputes a_e from lse.  Outputs are write-only and every element of every row is
 * written, nothing between the rows of a pitched output.  One wave per row (per column), no atomics, no LDS, a fixed order of
 * operations: two launches give equal bits.  The entries neither allocate nor synchronise.
 * Domain: isplib_gat_serves(rows_gathered, heads, d, ld) for the GATHERED wide operand (y with n rows in the first two entries, g
 * with m rows in the third): 1 <= heads, 1 <= d, heads * d <= 512; heads == 1 (any d) or d a power of two >= 4 (a head is then an
 * aligned group of lanes and a lane's four columns never straddle heads); ld >= heads * d; rows_gathered < 2^31 and the operand
 * inside one buffer descriptor.  Outside the domain: ISPLIB_NO_OPT_IMPL.  A negative dimension, a null operand, a k that is no
 * multiple of heads, or a pitch of a row-resident operand or output below k: ISPLIB_FAIL.  All refusals come before any launch.
 * m == 0 or k == 0 (n == 0 or k == 0 in the third entry) succeeds without a launch.
 */
#define ISPLIB_GAT_K_MAX               512          /* heads * d: a row sits in registers, two 16-byte chunks per lane */
static inline int isplib_gat_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   if (heads < 1 || d < 1 || heads > ISPLIB_GAT_K_MAX || d > ISPLIB_GAT_K_MAX || heads * d > ISPLIB_GAT_K_MAX) return 0;
   if (heads > 1 && (d < 4 || (d & (d - 1)) != 0)) return 0;
   return ld >= heads * d && rows_gathered < (1LL << 31) && isplib_dense_in_descriptor(rows_gathered, ld);
}
int    isplib_gat_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_gat_serves as a symbol */
int    isplib_gat_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                          const int64_t *pntre, const float *a_dst /* m x heads */, const float *y, int64_t ldy,
                          const float *a_src /* n x heads */, int64_t heads, float negative_slope, float *z, int64_t ldz,
                          float *lse /* m x heads */, void *stream);
int    isplib_gat_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                              const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                              int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz,
                              const float *lse, float *d_a_dst /* m x heads */, float *dsum /* m x heads */, void *stream);
int    isplib_gat_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                              const int64_t *cole, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                              int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *lse,
                              const float *dsum, float *dy, int64_t lddy, float *d_a_src /* n x heads */, void *stream);
/*
 * The GAT aggregation above with a per-edge score term (GATConv's edge_dim), fp32: a_edge [nnz, heads] (dense: a row pitch of
 * `heads`), one row per stored entry IN CSR POSITION ORDER -- row e of a_edge belongs to the entry indx[e] -- and
 *   u_e  = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h]       TWO fp32 adds, in this order, in all three entries
 *   s_e, a_e, lse, z, D, t_e, du_e, d a_dst, d a_src, dy  as above          d a_edge[e,h] = du_e
 * The slope branch is taken on this fp32 u_e (u_e == 0 takes ns): with three terms its sign is no longer the sign of the exact sum,
 * so the order of the adds is part of the contract -- the forward and both backward entries agree on the branch of every edge.
 * Every stored entry is its own edge: duplicates (i, j) each have their own a_edge row.  With a_edge = 0 the results are those of the
 * entries above bit for bit ((a + b) + 0 is exact).  A NaN in a_edge[e,h] reaches head h of row i(e) and nothing else.
 *   isplib_gat_edge_csr_hip      isplib_gat_csr_hip with `a_edge` after `a_src`; a_edge is a streamed read.
 *   isplib_gat_edge_bw_rows_hip  isplib_gat_bw_rows_hip with `a_edge` after `a_src` and a TRAILING `d_a_edge` (nnz x heads, after
 *                                `stream`), which may be NULL: then nothing per edge is written.  Otherwise every element of
 *                                d_a_edge is written exactly once (write-only).
 *   isplib_gat_edge_bw_cols_hip  isplib_gat_bw_cols_hip with `csr2csc` after `cole` (int64 [nnz]: the CSR position of every entry of
 *                                the transposed structure, what isplib_csr2csc_hip writes as its permutation) and `a_edge` after
 *                                `a_src`; a_edge[csr2csc[q], h] is a 4-byte gather behind one descriptor.  A csr2csc value outside
 *                                [0, nnz) reads as 0, never outside a_edge.
 * Domain: isplib_gat_serves as above AND isplib_gat_edge_serves(nnz, heads): 1 <= heads, 0 <= nnz < 2^31 and a_edge inside one buffer
 * descriptor, nnz * heads * 4 <= ISPLIB_DENSE_BYTES_MAX (the way out: fewer heads per call, on column views of y).  Outside either:
 * ISPLIB_NO_OPT_IMPL; null operands (a_edge or csr2csc with nnz > 0 included) and the refusals above: ISPLIB_FAIL; all before any
 * launch.  Nothing outside [0, nnz * heads) of a_edge is read.
 */
static inline int isplib_gat_edge_serves(int64_t nnz, int64_t heads) {
   return heads >= 1 && nnz >= 0 && nnz < (1LL << 31) && isplib_dense_in_descriptor(nnz, heads);
}
int    isplib_gat_edge_domain(int64_t nnz, int64_t heads);                        /* isplib_gat_edge_serves as a symbol */
int    isplib_gat_edge_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                               const int64_t *pntre, const float *a_dst /* m x heads */, const float *y, int64_t ldy,
                               const float *a_src /* n x heads */, const float *a_edge /* nnz x heads */, int64_t heads,
                               float negative_slope, float *z, int64_t ldz, float *lse /* m x heads */, void *stream);
int    isplib_gat_edge_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                   const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                   const float *a_edge, int64_t heads, float negative_slope, const float *g, int64_t ldg,
                                   const float *z, int64_t ldz, const float *lse, float *d_a_dst /* m x heads */,
                                   float *dsum /* m x heads */, void *stream, float *d_a_edge /* nnz x heads, or NULL */);
int    isplib_gat_edge_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                   const int64_t *cole, const int64_t *csr2csc /* nnz */, const float *a_dst, const float *y,
                                   int64_t ldy, const float *a_src, const float *a_edge, int64_t heads, float negative_slope,
                                   const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy,
                                   float *d_a_src /* n x heads */, void *stream);
/*
 * The GAT aggregation above with attention dropout (GATConv's `dropout`: the coefficients are dropped after the softmax, per stored
 * entry and per head), fp32, with or without the per-edge term.  With the keep bit q_e,h in {0, 1} and c = `scale` =
 * float32(1 / (1 - p)):
 *   a_e, lse, s_e, u_e   exactly as without dropout: the softmax runs over ALL stored entries, lse does not see the mask
 *   z_i[head h]  = c sum_e q_e a_e y_j[head h]            D[i,h] = <g_i, z_i>_h  (= sum_e a_e t_e)
 *   t_e          = q_e c <g_i, y_j>_h                     du_e   = a_e (t_e - D[i,h]) slope_e      (a dropped edge still gets -a_e D slope)
 *   d a_dst, d a_src, d a_edge  sums of du_e as above     dy_j[head h] = c sum_{e -> j} q_e a_e g_i[head h]
 * The keep bit is a pure function of (seed, CSR position of the entry, head), recomputed in all three entries -- no mask is stored, no
 * RNG state is kept, and equal arguments give equal bits:
 *   fmix32(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16                  (uint32 arithmetic)
 *   word(seed, pos, h) = fmix32( fmix32(uint32(pos) ^ uint32(seed)) + uint32(h) * 0x9E3779B9 + uint32(seed >> 32) )
 *   T(p) = min(2^32 - 1, floor(p * 2^32))  in double           q = word >= T                               T(0) = 0 keeps everything
 * isplib_gat_drop_threshold(p) is T(p) and isplib_gat_drop_word(seed, pos, head) is `word` (host functions; isplib_amd/csrc/
 * gat_dropout.h states both for the kernels and the host).  seed < 2^63, pos < 2^31 (the position in indx), heads numbered from 0.
 * Every stored entry has its own bit, duplicates (i, j) included.  An empty row has z = 0, lse = -inf, D = 0; a row whose entries are
 * all dropped for head h has z = 0 exactly there and a finite lse.  With threshold = 0 and scale = 1 the results are those of the
 * entries without dropout bit for bit.
 *   isplib_gat_drop_csr_hip      the arguments of isplib_gat_edge_csr_hip, then threshold, scale, seed.
 *   isplib_gat_drop_bw_rows_hip  the arguments of isplib_gat_edge_bw_rows_hip (d_a_edge after stream), then threshold, scale, seed.
 *   isplib_gat_drop_bw_cols_hip  the arguments of isplib_gat_edge_bw_cols_hip, then threshold, scale, seed; csr2csc is REQUIRED (the
 *                                keep bit is a function of the CSR position), with or without a_edge.
 * a_edge may be NULL in all three (and d_a_edge with it): then there is no per-edge term, u_e = a_dst[i,h] + a_src[j,h].
 * Domain: isplib_gat_serves; with a_edge also isplib_gat_edge_serves.  Outside: ISPLIB_NO_OPT_IMPL.  A scale that is not a positive
 * finite number, a null csr2csc with nnz > 0, and the refusals of the entries above: ISPLIB_FAIL; all before any launch.
 */
uint32_t isplib_gat_drop_threshold(double p);
uint32_t isplib_gat_drop_word(uint64_t seed, int64_t pos, int64_t head);
int    isplib_gat_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                               const int64_t *pntre, const float *a_dst /* m x heads */, const float *y, int64_t ldy,
                               const float *a_src /* n x heads */, const float *a_edge /* nnz x heads, or NULL */, int64_t heads,
                               float negative_slope, float *z, int64_t ldz, float *lse /* m x heads */, void *stream,
                               uint32_t threshold, float scale, uint64_t seed);
int    isplib_gat_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                   const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                   const float *a_edge /* or NULL */, int64_t heads, float negative_slope, const float *g,
                                   int64_t ldg, const float *z, int64_t ldz, const float *lse, float *d_a_dst /* m x heads */,
                                   float *dsum /* m x heads */, void *stream, float *d_a_edge /* nnz x heads, or NULL */,
                                   uint32_t threshold, float scale, uint64_t seed);
int    isplib_gat_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                   const int64_t *cole, const int64_t *csr2csc /* nnz */, const float *a_dst, const float *y,
                                   int64_t ldy, const float *a_src, const float *a_edge /* or NULL */, int64_t heads,
                                   float negative_slope, const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy,
                                   int64_t lddy, float *d_a_src /* n x heads */, void *stream, uint32_t threshold, float scale,
                                   uint64_t seed);
/*
 * The row-softmax attention aggregation above for dense operands of 16-bit elements (dtype: ISPLIB_DTYPE_BF16 | _F16), forward and
 * backward, on the same mapping (one wave per row or column, one 16-byte gather of EIGHT columns per lane and edge, one chunk per
 * lane).  x, y and g are `dtype` and no operand is widened in memory; widening is exact, every product, sum, exponential and division
 * is fp32, and z, dx and dy are rounded ONCE, to nearest even, to `dtype` (an fp16 result beyond 65504 rounds to Inf as the cast does;
 * nothing is clamped or flushed).  lse and dsum (D_i) stay fp32.  The special values are the fp32 entries': an empty row has z_i = 0,
 * lse_i = -inf, dx_i = 0, D_i = 0; a column no entry points at has dy_j = 0; a row of one entry returns y_j's 16 bits unchanged; a
 * +inf score, or a NaN anywhere in a row's operands, makes that row NaN and no other.
 *   isplib_attention16_csr_hip      writes z (m x ldz, `dtype`) and lse (m, fp32).
 *   isplib_attention16_bw_rows_hip  reads x, y, g and lse -- NOT z: the rounded z would carry u * sum_c |g_ic z_ic| into every ds_e
 *                                   through D_i = <g_i, z_i>.  D_i = sum_e a_e t_e is formed in fp32 from the row's own edges, in the
 *                                   same pass as dx (D_i = Dacc / l, dx_i = p (A1 - D_i Z) with l = sum a_e, Dacc = sum a_e t_e,
 *                                   Z = sum a_e y_j, A1 = sum a_e t_e y_j).  Writes dx (m x lddx, `dtype`) and dsum (m, fp32).
 *   isplib_attention16_bw_cols_hip  on the transposed structure; reads x, y, g, lse and dsum, writes dy (n x lddy, `dtype`).
 * Nothing is kept per edge and autograd needs x, y and lse only.  Outputs are write-only, every element of every row is written,
 * nothing between the rows of a pitched output, nothing outside a row's k columns is used (a head view of a wider tensor goes in as
 * it lies).  No atomics, no LDS, a fixed order of operations: two launches give equal bits.  The entries neither allocate nor
 * synchronise.
 * Domain: isplib_attention16_serves(rows_gathered, k, ld) for every GATHERED operand (y with n rows in the first two entries; x and g
 * with m rows in the third): 8 <= k <= 512 (a lane holds eight columns, one chunk per lane), k and the pitch even, ld >= k,
 * rows_gathered < 2^31 and the operand inside one buffer descriptor at 2 bytes per element; the pitches of the row-resident operands
 * and of the output must be even too.  Outside the domain: ISPLIB_NO_OPT_IMPL.  Another dtype, a negative dimension, a null operand, a
 * pitch of a row-resident operand or output below k, or a 16-bit base that is not 4-byte aligned: ISPLIB_FAIL.  All refusals come
 * before any launch and leave the outputs untouched.  m == 0 or k == 0 (n == 0 or k == 0 in the third entry) succeeds without a launch.
 * isplib_attention16_native_pays is the measured rule of the layers above (forward + backward against "widen, the fp32 entries,
 * narrow"; profiles/attention16_ab.txt), over the family's classes (the gathered operand beyond 256 MiB at 2 bytes per
 * element or not): nonzero only where EVERY native run was faster than EVERY run of the conversion route on every measured shape of the
 * class.
 */
#define ISPLIB_ATTENTION16_K_MIN       8            /* a lane gathers eight columns */
#define ISPLIB_ATTENTION16_K_MAX       512          /* one 16-byte chunk per lane, 64 lanes */
static inline int isplib_attention16_serves(int64_t rows_gathered, int64_t k, int64_t ld) {
   return k >= ISPLIB_ATTENTION16_K_MIN && k <= ISPLIB_ATTENTION16_K_MAX && (k % 2) == 0 && (ld % 2) == 0 && ld >= k &&
          rows_gathered < (1LL << 31) && isplib_rows_within(rows_gathered, ld, 2ull * ISPLIB_DENSE_BYTES_MAX);
}
int    isplib_attention16_domain(int64_t rows_gathered, int64_t k, int64_t ld);   /* isplib_attention16_serves as a symbol */
int    isplib_attention16_csr_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                  const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const void *x, int64_t ldx,
                                  const void *y, int64_t ldy, float scale, void *z, int64_t ldz, float *lse /* m */, void *stream);
int    isplib_attention16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                      const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy, float scale,
                                      const void *g, int64_t ldg, const float *lse, void *dx, int64_t lddx, float *dsum /* m */,
                                      void *stream);
int    isplib_attention16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                      const int64_t *cole, const void *x, int64_t ldx, const void *y, int64_t ldy, float scale,
                                      const void *g, int64_t ldg, const float *lse, const float *dsum, void *dy, int64_t lddy,
                                      void *stream);
static inline int isplib_attention16_native_pays(int64_t rows_gathered, int64_t ld) {
   /* measured (profiles/attention16_ab.txt: the Reddit shape at K = 64 and 128 -- gathered operand inside 256 MiB -- and the ogbn-products
    * shape at K = 128 -- beyond it; bf16, forward + backward, 5 alternating runs of 5 steps): every native run is below every run of the
    * conversion route in both classes -- 0.51-0.52 of its time inside 256 MiB, 0.55 beyond (forward alone 0.47-0.52), at 0.09-0.10 of its
    * peak memory.  Both classes pay. */
   return (rows_gathered > 0 && ld > 0) ? 1 : 0;
}
int    isplib_attention16_auto(int64_t rows_gathered, int64_t ld);                /* the same rule as a symbol */
/*
 * The GAT attention aggregation above (isplib_gat_*) for a wide operand of 16-bit elements (dtype: ISPLIB_DTYPE_BF16 | _F16), all heads
 * in one launch, forward and backward, on the mapping of the 16-bit attention entries (one wave per row or column, one 16-byte gather
 * of EIGHT columns per lane and edge, one chunk per lane).  y, g, z and dy are `dtype` and are never widened in memory; widening is
 * exact, every product, sum, exponential and division is fp32, and z and dy are rounded ONCE, to nearest even, to `dtype`.  a_dst,
 * a_src, lse, dsum (D), d_a_dst and d_a_src are fp32 [rows, heads] tables exactly as in the fp32 entries (1/d of y), so u_e is one fp32
 * add and the slope branch is decided by the sign of the exact sum.  The special values are the fp32 entries': an empty row has
 * z_i = 0, lse = -inf, D = 0, d a_dst = 0; a column no entry points at has dy_j = 0 and d a_src = 0; a row of one entry returns y_j's
 * 16 bits unchanged and lse = s_e; a NaN in a_src[j,h] reaches head h of the rows that reference j and nothing else.
 *   isplib_gat16_csr_hip      writes z (m x ldz, `dtype`) and lse (m x heads, fp32).
 *   isplib_gat16_bw_rows_hip  reads a_dst, y, a_src, g and lse -- NOT z: the rounded z would carry u * sum_c |g_ic z_ic| into every du_e
 *                             through D = <g_i, z_i>_h.  In one pass over the row's edges it forms, per head, l = sum a_e, Dacc = sum a_e
 *                             t_e, P = sum a_e sl_e t_e and Q = sum a_e sl_e (sl_e the slope, t_e = <g_i, y_j>_h), then D = Dacc / l and
 *                             d a_dst = P - D Q.  Writes d_a_dst and dsum (both m x heads, fp32).
 *   isplib_gat16_bw_cols_hip  on the transposed structure; reads a_dst, y, a_src, g, lse and dsum, writes dy (n x lddy, `dtype`) and
 *                             d_a_src (n x heads, fp32).
 * Nothing is kept per edge and autograd needs y, the two score tables and lse only.  Outputs are write-only, every element of every row
 * is written, nothing between the rows of a pitched output, nothing outside a row's k columns is used.  No atomics, no LDS, a fixed
 * order of operations: two launches give equal bits.  The entries neither allocate nor synchronise.
 * Domain: isplib_gat16_serves(rows_gathered, heads, d, ld) for the GATHERED wide operand (y with n rows in the first two entries, g
 * with m rows in the third): 1 <= heads, 8 <= heads * d <= 512 (a lane holds eight columns, one chunk per lane); heads == 1 with d
 * even, or d a power of two >= 8 (a head is then an aligned group of d / 8 lanes and a lane's eight columns never straddle heads);
 * ld even and >= heads * d; rows_gathered < 2^31 and the operand inside one buffer descriptor at 2 bytes per element; the pitches of
 * the row-resident operand and of the wide output must be even too.  Outside the domain: ISPLIB_NO_OPT_IMPL.  Another dtype, a negative
 * dimension, a null operand, a k that is no multiple of heads, a pitch of a row-resident operand or output below k, or a 16-bit base
 * that is not 4-byte aligned: ISPLIB_FAIL.  All refusals come before any launch and leave the outputs untouched.  m == 0 or k == 0
 * (n == 0 or k == 0 in the third entry) succeeds without a launch.
 * isplib_gat16_native_pays is the measured rule of the layers above (forward + backward against "widen, the fp32 entries, narrow";
 * profiles/gat16_ab.txt), over the family's classes (the gathered operand beyond 256 MiB at 2 bytes per element or
 * not): nonzero only where EVERY native run was faster than EVERY run of the conversion route on every measured shape of the class.
 */
#define ISPLIB_GAT16_K_MIN             8            /* heads * d: a lane gathers eight columns */
#define ISPLIB_GAT16_K_MAX             512          /* heads * d: one 16-byte chunk per lane, 64 lanes */
static inline int isplib_gat16_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   if (heads < 1 || d < 1 || heads > ISPLIB_GAT16_K_MAX || d > ISPLIB_GAT16_K_MAX) return 0;
   if (heads * d < ISPLIB_GAT16_K_MIN || heads * d > ISPLIB_GAT16_K_MAX) return 0;
   if (heads == 1 ? (d % 2) != 0 : (d < 8 || (d & (d - 1)) != 0)) return 0;
   return (ld % 2) == 0 && ld >= heads * d && rows_gathered < (1LL << 31) &&
          isplib_rows_within(rows_gathered, ld, 2ull * ISPLIB_DENSE_BYTES_MAX);
}
int    isplib_gat16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_gat16_serves as a symbol */
int    isplib_gat16_csr_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                            const int64_t *pntrb, const int64_t *pntre, const float *a_dst /* m x heads */, const void *y, int64_t ldy,
                            const float *a_src /* n x heads */, int64_t heads, float negative_slope, void *z, int64_t ldz,
                            float *lse /* m x heads */, void *stream);
int    isplib_gat16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                const int64_t *pntre, const float *a_dst, const void *y, int64_t ldy, const float *a_src, int64_t heads,
                                float negative_slope, const void *g, int64_t ldg, const float *lse, float *d_a_dst /* m x heads */,
                                float *dsum /* m x heads */, void *stream);
int    isplib_gat16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                const int64_t *cole, const float *a_dst, const void *y, int64_t ldy, const float *a_src, int64_t heads,
                                float negative_slope, const void *g, int64_t ldg, const float *lse, const float *dsum, void *dy,
                                int64_t lddy, float *d_a_src /* n x heads */, void *stream);
static inline int isplib_gat16_native_pays(int64_t rows_gathered, int64_t ld) {
   /* measured (profiles/gat16_ab.txt: the Reddit shape at (H, d) = (8, 8) and (8, 16) -- gathered operand inside 256 MiB -- and the
    * ogbn-products shape at (8, 16) -- beyond it; bf16, forward + backward, 5 alternating runs of 5 steps): every native run is below every
    * run of the conversion route in both classes -- 0.63-0.68 of its time inside 256 MiB, 0.62 beyond (forward alone 0.57-0.60), at
    * 0.19-0.24 of its peak memory.  Both classes pay. */
   return (rows_gathered > 0 && ld > 0) ? 1 : 0;
}
int    isplib_gat16_auto(int64_t rows_gathered, int64_t ld);                      /* the same rule as a symbol */
/*
 * GATv2 attention aggregation over the stored entries e = (i, j) of a CSR matrix A [m, n], all heads in one launch, forward and
 * backward, fp32.  With x: m x ldx (the target side, the wave's own row), y: n x ldy (the source side: gathered, and what is
 * aggregated), both of k = heads * d columns (head h owns the columns [h*d, (h+1)*d)), att: heads x d (k contiguous floats) and a
 * slope `negative_slope` = ns, for every head h and c over the head's columns:
 *   u_ec = x_ic + y_jc         sl_ec = u_ec > 0 ? 1 : ns       v_ec = sl_ec u_ec           s_e = sum_c att_c v_ec
 *   a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_{e in row i} exp(s_e)                  z_i[head h] = sum_e a_e y_j[head h]
 * and, for g = dL/dz (m x ldg),
 *   D[i,h] = <g_i, z_i>_h      t_e = <g_i, y_j>_h              ds_e = a_e (t_e - D[i,h])   q_ec = ds_e att_c sl_ec
 *   dx_ic  = sum_e q_ec        dy_jc = sum_{e -> j} (a_e g_ic + q_ec)                      datt_c = sum_{all e} ds_e v_ec.
 * This is the aggregation of GATv2Conv: the nonlinearity sits inside the dot product, so the score is no sum of per-node scalars
 * and isplib_gat_csr_hip cannot express it.  Stored values of A are not read; every stored entry is its own edge, so a duplicate
 * counts twice; the column order inside a row is free.  u_ec is one fp32 add, so the slope branch is decided by the sign of the
 * exact sum; u_ec == 0 takes ns.  An empty row has z_i = 0, lse = -inf, D = 0 and dx_i = 0; a column no entry points at has
 * dy_j = 0.  The softmax is computed relative to a running maximum, so no score overflows: a row of one entry returns y_j bit for
 * bit.  A NaN in y_jc reaches the head of c in the rows that reference j, and nothing else.
 *   isplib_gatv2_csr_hip      writes z (m x ldz) and lse (m x heads).
 *   isplib_gatv2_bw_rows_hip  reads x, y, att, g, z and lse, writes dx (m x lddx) and dsum (m x heads: D, which the next entry
 *                             reads) and, where datt is not NULL, datt (k floats): every block of the kernel writes one partial
 *                             row into `workspace` (at least isplib_gatv2_bw_rows_workspace_bytes(m, k) bytes, 256-byte aligned;
 *                             too small: ISPLIB_NOT_ENOUGH_MEM) and a second kernel adds the rows up in a fixed order.  datt ==
 *                             NULL runs a kernel without that sum and ignores the workspace.
 *   isplib_gatv2_bw_cols_hip  runs on the transposed structure (colb / cole: n column ranges into row_t); reads x, y, att, g, lse
 *                             and dsum, writes dy (n x lddy).
 * Nothing is kept per edge: the backward recomputes a_e from lse.  Outputs and the workspace are write-only and every element of
 * every row is written, nothing between the rows of a pitched output.  One wave per row (per column), no atomics, a fixed order of
 * operations: two launches give equal bits, datt included.  The entries neither allocate nor synchronise.
 * Domain: isplib_gatv2_serves(rows_gathered, heads, d, ld) = isplib_gat_serves, for every GATHERED wide operand (y with n rows in
 * the first two entries; x and g with m rows in the third).  Outside the domain: ISPLIB_NO_OPT_IMPL.  A negative dimension, a null
 * operand, a k that is no multiple of heads, or a pitch of a row-resident operand or output below k: ISPLIB_FAIL.  All refusals
 * come before any launch.  m == 0 or k == 0 (n == 0 or k == 0 in the third entry) succeeds without a launch and writes nothing.
 */
static inline int isplib_gatv2_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gat_serves(rows_gathered, heads, d, ld);
}
int    isplib_gatv2_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_gatv2_serves as a symbol */
int    isplib_gatv2_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                            const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy,
                            const float *att /* heads x d */, int64_t heads, float negative_slope, float *z, int64_t ldz,
                            float *lse /* m x heads */, void *stream);
size_t isplib_gatv2_bw_rows_workspace_bytes(int64_t m, int64_t k);
int    isplib_gatv2_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz,
                                const float *lse, float *dx, int64_t lddx, float *dsum /* m x heads */, float *datt /* k, or NULL */,
                                void *workspace, size_t workspace_bytes, void *stream);
int    isplib_gatv2_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                const int64_t *cole, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *lse,
                                const float *dsum, float *dy, int64_t lddy, void *stream);
/*
 * Staged column panels (sum / mean on 64-column slots only).  What a gather of a 128-byte line costs depends on the line's
 * ADDRESS: profiles/line_classes.txt (scripts/ubench/line_classes.hip) is the table, DESIGN.md section 5 reads it.  Before the
 * dispatches of a panel whose lines sit in a slow class, fusedMM_csr_stream_hip may copy the panel's 64 columns into the tail
 * of its workspace -- rows at a 512-byte pitch, data in bytes 0..255 of every 512, base 512-byte aligned: the address pattern
 * of columns 0..63 of a contiguous K=128 operand -- and gather from the copy.  Same kernel, same plan, same order of additions:
 * the result is the same bit for bit.  The copy is made inside every call that stages; nothing is kept between calls.
 * isplib_spmm_stream_workspace_bytes includes the staging area (cols * 512 + 512 bytes behind the partial rows, for 4-stream
 * plans, while that is at most ISPLIB_STREAM_STAGE_BYTES_MAX); a workspace that only holds the partial rows is served
 * unstaged.  max / min and the FusedMM words never stage.
 * isplib_stream_stage_panel is THE rule, for the panel of columns [c0, c0 + 64) of an n x k operand at y_addr with leading
 * dimension ldy (it looks at the address y_addr + 4 * c0, not at the column number: a column view of a wider tensor gets the
 * answer of its own bytes); room_bytes: what the workspace holds behind the partial rows, from the first 512-byte boundary on.
 *   eligible: a whole 64-column panel of a 4-stream plan, a row pitch that is a multiple of 512 bytes, the panel's first byte
 *             256-byte aligned (so its two lines keep their class in every row), the copy fits (n * 512 <= room_bytes and
 *             <= ISPLIB_STREAM_STAGE_BYTES_MAX)
 *   mode ISPLIB_STAGE_OFF: never; ISPLIB_STAGE_FORCE: every eligible panel (A/B runs, tests); ISPLIB_STAGE_AUTO: an eligible
 *             panel some of whose lines are in the slow class, and whose launch is large enough for the copy to pay:
 *             nnz >= n * ISPLIB_STREAM_STAGE_MIN_DEGREE (profiles/stream_stage_panels.txt: the copy's time against the
 *             per-panel gain).
 *   the slow class (profiles/line_classes.txt): address bits [9:7] = 011 -- bit 10 does not matter, 111 is as fast as the
 *             rest -- and only for lines that come from beyond the L2.  A 256-byte aligned panel holds such lines when its
 *             address has bit 8 set (its second line then has bits [8:7] = 11) and bit 9 is clear in some row: in every
 *             other row when the pitch is an odd multiple of 512 bytes, in every row or in none -- by bit 9 of the panel's
 *             own address -- when the pitch is a multiple of 1024.  The copy's lines have bits [8:7] = 00 and 01: never slow.
 * The process-wide mode is read once from the environment: ISPLIB_STREAM_STAGE=auto|0|1 (unset: auto; the A/B that made the rule
 * the default is profiles/stream_stage_panels.txt: Reddit shape, K=128, 2.686 -> 2.528 ms).
 */
#define ISPLIB_STAGE_OFF   0
#define ISPLIB_STAGE_FORCE 1
#define ISPLIB_STAGE_AUTO  2
#define ISPLIB_STREAM_STAGE_PITCH      512            /* bytes between rows of the staged copy */
#define ISPLIB_STREAM_STAGE_BYTES_MAX  (1u << 30)     /* no staging area beyond 1 GiB */
#define ISPLIB_STREAM_STAGE_MIN_DEGREE 128            /* auto: stored entries per row of y from which the copy pays: it costs 0.0204 ms and
                                                         the panel gains 0.175 ms at nnz / n = 492, even at 57; twice that, rounded up */
static inline int isplib_stream_stage_panel(uint64_t y_addr, int64_t ldy, int64_t c0, int64_t k, int streams, int64_t n, int64_t nnz,
                                            uint64_t room_bytes, int mode) {
   const uint64_t addr = y_addr + 4u * (uint64_t)c0;
   if (mode == ISPLIB_STAGE_OFF || streams != 4 || n <= 0 || c0 < 0 || c0 + 64 > k) return 0;
   if (((uint64_t)ldy * 4u) % ISPLIB_STREAM_STAGE_PITCH != 0 || (addr & 255u) != 0) return 0;
   if ((uint64_t)n > ISPLIB_STREAM_STAGE_BYTES_MAX / ISPLIB_STREAM_STAGE_PITCH || (uint64_t)n * ISPLIB_STREAM_STAGE_PITCH > room_bytes) return 0;
   if (mode == ISPLIB_STAGE_FORCE) return 1;
   if ((addr & 256u) == 0 || ((((uint64_t)ldy * 4u) % 1024u) == 0 && (addr & 512u) != 0)) return 0;      /* no line with bits [9:7] = 011 */
   return nnz / n >= ISPLIB_STREAM_STAGE_MIN_DEGREE;
}

/*
 * The two SDDMM-fused words of the generic pipeline that graph embedding runs on -- COPY_RHS|DOT|UDEF|MUL|ADD (sigmoid embedding,
 * attention scores: z_i = sum_j f(<x_i, y_j>) y_j) and SUBR|NORMR|UDEF|MUL|ADD (t-distribution: z_i = sum_j f(|y_j - x_i|^2)
 * (y_j - x_i)), f from enum isplib_sop_udef -- on the stream schedule's front end: rows of x and of z resident in LDS, a slot as
 * wide as the row (k <= 128: the reduce stage needs the whole row), four steps' dot products summed by one transposed
 * butterfly.  Reddit shape, K=128: the task-list form (fusedMM_csr_udef_tasks_hip) takes 6.3 ms.  Same result as
 * fusedMM_csr_udef_hip up to the order of the sums (bitwise reproducible from run to run); edge weights are not read (SOP is
 * the user function).  Plans: isplib_stream_plan_build_fusedmm_hip (its own geometry: isplib_fusedmm_stream_geometry; streams
 * 2 / 4 / 8 = slots of 128 / 64 / 32 columns); isplib_suggest_fusedmm_stream is the rule (0: stay on the task list);
 * workspace: isplib_spmm_stream_workspace_bytes(plan).  k a multiple of 4, ldx and ldz multiples of 4, x and z 16-byte
 * aligned, n < ISPLIB_STREAM_N_END, ldy < ISPLIB_STREAM_LDY_END, n*ldy*4 <= ISPLIB_DENSE_BYTES_MAX.  Other words return ISPLIB_NO_OPT_IMPL.
 */
int    isplib_fusedmm_stream_geometry(int streams, int *rows_per_wave /*out*/, int *waves_resident /*out*/);
int    isplib_suggest_fusedmm_stream(int32_t imessage, int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk);
int    isplib_stream_plan_build_fusedmm_hip(int64_t m, int64_t n, int64_t nnz, const int64_t *rowptr, const int64_t *col,
                                            int streams, int slices, int chunk, int waves_per_gen,
                                            isplib_stream_plan *out /*host*/, void *stream);
int    fusedMM_csr_udef_stream_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                   const int64_t *pntrb, const int64_t *pntre, const isplib_stream_plan *plan /*host*/,
                                   const float *x /*[dev] m x ldx*/, int64_t ldx, const float *y /*[dev] n x ldy*/, int64_t ldy,
                                   float *z /*[dev] m x ldz*/, int64_t ldz, int sop_udef /*enum isplib_sop_udef*/, float sop_param,
                                   void *workspace, size_t workspace_bytes, void *stream);

/* The plain row-per-wave kernel of fusedMM_csr_hip with the rows taken in a caller-given ORDER (`row_order`: position ->
 * row, a permutation of [0, m), [dev] int32; NULL = fusedMM_csr_hip).  For operands larger than the Infinity Cache (the
 * ogbn-products shape: y = 2.5 GB) no schedule of this library reuses a gathered row -- unless rows that share neighbours
 * are worked on at the same time on the same XCD: the workgroups of an XCD walk a contiguous range of positions, so a
 * community-grouped order (isplib_amd/reorder.py: label propagation, once per graph) turns the gathers of a community's
 * rows into hits of that XCD's L2.  Nothing is moved: y is gathered and z written where they are, every row is computed
 * by the same code in the same edge order -- the result is bit for bit the same for any order.  (row_order == NULL on an
 * operand beyond the Infinity Cache, n * ldy * 4 > 256 MiB, runs k > 128 in 128-column panels -- two rows per gather: 9 % faster
 * on the ogbn-products shape, the sums of a row associated over two slots instead of one; isplib_hip_tune(0, 64) keeps the
 * index-order launch on the one-pass form a given order runs.)
 * No reference counterpart (the reference's CPU kernel walks rows in index order, csrc/fusedmm.cpp:198). */
int    fusedMM_csr_ordered_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                               const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                               const int32_t *row_order /*[dev] m | NULL*/, const float *y, int64_t ldy, float *z,
                               int64_t ldz, int64_t *z_arg, void *stream);

/* 1 when fusedMM_csr_hip (rows in index order) switches to the 128-column panel form above for a dense operand of n rows
 * with leading dimension ldy (n * ldy * 4 > 256 MiB; it applies to k > 128 on 16-byte rows), else 0.  A caller that must
 * reproduce the bits of a call on another operand size -- a row shard reading a padded gather buffer of more rows than
 * the single-device operand -- runs fusedMM_csr_ordered_hip with the identity order where only its own size is past
 * the switch: that launch never panels and is otherwise the index-order one. */
int    isplib_plain_panels(int64_t n, int64_t ldy);

/* The order for fusedMM_csr_ordered_hip, found on the device (square graphs): synchronous label propagation -- every
 * row takes the label most of its stored entries' columns carry, ties by a per-round hash of the label, at most `rounds`
 * rounds (8 is plenty; it stops when fewer than 1 % of the rows change) -- then the rows sorted by label, index order
 * inside a label.  order: [dev] m int32, position -> row.  labels (may be NULL): [dev] m int32, the label of every row.
 * One radix sort of nnz 64-bit keys per round: ~0.2 s for the ogbn-products shape, once per graph.  The result only
 * affects speed.  isplib_order_locality_hip reports what an order found: the share of stored entries whose column lies
 * within `window` positions of its row (order NULL: index order) -- a community order of a graph WITH structure lifts it
 * from ~0 to the share of edges inside communities; one that lifts nothing is not worth passing on. */
size_t isplib_community_order_workspace_bytes(int64_t m, int64_t nnz);
int    isplib_community_order_hip(int64_t m, int64_t nnz, const int64_t *rowptr, const int64_t *col, int rounds, int seed,
                                  int32_t *order, int32_t *labels /*may be NULL*/, int *rounds_run /*host, may be NULL*/,
                                  void *workspace, size_t workspace_bytes, void *stream);
int    isplib_order_locality_hip(int64_t m, int64_t nnz, const int64_t *rowptr, const int64_t *col, const int32_t *order,
                                 int64_t window, double *share /*host*/, void *workspace /*4 m + 512 bytes*/,
                                 size_t workspace_bytes, void *stream);

/* Tuning knobs of the shipped kernels, for experiments (process-wide, not thread-safe; every setting gives the same results):
 *   0  lanes per row slot of the row kernels (0 = by k)      1  0: 64-bit addressing instead of buffer descriptors
 *   2  consecutive tasks per wave of the task kernel (0=auto) 4  column-panel width of the task entries, sum / mean (64)
 *   5  the same for max / min (64)                            8  per-slice footprint of whole rows (KiB) up to which a
 *      returns ISPLIB_FAIL for an unknown key                    task plan runs in one pass (9216; 0 = always panels)
 * (the knobs of the forms that were measured slower live with them: include/isplib_hip_experimental.h) */
int isplib_hip_tune(int key, int value);

/* Warm-up hook with the reference's name; launches one empty kernel. */
void performDummySpMM_hip(int64_t flag, void *stream);

/*
 * Fused backward of SpMM-max/min (one pass, float atomics):
 *   for every (i,c) with a = arg[i,c] != nnz, j = indx[a]:
 *     grad_mat[j,c]  += (val ? val[a] : 1) * grad_out[i,c]      (if grad_mat)
 *     grad_val[a]    += mat[j,c] * grad_out[i,c]                (if grad_val)
 * grad_mat (n x k) and grad_val (nnz) are zero-filled by this call first.
 * All dense operands contiguous with leading dimension k.
 */
int isplib_spmm_minmax_bw_hip(int64_t m, int64_t n, int64_t k, int64_t nnz,
                              const int64_t *indx, const float *val,
                              const float *mat, const int64_t *arg,
                              const float *grad_out, float *grad_mat,
                              float *grad_val, void *stream);

/*
 * The same gradients WITHOUT atomics: bitwise reproducible from launch to launch, like the reference's CPU
 * scatter_add_ (csrc/fusedmm.cpp:421-446).  grad_mat: the (destination, value) pairs of all (row, feature)
 * elements are sorted by destination with a stable radix sort and every run is added up in ascending row order by one
 * thread; grad_val: every destination of row i is an entry of row i, so one thread per row updates them in feature
 * order.  workspace: isplib_spmm_minmax_bw_workspace_bytes(m, n, k) bytes, 256-byte aligned (0 = not served:
 * n*k + 1 or m*k beyond 32-bit keys -- use the atomic form above).
 */
size_t isplib_spmm_minmax_bw_workspace_bytes(int64_t m, int64_t n, int64_t k);
int isplib_spmm_minmax_bw_det_hip(int64_t m, int64_t n, int64_t k, int64_t nnz,
                                  const int64_t *indx, const float *val,
                                  const float *mat, const int64_t *arg,
                                  const float *grad_out, float *grad_mat,
                                  float *grad_val, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The local half of the max / min backward under the 1-D row partition (isplib_amd/dist.py; no reference counterpart: the
 * reference has no distributed path).  After the exchange every rank holds, in global row order, the winners' columns
 * dest[i,c] (int32 global row of the dense operand, < 0 = no winner) and the weighted gradients gval[i,c] = val[arg] *
 * grad_out[i,c] of ALL rows; it keeps the destinations that are its own rows [lo, lo + n):
 *     grad_mat[d - lo, c] = sum over i, ascending, of gval[i,c] where dest[i,c] == d
 * Same stable sort + ordered run sums as isplib_spmm_minmax_bw_det_hip (no atomics, bitwise reproducible), same
 * workspace: isplib_spmm_minmax_bw_workspace_bytes(m, n, k).  grad_mat (n x k, contiguous) is zero-filled first.
 */
int isplib_scatter_rows_det_hip(int64_t m, int64_t n, int64_t k, int64_t lo,
                                const int32_t *dest /*[dev] m x k*/, const float *gval /*[dev] m x k*/,
                                float *grad_mat /*[dev] n x k*/, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The same backward with an owner-bucketed exchange: a rank sends every other rank only the winners that land in that rank's
 * rows, and an owner sorts about m*k / world pairs instead of all m*k (isplib_amd/dist.py, ISPLIB_DIST_MINMAX_BW=owner).
 * Domain: isplib_owner_exchange_serves (address-domain block above).  Neither entry allocates or synchronises.
 *
 * Sender's half.  For every (i, c) of this rank's m x k winners:
 *   a = arg[i,c] - edge0; no winner unless 0 <= a < nnz; d = indx[a] (GLOBAL row of the dense operand);
 *   owner p: cuts[p] <= d < cuts[p+1] (d outside [cuts[0], cuts[world]) is dropped);
 *   key = (d - cuts[p]) * k + c;  value = (val ? val[a] : 1) * grad_out[i,c].
 * keys / vals [seg_off[p], seg_off[p+1]) hold owner p's pairs in ASCENDING t = i*k + c (a stable split: three launches --
 * per-block histograms, one exclusive scan, the scatter; no atomic decides a placement, so two launches give the same bytes);
 * seg_off[world] = number of pairs with a winner.  Nothing is written past it.  The cuts are read on the host, during the
 * call (they travel by value).  workspace: isplib_minmax_bw_bucket_workspace_bytes bytes, 256-byte aligned (0 = not served).
 */
size_t isplib_minmax_bw_bucket_workspace_bytes(int64_t m, int64_t k, int world);
int    isplib_minmax_bw_bucket_hip(int64_t m, int64_t k, int64_t nnz, int64_t edge0,
                                   const int64_t *arg /*[dev] m x k contiguous*/, const int64_t *indx /*[dev] nnz*/,
                                   const float *val /*[dev] nnz | NULL*/, const float *grad_out /*[dev] m x k contiguous*/,
                                   int world, const int64_t *cuts_host /*world + 1, ascending, HOST*/,
                                   uint32_t *keys /*[dev] m*k*/, float *vals /*[dev] m*k*/, int64_t *seg_off /*[dev] world + 1*/,
                                   void *workspace, size_t workspace_bytes, void *stream);

/*
 * Receiver's half.  grad_mat[key / k, key % k] = sum of vals over equal keys IN THE ORDER GIVEN
 * (stable sort + the ordered run sums of isplib_spmm_minmax_bw_det_hip, sorted straight from the caller's arrays).
 * grad_mat (n x k) is zero-filled first.  keys >= n*k are ignored, never written.  Fed the owners' segments in source-rank
 * order it forms every sum in the order isplib_scatter_rows_det_hip does: the same bits.
 * workspace: isplib_scatter_keys_workspace_bytes bytes, 256-byte aligned (0 = not served: total >= ISPLIB_MINMAX_BW_PAIRS_END
 * or n*k > ISPLIB_MINMAX_BW_KEYS_MAX).
 */
size_t isplib_scatter_keys_workspace_bytes(int64_t total, int64_t n, int64_t k);
int    isplib_scatter_keys_det_hip(int64_t total, int64_t n, int64_t k, const uint32_t *keys /*[dev] total*/,
                                   const float *vals /*[dev] total*/, float *grad_mat /*[dev] n x k*/,
                                   void *workspace, size_t workspace_bytes, void *stream);

/*
 * SDDMM-style value gradient of SpMM-sum / SpMM-mean:
 *   dval[j] = < y[indx[j], :], g[i, :] > * (mean ? 1/max(deg_i,1) : 1),  j in row i
 * Every dval[j], j in [0, nnz), is written and nothing outside that range is; it lies within 1e-5 * <|y|, |g|> + 64 * 2^-149 of
 * the exact value (exact where the fp32 sums are exact in any order), a non-finite value in column c of y or g enters it only
 * through the product of column c, and nothing is flushed to zero.
 */
int isplib_sddmm_csr_hip(int64_t m, int64_t k, const int64_t *indx,
                         const int64_t *pntrb, const int64_t *pntre,
                         const float *y, int64_t ldy, const float *g,
                         int64_t ldg, int mean, float *dval, void *stream);
/* The same over the task plan of the SpMM (one wave per task, XCD-lane grouping -> the L2 affinity of
 * the task-list SpMM; dval is per edge, so no workspace and no combine).  Domain: isplib_sddmm_tasks_serve(n, k, ldy) --
 * ISPLIB_K_MIN <= k <= ISPLIB_SDDMM_TASKS_K_MAX, n*ldy*4 <= ISPLIB_DENSE_BYTES_MAX.  The same contract as isplib_sddmm_csr_hip for
 * every edge a task covers: the bound, exactness on exactly summable data, a non-finite value in column c reaching an edge only
 * through the product of column c at any k (a ragged k's shifted last vector included), no flush to zero, no write outside
 * dval[0, nnz). */
int isplib_sddmm_csr_tasks_hip(int64_t m, int64_t n, int64_t k, const int64_t *indx,
                               const int32_t *indx32 /*optional, as in fusedMM_csr_tasks_hip*/,
                               const int64_t *pntrb, const int64_t *pntre,
                               int64_t n_tasks, const int32_t *task_row,
                               const int64_t *task_b, const int32_t *task_len,
                               const int64_t *lane_off_host /*9, host*/,
                               const float *y, int64_t ldy, const float *g, int64_t ldg,
                               int mean, float *dval, void *stream);

/*
 * Graph preparation on the device (the step immediately before the path).
 *   isplib_csr_row_ids_hip : row[j] = i for j in [rowptr[i], rowptr[i+1])
 *   isplib_csr2csc_hip     : stable counting sort of the CSR entries by column:
 *        colptr[n+1], csr2csc[nnz] (CSC position -> CSR position),
 *        row_t[nnz] = row[csr2csc], and, when val_t != NULL,
 *        val_t[nnz] = (val ? val[csr2csc] : 1) / (mean_scale ? max(deg(row),1) : 1)
 *     i.e. exactly the cached operands of isplib/__init__.py:79-80 (sum) and the
 *     intended form of :86-99 (mean; csrc/fusedmm.cpp:357-364).
 *     Deterministic (no atomics decide placement).  Workspace: see query.
 */
int    isplib_csr_row_ids_hip(int64_t m, int64_t nnz, const int64_t *rowptr,
                              int64_t *row, void *stream);
size_t isplib_csr2csc_workspace_bytes(int64_t m, int64_t n, int64_t nnz);
int    isplib_csr2csc_hip(int64_t m, int64_t n, int64_t nnz,
                          const int64_t *rowptr, const int64_t *col,
                          const float *val, int mean_scale, int64_t *colptr,
                          int64_t *csr2csc, int64_t *row_t, float *val_t,
                          void *workspace, size_t workspace_bytes, void *stream);

/*
 * isplib_graph: a handle that owns what a graph needs for the fast path -- the per-graph operands the
 * stateless entries above leave to the caller (slice tables, task plans per slice count, the packed column
 * ids, the CSC operands of the backward, one grow-only workspace), built lazily on the device.  It is what
 * the reference's C++ layer (csrc/fusedmm.cpp:113-203) would hold per graph in place of the pointer-keyed
 * dicts of isplib/__init__.py:35-40.
 *   isplib_graph_create   borrows rowptr[m+1] / col[nnz] / val[nnz]|NULL (device; must outlive the handle and
 *                         must not change without isplib_graph_set_values: val is examined once, and a vector
 *                         of exact 1.0f -- what isplib/__init__.py:51-57 materialises for an unweighted graph -- is
 *                         treated as NULL)
 *   isplib_graph_spmm     z = A (x) y for one of the four SpMM words; schedule by the measured rules: the stream
 *                         schedule where isplib_suggest_stream (sum / mean) or isplib_suggest_stream_minmax (max / min,
 *                         column-sorted rows) accepts the call, else isplib_suggest_slices
 *                         (or isplib_graph_set_slices: -1 rules, 0 plain kernel, 1..4096 task list)
 *   isplib_graph_spmm_backward   dx = A^T dy (mean != 0: with weights val/max(deg,1), the mean forward's
 *                         backward, csrc/fusedmm.cpp:375); the CSC operands are built on first use
 *   isplib_suggest_slices the measured rule (0 = plain row-per-wave kernel)
 * The first call that needs a new plan (or the transpose) allocates device memory and synchronises the
 * stream once; every later call is asynchronous and allocation-free.  Not thread-safe (serialise the calls of
 * one handle), but usable on several streams: each stream it is used on gets its own workspace.
 */
typedef struct isplib_graph isplib_graph;
int  isplib_suggest_slices(int64_t m, int64_t n, int64_t nnz, int64_t k, int minmax /*nonzero for max / min*/);
int  isplib_graph_create(int64_t m, int64_t n, int64_t nnz, const int64_t *rowptr, const int64_t *col,
                         const float *val, isplib_graph **out);
int  isplib_graph_set_slices(isplib_graph *g, int slices);
/* The order in which the plain kernel takes the rows of A (order: [dev] m int32, position -> row) and of A^T (order_t:
 * [dev] n int32) -- fusedMM_csr_ordered_hip; borrowed, NULL = index order.  Without this call the handle looks for a
 * community order itself (isplib_community_order_hip, once, ~0.2 s for the ogbn-products shape) the first time a square
 * graph reaches the plain kernel with a dense operand larger than the Infinity Cache (n k 4 > 256 MiB), and keeps it
 * only if it found structure.  Speed only: any order gives the same bits. */
int  isplib_graph_set_row_order(isplib_graph *g, const int32_t *order, const int32_t *order_t);
/* New weights for the same structure (val: [dev] nnz | NULL, borrowed like create's; also to be called when the
 * CONTENTS of the array given before have changed): plans, packed column ids and the CSC structure stay; the
 * unit-weight test, the stream plans' copies of the weights and the transposed weights of the backward are refreshed
 * by the next call that needs them, on that call's stream.  Never synchronises, never frees. */
int  isplib_graph_set_values(isplib_graph *g, const float *val);
int  isplib_graph_spmm(isplib_graph *g, int32_t imessage, int64_t k, const float *y, int64_t ldy,
                       float *z, int64_t ldz, int64_t *z_arg, void *stream);
int  isplib_graph_spmm_backward(isplib_graph *g, int mean, int64_t k, const float *dy, int64_t lddy,
                                float *dx, int64_t lddx, void *stream);
/* dA[e] = <y[col[e],:], g[row(e),:]> (mean != 0: / max(deg,1)); its plan is sized for whole rows of y (the dot
 * product cannot run in column panels): isplib_suggest_slices_whole_rows */
int  isplib_suggest_slices_whole_rows(int64_t m, int64_t n, int64_t nnz, int64_t k);
int  isplib_graph_sddmm(isplib_graph *g, int mean, int64_t k, const float *y, int64_t ldy,
                        const float *gmat, int64_t ldg, float *dval, void *stream);
void isplib_graph_destroy(isplib_graph *g);

#ifdef __cplusplus
}
#endif

/* the GATv2 aggregation for bf16 / fp16 operands (isplib_gatv2_16_*): part of this interface, declared in a file of its own */
#include "isplib_hip_gatv2_16.h"

/* the GATv2 aggregation with attention dropout (isplib_gatv2_drop_*): part of this interface, declared in a file of its own */
#include "isplib_hip_gatv2_drop.h"

/* sparse multi-head dot-product attention with separate keys and values (isplib_mha_*): part of this interface, declared in a file of
 * its own */
#include "isplib_hip_mha.h"

/* the same attention with attention dropout, fp32 (isplib_qkv_drop_*): part of this interface, declared in a file of its own, beside
 * the entries it extends */
#include "isplib_hip_mha_drop.h"

/* the same attention with attention dropout for bf16 / fp16 operands (isplib_qkv_half_drop_*): part of this interface, declared in a
 * file of its own */
#include "isplib_hip_mha16_drop.h"

/* the same attention for bf16 / fp16 operands (isplib_qkv16_*): part of this interface, declared in a file of its own */
#include "isplib_hip_mha16.h"

#endif /* ISPLIB_HIP_H */
