/*
 * isplib_hip_mha16.h -- the 16-bit multi-head attention entries (q, k, v) of libisplib_hip.so.  isplib_hip.h includes this file at its
 * end, so a program that includes isplib_hip.h has these entries too; they are kept in a file of their own, with a name list of their
 * own in isplib_amd/cabi.py (MHA16_EXPORTS), for the reason isplib_hip_gatv2_16.h gives.  Their names start with isplib_qkv16_, not
 * isplib_mha: the set of exported symbols that start with isplib_mha is pinned to the four fp32 entries (tests/test_mha_host.py).
 * tests/test_mha16_host.py compares this header, MHA16_EXPORTS and the library's symbols.
 *
 * The sparse multi-head dot-product attention of isplib_hip_mha.h (isplib_mha_*) for wide operands of 16-bit elements (dtype:
 * ISPLIB_DTYPE_BF16 | _F16), all heads in one launch, forward and backward, on the mapping of the 16-bit GATv2 entries (one wave per
 * row or column, one 16-byte gather of EIGHT columns per lane, edge and gathered table, one chunk per lane).  q, key, v, g, z, dq,
 * dkey and dv are `dtype` and are never widened in memory; widening is exact, every product, sum, exponential and division is fp32,
 * and each wide output is rounded ONCE, to nearest even, to `dtype`.  lse and dsum (D) are fp32 exactly as in the fp32 entries.
 * p = `scale` multiplies the finished dot product in all three kernels.  The special values are the fp32 entries': an empty row has
 * z_i = 0, lse = -inf, D = 0, dq_i = 0; a column no entry points at has dkey_j = dv_j = 0; a row of one entry returns v_j's 16 bits
 * unchanged; a NaN in key_jc reaches the head of c of z in the rows that reference j, a NaN in v_jc column c of those rows, and
 * nothing else.
 *   isplib_qkv16_csr_hip      writes z (m x ldz, `dtype`) and lse (m x heads, fp32).
 *   isplib_qkv16_bw_rows_hip  reads q, key, v, g and lse -- NOT z: the rounded z would carry u * sum_c |g_ic z_ic| into every ds_e
 *                             through D = <g_i, z_i>_h.  In one pass over the row's edges it forms, per head, l = sum a_e and
 *                             Dacc = sum a_e t_e (t_e = <g_i, v_j>_h) and, per column, P_c = sum a_e t_e key_jc and
 *                             Q_c = sum a_e key_jc; then D = Dacc / l and dq_ic = p (P_c - D Q_c).  Writes dq (m x lddq, `dtype`)
 *                             and dsum (m x heads, fp32: D, which the next entry reads).
 *   isplib_qkv16_bw_cols_hip  on the transposed structure (colb / cole: n column ranges into row_t); reads q, g, lse, dsum, key and
 *                             v, writes dkey (n x lddk) and dv (n x lddv), both `dtype`, each at its own pitch.
 * Nothing is kept per edge and autograd needs q, key, v and lse only.  Outputs are write-only, every element of every row is written,
 * nothing between the rows of a pitched output, nothing outside a row's k columns is used.  No atomics, no LDS, a fixed order of
 * operations: two launches give equal bits.  The entries neither allocate nor synchronise.
 * Domain: isplib_qkv16_serves(rows_gathered, heads, d, ld) = isplib_gat16_serves, for every GATHERED wide operand at its own row count
 * and pitch (key and v with n rows in the first two entries; q and g with m rows in the third); the pitches of the row-resident
 * operands and of the wide outputs must be even too.  The refusals come in one order: another dtype, a negative dimension:
 * ISPLIB_FAIL; m == 0 or k == 0 (n == 0 or k == 0 in the third entry) succeeds without a launch; a pitch of a row-resident operand or
 * output below k, a k that is no multiple of heads, a scale that is not finite: ISPLIB_FAIL; outside the domain: ISPLIB_NO_OPT_IMPL;
 * a null operand: ISPLIB_FAIL; a 16-bit base that is not 4-byte aligned: ISPLIB_FAIL.  All refusals come before any launch and leave
 * the outputs untouched.
 * isplib_qkv16_native_pays is the measured rule of the layers above (forward + backward against "widen, the fp32 entries, narrow";
 * profiles/mha16_ab.txt), over the family's classes (the gathered operand beyond 256 MiB at 2 bytes per element or
 * not): nonzero only where EVERY native run was faster than EVERY run of the conversion route on every measured shape of the class.
 */
#ifndef ISPLIB_HIP_MHA16_H
#define ISPLIB_HIP_MHA16_H

#include "isplib_hip.h"        /* ISPLIB_DTYPE_*, the status codes, isplib_gat16_serves */

#ifdef __cplusplus
extern "C" {
#endif

static inline int isplib_qkv16_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gat16_serves(rows_gathered, heads, d, ld);
}
int    isplib_qkv16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_qkv16_serves as a symbol */
int    isplib_qkv16_csr_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                            const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale,
                            const void *q, int64_t ldq, const void *key, int64_t ldk, const void *v, int64_t ldv, void *z,
                            int64_t ldz, float *lse /* m x heads */, void *stream);
int    isplib_qkv16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                const int64_t *pntre, int64_t heads, float scale, const void *q, int64_t ldq, const void *key,
                                int64_t ldk, const void *v, int64_t ldv, const void *g, int64_t ldg, const float *lse, void *dq,
                                int64_t lddq, float *dsum /* m x heads */, void *stream);
int    isplib_qkv16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                const int64_t *cole, int64_t heads, float scale, const void *q, int64_t ldq, const void *g,
                                int64_t ldg, const float *lse, const float *dsum, const void *key, int64_t ldk, const void *v,
                                int64_t ldv, void *dkey, int64_t lddk, void *dv, int64_t lddv, void *stream);
static inline int isplib_qkv16_native_pays(int64_t rows_gathered, int64_t ld) {
   /* measured (profiles/mha16_ab.txt: the Reddit shape at (H, d) = (8, 8) and (8, 16) -- gathered operand inside 256 MiB -- and the
    * ogbn-products shape at (8, 16) -- beyond it; bf16, scale 1/sqrt(d), forward + backward, 5 alternating runs of 10 steps, run spread
    * at most 0.3 % on the native side and 0.5 % on the other): every native run is below every run of the conversion route in both
    * classes -- 0.541-0.565 of its time inside 256 MiB, 0.518 beyond (forward alone 0.502-0.507 and 0.448), at 0.09-0.10 of its peak
    * memory.  Both classes pay. */
   return (rows_gathered > 0 && ld > 0) ? 1 : 0;
}
int    isplib_qkv16_auto(int64_t rows_gathered, int64_t ld);                      /* the same rule as a symbol */

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_MHA16_H */
