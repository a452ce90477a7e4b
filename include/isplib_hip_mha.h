/*
 * isplib_hip_mha.h -- sparse multi-head dot-product attention with separate keys and values of libisplib_hip.so.  isplib_hip.h
 * includes this file at its end, so a program that includes isplib_hip.h has these entries too; they are kept in a file of their own,
 * with a name list of their own in isplib_amd/cabi.py (MHA_EXPORTS), for the reason isplib_hip_gatv2_16.h gives: every function
 * isplib_hip.h itself declares must be in cabi.EXPORTS (tests/test_host.py), and that list is pinned.  tests/test_mha_host.py compares
 * this header, MHA_EXPORTS and the library.
 *
 * Scaled dot-product attention over the stored entries of a CSR matrix, all heads in one launch, fp32 (PyG's TransformerConv without
 * edge features, root weight and beta gate; the local attention of sparse graph transformers).  q is m x k, key and v are n x k,
 * k = heads * d, head h owns the columns [h*d, (h+1)*d), p = `scale`.  For row i, stored entry e = (i, j) and head h:
 *   s_e  = p <q_i, key_j>_h     a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)     z_i[head h] = sum_e a_e v_j[head h]
 * and for g = dL/dz
 *   D[i,h] = <g_i, z_i>_h       t_e = <g_i, v_j>_h          ds_e = a_e (t_e - D[i,h])
 *   dq_i[head h]   = p sum_e ds_e key_j[head h]
 *   dkey_j[head h] = p sum_{e -> j} ds_e q_i[head h]
 *   dv_j[head h]   = sum_{e -> j} a_e g_i[head h].
 * Stored values are not read; every stored entry is its own edge, duplicates (i, j) included.  An empty row has z = 0, lse = -inf,
 * dq = 0, D = 0; a column that no entry references has dkey = dv = 0.
 *   isplib_mha_csr_hip      writes z (m x ldz) and lse (m x heads).
 *   isplib_mha_bw_rows_hip  reads q, key, v, g, z and lse, writes dq (m x lddq) and dsum (m x heads: D, which the next entry reads).
 *   isplib_mha_bw_cols_hip  runs on the transposed structure (colb / cole: n column ranges into row_t); reads q, g, lse, dsum, key
 *                           and v, writes dkey (n x lddk) and dv (n x lddv).
 * Nothing is kept per edge: the backward recomputes a_e from lse.  Outputs are write-only and every element of every row is written,
 * nothing between the rows of a pitched output.  One wave per row (per column), no atomics, no LDS, a fixed order of operations: two
 * launches give equal bits.  The entries neither allocate nor synchronise.
 * Domain: isplib_mha_serves(rows_gathered, heads, d, ld) = isplib_gat_serves, for EVERY gathered wide operand at its own row count and
 * pitch (key and v with n rows in the first two entries, q and g with m rows in the third).  Outside the domain: ISPLIB_NO_OPT_IMPL.
 * A negative dimension, a null operand, a k that is no multiple of heads, a scale that is not finite, or a pitch of a row-resident
 * operand or output below k: ISPLIB_FAIL.  All refusals come before any launch.  m == 0 or k == 0 (n == 0 or k == 0 in the third
 * entry) succeeds without a launch.
 */
#ifndef ISPLIB_HIP_MHA_H
#define ISPLIB_HIP_MHA_H

#include "isplib_hip.h"        /* the status codes, isplib_gat_serves */

#ifdef __cplusplus
extern "C" {
#endif

static inline int isplib_mha_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gat_serves(rows_gathered, heads, d, ld);
}
int    isplib_mha_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_mha_serves as a symbol */
int    isplib_mha_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                          const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                          int64_t ldk, const float *v, int64_t ldv, float *z, int64_t ldz, float *lse /* m x heads */, void *stream);
int    isplib_mha_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                              const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                              int64_t ldk, const float *v, int64_t ldv, const float *g, int64_t ldg, const float *z, int64_t ldz,
                              const float *lse, float *dq, int64_t lddq, float *dsum /* m x heads */, void *stream);
int    isplib_mha_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                              const int64_t *cole, int64_t heads, float scale, const float *q, int64_t ldq, const float *g,
                              int64_t ldg, const float *lse, const float *dsum, const float *key, int64_t ldk, const float *v,
                              int64_t ldv, float *dkey, int64_t lddk, float *dv, int64_t lddv, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_MHA_H */
