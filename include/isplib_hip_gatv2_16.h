/*
 * isplib_hip_gatv2_16.h -- the 16-bit GATv2 entries of libisplib_hip.so.  isplib_hip.h includes this file at its end, so a program
 * that includes isplib_hip.h has these entries too; they are kept in a file of their own, with a name list of their own in
 * isplib_amd/cabi.py (GATV2_16_EXPORTS), because the list of isplib_hip.h's own symbols that mention GATv2 is pinned to the five fp32
 * entries (tests/test_gatv2_host.py) while every function isplib_hip.h itself declares must be in cabi.EXPORTS (tests/test_host.py).
 * tests/test_gatv2_16_host.py compares this header, GATV2_16_EXPORTS and the library's symbols.
 *
 * The GATv2 attention aggregation of isplib_hip.h (isplib_gatv2_*) for wide operands of 16-bit elements (dtype: ISPLIB_DTYPE_BF16 |
 * _F16), all heads in one launch, forward and backward, on the mapping of the 16-bit GAT entries (one wave per row or column, one
 * 16-byte gather of EIGHT columns per lane and edge, one chunk per lane).  x, y, g, z, dx and dy are `dtype` and are never widened in
 * memory; widening is exact, every sum, product, exponential and division is fp32, and z, dx and dy are rounded ONCE, to nearest even,
 * to `dtype`.  att (heads x d, k contiguous floats), lse, dsum (D), datt and the datt workspace are fp32 exactly as in the fp32
 * entries.  u_ec = widen(x_ic) + widen(y_jc) is one unfused fp32 add, so the slope branch is decided by the sign of the exact sum;
 * u_ec == 0 takes ns.  The special values are the fp32 entries': an empty row has z_i = 0, lse = -inf, D = 0, dx_i = 0; a column no
 * entry points at has dy_j = 0; a row of one entry returns y_j's 16 bits unchanged; a NaN in y_jc reaches the head of c in the rows
 * that reference j and nothing else.
 *   isplib_gatv2_16_csr_hip      writes z (m x ldz, `dtype`) and lse (m x heads, fp32).
 *   isplib_gatv2_16_bw_rows_hip  reads x, y, att, g and lse -- NOT z: the rounded z would carry u * sum_c |g_ic z_ic| into every ds_e
 *                                through D = <g_i, z_i>_h.  In one pass over the row's edges it forms, per head, l = sum a_e and
 *                                Dacc = sum a_e t_e (t_e = <g_i, y_j>_h), per column P_c = sum a_e sl_ec t_e and Q_c = sum a_e sl_ec
 *                                and, where datt is not NULL, R_c = sum a_e t_e v_ec and S_c = sum a_e v_ec; then D = Dacc / l,
 *                                dx_ic = att_c (P_c - D Q_c), and the row's part of datt_c is R_c - D S_c.  Writes dx (m x lddx,
 *                                `dtype`) and dsum (m x heads, fp32: D, which the next entry reads) and, where datt is not NULL,
 *                                datt (k floats): every block of the kernel writes one partial row into `workspace` (at least
 *                                isplib_gatv2_16_bw_rows_workspace_bytes(m, k) bytes, 256-byte aligned; too small:
 *                                ISPLIB_NOT_ENOUGH_MEM) and a second kernel adds the rows up in a fixed order.  datt == NULL runs a
 *                                kernel without that sum and ignores the workspace; dx and dsum have the same bits either way.
 *   isplib_gatv2_16_bw_cols_hip  on the transposed structure; reads x, y, att, g, lse and dsum, writes dy (n x lddy, `dtype`).
 * Nothing is kept per edge and autograd needs x, y, att and lse only.  Outputs and the workspace are write-only, every element of
 * every row is written, nothing between the rows of a pitched output, nothing outside a row's k columns is used.  No atomics, a
 * fixed order of operations: two launches give equal bits, datt included.  The entries neither allocate nor synchronise.
 * Domain: isplib_gatv2_16_serves(rows_gathered, heads, d, ld) = isplib_gat16_serves, for every GATHERED wide operand (y with n rows
 * in the first two entries; x and g with m rows in the third); the pitches of the row-resident operands and of the wide outputs must
 * be even too.  The refusals come in one order: another dtype, a negative dimension: ISPLIB_FAIL; m == 0 or k == 0 (n == 0 or k == 0
 * in the third entry) succeeds without a launch; a pitch of a row-resident operand or output below k, a k that is no multiple of
 * heads: ISPLIB_FAIL; outside the domain: ISPLIB_NO_OPT_IMPL; a null operand: ISPLIB_FAIL; a workspace too small:
 * ISPLIB_NOT_ENOUGH_MEM, or not 256-byte aligned: ISPLIB_FAIL; a 16-bit base that is not 4-byte aligned: ISPLIB_FAIL.  All refusals
 * come before any launch and leave the outputs untouched.
 * isplib_gatv2_16_native_pays is the measured rule of the layers above (forward + backward against "widen, the fp32 entries,
 * narrow"; profiles/gatv2_16_ab.txt), over the family's classes (the gathered operand beyond 256 MiB at 2 bytes per
 * element or not): nonzero only where EVERY native run was faster than EVERY run of the conversion route on every measured shape of
 * the class.
 */
#ifndef ISPLIB_HIP_GATV2_16_H
#define ISPLIB_HIP_GATV2_16_H

#include "isplib_hip.h"        /* ISPLIB_DTYPE_*, the status codes, isplib_gat16_serves */

#ifdef __cplusplus
extern "C" {
#endif

static inline int isplib_gatv2_16_serves(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gat16_serves(rows_gathered, heads, d, ld);
}
int    isplib_gatv2_16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld);   /* isplib_gatv2_16_serves as a symbol */
int    isplib_gatv2_16_csr_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                               const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const void *x, int64_t ldx,
                               const void *y, int64_t ldy, const float *att /* heads x d */, int64_t heads, float negative_slope,
                               void *z, int64_t ldz, float *lse /* m x heads */, void *stream);
size_t isplib_gatv2_16_bw_rows_workspace_bytes(int64_t m, int64_t k);
int    isplib_gatv2_16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                   const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy, const float *att,
                                   int64_t heads, float negative_slope, const void *g, int64_t ldg, const float *lse, void *dx,
                                   int64_t lddx, float *dsum /* m x heads */, float *datt /* k floats, or NULL */, void *workspace,
                                   size_t workspace_bytes, void *stream);
int    isplib_gatv2_16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                   const int64_t *cole, const void *x, int64_t ldx, const void *y, int64_t ldy, const float *att,
                                   int64_t heads, float negative_slope, const void *g, int64_t ldg, const float *lse,
                                   const float *dsum, void *dy, int64_t lddy, void *stream);
static inline int isplib_gatv2_16_native_pays(int64_t rows_gathered, int64_t ld) {
   /* measured (profiles/gatv2_16_ab.txt: the Reddit shape at (H, d) = (8, 8) and (8, 16) -- gathered operand inside 256 MiB -- and the
    * ogbn-products shape at (8, 16) -- beyond it; bf16, negative_slope 0.2, forward + backward, 5 alternating runs of 5 steps, run
    * spread at most 0.8 % on the native side and 0.5 % on the other): every native run is below every run of the conversion route in
    * both classes -- 0.715-0.754 of its time inside 256 MiB, 0.825 beyond (forward alone 0.711-0.761 and 0.689), at 0.11-0.13 of its
    * peak memory.  Both classes pay. */
   return (rows_gathered > 0 && ld > 0) ? 1 : 0;
}
int    isplib_gatv2_16_auto(int64_t rows_gathered, int64_t ld);                   /* the same rule as a symbol */

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_GATV2_16_H */
