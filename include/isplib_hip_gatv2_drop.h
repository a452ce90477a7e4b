/*
 * isplib_hip_gatv2_drop.h -- the GATv2 entries with attention dropout of libisplib_hip.so.  isplib_hip.h includes this file at its end,
 * so a program that includes isplib_hip.h has these entries too; they are kept in a file of their own, with a name list of their own in
 * isplib_amd/cabi.py (GATV2_DROP_EXPORTS), for the reason isplib_hip_gatv2_16.h gives: the list of isplib_hip.h's own symbols that
 * mention GATv2 is pinned to the five fp32 entries (tests/test_gatv2_host.py) while every function isplib_hip.h itself declares must be
 * in cabi.EXPORTS (tests/test_host.py).  tests/test_gatv2_dropout_host.py compares this header, GATV2_DROP_EXPORTS and the library.
 *
 * The GATv2 aggregation of isplib_hip.h (isplib_gatv2_*) with attention dropout (GATv2Conv's `dropout`: the coefficients are dropped
 * after the softmax, per stored entry and per head), fp32.  With the keep bit q_e,h in {0, 1}, c = `scale` = float32(1 / (1 - p)) and
 * r_ec what isplib_hip.h calls q_ec:
 *   u_ec, sl_ec, v_ec, s_e, a_e, lse   exactly as without dropout: the softmax runs over ALL stored entries, lse does not see the mask
 *   z_i[head h] = c sum_e q_e a_e y_j[head h]             D[i,h] = <g_i, z_i>_h  (= sum_e a_e t_e)
 *   t_e         = q_e c <g_i, y_j>_h                      ds_e   = a_e (t_e - D[i,h])       (a dropped edge still gets -a_e D)
 *   r_ec        = ds_e att_c sl_ec                        dx_ic  = sum_e r_ec
 *   dy_jc       = sum_{e -> j} (q_e c a_e g_ic + r_ec)    datt_c = sum_{all e} ds_e v_ec.
 * The keep bit is the one of isplib_gat_drop_*_hip, unchanged: q_e,h = isplib_gat_drop_word(seed, pos_e, h) >= threshold, pos_e the
 * position of the entry in indx (its CSR position), threshold = isplib_gat_drop_threshold(p); a pure function recomputed in all three
 * entries -- no mask is stored, no RNG state is kept, and equal arguments give equal bits.  seed < 2^63, nnz < 2^31.  Every stored
 * entry has its own bit, duplicates (i, j) included.  An empty row has z = 0, lse = -inf, D = 0, dx = 0; a row whose entries are all
 * dropped for head h has z = 0 exactly there and a finite lse.  With threshold = 0 and scale = 1 the results are those of the entries
 * without dropout bit for bit.  The seed is an argument of the launch: a captured graph replays one mask.
 *   isplib_gatv2_drop_csr_hip      the arguments of isplib_gatv2_csr_hip, then threshold, scale, seed.
 *   isplib_gatv2_drop_bw_rows_hip  the arguments of isplib_gatv2_bw_rows_hip (workspace: isplib_gatv2_bw_rows_workspace_bytes), then
 *                                  threshold, scale, seed.
 *   isplib_gatv2_drop_bw_cols_hip  the arguments of isplib_gatv2_bw_cols_hip with csr2csc (nnz entries: the CSR position of every
 *                                  entry of the transposed structure) after cole, then threshold, scale, seed.
 * Domain: isplib_gatv2_serves, as for the entries without dropout.  A scale that is not a positive finite number, nnz >= 2^31, a null
 * csr2csc with nnz > 0 (third entry), and the refusals of the entries without dropout: ISPLIB_FAIL (outside the domain:
 * ISPLIB_NO_OPT_IMPL); all before any launch.
 */
#ifndef ISPLIB_HIP_GATV2_DROP_H
#define ISPLIB_HIP_GATV2_DROP_H

#include "isplib_hip.h"        /* the status codes, isplib_gatv2_serves, isplib_gat_drop_threshold / isplib_gat_drop_word */

#ifdef __cplusplus
extern "C" {
#endif

int    isplib_gatv2_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                 const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy,
                                 const float *att /* heads x d */, int64_t heads, float negative_slope, float *z, int64_t ldz,
                                 float *lse /* m x heads */, void *stream, uint32_t threshold, float scale, uint64_t seed);
int    isplib_gatv2_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                     const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                     int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz,
                                     const float *lse, float *dx, int64_t lddx, float *dsum /* m x heads */,
                                     float *datt /* k, or NULL */, void *workspace, size_t workspace_bytes, void *stream,
                                     uint32_t threshold, float scale, uint64_t seed);
int    isplib_gatv2_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                     const int64_t *cole, const int64_t *csr2csc /* nnz */, const float *x, int64_t ldx,
                                     const float *y, int64_t ldy, const float *att, int64_t heads, float negative_slope,
                                     const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy,
                                     void *stream, uint32_t threshold, float scale, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_GATV2_DROP_H */
