/*
 * isplib_hip_mha_drop.h -- the multi-head attention entries (q, k, v) with attention dropout of libisplib_hip.so.  isplib_hip.h includes
 * this file near its end, right after isplib_hip_mha.h (the last include stays isplib_hip_mha16.h), so a program that includes isplib_hip.h has these entries too; they are kept in a file of their own, with a name
 * list of their own in isplib_amd/cabi.py (MHA_DROP_EXPORTS), for the reason isplib_hip_gatv2_16.h gives.  Their names start with
 * isplib_qkv_drop_, not isplib_mha or isplib_qkv16: the symbols with those two prefixes are pinned to MHA_EXPORTS and MHA16_EXPORTS
 * (tests/test_mha_host.py, tests/test_mha16_host.py).  tests/test_mha_dropout_host.py compares this header, MHA_DROP_EXPORTS and the
 * library.
 *
 * The attention of isplib_hip_mha.h (isplib_mha_*) with attention dropout (TransformerConv's `dropout`, a graph transformer's
 * `attn_dropout`: the coefficients are dropped after the softmax, per stored entry and per head), fp32.  With the keep bit q_e,h in
 * {0, 1}, c = `keep_scale` = float32(1 / (1 - p)) and p_s = `scale`, the score scale of isplib_hip_mha.h:
 *   s_e, a_e, lse[i,h]   exactly as without dropout: the softmax runs over ALL stored entries, lse does not see the mask
 *   z_i[head h]    = c sum_e q_e a_e v_j[head h]          D[i,h] = <g_i, z_i>_h  (= sum_e a_e t_e)
 *   t_e            = q_e c <g_i, v_j>_h                   ds_e   = a_e (t_e - D[i,h])       (a dropped edge still gets -a_e D)
 *   dq_i[head h]   = p_s sum_e ds_e key_j[head h]
 *   dkey_j[head h] = p_s sum_{e -> j} ds_e q_i[head h]
 *   dv_j[head h]   = sum_{e -> j} q_e c a_e g_i[head h].
 * The keep bit is the one of isplib_gat_drop_*_hip and isplib_gatv2_drop_*_hip, unchanged: q_e,h = isplib_gat_drop_word(seed, pos_e, h)
 * >= threshold, pos_e the position of the entry in indx (its CSR position), threshold = isplib_gat_drop_threshold(p); a pure function
 * recomputed in all three entries -- no mask is stored, no RNG state is kept, and equal arguments give equal bits.  seed < 2^63,
 * nnz < 2^31.  Every stored entry has its own bit, duplicates (i, j) included.  An empty row has z = 0, lse = -inf, D = 0, dq = 0; a
 * live (row, head) whose entries are all dropped has z = 0 exactly there and a finite lse.  With threshold = 0 and keep_scale = 1 the
 * results are those of the entries without dropout bit for bit.  The seed is an argument of the launch: a captured graph replays one
 * mask.
 *   isplib_qkv_drop_csr_hip      the arguments of isplib_mha_csr_hip, then threshold, keep_scale, seed.
 *   isplib_qkv_drop_bw_rows_hip  the arguments of isplib_mha_bw_rows_hip, then threshold, keep_scale, seed.
 *   isplib_qkv_drop_bw_cols_hip  the arguments of isplib_mha_bw_cols_hip with csr2csc (nnz entries: the CSR position of every entry of
 *                                the transposed structure) after cole, then threshold, keep_scale, seed.
 * Domain: isplib_mha_serves, as for the entries without dropout (outside it: ISPLIB_NO_OPT_IMPL).  A keep_scale that is not a positive
 * finite number, nnz >= 2^31, seed >= 2^63, a null csr2csc with nnz > 0 (third entry), and the refusals of the entries without
 * dropout: ISPLIB_FAIL; all before any launch.  The ABI version stays 1.
 */
#ifndef ISPLIB_HIP_MHA_DROP_H
#define ISPLIB_HIP_MHA_DROP_H

#include "isplib_hip.h"        /* the status codes, isplib_mha_serves, isplib_gat_drop_threshold / isplib_gat_drop_word */

#ifdef __cplusplus
extern "C" {
#endif

int    isplib_qkv_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                               const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                               int64_t ldk, const float *v, int64_t ldv, float *z, int64_t ldz, float *lse /* m x heads */,
                               void *stream, uint32_t threshold, float keep_scale, uint64_t seed);
int    isplib_qkv_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                   const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                                   int64_t ldk, const float *v, int64_t ldv, const float *g, int64_t ldg, const float *z, int64_t ldz,
                                   const float *lse, float *dq, int64_t lddq, float *dsum /* m x heads */, void *stream,
                                   uint32_t threshold, float keep_scale, uint64_t seed);
int    isplib_qkv_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                   const int64_t *cole, const int64_t *csr2csc /* nnz */, int64_t heads, float scale, const float *q,
                                   int64_t ldq, const float *g, int64_t ldg, const float *lse, const float *dsum, const float *key,
                                   int64_t ldk, const float *v, int64_t ldv, float *dkey, int64_t lddk, float *dv, int64_t lddv,
                                   void *stream, uint32_t threshold, float keep_scale, uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_MHA_DROP_H */
