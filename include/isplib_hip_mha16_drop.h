/*
 * isplib_hip_mha16_drop.h -- the 16-bit multi-head attention entries (q, k, v) with attention dropout of libisplib_hip.so.  isplib_hip.h
 * includes this file near its end, right before isplib_hip_mha16.h (which stays its last include), so a program that includes
 * isplib_hip.h has these entries too; a program may also include this file alone.  They are kept in a file of their own, with a name
 * list of their own in isplib_amd/cabi.py (MHA16_DROP_EXPORTS), for the reason isplib_hip_gatv2_16.h gives.  Their names start with
 * isplib_qkv_half_drop_: the symbols that start with isplib_mha, isplib_qkv16 and isplib_qkv_drop are pinned to MHA_EXPORTS,
 * MHA16_EXPORTS and MHA_DROP_EXPORTS (tests/test_mha_host.py, tests/test_mha16_host.py, tests/test_mha_dropout_host.py).
 * tests/test_mha16_dropout_host.py compares this header, MHA16_DROP_EXPORTS and the library.
 *
 * The attention with attention dropout of isplib_hip_mha_drop.h (isplib_qkv_drop_*) for wide operands of 16-bit elements (dtype:
 * ISPLIB_DTYPE_BF16 | _F16), on the kernels and under the contract of isplib_hip_mha16.h (isplib_qkv16_*): q, key, v, g, z, dq, dkey and
 * dv are `dtype` and are never widened in memory; widening is exact, every product, sum, exponential and division is fp32, each wide
 * output is rounded ONCE, to nearest even; lse and dsum (D) are fp32.  With the keep bit q_e,h in {0, 1}, c = `keep_scale` =
 * float32(1 / (1 - p)) and p_s = `scale`:
 *   s_e, a_e, lse[i,h]   exactly as without dropout: the softmax runs over ALL stored entries, lse does not see the mask
 *   z_i[head h]    = round16( c (sum_e q_e a_e v_j[head h]) )     the finished row times c, then the one rounding
 *   t_e            = q_e c <g_i, v_j>_h                           D[i,h] = sum_e a_e t_e     (fp32, from the row's edges: z is NOT read)
 *   ds_e           = a_e (t_e - D[i,h])                           (a dropped edge still gets -a_e D)
 *   dq_i[head h]   = p_s sum_e ds_e key_j[head h]                 (one pass: p_s (P - D Q), P_c = sum a_e t_e key_jc, Q_c = sum a_e key_jc)
 *   dkey_j[head h] = p_s sum_{e -> j} ds_e q_i[head h]
 *   dv_j[head h]   = sum_{e -> j} q_e c a_e g_i[head h].
 * The keep bit is the one of isplib_gat_drop_*_hip, isplib_gatv2_drop_*_hip and isplib_qkv_drop_*_hip, unchanged: q_e,h =
 * isplib_gat_drop_word(seed, pos_e, h) >= threshold, pos_e the position of the entry in indx (its CSR position), threshold =
 * isplib_gat_drop_threshold(p); a pure function recomputed in all three entries -- no mask is stored, no RNG state is kept, and equal
 * arguments give equal bits.  Under one seed the mask is the fp32 entries' mask.  seed < 2^63, nnz < 2^31.  Every stored entry has its
 * own bit, duplicates (i, j) included.  An empty row has z = 0, lse = -inf, D = 0, dq = 0; a live (row, head) whose entries are all
 * dropped has z = 0 exactly there and a finite lse; a row of one kept entry has z_i = round16(float32(v_j c)).  With threshold = 0 and
 * keep_scale = 1 the results are those of isplib_qkv16_*_hip bit for bit.  The seed is an argument of the launch: a captured graph
 * replays one mask.  No atomics, no LDS, a fixed order of operations: two launches give equal bits.
 *   isplib_qkv_half_drop_csr_hip      the arguments of isplib_qkv16_csr_hip, then threshold, keep_scale, seed.
 *   isplib_qkv_half_drop_bw_rows_hip  the arguments of isplib_qkv16_bw_rows_hip, then threshold, keep_scale, seed.
 *   isplib_qkv_half_drop_bw_cols_hip  the arguments of isplib_qkv16_bw_cols_hip with csr2csc (nnz entries: the CSR position of every
 *                                     entry of the transposed structure) after cole, then threshold, keep_scale, seed.
 * Domain: isplib_qkv16_serves, as for the 16-bit entries without dropout.  The refusals come in one order, all before any launch, and
 * leave the outputs untouched: first those of the matching isplib_qkv16_* entry in its own order (another dtype, a negative dimension:
 * ISPLIB_FAIL; m == 0 or k == 0 -- n == 0 or k == 0 in the third entry -- succeeds without a launch; a short pitch, k % heads, a scale
 * that is not finite: ISPLIB_FAIL; outside the domain: ISPLIB_NO_OPT_IMPL; a null operand, a misaligned base: ISPLIB_FAIL), then those
 * of the fp32 dropout entries: a keep_scale that is not a positive finite number, nnz >= 2^31, seed >= 2^63, a null csr2csc with
 * nnz > 0 (third entry): ISPLIB_FAIL.  The ABI version stays 1.
 * isplib_qkv_half_drop_native_pays is the measured rule of the layers above (forward + backward of mha_matmul with dropout on bf16
 * operands: these entries against "widen, the fp32 dropout entries, narrow"; profiles/mha16_dropout_ab.txt), over the
 * family's classes (the gathered operand beyond 256 MiB at 2 bytes per element or not): nonzero only where EVERY native run was faster
 * than EVERY run of the conversion route on every measured shape of the class.
 */
#ifndef ISPLIB_HIP_MHA16_DROP_H
#define ISPLIB_HIP_MHA16_DROP_H

#include "isplib_hip.h"        /* ISPLIB_DTYPE_*, the status codes, isplib_gat_drop_threshold / isplib_gat_drop_word */

#ifdef __cplusplus
extern "C" {
#endif

int    isplib_qkv_half_drop_csr_hip(int dtype /* ISPLIB_DTYPE_BF16 | _F16 */, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                    const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale,
                                    const void *q, int64_t ldq, const void *key, int64_t ldk, const void *v, int64_t ldv, void *z,
                                    int64_t ldz, float *lse /* m x heads */, void *stream, uint32_t threshold, float keep_scale,
                                    uint64_t seed);
int    isplib_qkv_half_drop_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                                        const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale, const void *q,
                                        int64_t ldq, const void *key, int64_t ldk, const void *v, int64_t ldv, const void *g,
                                        int64_t ldg, const float *lse, void *dq, int64_t lddq, float *dsum /* m x heads */,
                                        void *stream, uint32_t threshold, float keep_scale, uint64_t seed);
int    isplib_qkv_half_drop_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t,
                                        const int64_t *colb, const int64_t *cole, const int64_t *csr2csc /* nnz */, int64_t heads,
                                        float scale, const void *q, int64_t ldq, const void *g, int64_t ldg, const float *lse,
                                        const float *dsum, const void *key, int64_t ldk, const void *v, int64_t ldv, void *dkey,
                                        int64_t lddk, void *dv, int64_t lddv, void *stream, uint32_t threshold, float keep_scale,
                                        uint64_t seed);
static inline int isplib_qkv_half_drop_native_pays(int64_t rows_gathered, int64_t ld) {
   /* measured (profiles/mha16_dropout_ab.txt: the Reddit shape at (H, d) = (8, 8) and (8, 16) -- gathered operand inside 256 MiB -- and
    * the ogbn-products shape at (8, 16) -- beyond it; bf16, p = 0.6, scale 1/sqrt(d), forward + backward, 5 alternating runs of 5 steps,
    * run spread at most 0.6 % on either side): every native run is below every run of the conversion route in both classes --
    * 0.562-0.564 of its time inside 256 MiB, 0.494 beyond (forward alone 0.508-0.522 and 0.431), at 0.09-0.10 of its peak memory.  Both
    * classes pay. */
   return (rows_gathered > 0 && ld > 0) ? 1 : 0;
}
int    isplib_qkv_half_drop_auto(int64_t rows_gathered, int64_t ld);              /* the same rule as a symbol */

#ifdef __cplusplus
}
#endif
#endif /* ISPLIB_HIP_MHA16_DROP_H */
