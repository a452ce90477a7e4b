// mha.hip -- sparse multi-head dot-product attention with separate keys and values over the stored entries of a CSR matrix, all heads in
// one launch, forward and backward (include/isplib_hip_mha.h: isplib_mha_csr_hip, isplib_mha_bw_rows_hip, isplib_mha_bw_cols_hip).  For
// every row i, stored entry e = (i, j) and head h, with q [m, k], key [n, k], v [n, k], k = H*d (head h owns the columns [h*d, (h+1)*d))
// and a scalar scale p:
//    s_e  = p <q_i, key_j>_h     a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)     z_i[head h] = sum_e a_e v_j[head h]
// and for g = dL/dz
//    D[i,h] = <g_i, z_i>_h       t_e = <g_i, v_j>_h          ds_e = a_e (t_e - D[i,h])
//    dq_i[head h]   = p sum_e ds_e key_j[head h]
//    dkey_j[head h] = p sum_{e -> j} ds_e q_i[head h]
//    dv_j[head h]   = sum_{e -> j} a_e g_i[head h].
// Stored values are not read; every stored entry is its own edge; an empty row has z_i = 0, lse = -inf, D = 0, dq_i = 0; a column no
// entry references has dkey_j = dv_j = 0.
//
// Mapping: that of gatv2.hip -- one wave per row (per column of A in the columns kernel), G = 64 / LPR edge slots, NCH chunks of 4
// consecutive columns per lane, the same (LPR, NCH) instantiations, head geometry and per-head butterfly.  What is new is the second
// gathered operand: per edge and chunk the forward and the rows kernel issue TWO 16-byte gathers, key_j for the score and v_j for the
// value, each behind its own descriptor.  The dot products of a step (U scores in the forward, U scores and U <g_i, v_j>_h in the
// backward kernels) go through the levels of ONE butterfly together.  p multiplies the finished dot product, in all three kernels alike,
// and the finished rows of dq and dkey.
//
// The softmax is the online form of gatv2.hip per chunk: (m, l, acc) rescaled once per step, a finite "no edge yet" sentinel, the G
// slots merged pairwise at the end of the row.  The backward stores nothing per edge: a_e is recomputed from lse.  The rows kernel
// holds q_i, g_i and z_i, forms D[i,h] from them and writes dq and D.  The columns kernel walks the transposed structure with key_j
// and v_j in registers, gathers q_i and g_i (16 bytes each) and lse, D of [i, head] (4 bytes each, two tables, each behind its own
// descriptor), and writes dkey and dv as two outputs.
//
// Every gathered table sits behind a buffer descriptor of exactly the extent it owns; dead edges and lanes past k carry BUF_OOB, which
// the descriptor answers with 0.  No atomics, no LDS, a fixed order of operations: two launches give equal bits.  The column
// map, the descriptor, the gathers and the butterfly are those of attn_common.h, shared with gat.hip and gatv2.hip.  DESIGN.md 4.6k, 4.6n.
//
// Attention dropout (include/isplib_hip_mha_drop.h: isplib_qkv_drop_*_hip): the three kernels are templates on DROP.
// Every stored entry e and head h has a keep bit q_e,h = word(seed, CSR position of e, h) >= T (gat_dropout.h: the bit of gat.hip and
// gatv2.hip, a pure function, recomputed in all three kernels, nothing stored), and with c = float32(1 / (1 - p)):
//    z_i = c sum_e q_e a_e v_j      t_e = q_e c <g_i, v_j>_h      dv_j = sum_{e -> j} q_e c a_e g_i
//    a_e, lse, s_e and the form of ds_e unchanged
// The softmax runs over ALL stored entries: l, m and lse do not see the mask, and a dropped edge still gets ds_e = -a_e D.  The lane that
// loads an entry's index hashes the entry's position (base + lane in the forward and the rows kernel; csr2csc[pos] in the columns
// kernel, which walks the transposed structure and therefore takes csr2csc) and hands the word across with the index; per edge and chunk
// one add of a per-lane constant, one fmix32, one compare and one select remain.  c multiplies the finished row of z and t_e per edge;
// the value coefficient of dv is q_e ? a_e c : 0 per edge and head.  The seed is a kernel argument: a captured graph replays one mask.
// DROP = false is the code it was (profiles/mha_dropout_isa.txt).
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "gat_dropout.h"
#include "attn_common.h"

namespace isplib {

constexpr float MHA_NONE = -FLT_MAX;       // the running maximum of a chunk that saw no edge
constexpr int MHA_WAVES = 4;               // rows per block

struct MhaArgs {
   int64_t rows, k;                        // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                             // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                             // lanes of one chunk that share a head: d / 4 (H == 1: 64, the whole slot)
   unsigned hmask;                         // c & hmask == 0: the first column of a head (H == 1: only column 0)
   int whole;                              // H == 1: the head spans both chunks of a lane
   const int64_t *indx, *pntrb, *pntre;
   float p;                                // the scale of the scores
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const float *own;                       // forward, rows: q | columns: key
   int64_t ldown;
   const float *own2;                      // columns: v
   int64_t ldown2;
   const float *g;                         // rows: dL/dz
   int64_t ldg;
   const float *zin;                       // rows: z of the forward
   int64_t ldzin;
   const float *lse_in;                    // rows: lse [rows, H]
   float *out;                             // z | dq | dkey
   int64_t ldout;
   float *out2;                            // columns: dv
   int64_t ldout2;
   float *hout;                            // [rows, H]: forward lse | rows: D
   // the gathered operands, each behind one descriptor
   const float *ga;                        // forward, rows: key | columns: q
   int64_t ldga;
   unsigned gabytes;
   const float *gb;                        // forward, rows: v | columns: g
   int64_t ldgb;
   unsigned gbbytes;
   const float *t1, *t2;                   // columns: lse, D; both [gathered rows, H]
   unsigned tbytes;
   // DROP only (appended)
   const int64_t *epos;                    // columns: csr2csc [nnz], the CSR position of every entry of the transposed structure
   unsigned seed_lo, seed_hi;              // the two halves of the seed
   unsigned T;                             // keep: word >= T
   float c;                                // float32(1 / (1 - p))
};

template <int LPR, int NCH, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha_fw_kernel(const MhaArgs a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsk = attn_rsrc(a.ga, a.gabytes), rsv = attn_rsrc(a.gb, a.gbbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float qv[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, qv);
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   float mrun[NCH], l[NCH], acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      mrun[j] = MHA_NONE;
      l[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;
   }

   const unsigned ldkb = (unsigned)a.ldga * 4u, ldvb = (unsigned)a.ldgb * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t kv[U][NCH], vv[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            attn_load_wide<LPR, NCH>(rsk, attn_off(id, ldkb), cm, kv[u]);
            attn_load_wide<LPR, NCH>(rsv, attn_off(id, ldvb), cm, vv[u]);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float sc[U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < NCH; j++) sc[u][j] = attn_dot_part(qv[j], kv[u][j], cm.ok[j]);
         attn_head_reduce<LPR, NCH, U>(sc, a.whole, a.hlanes);
#pragma unroll
         for (int j = 0; j < NCH; j++) {
            float mnew = mrun[j];
#pragma unroll
            for (int u = 0; u < U; u++) {
               sc[u][j] *= a.p;
               mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u][j]) : mnew;      // a NaN score is not a maximum; it enters through exp below
            }
            const float r = __expf(mrun[j] - mnew);
            mrun[j] = mnew;
            l[j] *= r;
#pragma unroll
            for (int v = 0; v < 4; v++) acc[j][v] *= r;
#pragma unroll
            for (int u = 0; u < U; u++) {
               const float w = (s0 + u * G + g < cnt) ? __expf(sc[u][j] - mnew) : 0.0f;
               l[j] += w;                                 // the softmax runs over every stored entry: the mask reaches the values only
               float wk = w;
               if constexpr (DROP) wk = gat_drop_mix(hw[u], hk[j]) >= a.T ? w : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(wk, __int_as_float(vv[u][j][v]), acc[j][v]);
            }
         }
      }
   }
   // merge the G slots pairwise, by the rule of a step
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const float mo = __shfl_xor(mrun[j], o), lo = __shfl_xor(l[j], o);
         const float mnew = fmaxf(mrun[j], mo);
         const float ra = __expf(mrun[j] - mnew), rb = __expf(mo - mnew);
         l[j] = l[j] * ra + lo * rb;
#pragma unroll
         for (int v = 0; v < 4; v++) acc[j][v] = acc[j][v] * ra + __shfl_xor(acc[j][v], o) * rb;
         mrun[j] = mnew;
      }
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
#pragma unroll
      for (int v = 0; v < 4; v++) {
         acc[j][v] = empty ? 0.0f : acc[j][v] / l[j];
         if constexpr (DROP) acc[j][v] *= a.c;
      }
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? -INFINITY : mrun[j] + logf(l[j]);
   }
   attn_store_row<LPR, NCH>(a.out, row, a.ldout, lc, cm.ok, acc);
}

// one wave per row i: q_i, g_i and D[i,h] in registers; key_j and v_j gathered
template <int LPR, int NCH, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha_bw_rows_kernel(const MhaArgs a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsk = attn_rsrc(a.ga, a.gabytes), rsv = attn_rsrc(a.gb, a.gbbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float qv[NCH][4], gv[NCH][4], lse[NCH], dsum[NCH];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, qv);
   attn_own_row<LPR, NCH>(a.g, row, a.ldg, lc, cm.ok, gv);
   attn_own_head<LPR, NCH>(a.lse_in, row, a.heads, cm, lse);
   {
      // D[i,h] = <g_i, z_i>_h: every slot holds the row, so every lane of a head ends with it
      float zv[NCH][4], dp[1][NCH];
      attn_own_row<LPR, NCH>(a.zin, row, a.ldzin, lc, cm.ok, zv);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         dp[0][j] = 0.0f;
#pragma unroll
         for (int v = 0; v < 4; v++) dp[0][j] = fmaf(gv[j][v], zv[j][v], dp[0][j]);
      }
      attn_head_reduce<LPR, NCH, 1>(dp, a.whole, a.hlanes);
#pragma unroll
      for (int j = 0; j < NCH; j++) dsum[j] = dp[0][j];
   }

   float acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   const unsigned ldkb = (unsigned)a.ldga * 4u, ldvb = (unsigned)a.ldgb * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t kv[U][NCH], vv[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            attn_load_wide<LPR, NCH>(rsk, attn_off(id, ldkb), cm, kv[u]);
            attn_load_wide<LPR, NCH>(rsv, attn_off(id, ldvb), cm, vv[u]);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float part[2 * U][NCH];                       // <q_i, key_j>_h and t_e of the step through one butterfly
#pragma unroll
         for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               part[u][j] = attn_dot_part(qv[j], kv[u][j], cm.ok[j]);
               part[U + u][j] = attn_dot_part(gv[j], vv[u][j], cm.ok[j]);
            }
         attn_head_reduce<LPR, NCH, 2 * U>(part, a.whole, a.hlanes);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               if constexpr (DROP) part[U + u][j] *= gat_drop_mix(hw[u], hk[j]) >= a.T ? a.c : 0.0f;      // t_e = q_e c <g_i, v_j>_h
               const float ds = live ? __expf(part[u][j] * a.p - lse[j]) * (part[U + u][j] - dsum[j]) : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(ds, __int_as_float(kv[u][j][v]), acc[j][v]);
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 4; v++) acc[j][v] += __shfl_xor(acc[j][v], o);
   if (g != 0) return;
   const bool empty = ee <= eb;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = empty ? 0.0f : a.p * acc[j][v];
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? 0.0f : dsum[j];
   }
   attn_store_row<LPR, NCH>(a.out, row, a.ldout, lc, cm.ok, acc);
}

// one wave per column j of A (a row of the transposed structure): key_j and v_j in registers; q_i, g_i and lse, D of [i, head] gathered
template <int LPR, int NCH, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha_bw_cols_kernel(const MhaArgs a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsq = attn_rsrc(a.ga, a.gabytes), rsg = attn_rsrc(a.gb, a.gbbytes);
   const __amdgpu_buffer_rsrc_t rs1 = attn_rsrc(a.t1, a.tbytes), rs2 = attn_rsrc(a.t2, a.tbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float kv[NCH][4], vv[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, kv);
   attn_own_row<LPR, NCH>(a.own2, row, a.ldown2, lc, cm.ok, vv);

   float dk[NCH][4], dv[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) dk[j][v] = dv[j][v] = 0.0f;
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   const unsigned ldqb = (unsigned)a.ldga * 4u, ldgb = (unsigned)a.ldgb * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, of its CSR position (nnz < 2^31)
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, pos < ee ? (unsigned)a.epos[pos] : 0u);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t qg[U][NCH], gg[U][NCH];
         float ls[U][NCH], dd[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            attn_load_wide<LPR, NCH>(rsq, attn_off(id, ldqb), cm, qg[u]);
            attn_load_wide<LPR, NCH>(rsg, attn_off(id, ldgb), cm, gg[u]);
            attn_load_head<LPR, NCH>(rs1, attn_off(id, hb), cm, ls[u]);
            attn_load_head<LPR, NCH>(rs2, attn_off(id, hb), cm, dd[u]);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float part[2 * U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               part[u][j] = attn_dot_part(kv[j], qg[u][j], cm.ok[j]);
               part[U + u][j] = attn_dot_part(vv[j], gg[u][j], cm.ok[j]);
            }
         attn_head_reduce<LPR, NCH, 2 * U>(part, a.whole, a.hlanes);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               const float ae = live ? __expf(part[u][j] * a.p - ls[u][j]) : 0.0f;
               float aev = ae;                            // the value coefficient: q_e c a_e
               if constexpr (DROP) {
                  const bool keep = gat_drop_mix(hw[u], hk[j]) >= a.T;
                  part[U + u][j] *= keep ? a.c : 0.0f;    // t_e = q_e c <g_i, v_j>_h
                  aev = keep ? ae * a.c : 0.0f;
               }
               const float ds = live ? ae * (part[U + u][j] - dd[u][j]) : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) {
                  dk[j][v] = fmaf(ds, __int_as_float(qg[u][j][v]), dk[j][v]);
                  dv[j][v] = fmaf(aev, __int_as_float(gg[u][j][v]), dv[j][v]);
               }
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 4; v++) {
            dk[j][v] += __shfl_xor(dk[j][v], o);
            dv[j][v] += __shfl_xor(dv[j][v], o);
         }
   if (g != 0) return;
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) dk[j][v] *= a.p;    // no incoming entry: 0
   attn_store_row<LPR, NCH>(a.out, row, a.ldout, lc, cm.ok, dk);
   attn_store_row<LPR, NCH>(a.out2, row, a.ldout2, lc, cm.ok, dv);
}

enum { MHA_FW = 0, MHA_BW_ROWS = 1, MHA_BW_COLS = 2 };

// edges of a slot per step: 4 in the forward and the rows kernel; the columns kernel gathers four tables per edge and takes half the
// edges per step where a lane holds two chunks (profiles/mha_isa.txt: no instantiation uses scratch)
template <int LPR, int NCH, bool DROP>
static int launch_mha(int which, const MhaArgs &a, const char *entry, hipStream_t st) {
   constexpr int UC = NCH >= 2 ? 2 : 4;
   const int64_t nb = (a.rows + MHA_WAVES - 1) / MHA_WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block((unsigned)MHA_WAVES * 64u);
   if (which == MHA_FW) hipLaunchKernelGGL((mha_fw_kernel<LPR, NCH, MHA_WAVES, 4, DROP>), grid, block, 0, st, a);
   else if (which == MHA_BW_ROWS) hipLaunchKernelGGL((mha_bw_rows_kernel<LPR, NCH, MHA_WAVES, 4, DROP>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((mha_bw_cols_kernel<LPR, NCH, MHA_WAVES, UC, DROP>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the width ladder (attn_by_width); DROP: the kernels with attention dropout
static int mha_by_width(int which, const MhaArgs &a, bool drop, const char *entry, hipStream_t st) {
   return attn_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      return drop ? launch_mha<LPR, NCH, true>(which, a, entry, st) : launch_mha<LPR, NCH, false>(which, a, entry, st);
   });
}

// what the dropout entries (isplib_qkv_drop_*_hip) refuse before a launch: attn_drop_refusal, and the keep bit is a function of a seed
// below 2^63
static const char *mha_drop_refusal(const AttnDrop &dr, int64_t nnz) {
   if (const char *why = attn_drop_refusal(dr, nnz, "keep_scale must be a positive finite number")) return why;
   return dr.on && dr.seed >= (1ull << 63) ? "seed must be below 2^63" : nullptr;
}

static const char *const MHA_DOMAIN = "outside isplib_mha_serves(rows_gathered, heads, d, ld) = isplib_gat_serves: 1 <= heads, 1 <= d, "
                                      "heads*d <= 512, heads == 1 or d a power of two >= 4, ld >= heads*d, rows_gathered < 2^31, "
                                      "rows_gathered*ld*4 <= 3.5 GiB";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_mha_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_mha_serves(rows_gathered, heads, d, ld);
}

// The three entries, with and without attention dropout.
static int mha_forward(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                       const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key, int64_t ldk,
                       const float *v, int64_t ldv, float *z, int64_t ldz, float *lse, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = mha_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !q || !z || !lse || (nnz > 0 && (!indx || !key || !v))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldq < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_mha_serves(n, heads, k / heads, ldk) || !isplib_mha_serves(n, heads, k / heads, ldv))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA_DOMAIN);
   MhaArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = q; a.ldown = ldq;
   a.out = z; a.ldout = ldz; a.hout = lse;
   a.ga = key; a.ldga = ldk; a.gabytes = nnz > 0 ? attn_extent(n, k, ldk) : 0u;
   a.gb = v; a.ldgb = ldv; a.gbbytes = nnz > 0 ? attn_extent(n, k, ldv) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha_by_width(MHA_FW, a, dr.on, entry, (hipStream_t)stream);
}

static int mha_backward_rows(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                             const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                             int64_t ldk, const float *v, int64_t ldv, const float *g, int64_t ldg, const float *z, int64_t ldz,
                             const float *lse, float *dq, int64_t lddq, float *dsum, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = mha_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !q || !g || !z || !lse || !dq || !dsum || (nnz > 0 && (!indx || !key || !v)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldq < k || ldg < k || ldz < k || lddq < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_mha_serves(n, heads, k / heads, ldk) || !isplib_mha_serves(n, heads, k / heads, ldv))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA_DOMAIN);
   MhaArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = q; a.ldown = ldq; a.g = g; a.ldg = ldg; a.zin = z; a.ldzin = ldz; a.lse_in = lse;
   a.out = dq; a.ldout = lddq; a.hout = dsum;
   a.ga = key; a.ldga = ldk; a.gabytes = nnz > 0 ? attn_extent(n, k, ldk) : 0u;
   a.gb = v; a.ldgb = ldv; a.gbbytes = nnz > 0 ? attn_extent(n, k, ldv) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha_by_width(MHA_BW_ROWS, a, dr.on, entry, (hipStream_t)stream);
}

static int mha_backward_cols(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                             const int64_t *cole, const int64_t *csr2csc, int64_t heads, float scale, const float *q, int64_t ldq,
                             const float *g, int64_t ldg, const float *lse, const float *dsum, const float *key, int64_t ldk,
                             const float *v, int64_t ldv, float *dkey, int64_t lddk, float *dv, int64_t lddv, void *stream,
                             const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = mha_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (dr.on && nnz > 0 && !csr2csc) return fail(ISPLIB_FAIL, entry, "null csr2csc: the keep bit is a function of the CSR position");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!colb || !cole || !key || !v || !dkey || !dv || (nnz > 0 && (!row_t || !q || !g || !lse || !dsum)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldk < k || ldv < k || lddk < k || lddv < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_mha_serves(m, heads, k / heads, ldq) || !isplib_mha_serves(m, heads, k / heads, ldg))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA_DOMAIN);
   MhaArgs a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.p = scale;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = key; a.ldown = ldk; a.own2 = v; a.ldown2 = ldv;
   a.out = dkey; a.ldout = lddk; a.out2 = dv; a.ldout2 = lddv;
   a.ga = q; a.ldga = ldq; a.gabytes = nnz > 0 ? attn_extent(m, k, ldq) : 0u;
   a.gb = g; a.ldgb = ldg; a.gbbytes = nnz > 0 ? attn_extent(m, k, ldg) : 0u;
   a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn_extent(m, heads, heads) : 0u;
   if (dr.on) a.epos = csr2csc;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha_by_width(MHA_BW_COLS, a, dr.on, entry, (hipStream_t)stream);
}

extern "C" int isplib_mha_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                  const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                                  int64_t ldk, const float *v, int64_t ldv, float *z, int64_t ldz, float *lse, void *stream) {
   return mha_forward("isplib_mha_csr_hip", m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, z, ldz, lse, stream);
}

extern "C" int isplib_mha_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                      const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                                      int64_t ldk, const float *v, int64_t ldv, const float *g, int64_t ldg, const float *z,
                                      int64_t ldz, const float *lse, float *dq, int64_t lddq, float *dsum, void *stream) {
   return mha_backward_rows("isplib_mha_bw_rows_hip", m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, g, ldg, z,
                            ldz, lse, dq, lddq, dsum, stream);
}

extern "C" int isplib_mha_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                      const int64_t *cole, int64_t heads, float scale, const float *q, int64_t ldq, const float *g,
                                      int64_t ldg, const float *lse, const float *dsum, const float *key, int64_t ldk, const float *v,
                                      int64_t ldv, float *dkey, int64_t lddk, float *dv, int64_t lddv, void *stream) {
   return mha_backward_cols("isplib_mha_bw_cols_hip", m, n, k, nnz, row_t, colb, cole, nullptr, heads, scale, q, ldq, g, ldg, lse, dsum,
                            key, ldk, v, ldv, dkey, lddk, dv, lddv, stream);
}

// attention dropout: the argument lists of the entries above (the columns entry with csr2csc after cole), then threshold, keep_scale, seed
extern "C" int isplib_qkv_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                       const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq, const float *key,
                                       int64_t ldk, const float *v, int64_t ldv, float *z, int64_t ldz, float *lse, void *stream,
                                       uint32_t threshold, float keep_scale, uint64_t seed) {
   return mha_forward("isplib_qkv_drop_csr_hip", m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, z, ldz, lse,
                      stream, AttnDrop{true, threshold, keep_scale, seed});
}

extern "C" int isplib_qkv_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                           const int64_t *pntre, int64_t heads, float scale, const float *q, int64_t ldq,
                                           const float *key, int64_t ldk, const float *v, int64_t ldv, const float *g, int64_t ldg,
                                           const float *z, int64_t ldz, const float *lse, float *dq, int64_t lddq, float *dsum,
                                           void *stream, uint32_t threshold, float keep_scale, uint64_t seed) {
   return mha_backward_rows("isplib_qkv_drop_bw_rows_hip", m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, g,
                            ldg, z, ldz, lse, dq, lddq, dsum, stream, AttnDrop{true, threshold, keep_scale, seed});
}

extern "C" int isplib_qkv_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                           const int64_t *cole, const int64_t *csr2csc, int64_t heads, float scale, const float *q,
                                           int64_t ldq, const float *g, int64_t ldg, const float *lse, const float *dsum,
                                           const float *key, int64_t ldk, const float *v, int64_t ldv, float *dkey, int64_t lddk,
                                           float *dv, int64_t lddv, void *stream, uint32_t threshold, float keep_scale, uint64_t seed) {
   return mha_backward_cols("isplib_qkv_drop_bw_cols_hip", m, n, k, nnz, row_t, colb, cole, csr2csc, heads, scale, q, ldq, g, ldg, lse,
                            dsum, key, ldk, v, ldv, dkey, lddk, dv, lddv, stream, AttnDrop{true, threshold, keep_scale, seed});
}
