// gatv2.hip -- GATv2 attention aggregation over the stored entries of a CSR matrix, all heads in one launch, forward and backward
// (include/isplib_hip.h: isplib_gatv2_csr_hip, isplib_gatv2_bw_rows_hip, isplib_gatv2_bw_cols_hip).  For every row i, stored entry
// e = (i, j) and head h, with x [m, k], y [n, k], k = H*d (head h owns the columns [h*d, (h+1)*d)), att [H, d] (k contiguous floats) and
// a slope ns, c running over the head's columns:
//    u_ec = x_ic + y_jc          sl_ec = u_ec > 0 ? 1 : ns        v_ec = sl_ec u_ec          s_e = sum_c att_c v_ec
//    a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)                              z_i[head h] = sum_e a_e y_j[head h]
// and for g = dL/dz
//    D[i,h] = <g_i, z_i>_h       t_e = <g_i, y_j>_h               ds_e = a_e (t_e - D[i,h])  q_ec = ds_e att_c sl_ec
//    dx_ic  = sum_e q_ec         dy_jc = sum_{e -> j} (a_e g_ic + q_ec)                      datt_c = sum_{all e} ds_e v_ec.
// Stored values are not read; every stored entry is its own edge; an empty row has z_i = 0, lse = -inf, D = 0, dx_i = 0.
//
// Mapping: that of gat.hip -- one wave per row (per column of A in the columns kernel), G = 64 / LPR edge slots, NCH chunks of 4
// consecutive columns per lane, the head geometry and the per-head butterfly of gat.hip.  The gathered row y_j serves both the score and
// the value, as in attention.hip: one 16-byte gather per lane and edge is all the memory work of the forward.  u_ec is ONE fp32 add and
// the branch is taken on it, so the slope is that of the exact sum; the add is not fused with anything.  The dot products of a step (U
// scores in the forward, U scores and U <g_i, y_j>_h in the backward kernels) go through the levels of ONE butterfly together: the
// transposed butterfly of gather.h needs a compile-time group width and the head width is a launch argument, so every value keeps its
// lane and the levels are shared instead.
//
// The softmax is the online form of gat.hip per chunk.  The backward stores nothing per edge: a_e is recomputed from lse.  The rows kernel
// holds x_i, g_i and att, forms D[i,h] from z_i and writes dx and D; for datt every lane sums ds_e v_ec over its row's edges, the waves
// of a block fold those sums through LDS (one __syncthreads; every wave of the block reaches it, rows past m contribute zeros) and the
// block writes ONE partial row to the caller's workspace, which gatv2_fold_kernel adds up in a fixed order.  datt == NULL selects an
// instantiation without any of that.  The columns kernel walks the transposed structure with y_j and att in registers, gathers x_i and
// g_i (16 bytes each) and lse, D of [i, head] (4 bytes each, two tables, each behind its own descriptor), and writes dy.
//
// Every gathered table sits behind a buffer descriptor of exactly the extent it owns; dead edges and lanes past k carry BUF_OOB, which
// the descriptor answers with 0.  No atomics, a fixed order of operations: two launches give equal bits.  The column map, the
// descriptor, the gathers and the butterfly are those of attn_common.h, shared with gat.hip and mha.hip.  DESIGN.md 4.6f, 4.6n.
//
// Attention dropout (include/isplib_hip_gatv2_drop.h: isplib_gatv2_drop_*_hip): the three kernels are templates on
// DROP.  Every stored entry e and head h has a keep bit q_e,h = word(seed, CSR position of e, h) >= T (gat_dropout.h: the bit of
// gat.hip, a pure function, recomputed in all three kernels, nothing stored), and with c = float32(1 / (1 - p)), r_ec the q_ec above:
//    z_i = c sum_e q_e a_e y_j      t_e = q_e c <g_i, y_j>_h      dy_jc = sum_{e -> j} (q_e c a_e g_ic + r_ec)
//    a_e, lse, s_e and the form of ds_e unchanged
// The softmax runs over ALL stored entries: l, m and lse do not see the mask, and a dropped edge still gets ds_e = -a_e D.  The lane that
// loads an entry's index hashes the entry's position (base + lane in the forward and the rows kernel; csr2csc[pos] in the columns
// kernel, which walks the transposed structure and therefore takes csr2csc) and hands the word across with the index; per edge and chunk
// one add of a per-lane constant, one fmix32, one compare and one select remain.  c multiplies the finished row of z and t_e per edge; dy
// mixes a masked term with an unmasked one, so its value coefficient is q_e ? a_e c : 0 per edge and head.  The seed is a kernel
// argument: a captured graph replays one mask.  DROP = false is the code it was (profiles/gatv2_dropout_isa.txt).
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "gat_dropout.h"
#include "attn_common.h"

namespace isplib {

constexpr float GATV2_NONE = -FLT_MAX;     // the running maximum of a chunk that saw no edge
constexpr int GATV2_WAVES = 4;             // rows per block: forward and columns kernel
constexpr int GATV2_ROWS_WAVES = 8;        // rows per block of the rows kernel: one partial row of datt per 8 rows

struct Gatv2Args {
   int64_t rows, k;                        // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                             // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                             // lanes of one chunk that share a head: d / 4 (H == 1: 64, the whole slot)
   unsigned hmask;                         // c & hmask == 0: the first column of a head (H == 1: only column 0)
   int whole;                              // H == 1: the head spans both chunks of a lane
   const int64_t *indx, *pntrb, *pntre;
   float ns;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const float *own;                       // forward, rows: x | columns: y
   int64_t ldown;
   const float *g;                         // rows: dL/dz
   int64_t ldg;
   const float *zin;                       // rows: z of the forward
   int64_t ldzin;
   const float *lse_in;                    // rows: lse [rows, H]
   const float *att;                       // [k]
   float *out;                             // z | dx | dy
   int64_t ldout;
   float *hout;                            // [rows, H]: forward lse | rows: D
   float *part;                            // rows, with datt: [blocks, k] partial rows of datt
   // the gathered operands, each behind one descriptor
   const float *y;                         // forward, rows: y | columns: x
   int64_t ldy;
   unsigned ybytes;
   const float *y2;                        // columns: g
   int64_t ldy2;
   unsigned y2bytes;
   const float *t1, *t2;                   // columns: lse, D; both [gathered rows, H]
   unsigned tbytes;
   // DROP only (appended)
   const int64_t *epos;                    // columns: csr2csc [nnz], the CSR position of every entry of the transposed structure
   unsigned seed_lo, seed_hi;              // the two halves of the seed
   unsigned T;                             // keep: word >= T
   float c;                                // float32(1 / (1 - p))
};

// v_ec = leaky_relu(u_ec), u_ec = r + t: ONE fp32 add, so its sign is the sign of the exact sum; u == 0 takes ns
__device__ __forceinline__ float gatv2_leaky(float r, float t, float ns, bool &pos) {
   const float u = r + t;
   pos = u > 0.0f;
   return pos ? u : ns * u;
}

// this lane's part of sum_c att_c v_ec for one chunk; a 16-byte load may run into the next row, the mask drops what it brought
__device__ __forceinline__ float gatv2_score_part(const float (&r)[4], const v4i_t &t, const float (&att)[4], const bool (&ok)[4], float ns) {
   float p = 0.0f;
#pragma unroll
   for (int v = 0; v < 4; v++) {
      bool pos;
      p = fmaf(att[v], gatv2_leaky(r[v], ok[v] ? __int_as_float(t[v]) : 0.0f, ns, pos), p);
   }
   return p;
}

template <int LPR, int NCH, int WAVES, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gatv2_fw_kernel(const Gatv2Args a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn_rsrc(a.y, a.ybytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float xv[NCH][4], av[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, xv);
   attn_own_row<LPR, NCH>(a.att, 0, a.k, lc, cm.ok, av);
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   float mrun[NCH], l[NCH], acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      mrun[j] = GATV2_NONE;
      l[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;
   }

   const unsigned ldyb = (unsigned)a.ldy * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            attn_load_wide<LPR, NCH>(rsy, attn_off(__shfl(id_l, (s0 + u * G + g) & 63), ldyb), cm, yv[u]);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float sc[U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < NCH; j++) sc[u][j] = gatv2_score_part(xv[j], yv[u][j], av[j], cm.ok[j], a.ns);
         attn_head_reduce<LPR, NCH, U>(sc, a.whole, a.hlanes);
#pragma unroll
         for (int j = 0; j < NCH; j++) {
            float mnew = mrun[j];
#pragma unroll
            for (int u = 0; u < U; u++)
               mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u][j]) : mnew;      // a NaN score is not a maximum; it enters through exp below
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
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(wk, __int_as_float(yv[u][j][v]), acc[j][v]);
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
      for (int v = 0; v < 4; v++)
         if (cm.ok[j][v]) {
            float zv = empty ? 0.0f : acc[j][v] / l[j];
            if constexpr (DROP) zv *= a.c;
            a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = zv;
         }
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? -INFINITY : mrun[j] + logf(l[j]);
   }
}

// DATT: every lane also sums ds_e v_ec; the block folds its waves' sums through LDS and writes one partial row.  That instantiation has
// a barrier, so no wave leaves before it: a wave whose row is past a.rows walks an empty row and contributes zeros.
template <int LPR, int NCH, int WAVES, bool DATT, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gatv2_bw_rows_kernel(const Gatv2Args a) {
   constexpr int G = 64 / LPR, U = 4, WCOLS = NCH * LPR * 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   const bool valid = row < a.rows;                    // wave-uniform
   if constexpr (!DATT) {
      if (!valid) return;
   }
   const int64_t eb = valid ? a.pntrb[row] : 0, ee = valid ? a.pntre[row] : 0;
   const __amdgpu_buffer_rsrc_t rsy = attn_rsrc(a.y, a.ybytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float xv[NCH][4], gv[NCH][4], av[NCH][4], lse[NCH], dsum[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      lse[j] = 0.0f;
      dsum[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) xv[j][v] = gv[j][v] = 0.0f;
   }
   attn_own_row<LPR, NCH>(a.att, 0, a.k, lc, cm.ok, av);
   if (valid) {
      attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, xv);
      attn_own_row<LPR, NCH>(a.g, row, a.ldg, lc, cm.ok, gv);
      attn_own_head<LPR, NCH>(a.lse_in, row, a.heads, cm, lse);
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

   float acc[NCH][4], pa[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = pa[j][v] = 0.0f;
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   const unsigned ldyb = (unsigned)a.ldy * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            attn_load_wide<LPR, NCH>(rsy, attn_off(__shfl(id_l, (s0 + u * G + g) & 63), ldyb), cm, yv[u]);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float part[2 * U][NCH];                       // s_e and t_e of the step through one butterfly
#pragma unroll
         for (int u = 0; u < U; u++)
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               part[u][j] = gatv2_score_part(xv[j], yv[u][j], av[j], cm.ok[j], a.ns);
               part[U + u][j] = attn_dot_part(gv[j], yv[u][j], cm.ok[j]);
            }
         attn_head_reduce<LPR, NCH, 2 * U>(part, a.whole, a.hlanes);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               if constexpr (DROP) part[U + u][j] *= gat_drop_mix(hw[u], hk[j]) >= a.T ? a.c : 0.0f;      // t_e = q_e c <g_i, y_j>_h
               const float ds = live ? __expf(part[u][j] - lse[j]) * (part[U + u][j] - dsum[j]) : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) {
                  bool pos;
                  const float lv = gatv2_leaky(xv[j][v], cm.ok[j][v] ? __int_as_float(yv[u][j][v]) : 0.0f, a.ns, pos);
                  const float dsa = ds * av[j][v];
                  acc[j][v] += pos ? dsa : a.ns * dsa;
                  if constexpr (DATT) pa[j][v] = fmaf(ds, lv, pa[j][v]);
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
            acc[j][v] += __shfl_xor(acc[j][v], o);
            if constexpr (DATT) pa[j][v] += __shfl_xor(pa[j][v], o);
         }
   if (valid && g == 0) {
      const bool empty = ee <= eb;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
         for (int v = 0; v < 4; v++)
            if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = empty ? 0.0f : acc[j][v];
         if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? 0.0f : dsum[j];
      }
   }
   if constexpr (DATT) {
      __shared__ float s_pa[WAVES][WCOLS];             // at most 2 KiB per wave
      if (g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 4; v++) s_pa[wave][(j * LPR + lc) * 4 + v] = pa[j][v];      // a row without edges, a lane past k: 0
      }
      __syncthreads();
      const int c = (int)threadIdx.x;                  // WAVES * 64 >= WCOLS: one column per thread
      if (c < WCOLS && c < (int)a.k) {
         float t = 0.0f;
#pragma unroll
         for (int w = 0; w < WAVES; w++) t += s_pa[w][c];      // fixed order
         a.part[(size_t)blockIdx.x * (size_t)a.k + (size_t)c] = t;
      }
   }
}

// one wave per column j of A (a row of the transposed structure): y_j and att in registers; x_i, g_i and lse, D of [i, head] gathered
template <int LPR, int NCH, int WAVES, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gatv2_bw_cols_kernel(const Gatv2Args a) {
   constexpr int G = 64 / LPR, U = NCH >= 2 ? 2 : 4;   // two gather streams: half the edges per step where a lane holds two chunks
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsx = attn_rsrc(a.y, a.ybytes), rsg = attn_rsrc(a.y2, a.y2bytes);
   const __amdgpu_buffer_rsrc_t rs1 = attn_rsrc(a.t1, a.tbytes), rs2 = attn_rsrc(a.t2, a.tbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float yv[NCH][4], av[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, yv);
   attn_own_row<LPR, NCH>(a.att, 0, a.k, lc, cm.ok, av);
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   float acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;

   const unsigned ldxb = (unsigned)a.ldy * 4u, ldgb = (unsigned)a.ldy2 * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, of its CSR position (nnz < 2^31)
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, pos < ee ? (unsigned)a.epos[pos] : 0u);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t xg[U][NCH], gg[U][NCH];
         float ls[U][NCH], dd[U][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            attn_load_wide<LPR, NCH>(rsx, attn_off(id, ldxb), cm, xg[u]);
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
               part[u][j] = gatv2_score_part(yv[j], xg[u][j], av[j], cm.ok[j], a.ns);      // x_ic + y_jc: the add commutes bit for bit
               part[U + u][j] = attn_dot_part(yv[j], gg[u][j], cm.ok[j]);
            }
         attn_head_reduce<LPR, NCH, 2 * U>(part, a.whole, a.hlanes);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               const float ae = live ? __expf(part[u][j] - ls[u][j]) : 0.0f;
               float aev = ae;                            // the value coefficient: q_e c a_e; dy mixes it with the unmasked r_ec
               if constexpr (DROP) {
                  const bool keep = gat_drop_mix(hw[u], hk[j]) >= a.T;
                  part[U + u][j] *= keep ? a.c : 0.0f;    // t_e = q_e c <g_i, y_j>_h
                  aev = keep ? ae * a.c : 0.0f;
               }
               const float ds = live ? ae * (part[U + u][j] - dd[u][j]) : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) {
                  bool pos;
                  gatv2_leaky(yv[j][v], cm.ok[j][v] ? __int_as_float(xg[u][j][v]) : 0.0f, a.ns, pos);
                  const float dsa = ds * av[j][v];
                  acc[j][v] += fmaf(aev, __int_as_float(gg[u][j][v]), pos ? dsa : a.ns * dsa);
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
         for (int v = 0; v < 4; v++) acc[j][v] += __shfl_xor(acc[j][v], o);
   if (g != 0) return;
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++)
         if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = acc[j][v];      // no incoming entry: 0
}

// datt[c] = the sum of the partial rows, one wave per column: lane l adds the rows l, l + 64, ... in ascending order, then the 64 lane
// sums are added by a fixed butterfly (the form of colsum_fold_kernel, epilogue.hip) -- one order of additions whatever the launch
__global__ __launch_bounds__(256) void gatv2_fold_kernel(int64_t blocks, int64_t k, const float *__restrict__ partial, float *__restrict__ datt) {
   const int lane = threadIdx.x & 63;
   const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
   if (c >= k) return;                                 // wave-uniform
   float t = 0.0f;
   for (int64_t b = lane; b < blocks; b += 64) t += partial[b * k + c];
#pragma unroll
   for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
   if (lane == 0) datt[c] = t;
}

enum { GATV2_FW = 0, GATV2_BW_ROWS = 1, GATV2_BW_ROWS_DATT = 2, GATV2_BW_COLS = 3 };

template <int LPR, int NCH, bool DROP>
static int launch_gatv2(int which, const Gatv2Args &a, const char *entry, hipStream_t st) {
   const int waves = which == GATV2_BW_ROWS || which == GATV2_BW_ROWS_DATT ? GATV2_ROWS_WAVES : GATV2_WAVES;
   const int64_t nb = (a.rows + waves - 1) / waves;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block((unsigned)waves * 64u);
   if (which == GATV2_FW) hipLaunchKernelGGL((gatv2_fw_kernel<LPR, NCH, GATV2_WAVES, DROP>), grid, block, 0, st, a);
   else if (which == GATV2_BW_ROWS) hipLaunchKernelGGL((gatv2_bw_rows_kernel<LPR, NCH, GATV2_ROWS_WAVES, false, DROP>), grid, block, 0, st, a);
   else if (which == GATV2_BW_ROWS_DATT) hipLaunchKernelGGL((gatv2_bw_rows_kernel<LPR, NCH, GATV2_ROWS_WAVES, true, DROP>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((gatv2_bw_cols_kernel<LPR, NCH, GATV2_WAVES, DROP>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the width ladder (attn_by_width); DROP: the kernels with attention dropout
static int gatv2_by_width(int which, const Gatv2Args &a, bool drop, const char *entry, hipStream_t st) {
   return attn_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      return drop ? launch_gatv2<LPR, NCH, true>(which, a, entry, st) : launch_gatv2<LPR, NCH, false>(which, a, entry, st);
   });
}

// what the dropout entries (isplib_gatv2_drop_*_hip) refuse before a launch
static const char *gatv2_drop_refusal(const AttnDrop &dr, int64_t nnz) {
   return attn_drop_refusal(dr, nnz, "scale must be a positive finite number");
}

static const char *const GATV2_DOMAIN = "outside isplib_gatv2_serves(rows_gathered, heads, d, ld) = isplib_gat_serves: 1 <= heads, 1 <= d, "
                                        "heads*d <= 512, heads == 1 or d a power of two >= 4, ld >= heads*d, rows_gathered < 2^31, "
                                        "rows_gathered*ld*4 <= 3.5 GiB";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_gatv2_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gatv2_serves(rows_gathered, heads, d, ld);
}

extern "C" size_t isplib_gatv2_bw_rows_workspace_bytes(int64_t m, int64_t k) {
   if (m <= 0 || k <= 0) return 256;
   const size_t blocks = (size_t)((m + GATV2_ROWS_WAVES - 1) / GATV2_ROWS_WAVES);
   return (blocks * (size_t)k * sizeof(float) + 255) & ~(size_t)255;
}

// The three entries, with and without attention dropout.
static int gatv2_forward(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                         const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att, int64_t heads,
                         float negative_slope, float *z, int64_t ldz, float *lse, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = gatv2_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !x || !att || !z || !lse || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldx < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_DOMAIN);
   Gatv2Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = x; a.ldown = ldx; a.att = att;
   a.out = z; a.ldout = ldz; a.hout = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return gatv2_by_width(GATV2_FW, a, dr.on, entry, (hipStream_t)stream);
}

static int gatv2_backward_rows(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                               const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                               int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz,
                               const float *lse, float *dx, int64_t lddx, float *dsum, float *datt, void *workspace,
                               size_t workspace_bytes, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = gatv2_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !x || !att || !g || !z || !lse || !dx || !dsum || (nnz > 0 && (!indx || !y)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldx < k || ldg < k || ldz < k || lddx < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_DOMAIN);
   if (datt) {
      if (!workspace || workspace_bytes < isplib_gatv2_bw_rows_workspace_bytes(m, k)) return fail(ISPLIB_NOT_ENOUGH_MEM, entry, "workspace too small");
      if (((uintptr_t)workspace & 255) != 0) return fail(ISPLIB_FAIL, entry, "workspace must be 256-byte aligned");
   }
   Gatv2Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = x; a.ldown = ldx; a.att = att; a.g = g; a.ldg = ldg; a.zin = z; a.ldzin = ldz; a.lse_in = lse;
   a.out = dx; a.ldout = lddx; a.hout = dsum; a.part = datt ? (float *)workspace : nullptr;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   int rc = gatv2_by_width(datt ? GATV2_BW_ROWS_DATT : GATV2_BW_ROWS, a, dr.on, entry, (hipStream_t)stream);
   if (rc || !datt) return rc;
   const int64_t blocks = (m + GATV2_ROWS_WAVES - 1) / GATV2_ROWS_WAVES;
   hipLaunchKernelGGL(gatv2_fold_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, (hipStream_t)stream, blocks, k, a.part, datt);
   return check_launch(entry);
}

static int gatv2_backward_cols(const char *entry, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                               const int64_t *cole, const int64_t *csr2csc, const float *x, int64_t ldx, const float *y, int64_t ldy,
                               const float *att, int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *lse,
                               const float *dsum, float *dy, int64_t lddy, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (const char *why = gatv2_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (dr.on && nnz > 0 && !csr2csc) return fail(ISPLIB_FAIL, entry, "null csr2csc: the keep bit is a function of the CSR position");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!colb || !cole || !y || !att || !dy || (nnz > 0 && (!row_t || !x || !g || !lse || !dsum))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_serves(m, heads, k / heads, ldx) || !isplib_gatv2_serves(m, heads, k / heads, ldg))
      return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_DOMAIN);
   Gatv2Args a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = y; a.ldown = ldy; a.att = att;
   a.out = dy; a.ldout = lddy;
   a.y = x; a.ldy = ldx; a.ybytes = nnz > 0 ? attn_extent(m, k, ldx) : 0u;
   a.y2 = g; a.ldy2 = ldg; a.y2bytes = nnz > 0 ? attn_extent(m, k, ldg) : 0u;
   a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn_extent(m, heads, heads) : 0u;
   if (dr.on) a.epos = csr2csc;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return gatv2_by_width(GATV2_BW_COLS, a, dr.on, entry, (hipStream_t)stream);
}

extern "C" int isplib_gatv2_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                    const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                    int64_t heads, float negative_slope, float *z, int64_t ldz, float *lse, void *stream) {
   return gatv2_forward("isplib_gatv2_csr_hip", m, n, k, nnz, indx, pntrb, pntre, x, ldx, y, ldy, att, heads, negative_slope, z, ldz, lse,
                        stream);
}

extern "C" int isplib_gatv2_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                        const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                        int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz,
                                        const float *lse, float *dx, int64_t lddx, float *dsum, float *datt, void *workspace,
                                        size_t workspace_bytes, void *stream) {
   return gatv2_backward_rows("isplib_gatv2_bw_rows_hip", m, n, k, nnz, indx, pntrb, pntre, x, ldx, y, ldy, att, heads, negative_slope, g,
                              ldg, z, ldz, lse, dx, lddx, dsum, datt, workspace, workspace_bytes, stream);
}

extern "C" int isplib_gatv2_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                        const int64_t *cole, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                        int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *lse,
                                        const float *dsum, float *dy, int64_t lddy, void *stream) {
   return gatv2_backward_cols("isplib_gatv2_bw_cols_hip", m, n, k, nnz, row_t, colb, cole, nullptr, x, ldx, y, ldy, att, heads,
                              negative_slope, g, ldg, lse, dsum, dy, lddy, stream);
}

// attention dropout: the argument lists of the entries above (the columns entry with csr2csc after cole), then threshold, scale, seed
extern "C" int isplib_gatv2_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                         const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, const float *att,
                                         int64_t heads, float negative_slope, float *z, int64_t ldz, float *lse, void *stream,
                                         uint32_t threshold, float scale, uint64_t seed) {
   return gatv2_forward("isplib_gatv2_drop_csr_hip", m, n, k, nnz, indx, pntrb, pntre, x, ldx, y, ldy, att, heads, negative_slope, z, ldz,
                        lse, stream, AttnDrop{true, threshold, scale, seed});
}

extern "C" int isplib_gatv2_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                             const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy,
                                             const float *att, int64_t heads, float negative_slope, const float *g, int64_t ldg,
                                             const float *z, int64_t ldz, const float *lse, float *dx, int64_t lddx, float *dsum,
                                             float *datt, void *workspace, size_t workspace_bytes, void *stream, uint32_t threshold,
                                             float scale, uint64_t seed) {
   return gatv2_backward_rows("isplib_gatv2_drop_bw_rows_hip", m, n, k, nnz, indx, pntrb, pntre, x, ldx, y, ldy, att, heads,
                              negative_slope, g, ldg, z, ldz, lse, dx, lddx, dsum, datt, workspace, workspace_bytes, stream,
                              AttnDrop{true, threshold, scale, seed});
}

extern "C" int isplib_gatv2_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                             const int64_t *cole, const int64_t *csr2csc, const float *x, int64_t ldx, const float *y,
                                             int64_t ldy, const float *att, int64_t heads, float negative_slope, const float *g,
                                             int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy, void *stream,
                                             uint32_t threshold, float scale, uint64_t seed) {
   return gatv2_backward_cols("isplib_gatv2_drop_bw_cols_hip", m, n, k, nnz, row_t, colb, cole, csr2csc, x, ldx, y, ldy, att, heads,
                              negative_slope, g, ldg, lse, dsum, dy, lddy, stream, AttnDrop{true, threshold, scale, seed});
}
