// gatv2_16.hip -- the GATv2 attention aggregation of gatv2.hip for dense operands of 16-bit elements (bf16, fp16), all heads in one
// launch, forward and backward (include/isplib_hip_gatv2_16.h: isplib_gatv2_16_csr_hip, isplib_gatv2_16_bw_rows_hip,
// isplib_gatv2_16_bw_cols_hip).  The mathematics is gatv2.hip's, stated in its header: for every row i, stored entry e = (i, j) and head
// h, with x [m, k], y [n, k], k = H*d, att [H, d] (k contiguous floats), a slope ns and g = dL/dz, c running over the head's columns:
//    u_ec = x_ic + y_jc          sl_ec = u_ec > 0 ? 1 : ns        v_ec = sl_ec u_ec          s_e = sum_c att_c v_ec
//    a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)                              z_i[head h] = sum_e a_e y_j[head h]
//    D[i,h] = sum_e a_e t_e      t_e = <g_i, y_j>_h               ds_e = a_e (t_e - D[i,h])  q_ec = ds_e att_c sl_ec
//    dx_ic  = sum_e q_ec         dy_jc = sum_{e -> j} (a_e g_ic + q_ec)                      datt_c = sum_{all e} ds_e v_ec.
// No wide operand is widened in memory: a gathered row of x, y or g is half the bytes of the fp32 kernels', and the operator is bound by
// gathered bytes.
//
// The 16-bit family's contract: x, y, g, z, dx and dy are 16-bit and widening is exact (half16.h: widen2); every sum,
// product, exponential and division is fp32; z, dx and dy are rounded ONCE, to nearest even (narrow2).  att, lse, D, datt and the datt
// workspace stay fp32.  u_ec = widen(x_ic) + widen(y_jc) is ONE unfused fp32 add and the branch is taken on it, so its sign is the sign
// of the exact sum; u == 0 takes ns.
//
// Mapping: gat16.hip's -- one wave per row (per column of A in the columns kernel), always ONE 16-byte buffer load of EIGHT columns per
// lane and edge, LPR = 4 / 8 / 16 / 32 / 64 for ceil(k / 8) up to 4 / 8 / 16 / 32 / 64 and G = 64 / LPR edge slots.  With H > 1, d is a
// power of two >= 8: a lane's eight columns never straddle heads and a head is an aligned group of d / 8 lanes (at d = 8 one lane: the
// per-head sum has no cross-lane step).  With H == 1 the head is the whole slot and k may be any even width >= 8; the ragged last vector
// (k % 8 != 0) over-reads, and each over-read dword is dropped by a per-dword select before it is widened, never by a multiply.  There is
// one chunk per lane always, so the `whole` / two-chunk handling of gatv2.hip has no counterpart here.  The dot products of a step (U
// scores in the forward, U scores and U <g_i, y_j>_h in the backward kernels) go through the levels of ONE butterfly together, as in
// gatv2.hip.  Every gathered table sits behind a buffer descriptor of exactly the extent it owns (2 bytes per element for the wide
// tables, 4 for lse / D); dead edges and lanes past k carry BUF_OOB, which the descriptor answers with 0.  No atomics, a fixed order of
// operations: two launches give equal bits.
//
// The forward is gat16.hip's online softmax per lane: (m, l, acc[8]), one rescale per step of U edges, -FLT_MAX for "no edge yet", the
// slots merged pairwise; the gathered y_j serves both score and value, x_i and the lane's eight columns of att sit in registers.  A row
// of one entry has weight exp(0) = 1 and l = 1: z_i is y_j's 16 bits.  fmaxf drops a NaN score from the maximum, so it enters l through
// exp(NaN - m): a NaN in y[j,c] makes the head of c NaN in the rows that reference j and nothing else.
//
// The backward over the rows does NOT read z: in 16 bits z is rounded, and D = <g_i, z16_i>_h would carry u * sum_c |g_ic z_ic| into
// every ds_e.  One pass over the row's edges accumulates, per head and slot, l = sum a_e and Dacc = sum a_e t_e,
// per column P_c = sum a_e sl_ec t_e and Q_c = sum a_e sl_ec and, in the datt instantiation only, R_c = sum a_e t_e v_ec and
// S_c = sum a_e v_ec; the slots merge by plain sums; D = Dacc / l, dx_ic = att_c (P_c - D Q_c), and the row's part of datt_c is
// R_c - D S_c.  That part goes through the LDS fold of gatv2.hip (one __syncthreads; every wave of the block reaches it, rows past m
// contribute zeros), one partial row per block into the caller's workspace, which gatv2_16_fold_kernel adds up in a fixed order.
// datt == NULL selects an instantiation without LDS, without the barrier and with the early return; it gives the same dx and D bits.
// The columns kernel walks the transposed structure with y_j (widened) and att in registers, gathers x_i and g_i (16 bytes each) and
// lse, D of [i, head] (4 bytes each, two tables, each behind its own descriptor), and writes dy, rounded once.  DESIGN.md 4.6g.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "half16.h"
#include "attn16_common.h"

namespace isplib {

constexpr float GATV2_16_NONE = -FLT_MAX;    // the running maximum of a lane that saw no edge
constexpr int GATV2_16_WAVES = 4;            // rows per block: forward and columns kernel
constexpr int GATV2_16_ROWS_WAVES = 8;       // rows per block of the rows kernel: one partial row of datt per 8 rows
constexpr int GATV2_16_FW_U = 2;             // gathers per slot and step: forward (measured against 4: DESIGN.md 4.6g)
constexpr int GATV2_16_BW_U = 4;             // ... and both backward kernels

struct Gatv2h16Args {
   int64_t rows, k;                          // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                               // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                               // lanes that share a head: d / 8 (H == 1: 64, the whole slot)
   unsigned hmask;                           // c & hmask == 0: the first column of a head (H == 1: only column 0)
   const int64_t *indx, *pntrb, *pntre;
   float ns;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const unsigned short *own;                // forward, rows: x | columns: y
   int64_t ldown;
   const unsigned short *g;                  // rows: dL/dz
   int64_t ldg;
   const float *lse_in;                      // rows: lse [rows, H]
   const float *att;                         // [k]
   unsigned short *out;                      // z | dx | dy
   int64_t ldout;
   float *hout;                              // [rows, H]: forward lse | rows: D
   float *part;                              // rows, with datt: [blocks, k] partial rows of datt
   // the gathered operands, each behind one descriptor
   const void *y;                            // forward, rows: y | columns: x
   int64_t ldy;
   unsigned ybytes;
   const void *y2;                           // columns: g
   int64_t ldy2;
   unsigned y2bytes;
   const float *t1, *t2;                     // columns: lse, D; both [gathered rows, H]
   unsigned tbytes;
};

// this lane's eight columns of att (k contiguous floats); a column past k: 0
__device__ __forceinline__ void gatv2_16_own_att(const float *att, const Attn16HeadCols &cm, float (&r)[8]) {
#pragma unroll
   for (int v = 0; v < 8; v++) r[v] = cm.ok[v >> 1] ? att[cm.col + v] : 0.0f;
}

// v_ec = leaky_relu(u_ec), u_ec = r + t: ONE fp32 add, so its sign is the sign of the exact sum; u == 0 takes ns
__device__ __forceinline__ float gatv2_16_leaky(float r, float t, float ns, bool &pos) {
   const float u = r + t;
   pos = u > 0.0f;
   return pos ? u : ns * u;
}

// this lane's part of sum_c att_c v_ec; a column past k has r = t = att = 0
__device__ __forceinline__ float gatv2_16_score_part(const float (&r)[8], const float (&t)[8], const float (&att)[8], float ns) {
   float p = 0.0f;
#pragma unroll
   for (int v = 0; v < 8; v++) {
      bool pos;
      p = fmaf(att[v], gatv2_16_leaky(r[v], t[v], ns, pos), p);
   }
   return p;
}

template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gatv2_16_fw_kernel(const Gatv2h16Args a) {
   constexpr int G = 64 / LPR, U = GATV2_16_FW_U;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn16_desc(a.y, a.ybytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float xv[8], av[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, xv);
   gatv2_16_own_att(a.att, cm, av);

   float mrun = GATV2_16_NONE, l = 0.0f, acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U];
#pragma unroll
         for (int u = 0; u < U; u++) yv[u] = attn16_load_wide(rsy, attn16_off(__shfl(id_l, (s0 + u * G + g) & 63), ldyb), cm);
         float y8[U][8], sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            attn16_widen<ELT>(yv[u], cm.ok, y8[u]);
            sc[u] = gatv2_16_score_part(xv, y8[u], av, a.ns);
         }
         attn16_head_sum<LPR, U>(sc, a.hlanes);
         float mnew = mrun;
#pragma unroll
         for (int u = 0; u < U; u++)
            mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u]) : mnew;      // a NaN score is not a maximum; it enters through exp below
         const float r = __expf(mrun - mnew);
         mrun = mnew;
         l *= r;
#pragma unroll
         for (int v = 0; v < 8; v++) acc[v] *= r;
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float w = (s0 + u * G + g < cnt) ? __expf(sc[u] - mnew) : 0.0f;
            l += w;
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] = fmaf(w, y8[u][v], acc[v]);
         }
      }
   }
   // merge the G slots pairwise, by the rule of a step
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      const float mo = __shfl_xor(mrun, o), lo = __shfl_xor(l, o);
      const float mnew = fmaxf(mrun, mo);
      const float ra = __expf(mrun - mnew), rb = __expf(mo - mnew);
      l = l * ra + lo * rb;
#pragma unroll
      for (int v = 0; v < 8; v++) acc[v] = acc[v] * ra + __shfl_xor(acc[v], o) * rb;
      mrun = mnew;
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
   float zr[8];
#pragma unroll
   for (int v = 0; v < 8; v++) zr[v] = empty ? 0.0f : acc[v] / l;
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, zr);
   if (cm.first) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = empty ? -INFINITY : mrun + logf(l);
}

// the one-pass backward over the rows: no z, D[i,h] from the row's own edges.  DATT: every lane also sums a_e t_e v_ec and a_e v_ec; the
// block folds its waves' R - D S through LDS and writes one partial row.  That instantiation has a barrier, so no wave leaves before
// it: a wave whose row is past a.rows walks an empty row and contributes zeros.
template <int ELT, int LPR, int WAVES, bool DATT>
__global__ __launch_bounds__(WAVES * 64) void gatv2_16_bw_rows_kernel(const Gatv2h16Args a) {
   constexpr int G = 64 / LPR, U = GATV2_16_BW_U, WCOLS = LPR * 8;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   const bool valid = row < a.rows;                    // wave-uniform
   if constexpr (!DATT) {
      if (!valid) return;
   }
   const int64_t eb = valid ? a.pntrb[row] : 0, ee = valid ? a.pntre[row] : 0;
   const __amdgpu_buffer_rsrc_t rsy = attn16_desc(a.y, a.ybytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float xv[8], gv[8], av[8], lse = 0.0f;
#pragma unroll
   for (int v = 0; v < 8; v++) xv[v] = gv[v] = 0.0f;
   gatv2_16_own_att(a.att, cm, av);
   if (valid) {
      attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, xv);
      attn16_own_row<ELT>(a.g, row, a.ldg, cm.col, cm.ok, gv);
      lse = attn16_own_head(a.lse_in, row, a.heads, cm);
   }

   float l = 0.0f, dacc = 0.0f;                        // per head: sum a_e, sum a_e t_e
   float pc[8], qc[8], rc[8], sc8[8];                  // per column: sum a_e sl_ec t_e, sum a_e sl_ec | datt: sum a_e t_e v_ec, sum a_e v_ec
#pragma unroll
   for (int v = 0; v < 8; v++) pc[v] = qc[v] = rc[v] = sc8[v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U];
#pragma unroll
         for (int u = 0; u < U; u++) yv[u] = attn16_load_wide(rsy, attn16_off(__shfl(id_l, (s0 + u * G + g) & 63), ldyb), cm);
         float part[2 * U];                            // s_e and t_e of the step through one butterfly
#pragma unroll
         for (int u = 0; u < U; u++) {
            float y8[8];
            attn16_widen<ELT>(yv[u], cm.ok, y8);
            part[u] = gatv2_16_score_part(xv, y8, av, a.ns);
            part[U + u] = attn16_dot_part(gv, y8);
         }
         attn16_head_sum<LPR, 2 * U>(part, a.hlanes);      // every lane takes part: not under `live`
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
            const float t = part[U + u];
            const float ae = live ? __expf(part[u] - lse) : 0.0f;
            const float aet = live ? ae * t : 0.0f;
            l += ae;
            dacc += aet;
            float y8[8];
            attn16_widen<ELT>(yv[u], cm.ok, y8);
#pragma unroll
            for (int v = 0; v < 8; v++) {
               bool pos;
               const float lv = gatv2_16_leaky(xv[v], y8[v], a.ns, pos);
               pc[v] += pos ? aet : a.ns * aet;
               qc[v] += pos ? ae : a.ns * ae;
               if constexpr (DATT) {
                  rc[v] = fmaf(aet, lv, rc[v]);
                  sc8[v] = fmaf(ae, lv, sc8[v]);
               }
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      l += __shfl_xor(l, o);
      dacc += __shfl_xor(dacc, o);
#pragma unroll
      for (int v = 0; v < 8; v++) {
         pc[v] += __shfl_xor(pc[v], o);
         qc[v] += __shfl_xor(qc[v], o);
         if constexpr (DATT) {
            rc[v] += __shfl_xor(rc[v], o);
            sc8[v] += __shfl_xor(sc8[v], o);
         }
      }
   }
   const bool empty = ee <= eb;
   const float dsum = (empty || cm.poison != 0u) ? 0.0f : dacc / l;      // a lane past k saw no weight: l = 0
   if (valid && g == 0) {
      float dx[8];
#pragma unroll
      for (int v = 0; v < 8; v++) dx[v] = empty ? 0.0f : av[v] * (pc[v] - dsum * qc[v]);
      attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, dx);
      if (cm.first) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = dsum;
   }
   if constexpr (DATT) {
      __shared__ float s_pa[WAVES][WCOLS];             // at most 2 KiB per wave
      if (g == 0) {
#pragma unroll
         for (int v = 0; v < 8; v++) s_pa[wave][lc * 8 + v] = empty ? 0.0f : rc[v] - dsum * sc8[v];      // a lane past k: 0
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
template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gatv2_16_bw_cols_kernel(const Gatv2h16Args a) {
   constexpr int G = 64 / LPR, U = GATV2_16_BW_U;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsx = attn16_desc(a.y, a.ybytes), rsg = attn16_desc(a.y2, a.y2bytes);
   const __amdgpu_buffer_rsrc_t rs1 = attn16_desc(a.t1, a.tbytes), rs2 = attn16_desc(a.t2, a.tbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float yv[8], av[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, yv);
   gatv2_16_own_att(a.att, cm, av);

   float acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldxb = (unsigned)a.ldy * 2u, ldgb = (unsigned)a.ldy2 * 2u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t xg[U], gg[U];
         float ls[U], dd[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            xg[u] = attn16_load_wide(rsx, attn16_off(id, ldxb), cm);
            gg[u] = attn16_load_wide(rsg, attn16_off(id, ldgb), cm);
            ls[u] = attn16_load_head(rs1, attn16_off(id, hb), cm);
            dd[u] = attn16_load_head(rs2, attn16_off(id, hb), cm);
         }
         float part[2 * U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float x8[8], g8[8];
            attn16_widen<ELT>(xg[u], cm.ok, x8);
            attn16_widen<ELT>(gg[u], cm.ok, g8);
            part[u] = gatv2_16_score_part(yv, x8, av, a.ns);      // x_ic + y_jc: the add commutes bit for bit
            part[U + u] = attn16_dot_part(yv, g8);
         }
         attn16_head_sum<LPR, 2 * U>(part, a.hlanes);      // every lane takes part: not under `live`
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
            const float ae = live ? __expf(part[u] - ls[u]) : 0.0f;
            const float ds = live ? ae * (part[U + u] - dd[u]) : 0.0f;
            float x8[8], g8[8];
            attn16_widen<ELT>(xg[u], cm.ok, x8);
            attn16_widen<ELT>(gg[u], cm.ok, g8);
#pragma unroll
            for (int v = 0; v < 8; v++) {
               bool pos;
               gatv2_16_leaky(yv[v], x8[v], a.ns, pos);
               const float dsa = ds * av[v];
               acc[v] += fmaf(ae, g8[v], pos ? dsa : a.ns * dsa);
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int v = 0; v < 8; v++) acc[v] += __shfl_xor(acc[v], o);
   if (g != 0) return;
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, acc);      // no incoming entry: 0
}

// datt[c] = the sum of the partial rows, one wave per column: lane l adds the rows l, l + 64, ... in ascending order, then the 64 lane
// sums are added by a fixed butterfly (the form of gatv2_fold_kernel, gatv2.hip) -- one order of additions whatever the launch
__global__ __launch_bounds__(256) void gatv2_16_fold_kernel(int64_t blocks, int64_t k, const float *__restrict__ partial, float *__restrict__ datt) {
   const int lane = threadIdx.x & 63;
   const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
   if (c >= k) return;                                 // wave-uniform
   float t = 0.0f;
   for (int64_t b = lane; b < blocks; b += 64) t += partial[b * k + c];
#pragma unroll
   for (int o = 32; o >= 1; o >>= 1) t += __shfl_xor(t, o);
   if (lane == 0) datt[c] = t;
}

enum { GATV2_16_FW = 0, GATV2_16_BW_ROWS = 1, GATV2_16_BW_ROWS_DATT = 2, GATV2_16_BW_COLS = 3 };

template <int ELT, int LPR>
static int launch_gatv2_16(int which, const Gatv2h16Args &a, const char *entry, hipStream_t st) {
   const int waves = which == GATV2_16_BW_ROWS || which == GATV2_16_BW_ROWS_DATT ? GATV2_16_ROWS_WAVES : GATV2_16_WAVES;
   const int64_t nb = (a.rows + waves - 1) / waves;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block((unsigned)waves * 64u);
   if (which == GATV2_16_FW) hipLaunchKernelGGL((gatv2_16_fw_kernel<ELT, LPR, GATV2_16_WAVES>), grid, block, 0, st, a);
   else if (which == GATV2_16_BW_ROWS) hipLaunchKernelGGL((gatv2_16_bw_rows_kernel<ELT, LPR, GATV2_16_ROWS_WAVES, false>), grid, block, 0, st, a);
   else if (which == GATV2_16_BW_ROWS_DATT) hipLaunchKernelGGL((gatv2_16_bw_rows_kernel<ELT, LPR, GATV2_16_ROWS_WAVES, true>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((gatv2_16_bw_cols_kernel<ELT, LPR, GATV2_16_WAVES>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the element type and the slot width (attn16_run)
static int gatv2_16_run(int dtype, int which, const Gatv2h16Args &a, const char *entry, void *stream) {
   return attn16_run(dtype, a.k, [&](auto elt, auto lpr) {
      return launch_gatv2_16<decltype(elt)::value, decltype(lpr)::value>(which, a, entry, (hipStream_t)stream);
   });
}

static const char *const GATV2_16_DOMAIN = "outside isplib_gatv2_16_serves(rows_gathered, heads, d, ld) = isplib_gat16_serves: 1 <= heads, "
                                           "8 <= heads*d <= 512, heads == 1 with d even or d a power of two >= 8, every pitch even, "
                                           "ld >= heads*d, rows_gathered < 2^31, rows_gathered*ld*2 <= 3.5 GiB (convert the operands and "
                                           "use the fp32 entries)";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_gatv2_16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gatv2_16_serves(rows_gathered, heads, d, ld);
}

extern "C" int isplib_gatv2_16_auto(int64_t rows_gathered, int64_t ld) { return isplib_gatv2_16_native_pays(rows_gathered, ld); }

extern "C" size_t isplib_gatv2_16_bw_rows_workspace_bytes(int64_t m, int64_t k) {
   if (m <= 0 || k <= 0) return 256;
   const size_t blocks = (size_t)((m + GATV2_16_ROWS_WAVES - 1) / GATV2_16_ROWS_WAVES);
   return (blocks * (size_t)k * sizeof(float) + 255) & ~(size_t)255;
}

// the refusals of the three entries come in one order: dtype, negative dimension, nothing to do, a pitch below k, k % heads, the
// domain, a null operand, the workspace, alignment -- all before any launch
extern "C" int isplib_gatv2_16_csr_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                       const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy, const float *att,
                                       int64_t heads, float negative_slope, void *z, int64_t ldz, float *lse, void *stream) {
   const char *entry = "isplib_gatv2_16_csr_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldx < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_16_serves(n, heads, k / heads, ldy) || !attn16_even(ldx, ldz))
      return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_16_DOMAIN);
   if (!pntrb || !pntre || !x || !att || !z || !lse || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(x, y, z)) return fail(ISPLIB_FAIL, entry, "x, y and z must be 4-byte aligned");
   Gatv2h16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(x); a.ldown = ldx; a.att = att;
   a.out = reinterpret_cast<unsigned short *>(z); a.ldout = ldz; a.hout = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   return gatv2_16_run(dtype, GATV2_16_FW, a, entry, stream);
}

extern "C" int isplib_gatv2_16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                                           const int64_t *pntrb, const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy,
                                           const float *att, int64_t heads, float negative_slope, const void *g, int64_t ldg,
                                           const float *lse, void *dx, int64_t lddx, float *dsum, float *datt, void *workspace,
                                           size_t workspace_bytes, void *stream) {
   const char *entry = "isplib_gatv2_16_bw_rows_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldx < k || ldg < k || lddx < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_16_serves(n, heads, k / heads, ldy) || !attn16_even(ldx, ldg, lddx))
      return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_16_DOMAIN);
   if (!pntrb || !pntre || !x || !att || !g || !lse || !dx || !dsum || (nnz > 0 && (!indx || !y)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (datt) {
      if (!workspace || workspace_bytes < isplib_gatv2_16_bw_rows_workspace_bytes(m, k))
         return fail(ISPLIB_NOT_ENOUGH_MEM, entry, "workspace too small");
      if (((uintptr_t)workspace & 255) != 0) return fail(ISPLIB_FAIL, entry, "workspace must be 256-byte aligned");
   }
   if (!attn16_aligned(x, y, g, dx)) return fail(ISPLIB_FAIL, entry, "x, y, g and dx must be 4-byte aligned");
   Gatv2h16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(x); a.ldown = ldx; a.att = att;
   a.g = reinterpret_cast<const unsigned short *>(g); a.ldg = ldg; a.lse_in = lse;
   a.out = reinterpret_cast<unsigned short *>(dx); a.ldout = lddx; a.hout = dsum; a.part = datt ? (float *)workspace : nullptr;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   int rc = gatv2_16_run(dtype, datt ? GATV2_16_BW_ROWS_DATT : GATV2_16_BW_ROWS, a, entry, stream);
   if (rc || !datt) return rc;
   const int64_t blocks = (m + GATV2_16_ROWS_WAVES - 1) / GATV2_16_ROWS_WAVES;
   hipLaunchKernelGGL(gatv2_16_fold_kernel, dim3((unsigned)((k + 3) / 4)), dim3(256), 0, (hipStream_t)stream, blocks, k, a.part, datt);
   return check_launch(entry);
}

extern "C" int isplib_gatv2_16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t,
                                           const int64_t *colb, const int64_t *cole, const void *x, int64_t ldx, const void *y, int64_t ldy,
                                           const float *att, int64_t heads, float negative_slope, const void *g, int64_t ldg,
                                           const float *lse, const float *dsum, void *dy, int64_t lddy, void *stream) {
   const char *entry = "isplib_gatv2_16_bw_cols_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gatv2_16_serves(m, heads, k / heads, ldx) || !isplib_gatv2_16_serves(m, heads, k / heads, ldg) ||
       !attn16_even(ldy, lddy))
      return fail(ISPLIB_NO_OPT_IMPL, entry, GATV2_16_DOMAIN);
   if (!colb || !cole || !y || !att || !dy || (nnz > 0 && (!row_t || !x || !g || !lse || !dsum))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(x, y, g, dy)) return fail(ISPLIB_FAIL, entry, "x, y, g and dy must be 4-byte aligned");
   Gatv2h16Args a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(y); a.ldown = ldy; a.att = att;
   a.out = reinterpret_cast<unsigned short *>(dy); a.ldout = lddy;
   a.y = x; a.ldy = ldx; a.ybytes = nnz > 0 ? attn16_extent(m, k, ldx, 2u) : 0u;
   a.y2 = g; a.ldy2 = ldg; a.y2bytes = nnz > 0 ? attn16_extent(m, k, ldg, 2u) : 0u;
   a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn16_extent(m, heads, heads, 4u) : 0u;
   return gatv2_16_run(dtype, GATV2_16_BW_COLS, a, entry, stream);
}
