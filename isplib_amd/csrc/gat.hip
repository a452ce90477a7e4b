// gat.hip -- GAT attention aggregation over the stored entries of a CSR matrix, all heads in one launch, forward and backward
// (include/isplib_hip.h: isplib_gat_csr_hip, isplib_gat_bw_rows_hip, isplib_gat_bw_cols_hip).  For every row i, stored entry e = (i, j)
// and head h, with y [n, k], k = H*d (head h owns the columns [h*d, (h+1)*d)), a_dst [m, H], a_src [n, H] and a slope ns:
//    u_e  = a_dst[i,h] + a_src[j,h]      s_e = u_e > 0 ? u_e : ns u_e
//    a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)            z_i[head h] = sum_e a_e y_j[head h]
// and for g = dL/dz
//    D[i,h] = <g_i, z_i>_h       t_e = <g_i, y_j>_h        du_e = a_e (t_e - D[i,h]) (u_e > 0 ? 1 : ns)
//    d a_dst[i,h] = sum_e du_e   d a_src[j,h] = sum_{e -> j} du_e          dy_j[head h] = sum_{e -> j} a_e g_i[head h].
// Stored values are not read; every stored entry is its own edge; an empty row has z_i = 0, lse = -inf, D = 0, d a_dst = 0.
//
// Mapping: that of attention.hip -- one wave per row (per column of A in the columns kernel), G = 64 / LPR edge slots, NCH chunks of 4
// consecutive columns per lane, every gathered row fetched once with 16-byte buffer loads.  A lane knows the head of each of its
// chunks: with H > 1, d is a power of two >= 4, so a chunk never straddles heads and a head is an aligned group of d/4 lanes of one
// chunk; with H == 1 the head is the whole row (both chunks where a lane has two).  The score of an edge is one 4-byte gather
// a_src[j, head] (the lanes of a head read one address) and one add: the forward has no dot product and no cross-lane traffic in its
// loop -- the lanes of a head carry the same (m, l) redundantly, per chunk.
//
// The softmax is the online form of attention.hip per chunk: (m, l, acc[4]) with one rescale per step of U edges, m = -FLT_MAX for
// "no edge yet", the G slots merged pairwise at the end.  fmaxf drops a NaN score from the maximum, so the NaN enters l through
// exp(NaN - m): a NaN in a_src[j,h] makes head h of the rows that reference j NaN and nothing else.
//
// The backward stores nothing per edge: a_e is recomputed from lse.  The rows kernel holds g_i and z_i, forms D[i,h] and, per edge, t_e
// by an xor butterfly over the head's lanes, and writes d a_dst and D.  The columns kernel walks the transposed structure with y_j and
// a_src[j,.] in registers, gathers g_i (16 bytes) and a_dst, lse, D of [i, head] (4 bytes each, three tables, each behind its own
// descriptor), and writes dy and d a_src.
//
// Every gathered table sits behind a buffer descriptor of exactly the extent it owns; dead edges and lanes past k carry BUF_OOB, which
// the descriptor answers with 0.  No LDS, no atomics, a fixed order of operations: two launches give equal bits.  DESIGN.md 4.6d.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"

namespace isplib {

constexpr float GAT_NONE = -FLT_MAX;       // the running maximum of a chunk that saw no edge

struct GatArgs {
   int64_t rows, k;                        // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                             // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                             // lanes of one chunk that share a head: d / 4 (H == 1: 64, the whole slot)
   unsigned hmask;                         // c & hmask == 0: the first column of a head (H == 1: only column 0)
   int whole;                              // H == 1: the head spans both chunks of a lane
   const int64_t *indx, *pntrb, *pntre;
   float ns;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const float *own;                       // rows: g | columns: y
   int64_t ldown;
   const float *own_score;                 // forward, rows: a_dst [rows, H] | columns: a_src [rows, H]
   const float *zin;                       // rows: z of the forward
   int64_t ldzin;
   const float *lse_in;                    // rows: lse [rows, H]
   float *out;                             // z | dy
   int64_t ldout;
   float *hout, *hout2;                    // [rows, H]: forward lse | rows: d a_dst, D | columns: d a_src
   // the gathered operands, each behind one descriptor
   const float *y;                         // forward, rows: y | columns: g
   int64_t ldy;
   unsigned ybytes;
   const float *t0, *t1, *t2;              // forward, rows: t0 = a_src | columns: a_dst, lse, D; all [gathered rows, H]
   unsigned tbytes;
};

template <int LPR, int NCH> struct GatCols {
   unsigned cbyte[NCH], poison[NCH];       // this lane's 4 consecutive columns per chunk; past k: an offset the descriptor answers with 0
   unsigned hbyte[NCH];                    // byte offset of the chunk's head inside a row of a [., H] table
   int head[NCH];
   bool ok[NCH][4], first[NCH];            // first: this lane's chunk opens a head (and lies inside k)
   __device__ __forceinline__ GatCols(const GatArgs &a, int lc) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const int c = (j * LPR + lc) * 4;
         cbyte[j] = (unsigned)c * 4u;
         poison[j] = c < (int)a.k ? 0u : BUF_OOB;
         head[j] = c >> a.hshift;
         hbyte[j] = (unsigned)head[j] * 4u;
         first[j] = c < (int)a.k && ((unsigned)c & a.hmask) == 0u;
#pragma unroll
         for (int v = 0; v < 4; v++) ok[j][v] = c + v < (int)a.k;
      }
   }
};

// this lane's columns of row `row` of a dense operand; plain loads, nothing outside the row's k columns is read
template <int LPR, int NCH>
__device__ __forceinline__ void gat_own_row(const float *base, int64_t row, int64_t ld, int lc, const GatCols<LPR, NCH> &cm, float (&r)[NCH][4]) {
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) r[j][v] = cm.ok[j][v] ? base[(size_t)row * (size_t)ld + (size_t)((j * LPR + lc) * 4 + v)] : 0.0f;
}

// entry [row, head of chunk j] of a dense [rows, H] table, per chunk; a chunk past k reads nothing
template <int LPR, int NCH>
__device__ __forceinline__ void gat_own_head(const float *base, int64_t row, int heads, const GatCols<LPR, NCH> &cm, float (&r)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) r[j] = cm.ok[j][0] ? base[(size_t)row * (size_t)heads + (size_t)cm.head[j]] : 0.0f;
}

// byte offsets of the gathered row of edge `src` of the batch in the wide operand and in the [., H] tables; a dead edge: BUF_OOB
__device__ __forceinline__ void gat_edge(int id_l, int src, unsigned ldb, unsigned hb, unsigned &off, unsigned &offh) {
   const int id = __shfl(id_l, src);
   off = id < 0 ? BUF_OOB : (unsigned)id * ldb;
   offh = id < 0 ? BUF_OOB : (unsigned)id * hb;              // BUF_OOB + cbyte / hbyte (< 2^24) cannot wrap
}

template <int LPR, int NCH>
__device__ __forceinline__ void gat_load_wide(const __amdgpu_buffer_rsrc_t rsrc, unsigned off, const GatCols<LPR, NCH> &cm, v4i_t (&t)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) t[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((off + cm.cbyte[j]) | cm.poison[j]), 0, 0);
}

template <int LPR, int NCH>
__device__ __forceinline__ void gat_load_head(const __amdgpu_buffer_rsrc_t rsrc, unsigned offh, const GatCols<LPR, NCH> &cm, float (&t)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++)
      t[j] = __int_as_float((int)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)((offh + cm.hbyte[j]) | cm.poison[j]), 0, 0));
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t gat_rsrc(const float *p, unsigned bytes) {
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, (int)bytes, 0x00020000);
}

// sum over the lanes that share a head (an aligned group of `hlanes` lanes, a power of two <= LPR); every lane of the group ends
// with the same bits (each level adds the same two numbers on both sides)
template <int LPR, int O = 1> __device__ __forceinline__ float gat_head_sum(float v, int hlanes) {
   if constexpr (O < LPR) {
      const float w = lane_xor<O>(v);      // partners 1, 2, 4, 8 by DPP moves inside the 16-lane row (gather.h), wider ones by ds_bpermute
      return gat_head_sum<LPR, 2 * O>(O < hlanes ? v + w : v, hlanes);
   } else {
      return v;
   }
}

// <r, t>_h per chunk over this lane's columns, then over the head's lanes (and both chunks where the head is the whole row)
template <int LPR, int NCH>
__device__ __forceinline__ void gat_head_dot(const float (&r)[NCH][4], const v4i_t (&t)[NCH], const GatCols<LPR, NCH> &cm, const GatArgs &a,
                                             float (&d)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      d[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) d[j] = fmaf(r[j][v], cm.ok[j][v] ? __int_as_float(t[j][v]) : 0.0f, d[j]);
   }
   if (NCH == 2 && a.whole) {
      d[0] = gat_head_sum<LPR>(d[0] + d[NCH - 1], a.hlanes);
      d[NCH - 1] = d[0];
   } else {
#pragma unroll
      for (int j = 0; j < NCH; j++) d[j] = gat_head_sum<LPR>(d[j], a.hlanes);
   }
}

__device__ __forceinline__ float gat_score(float adst, float asrc, float ns, float &slope) {
   const float u = adst + asrc;            // ONE fp32 add: its sign is the sign of the exact sum
   slope = u > 0.0f ? 1.0f : ns;
   return u > 0.0f ? u : ns * u;
}

template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat_fw_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = gat_rsrc(a.y, a.ybytes), rss = gat_rsrc(a.t0, a.tbytes);
   const GatCols<LPR, NCH> cm(a, lc);
   float adst[NCH];
   gat_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, adst);

   float mrun[NCH], l[NCH], acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      mrun[j] = GAT_NONE;
      l[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;
   }

   const unsigned ldyb = (unsigned)a.ldy * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         float sc[U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            gat_load_wide<LPR, NCH>(rsy, off, cm, yv[u]);
            gat_load_head<LPR, NCH>(rss, offh, cm, sc[u]);
         }
#pragma unroll
         for (int j = 0; j < NCH; j++) {
            float mnew = mrun[j];
#pragma unroll
            for (int u = 0; u < U; u++) {
               float slope;
               sc[u][j] = gat_score(adst[j], sc[u][j], a.ns, slope);
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
               l[j] += w;
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(w, __int_as_float(yv[u][j][v]), acc[j][v]);
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
         if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = empty ? 0.0f : acc[j][v] / l[j];
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? -INFINITY : mrun[j] + logf(l[j]);
   }
}

template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat_bw_rows_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = gat_rsrc(a.y, a.ybytes), rss = gat_rsrc(a.t0, a.tbytes);
   const GatCols<LPR, NCH> cm(a, lc);
   float gv[NCH][4], adst[NCH], lse[NCH], dsum[NCH];
   gat_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm, gv);
   gat_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, adst);
   gat_own_head<LPR, NCH>(a.lse_in, row, a.heads, cm, lse);
   {                                                   // D[i,h] = <g_i, z_i>_h: every slot holds the row, so every lane of a head ends with it
      float zv[NCH][4];
      gat_own_row<LPR, NCH>(a.zin, row, a.ldzin, lc, cm, zv);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         dsum[j] = 0.0f;
#pragma unroll
         for (int v = 0; v < 4; v++) dsum[j] = fmaf(gv[j][v], zv[j][v], dsum[j]);
      }
      if (NCH == 2 && a.whole) {
         dsum[0] = gat_head_sum<LPR>(dsum[0] + dsum[NCH - 1], a.hlanes);
         dsum[NCH - 1] = dsum[0];
      } else {
#pragma unroll
         for (int j = 0; j < NCH; j++) dsum[j] = gat_head_sum<LPR>(dsum[j], a.hlanes);
      }
   }

   float acc[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) acc[j] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         float sc[U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            gat_load_wide<LPR, NCH>(rsy, off, cm, yv[u]);
            gat_load_head<LPR, NCH>(rss, offh, cm, sc[u]);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float t[NCH];
            gat_head_dot<LPR, NCH>(gv, yv[u], cm, a, t);
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               float slope;
               const float s = gat_score(adst[j], sc[u][j], a.ns, slope);
               acc[j] += live ? __expf(s - lse[j]) * (t[j] - dsum[j]) * slope : 0.0f;
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int j = 0; j < NCH; j++) acc[j] += __shfl_xor(acc[j], o);
   if (g != 0) return;
   const bool empty = ee <= eb;
#pragma unroll
   for (int j = 0; j < NCH; j++)
      if (cm.first[j]) {
         a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? 0.0f : acc[j];
         a.hout2[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = empty ? 0.0f : dsum[j];
      }
}

// one wave per column j of A (a row of the transposed structure): y_j and a_src[j,.] in registers; g_i, a_dst, lse, D of row i gathered
template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat_bw_cols_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = NCH >= 2 ? 2 : 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsg = gat_rsrc(a.y, a.ybytes);
   const __amdgpu_buffer_rsrc_t rs0 = gat_rsrc(a.t0, a.tbytes), rs1 = gat_rsrc(a.t1, a.tbytes), rs2 = gat_rsrc(a.t2, a.tbytes);
   const GatCols<LPR, NCH> cm(a, lc);
   float yv[NCH][4], asrc[NCH];
   gat_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm, yv);
   gat_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, asrc);

   float acc[NCH][4], accs[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      accs[j] = 0.0f;
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;
   }

   const unsigned ldgb = (unsigned)a.ldy * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t gg[U][NCH];
         float ad[U][NCH], ls[U][NCH], ds[U][NCH];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldgb, hb, off, offh);
            gat_load_wide<LPR, NCH>(rsg, off, cm, gg[u]);
            gat_load_head<LPR, NCH>(rs0, offh, cm, ad[u]);
            gat_load_head<LPR, NCH>(rs1, offh, cm, ls[u]);
            gat_load_head<LPR, NCH>(rs2, offh, cm, ds[u]);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float t[NCH];
            gat_head_dot<LPR, NCH>(yv, gg[u], cm, a, t);
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               float slope;
               const float s = gat_score(ad[u][j], asrc[j], a.ns, slope);
               const float ae = live ? __expf(s - ls[u][j]) : 0.0f;
               accs[j] += live ? ae * (t[j] - ds[u][j]) * slope : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(ae, __int_as_float(gg[u][j][v]), acc[j][v]);
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         accs[j] += __shfl_xor(accs[j], o);
#pragma unroll
         for (int v = 0; v < 4; v++) acc[j][v] += __shfl_xor(acc[j][v], o);
      }
   if (g != 0) return;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
#pragma unroll
      for (int v = 0; v < 4; v++)
         if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = acc[j][v];      // no incoming entry: 0
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = accs[j];
   }
}

enum { GAT_FW = 0, GAT_BW_ROWS = 1, GAT_BW_COLS = 2 };

template <int LPR, int NCH>
static int launch_gat(int which, const GatArgs &a, const char *entry, hipStream_t st) {
   constexpr int WAVES = 4;
   const int64_t nb = (a.rows + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block(WAVES * 64);
   if (which == GAT_FW) hipLaunchKernelGGL((gat_fw_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   else if (which == GAT_BW_ROWS) hipLaunchKernelGGL((gat_bw_rows_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((gat_bw_cols_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the width dispatch of attention.hip, up to two chunks per lane
static int gat_by_width(int which, const GatArgs &a, const char *entry, hipStream_t st) {
   const int64_t w = (a.k + 3) / 4;
   if (w <= 8) return launch_gat<8, 1>(which, a, entry, st);
   if (w <= 16) return launch_gat<16, 1>(which, a, entry, st);
   if (w <= 32) return launch_gat<32, 1>(which, a, entry, st);
   if (w <= 64) return launch_gat<64, 1>(which, a, entry, st);
   return launch_gat<64, 2>(which, a, entry, st);
}

// what a descriptor over `rows` rows of k floats at pitch ld may answer: the extent a row-strided view owns, not rows * ld
static unsigned gat_extent(int64_t rows, int64_t k, int64_t ld) {
   return rows <= 0 ? 0u : (unsigned)(((unsigned long long)(rows - 1) * (unsigned long long)ld + (unsigned long long)k) * 4ull);
}

// the head geometry of a launch; the domain (isplib_gat_serves) has been checked: H == 1, or d a power of two >= 4
static void gat_heads(GatArgs &a, int64_t heads, int64_t d) {
   a.heads = (int)heads;
   if (heads == 1) {
      a.hshift = 31; a.hlanes = 64; a.hmask = 0x7fffffffu; a.whole = 1;
   } else {
      int sh = 0;
      while ((1LL << sh) < d) sh++;
      a.hshift = sh; a.hlanes = (int)(d / 4); a.hmask = (unsigned)(d - 1); a.whole = 0;
   }
}

static const char *const GAT_DOMAIN = "outside isplib_gat_serves(rows_gathered, heads, d, ld): 1 <= heads, 1 <= d, heads*d <= 512, heads == 1 or "
                                      "d a power of two >= 4, ld >= heads*d, rows_gathered < 2^31, rows_gathered*ld*4 <= 3.5 GiB";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_gat_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) { return isplib_gat_serves(rows_gathered, heads, d, ld); }

extern "C" int isplib_gat_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                  const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads, float negative_slope,
                                  float *z, int64_t ldz, float *lse, void *stream) {
   const char *entry = "isplib_gat_csr_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !a_dst || !z || !lse || (nnz > 0 && (!indx || !y || !a_src))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   GatArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   gat_heads(a, heads, k / heads);
   a.own_score = a_dst;
   a.out = z; a.ldout = ldz; a.hout = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? gat_extent(n, k, ldy) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? gat_extent(n, heads, heads) : 0u;
   return gat_by_width(GAT_FW, a, entry, (hipStream_t)stream);
}

extern "C" int isplib_gat_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                      const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads,
                                      float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz, const float *lse,
                                      float *d_a_dst, float *dsum, void *stream) {
   const char *entry = "isplib_gat_bw_rows_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !a_dst || !g || !z || !lse || !d_a_dst || !dsum || (nnz > 0 && (!indx || !y || !a_src)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldg < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   GatArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   gat_heads(a, heads, k / heads);
   a.own = g; a.ldown = ldg; a.own_score = a_dst; a.zin = z; a.ldzin = ldz; a.lse_in = lse;
   a.hout = d_a_dst; a.hout2 = dsum;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? gat_extent(n, k, ldy) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? gat_extent(n, heads, heads) : 0u;
   return gat_by_width(GAT_BW_ROWS, a, entry, (hipStream_t)stream);
}

extern "C" int isplib_gat_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                      const int64_t *cole, const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads,
                                      float negative_slope, const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy,
                                      int64_t lddy, float *d_a_src, void *stream) {
   const char *entry = "isplib_gat_bw_cols_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!colb || !cole || !y || !a_src || !dy || !d_a_src || (nnz > 0 && (!row_t || !a_dst || !g || !lse || !dsum)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(m, heads, k / heads, ldg)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   GatArgs a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.ns = negative_slope;
   gat_heads(a, heads, k / heads);
   a.own = y; a.ldown = ldy; a.own_score = a_src;
   a.out = dy; a.ldout = lddy; a.hout = d_a_src;
   a.y = g; a.ldy = ldg; a.ybytes = nnz > 0 ? gat_extent(m, k, ldg) : 0u;
   a.t0 = a_dst; a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? gat_extent(m, heads, heads) : 0u;
   return gat_by_width(GAT_BW_COLS, a, entry, (hipStream_t)stream);
}
