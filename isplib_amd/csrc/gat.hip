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
//
// The per-edge score term (isplib_gat_edge_*_hip): the three kernels are templates on EDGE.  With a_edge [nnz, H], one row
// per stored entry in CSR position order,
//    u_e = (a_dst[i,h] + a_src[j,h]) + a_edge[e,h]        TWO fp32 adds, in this order, in all three kernels
// so that the forward and both backward kernels take the same branch of the slope on every edge (with three terms the sign of the fp32
// u_e is no longer the sign of the exact sum).  The forward and the rows kernel walk CSR positions, so the term is a streamed read: the
// edge in slot s of the batch at `base` is entry base + s, behind a descriptor rebased per batch on a_edge + base*H with the extent of
// the batch's live entries -- exact, and a dead slot is answered with 0.  The rows kernel also writes d a_edge[e,h] = du_e, every entry
// once (every stored entry belongs to one row).  The columns kernel walks the transposed structure and gathers a_edge[csr2csc[q], h]
// behind one descriptor of nnz*H*4 bytes.  EDGE = false is the code of the entries without the term, instruction for instruction
// (profiles/gat_edge_isa.txt).
//
// Attention dropout (isplib_gat_drop_*_hip): the three kernels are templates on DROP as well.  Every stored entry e and
// head h has a keep bit q_e,h = word(seed, CSR position of e, h) >= T (gat_dropout.h: a pure function, recomputed in all three
// kernels, nothing stored), and with c = float32(1 / (1 - p))
//    z_i = c sum_e q_e a_e y_j      t_e = q_e c <g_i, y_j>_h      dy_j = c sum_{e -> j} q_e a_e g_i      a_e, lse, s_e, du_e's form unchanged
// The softmax runs over ALL stored entries: l, m and lse do not see the mask.  The lane that loads an entry's index hashes the entry's
// position (base + lane in the forward and the rows kernel; csr2csc[pos] in the columns kernel, which therefore needs csr2csc whenever
// DROP is set) and hands the word across with the index; per edge and chunk one add of a per-lane constant, one fmix32, one compare and
// one select remain.  c multiplies the finished rows of z and dy, and t_e per edge.  DROP = false is the code it was.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "gat_dropout.h"
#include "attn_common.h"

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
   // EDGE only (appended: the layout of everything above is that of the kernels without the term)
   const float *edge;                      // a_edge [nnz, H], rows in CSR position order
   const int64_t *epos;                    // columns: csr2csc [nnz], the CSR position of every entry of the transposed structure
   float *dedge;                           // rows: d a_edge [nnz, H], or NULL
   unsigned ebytes;                        // columns: nnz * H * 4
   // DROP only (appended)
   unsigned seed_lo, seed_hi;              // the two halves of the seed
   unsigned T;                             // keep: word >= T
   float c;                                // float32(1 / (1 - p))
};

// byte offsets of the gathered row of edge `src` of the batch in the wide operand and in the [., H] tables; a dead edge: BUF_OOB
__device__ __forceinline__ void gat_edge(int id_l, int src, unsigned ldb, unsigned hb, unsigned &off, unsigned &offh) {
   const int id = __shfl(id_l, src);
   off = id < 0 ? BUF_OOB : (unsigned)id * ldb;
   offh = id < 0 ? BUF_OOB : (unsigned)id * hb;              // BUF_OOB + cbyte / hbyte (< 2^24) cannot wrap
}

// a descriptor whose base moves with the wave's batch: its inputs made provably wave-uniform, so that it is built with scalar
// instructions and no buffer load through it sits in a waterfall loop
__device__ __forceinline__ __amdgpu_buffer_rsrc_t gat_rsrc_uniform(const float *p, unsigned bytes) {
   const unsigned long long v = (unsigned long long)p;
   const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
   const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
   return attn_rsrc((const float *)(((unsigned long long)hi << 32) | (unsigned long long)lo), (unsigned)__builtin_amdgcn_readfirstlane((int)bytes));
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
__device__ __forceinline__ void gat_head_dot(const float (&r)[NCH][4], const v4i_t (&t)[NCH], const AttnHeadCols<LPR, NCH> &cm, const GatArgs &a,
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

// with the per-edge term: (a_dst + a_src) + a_edge, TWO fp32 adds in this order in every kernel; the branch is taken on this fp32 u
__device__ __forceinline__ float gat_score_edge(float adst, float asrc, float aedge, float ns, float &slope) {
   const float u = (adst + asrc) + aedge;
   slope = u > 0.0f ? 1.0f : ns;
   return u > 0.0f ? u : ns * u;
}

template <int LPR, int NCH, int WAVES, bool EDGE, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gat_fw_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn_rsrc(a.y, a.ybytes), rss = attn_rsrc(a.t0, a.tbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float adst[NCH];
   attn_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, adst);
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

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
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
      [[maybe_unused]] __amdgpu_buffer_rsrc_t rse;      // EDGE: the batch's rows of a_edge and nothing else
      if constexpr (EDGE) rse = gat_rsrc_uniform(a.edge + (size_t)base * (size_t)a.heads, (unsigned)cnt * hb);
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         float sc[U][NCH], se[EDGE ? U : 1][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            attn_load_wide<LPR, NCH>(rsy, off, cm, yv[u]);
            attn_load_head<LPR, NCH>(rss, offh, cm, sc[u]);
            if constexpr (EDGE) attn_load_head<LPR, NCH>(rse, (unsigned)((s0 + u * G + g) & 63) * hb, cm, se[u]);      // a slot past cnt: 0
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
#pragma unroll
         for (int j = 0; j < NCH; j++) {
            float mnew = mrun[j];
#pragma unroll
            for (int u = 0; u < U; u++) {
               float slope;
               if constexpr (EDGE) sc[u][j] = gat_score_edge(adst[j], sc[u][j], se[u][j], a.ns, slope);
               else sc[u][j] = gat_score(adst[j], sc[u][j], a.ns, slope);
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

template <int LPR, int NCH, int WAVES, bool EDGE, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gat_bw_rows_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn_rsrc(a.y, a.ybytes), rss = attn_rsrc(a.t0, a.tbytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float gv[NCH][4], adst[NCH], lse[NCH], dsum[NCH];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, gv);
   attn_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, adst);
   attn_own_head<LPR, NCH>(a.lse_in, row, a.heads, cm, lse);
   {                                                   // D[i,h] = <g_i, z_i>_h: every slot holds the row, so every lane of a head ends with it
      float zv[NCH][4];
      attn_own_row<LPR, NCH>(a.zin, row, a.ldzin, lc, cm.ok, zv);
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
   [[maybe_unused]] const bool store = EDGE && a.dedge != nullptr;      // wave-uniform: a kernel argument
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

   const unsigned ldyb = (unsigned)a.ldy * 4u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
      [[maybe_unused]] __amdgpu_buffer_rsrc_t rse;      // EDGE: the batch's rows of a_edge and nothing else
      if constexpr (EDGE) rse = gat_rsrc_uniform(a.edge + (size_t)base * (size_t)a.heads, (unsigned)cnt * hb);
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         float sc[U][NCH], se[EDGE ? U : 1][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            attn_load_wide<LPR, NCH>(rsy, off, cm, yv[u]);
            attn_load_head<LPR, NCH>(rss, offh, cm, sc[u]);
            if constexpr (EDGE) attn_load_head<LPR, NCH>(rse, (unsigned)((s0 + u * G + g) & 63) * hb, cm, se[u]);      // a slot past cnt: 0
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float t[NCH];
            gat_head_dot<LPR, NCH>(gv, yv[u], cm, a, t);
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               float slope;
               if constexpr (DROP) t[j] *= gat_drop_mix(hw[u], hk[j]) >= a.T ? a.c : 0.0f;      // t_e = q_e c <g_i, y_j>_h
               if constexpr (EDGE) {
                  const float s = gat_score_edge(adst[j], sc[u][j], se[u][j], a.ns, slope);
                  const float x = __expf(s - lse[j]) * (t[j] - dsum[j]);
                  const float du = x * slope;
                  // the bits of the kernel without the term: with one slot (G == 1) its first edge of a step is live whenever the step
                  // runs, and there the compiler contracts acc + x * slope into one fma; du has a second use here (the store), which
                  // would keep it from doing so -- so the fma is written out (profiles/gat_edge_isa.txt)
                  if (G == 1 && u == 0) acc[j] = fmaf(x, slope, acc[j]);
                  else acc[j] += live ? du : 0.0f;
                  if (store && live && cm.first[j])      // the lane that opens the head: every entry of d a_edge is written once
                     a.dedge[(size_t)(base + ((s0 + u * G + g) & 63)) * (size_t)a.heads + (size_t)cm.head[j]] = du;
               } else {
                  const float s = gat_score(adst[j], sc[u][j], a.ns, slope);
                  acc[j] += live ? __expf(s - lse[j]) * (t[j] - dsum[j]) * slope : 0.0f;
               }
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
template <int LPR, int NCH, int WAVES, bool EDGE, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void gat_bw_cols_kernel(const GatArgs a) {
   constexpr int G = 64 / LPR, U = NCH >= 2 ? 2 : 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsg = attn_rsrc(a.y, a.ybytes);
   const __amdgpu_buffer_rsrc_t rs0 = attn_rsrc(a.t0, a.tbytes), rs1 = attn_rsrc(a.t1, a.tbytes), rs2 = attn_rsrc(a.t2, a.tbytes);
   [[maybe_unused]] __amdgpu_buffer_rsrc_t rse;         // EDGE: all of a_edge, gathered by CSR position
   if constexpr (EDGE) rse = attn_rsrc(a.edge, a.ebytes);
   const AttnHeadCols<LPR, NCH> cm(a.k, a.hshift, a.hmask, lc);
   float yv[NCH][4], asrc[NCH];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, yv);
   attn_own_head<LPR, NCH>(a.own_score, row, a.heads, cm, asrc);
   [[maybe_unused]] unsigned hk[NCH];
   if constexpr (DROP) attn_drop_heads<LPR, NCH>(a.seed_hi, cm, hk);

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
      [[maybe_unused]] int ep_l = -1;                   // EDGE: the entry's CSR position (nnz < 2^31), handed across lanes like the row id
      if constexpr (EDGE || DROP) ep_l = pos < ee ? (int)a.epos[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, of its CSR position
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)ep_l);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t gg[U][NCH];
         float ad[U][NCH], ls[U][NCH], ds[U][NCH], se[EDGE ? U : 1][NCH];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat_edge(id_l, (s0 + u * G + g) & 63, ldgb, hb, off, offh);
            attn_load_wide<LPR, NCH>(rsg, off, cm, gg[u]);
            attn_load_head<LPR, NCH>(rs0, offh, cm, ad[u]);
            attn_load_head<LPR, NCH>(rs1, offh, cm, ls[u]);
            attn_load_head<LPR, NCH>(rs2, offh, cm, ds[u]);
            if constexpr (EDGE) {
               const int ep = __shfl(ep_l, (s0 + u * G + g) & 63);
               attn_load_head<LPR, NCH>(rse, ep < 0 ? BUF_OOB : (unsigned)ep * hb, cm, se[u]);      // ep * hb < nnz*H*4 <= 3.5 GiB
            }
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float t[NCH];
            gat_head_dot<LPR, NCH>(yv, gg[u], cm, a, t);
            const bool live = s0 + u * G + g < cnt;
#pragma unroll
            for (int j = 0; j < NCH; j++) {
               float slope;
               float s;
               if constexpr (EDGE) s = gat_score_edge(ad[u][j], asrc[j], se[u][j], a.ns, slope);
               else s = gat_score(ad[u][j], asrc[j], a.ns, slope);
               const float ae = live ? __expf(s - ls[u][j]) : 0.0f;
               [[maybe_unused]] bool keep = true;
               if constexpr (DROP) {
                  keep = gat_drop_mix(hw[u], hk[j]) >= a.T;
                  t[j] *= keep ? a.c : 0.0f;              // t_e = q_e c <g_i, y_j>_h
               }
               accs[j] += live ? ae * (t[j] - ds[u][j]) * slope : 0.0f;
               const float aek = keep ? ae : 0.0f;
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(aek, __int_as_float(gg[u][j][v]), acc[j][v]);
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
         if (cm.ok[j][v])                               // no incoming entry: 0
            a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = DROP ? acc[j][v] * a.c : acc[j][v];
      if (cm.first[j]) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head[j]] = accs[j];
   }
}

enum { GAT_FW = 0, GAT_BW_ROWS = 1, GAT_BW_COLS = 2 };

template <int LPR, int NCH, bool EDGE, bool DROP>
static int launch_gat(int which, const GatArgs &a, const char *entry, hipStream_t st) {
   constexpr int WAVES = 4;
   const int64_t nb = (a.rows + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block(WAVES * 64);
   if (which == GAT_FW) hipLaunchKernelGGL((gat_fw_kernel<LPR, NCH, WAVES, EDGE, DROP>), grid, block, 0, st, a);
   else if (which == GAT_BW_ROWS) hipLaunchKernelGGL((gat_bw_rows_kernel<LPR, NCH, WAVES, EDGE, DROP>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((gat_bw_cols_kernel<LPR, NCH, WAVES, EDGE, DROP>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the width ladder (attn_by_width); EDGE: the kernels with the per-edge term; DROP: with attention dropout
template <bool EDGE, bool DROP>
static int gat_by_width_of(int which, const GatArgs &a, const char *entry, hipStream_t st) {
   return attn_by_width(a.k, [&](auto lpr, auto nch) { return launch_gat<decltype(lpr)::value, decltype(nch)::value, EDGE, DROP>(which, a, entry, st); });
}

static int gat_by_width(int which, const GatArgs &a, bool edge, bool drop, const char *entry, hipStream_t st) {
   if (drop) return edge ? gat_by_width_of<true, true>(which, a, entry, st) : gat_by_width_of<false, true>(which, a, entry, st);
   return edge ? gat_by_width_of<true, false>(which, a, entry, st) : gat_by_width_of<false, false>(which, a, entry, st);
}

static const char *const GAT_DOMAIN = "outside isplib_gat_serves(rows_gathered, heads, d, ld): 1 <= heads, 1 <= d, heads*d <= 512, heads == 1 or "
                                      "d a power of two >= 4, ld >= heads*d, rows_gathered < 2^31, rows_gathered*ld*4 <= 3.5 GiB";
static const char *const GAT_EDGE_DOMAIN = "outside isplib_gat_edge_serves(nnz, heads): 1 <= heads, 0 <= nnz < 2^31, nnz*heads*4 <= 3.5 GiB "
                                           "(a_edge behind one buffer descriptor)";

// The three entries, with and without the per-edge term (edge: a_edge [nnz, heads]; csr2csc for the columns; d_a_edge may be NULL).
static int gat_forward(const char *entry, bool edge, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                       const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src, const float *a_edge,
                       int64_t heads, float negative_slope, float *z, int64_t ldz, float *lse, void *stream,
                       const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !a_dst || !z || !lse || (nnz > 0 && (!indx || !y || !a_src || (edge && !a_edge))))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   if (edge && !isplib_gat_edge_serves(nnz, heads)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_EDGE_DOMAIN);
   GatArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own_score = a_dst;
   a.out = z; a.ldout = ldz; a.hout = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? attn_extent(n, heads, heads) : 0u;
   a.edge = edge ? a_edge : nullptr;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return gat_by_width(GAT_FW, a, edge, dr.on, entry, (hipStream_t)stream);
}

static int gat_backward_rows(const char *entry, bool edge, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                             const int64_t *pntrb, const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                             const float *a_edge, int64_t heads, float negative_slope, const float *g, int64_t ldg, const float *z,
                             int64_t ldz, const float *lse, float *d_a_dst, float *dsum, float *d_a_edge, void *stream,
                             const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !a_dst || !g || !z || !lse || !d_a_dst || !dsum || (nnz > 0 && (!indx || !y || !a_src || (edge && !a_edge))))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldg < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(n, heads, k / heads, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   if (edge && !isplib_gat_edge_serves(nnz, heads)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_EDGE_DOMAIN);
   GatArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = g; a.ldown = ldg; a.own_score = a_dst; a.zin = z; a.ldzin = ldz; a.lse_in = lse;
   a.hout = d_a_dst; a.hout2 = dsum;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? attn_extent(n, heads, heads) : 0u;
   a.edge = edge ? a_edge : nullptr; a.dedge = edge ? d_a_edge : nullptr;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return gat_by_width(GAT_BW_ROWS, a, edge, dr.on, entry, (hipStream_t)stream);
}

static int gat_backward_cols(const char *entry, bool edge, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t,
                             const int64_t *colb, const int64_t *cole, const int64_t *csr2csc, const float *a_dst, const float *y, int64_t ldy,
                             const float *a_src, const float *a_edge, int64_t heads, float negative_slope, const float *g, int64_t ldg,
                             const float *lse, const float *dsum, float *dy, int64_t lddy, float *d_a_src, void *stream,
                             const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!colb || !cole || !y || !a_src || !dy || !d_a_src ||
       (nnz > 0 && (!row_t || !a_dst || !g || !lse || !dsum || (edge && !a_edge) || ((edge || dr.on) && !csr2csc))))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat_serves(m, heads, k / heads, ldg)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_DOMAIN);
   if (edge && !isplib_gat_edge_serves(nnz, heads)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT_EDGE_DOMAIN);
   GatArgs a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.ns = negative_slope;
   attn_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask, a.whole);
   a.own = y; a.ldown = ldy; a.own_score = a_src;
   a.out = dy; a.ldout = lddy; a.hout = d_a_src;
   a.y = g; a.ldy = ldg; a.ybytes = nnz > 0 ? attn_extent(m, k, ldg) : 0u;
   a.t0 = a_dst; a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn_extent(m, heads, heads) : 0u;
   if (edge) {
      a.edge = a_edge; a.ebytes = nnz > 0 ? attn_extent(nnz, heads, heads) : 0u;
   }
   if (edge || dr.on) a.epos = csr2csc;                  // DROP: the keep bit is a function of the entry's CSR position
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return gat_by_width(GAT_BW_COLS, a, edge, dr.on, entry, (hipStream_t)stream);
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_gat_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) { return isplib_gat_serves(rows_gathered, heads, d, ld); }

extern "C" int isplib_gat_edge_domain(int64_t nnz, int64_t heads) { return isplib_gat_edge_serves(nnz, heads); }

extern "C" int isplib_gat_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                  const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads, float negative_slope,
                                  float *z, int64_t ldz, float *lse, void *stream) {
   return gat_forward("isplib_gat_csr_hip", false, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, nullptr, heads, negative_slope, z, ldz,
                      lse, stream);
}

extern "C" int isplib_gat_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                      const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads,
                                      float negative_slope, const float *g, int64_t ldg, const float *z, int64_t ldz, const float *lse,
                                      float *d_a_dst, float *dsum, void *stream) {
   return gat_backward_rows("isplib_gat_bw_rows_hip", false, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, nullptr, heads, negative_slope,
                            g, ldg, z, ldz, lse, d_a_dst, dsum, nullptr, stream);
}

extern "C" int isplib_gat_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                      const int64_t *cole, const float *a_dst, const float *y, int64_t ldy, const float *a_src, int64_t heads,
                                      float negative_slope, const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy,
                                      int64_t lddy, float *d_a_src, void *stream) {
   return gat_backward_cols("isplib_gat_bw_cols_hip", false, m, n, k, nnz, row_t, colb, cole, nullptr, a_dst, y, ldy, a_src, nullptr, heads,
                            negative_slope, g, ldg, lse, dsum, dy, lddy, d_a_src, stream);
}

extern "C" int isplib_gat_edge_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                       const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                       const float *a_edge, int64_t heads, float negative_slope, float *z, int64_t ldz, float *lse,
                                       void *stream) {
   return gat_forward("isplib_gat_edge_csr_hip", true, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, a_edge, heads, negative_slope, z,
                      ldz, lse, stream);
}

extern "C" int isplib_gat_edge_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                           const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                           const float *a_edge, int64_t heads, float negative_slope, const float *g, int64_t ldg,
                                           const float *z, int64_t ldz, const float *lse, float *d_a_dst, float *dsum, void *stream,
                                           float *d_a_edge) {
   return gat_backward_rows("isplib_gat_edge_bw_rows_hip", true, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, a_edge, heads,
                            negative_slope, g, ldg, z, ldz, lse, d_a_dst, dsum, d_a_edge, stream);
}

extern "C" int isplib_gat_edge_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                           const int64_t *cole, const int64_t *csr2csc, const float *a_dst, const float *y, int64_t ldy,
                                           const float *a_src, const float *a_edge, int64_t heads, float negative_slope, const float *g,
                                           int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy, float *d_a_src,
                                           void *stream) {
   return gat_backward_cols("isplib_gat_edge_bw_cols_hip", true, m, n, k, nnz, row_t, colb, cole, csr2csc, a_dst, y, ldy, a_src, a_edge, heads,
                            negative_slope, g, ldg, lse, dsum, dy, lddy, d_a_src, stream);
}


// attention dropout: the argument lists of the isplib_gat_edge_* entries, a_edge / d_a_edge may be NULL (no per-edge term), then
// threshold, scale, seed.  A scale that is no positive finite number is refused: it would poison every row.
static bool gat_drop_ok(float scale) { return scale > 0.0f && scale <= FLT_MAX; }

extern "C" uint32_t isplib_gat_drop_threshold(double p) { return gat_drop_threshold(p); }

extern "C" uint32_t isplib_gat_drop_word(uint64_t seed, int64_t pos, int64_t head) { return gat_drop_word(seed, pos, head); }

extern "C" int isplib_gat_drop_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                       const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                       const float *a_edge, int64_t heads, float negative_slope, float *z, int64_t ldz, float *lse,
                                       void *stream, uint32_t threshold, float scale, uint64_t seed) {
   clear_error();
   if (!gat_drop_ok(scale)) return fail(ISPLIB_FAIL, "isplib_gat_drop_csr_hip", "scale must be a positive finite number");
   return gat_forward("isplib_gat_drop_csr_hip", a_edge != nullptr, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, a_edge, heads,
                      negative_slope, z, ldz, lse, stream, AttnDrop{true, threshold, scale, seed});
}

extern "C" int isplib_gat_drop_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                           const int64_t *pntre, const float *a_dst, const float *y, int64_t ldy, const float *a_src,
                                           const float *a_edge, int64_t heads, float negative_slope, const float *g, int64_t ldg,
                                           const float *z, int64_t ldz, const float *lse, float *d_a_dst, float *dsum, void *stream,
                                           float *d_a_edge, uint32_t threshold, float scale, uint64_t seed) {
   clear_error();
   if (!gat_drop_ok(scale)) return fail(ISPLIB_FAIL, "isplib_gat_drop_bw_rows_hip", "scale must be a positive finite number");
   return gat_backward_rows("isplib_gat_drop_bw_rows_hip", a_edge != nullptr, m, n, k, nnz, indx, pntrb, pntre, a_dst, y, ldy, a_src, a_edge,
                            heads, negative_slope, g, ldg, z, ldz, lse, d_a_dst, dsum, d_a_edge, stream, AttnDrop{true, threshold, scale, seed});
}

extern "C" int isplib_gat_drop_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                           const int64_t *cole, const int64_t *csr2csc, const float *a_dst, const float *y, int64_t ldy,
                                           const float *a_src, const float *a_edge, int64_t heads, float negative_slope, const float *g,
                                           int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy, float *d_a_src,
                                           void *stream, uint32_t threshold, float scale, uint64_t seed) {
   clear_error();
   if (!gat_drop_ok(scale)) return fail(ISPLIB_FAIL, "isplib_gat_drop_bw_cols_hip", "scale must be a positive finite number");
   return gat_backward_cols("isplib_gat_drop_bw_cols_hip", a_edge != nullptr, m, n, k, nnz, row_t, colb, cole, csr2csc, a_dst, y, ldy, a_src,
                            a_edge, heads, negative_slope, g, ldg, lse, dsum, dy, lddy, d_a_src, stream, AttnDrop{true, threshold, scale, seed});
}
