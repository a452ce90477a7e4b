// gat16.hip -- the GAT attention aggregation of gat.hip for dense operands of 16-bit elements (bf16, fp16), all heads in one launch,
// forward and backward (include/isplib_hip.h: isplib_gat16_csr_hip, isplib_gat16_bw_rows_hip, isplib_gat16_bw_cols_hip).  The
// mathematics is gat.hip's, stated in its header: for every row i, stored entry e = (i, j) and head h, with y [n, k], k = H*d, the fp32
// tables a_dst [m, H], a_src [n, H], a slope ns and g = dL/dz,
//    u_e  = a_dst[i,h] + a_src[j,h]      s_e = u_e > 0 ? u_e : ns u_e       sl_e = u_e > 0 ? 1 : ns
//    a_e  = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)             z_i[head h] = sum_e a_e y_j[head h]
//    D[i,h] = sum_e a_e t_e      t_e = <g_i, y_j>_h        du_e = a_e (t_e - D[i,h]) sl_e
//    d a_dst[i,h] = sum_e du_e   d a_src[j,h] = sum_{e -> j} du_e           dy_j[head h] = sum_{e -> j} a_e g_i[head h].
// No wide operand is widened in memory: a gathered row of y or g is half the bytes of the fp32 kernels', and the operator is bound by
// gathered bytes.
//
// The 16-bit family's contract: y, g, z and dy are 16-bit and widening is exact (half16.h: widen2); every product,
// sum, exponential and division is fp32; z and dy are rounded ONCE, to nearest even (narrow2).  a_dst, a_src, lse, D, d a_dst and
// d a_src stay fp32 -- [rows, H] tables, 1/d of y, gathered 4 bytes at a time exactly as in gat.hip -- so u_e is one fp32 add whose
// sign is the sign of the exact sum.
//
// Mapping: attention16.hip's -- one wave per row (per column of A in the columns kernel), always ONE 16-byte buffer load of EIGHT
// columns per lane and edge, LPR = 4 / 8 / 16 / 32 / 64 for ceil(k / 8) up to 4 / 8 / 16 / 32 / 64 and G = 64 / LPR edge slots, U = 4
// gathers per slot and step in all three kernels.  With H > 1, d is a power of two >= 8: a lane's eight columns never straddle heads
// and a head is an aligned group of d / 8 lanes (at d = 8 one lane: the per-head sum has no cross-lane step).  With H == 1 the head is
// the whole slot and k may be any even width >= 8; the ragged last vector (k % 8 != 0) over-reads, and each over-read dword is dropped
// by a per-lane select before it is widened, never by a multiply.  Every gathered table sits behind a buffer descriptor of exactly the
// extent it owns; dead edges and lanes past k carry BUF_OOB, which the descriptor answers with 0.  No LDS, no atomics, no scratch, a
// fixed order of operations: two launches give equal bits.
//
// The forward is gat.hip's online softmax per lane: (m, l, acc[8]), one rescale per step of U edges, -FLT_MAX for "no edge yet", the
// slots merged pairwise.  A row of one entry has weight exp(0) = 1 and l = 1: z_i is y_j's 16 bits, lse = s_e.  fmaxf drops a NaN
// score from the maximum, so it enters l through exp(NaN - m): a NaN in a_src[j,h] makes head h of the rows that reference j NaN and
// nothing else.
//
// The backward over the rows does NOT read z: in 16 bits z is rounded, and D = <g_i, z16_i>_h would carry u * sum_c |g_ic z_ic| into
// every du_e.  One pass over the row's edges accumulates, per head and slot, l = sum a_e, Dacc = sum a_e t_e,
// P = sum a_e sl_e t_e and Q = sum a_e sl_e; the slots merge by plain sums; D = Dacc / l and d a_dst = P - D Q.  The columns kernel
// is gat.hip's: y_j and a_src[j,.] in registers, g_i gathered in one 16-byte load, a_dst, lse and D of [i, head] from three 4-byte
// tables.  DESIGN.md 4.6e.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "half16.h"
#include "attn16_common.h"

namespace isplib {

constexpr float GAT16_NONE = -FLT_MAX;       // the running maximum of a lane that saw no edge

struct Gat16Args {
   int64_t rows, k;                          // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                               // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                               // lanes that share a head: d / 8 (H == 1: 64, the whole slot)
   unsigned hmask;                           // c & hmask == 0: the first column of a head (H == 1: only column 0)
   const int64_t *indx, *pntrb, *pntre;
   float ns;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const unsigned short *own;                // rows: g | columns: y
   int64_t ldown;
   const float *own_score;                   // forward, rows: a_dst [rows, H] | columns: a_src [rows, H]
   const float *lse_in;                      // rows: lse [rows, H]
   unsigned short *out;                      // z | dy
   int64_t ldout;
   float *hout, *hout2;                      // [rows, H]: forward lse | rows: d a_dst, D | columns: d a_src
   // the gathered operands, each behind one descriptor
   const void *y;                            // forward, rows: y | columns: g
   int64_t ldy;
   unsigned ybytes;
   const float *t0, *t1, *t2;                // forward, rows: t0 = a_src | columns: a_dst, lse, D; all [gathered rows, H]
   unsigned tbytes;
};

// byte offsets of the gathered row of edge `src` of the batch in the wide operand and in the [., H] tables; a dead edge: BUF_OOB
__device__ __forceinline__ void gat16_edge(int id_l, int src, unsigned ldb, unsigned hb, unsigned &off, unsigned &offh) {
   const int id = __shfl(id_l, src);
   off = id < 0 ? BUF_OOB : (unsigned)id * ldb;
   offh = id < 0 ? BUF_OOB : (unsigned)id * hb;              // BUF_OOB + cbyte / hbyte (< 2^10) cannot wrap
}

// <r, y>_h: over this lane's eight columns, then over the head's lanes
template <int LPR> __device__ __forceinline__ float gat16_head_dot(const float (&r)[8], const float (&y)[8], int hlanes) {
   float d[1] = {attn16_dot_part(r, y)};
   attn16_head_sum<LPR, 1>(d, hlanes);
   return d[0];
}

__device__ __forceinline__ float gat16_score(float adst, float asrc, float ns, float &slope) {
   const float u = adst + asrc;              // ONE fp32 add: its sign is the sign of the exact sum
   slope = u > 0.0f ? 1.0f : ns;
   return u > 0.0f ? u : ns * u;
}

template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat16_fw_kernel(const Gat16Args a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn16_desc(a.y, a.ybytes), rss = attn16_desc(a.t0, a.tbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   const float adst = attn16_own_head(a.own_score, row, a.heads, cm);

   float mrun = GAT16_NONE, l = 0.0f, acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 2u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U];
         float sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat16_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            yv[u] = attn16_load_wide(rsy, off, cm);
            sc[u] = attn16_load_head(rss, offh, cm);
         }
         float mnew = mrun;
#pragma unroll
         for (int u = 0; u < U; u++) {
            float slope;
            sc[u] = gat16_score(adst, sc[u], a.ns, slope);
            mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u]) : mnew;      // a NaN score is not a maximum; it enters through exp below
         }
         const float r = __expf(mrun - mnew);
         mrun = mnew;
         l *= r;
#pragma unroll
         for (int v = 0; v < 8; v++) acc[v] *= r;
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float w = (s0 + u * G + g < cnt) ? __expf(sc[u] - mnew) : 0.0f;
            l += w;
            float y8[8];
            attn16_widen<ELT>(yv[u], cm.ok, y8);
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] = fmaf(w, y8[v], acc[v]);
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

// the one-pass backward over the rows: no z, D[i,h] from the row's own edges
template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat16_bw_rows_kernel(const Gat16Args a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsy = attn16_desc(a.y, a.ybytes), rss = attn16_desc(a.t0, a.tbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float gv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, gv);
   const float adst = attn16_own_head(a.own_score, row, a.heads, cm), lse = attn16_own_head(a.lse_in, row, a.heads, cm);

   float l = 0.0f, dacc = 0.0f, pacc = 0.0f, qacc = 0.0f;      // sum a_e, sum a_e t_e, sum a_e sl_e t_e, sum a_e sl_e

   const unsigned ldyb = (unsigned)a.ldy * 2u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U];
         float sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat16_edge(id_l, (s0 + u * G + g) & 63, ldyb, hb, off, offh);
            yv[u] = attn16_load_wide(rsy, off, cm);
            sc[u] = attn16_load_head(rss, offh, cm);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float y8[8];
            attn16_widen<ELT>(yv[u], cm.ok, y8);
            const float t = gat16_head_dot<LPR>(gv, y8, a.hlanes);      // every lane takes part: not under `live`
            const bool live = s0 + u * G + g < cnt;
            float slope;
            const float s = gat16_score(adst, sc[u], a.ns, slope);
            const float ae = live ? __expf(s - lse) : 0.0f;
            const float as = live ? ae * slope : 0.0f;
            l += ae;
            dacc += live ? ae * t : 0.0f;
            pacc += live ? as * t : 0.0f;
            qacc += as;
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      l += __shfl_xor(l, o);
      dacc += __shfl_xor(dacc, o);
      pacc += __shfl_xor(pacc, o);
      qacc += __shfl_xor(qacc, o);
   }
   if (g != 0 || !cm.first) return;
   const bool empty = ee <= eb;
   const float dsum = empty ? 0.0f : dacc / l;
   a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = empty ? 0.0f : pacc - dsum * qacc;
   a.hout2[(size_t)row * (size_t)a.heads + (size_t)cm.head] = dsum;
}

// one wave per column j of A (a row of the transposed structure): y_j and a_src[j,.] in registers; g_i, a_dst, lse, D of row i gathered
template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void gat16_bw_cols_kernel(const Gat16Args a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsg = attn16_desc(a.y, a.ybytes);
   const __amdgpu_buffer_rsrc_t rs0 = attn16_desc(a.t0, a.tbytes), rs1 = attn16_desc(a.t1, a.tbytes), rs2 = attn16_desc(a.t2, a.tbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float yv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, yv);
   const float asrc = attn16_own_head(a.own_score, row, a.heads, cm);

   float acc[8], accs = 0.0f;
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldgb = (unsigned)a.ldy * 2u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t gg[U];
         float ad[U], ls[U], ds[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            unsigned off, offh;
            gat16_edge(id_l, (s0 + u * G + g) & 63, ldgb, hb, off, offh);
            gg[u] = attn16_load_wide(rsg, off, cm);
            ad[u] = attn16_load_head(rs0, offh, cm);
            ls[u] = attn16_load_head(rs1, offh, cm);
            ds[u] = attn16_load_head(rs2, offh, cm);
         }
#pragma unroll
         for (int u = 0; u < U; u++) {
            float g8[8];
            attn16_widen<ELT>(gg[u], cm.ok, g8);
            const float t = gat16_head_dot<LPR>(yv, g8, a.hlanes);      // every lane takes part: not under `live`
            const bool live = s0 + u * G + g < cnt;
            float slope;
            const float s = gat16_score(ad[u], asrc, a.ns, slope);
            const float ae = live ? __expf(s - ls[u]) : 0.0f;
            accs += live ? ae * (t - ds[u]) * slope : 0.0f;
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] = fmaf(ae, g8[v], acc[v]);
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      accs += __shfl_xor(accs, o);
#pragma unroll
      for (int v = 0; v < 8; v++) acc[v] += __shfl_xor(acc[v], o);
   }
   if (g != 0) return;
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, acc);      // no incoming entry: 0
   if (cm.first) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = accs;
}

enum { GAT16_FW = 0, GAT16_BW_ROWS = 1, GAT16_BW_COLS = 2 };

template <int ELT, int LPR>
static int launch_gat16(int which, const Gat16Args &a, const char *entry, hipStream_t st) {
   constexpr int WAVES = 4;
   const int64_t nb = (a.rows + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block(WAVES * 64);
   if (which == GAT16_FW) hipLaunchKernelGGL((gat16_fw_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   else if (which == GAT16_BW_ROWS) hipLaunchKernelGGL((gat16_bw_rows_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((gat16_bw_cols_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the element type and the slot width (attn16_run)
static int gat16_run(int dtype, int which, const Gat16Args &a, const char *entry, void *stream) {
   return attn16_run(dtype, a.k, [&](auto elt, auto lpr) {
      return launch_gat16<decltype(elt)::value, decltype(lpr)::value>(which, a, entry, (hipStream_t)stream);
   });
}

static const char *const GAT16_DOMAIN = "outside isplib_gat16_serves(rows_gathered, heads, d, ld): 1 <= heads, 8 <= heads*d <= 512, heads == 1 with d "
                                        "even or d a power of two >= 8, every pitch even, ld >= heads*d, rows_gathered < 2^31, "
                                        "rows_gathered*ld*2 <= 3.5 GiB (convert the operands and use the fp32 entries)";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_gat16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_gat16_serves(rows_gathered, heads, d, ld);
}

extern "C" int isplib_gat16_auto(int64_t rows_gathered, int64_t ld) { return isplib_gat16_native_pays(rows_gathered, ld); }

// the refusals of the three entries come in one order: dtype, negative dimension, nothing to do, a pitch below k, k % heads, the
// domain, a null operand, alignment -- all before any launch
extern "C" int isplib_gat16_csr_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                    const int64_t *pntre, const float *a_dst, const void *y, int64_t ldy, const float *a_src, int64_t heads,
                                    float negative_slope, void *z, int64_t ldz, float *lse, void *stream) {
   const char *entry = "isplib_gat16_csr_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat16_serves(n, heads, k / heads, ldy) || !attn16_even(ldz, 0)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT16_DOMAIN);
   if (!pntrb || !pntre || !a_dst || !z || !lse || (nnz > 0 && (!indx || !y || !a_src))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(y, z)) return fail(ISPLIB_FAIL, entry, "y and z must be 4-byte aligned");
   Gat16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own_score = a_dst;
   a.out = reinterpret_cast<unsigned short *>(z); a.ldout = ldz; a.hout = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? attn16_extent(n, heads, heads, 4u) : 0u;
   return gat16_run(dtype, GAT16_FW, a, entry, stream);
}

extern "C" int isplib_gat16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                        const int64_t *pntre, const float *a_dst, const void *y, int64_t ldy, const float *a_src, int64_t heads,
                                        float negative_slope, const void *g, int64_t ldg, const float *lse, float *d_a_dst, float *dsum,
                                        void *stream) {
   const char *entry = "isplib_gat16_bw_rows_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldg < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat16_serves(n, heads, k / heads, ldy) || !attn16_even(ldg, 0)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT16_DOMAIN);
   if (!pntrb || !pntre || !a_dst || !g || !lse || !d_a_dst || !dsum || (nnz > 0 && (!indx || !y || !a_src)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(y, g)) return fail(ISPLIB_FAIL, entry, "y and g must be 4-byte aligned");
   Gat16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(g); a.ldown = ldg; a.own_score = a_dst; a.lse_in = lse;
   a.hout = d_a_dst; a.hout2 = dsum;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   a.t0 = a_src; a.tbytes = nnz > 0 ? attn16_extent(n, heads, heads, 4u) : 0u;
   return gat16_run(dtype, GAT16_BW_ROWS, a, entry, stream);
}

extern "C" int isplib_gat16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                        const int64_t *cole, const float *a_dst, const void *y, int64_t ldy, const float *a_src, int64_t heads,
                                        float negative_slope, const void *g, int64_t ldg, const float *lse, const float *dsum, void *dy,
                                        int64_t lddy, float *d_a_src, void *stream) {
   const char *entry = "isplib_gat16_bw_cols_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (heads < 1 || !isplib_gat16_serves(m, heads, k / heads, ldg) || !attn16_even(ldy, lddy)) return fail(ISPLIB_NO_OPT_IMPL, entry, GAT16_DOMAIN);
   if (!colb || !cole || !y || !a_src || !dy || !d_a_src || (nnz > 0 && (!row_t || !a_dst || !g || !lse || !dsum)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(y, g, dy)) return fail(ISPLIB_FAIL, entry, "y, g and dy must be 4-byte aligned");
   Gat16Args a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.ns = negative_slope;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(y); a.ldown = ldy; a.own_score = a_src;
   a.out = reinterpret_cast<unsigned short *>(dy); a.ldout = lddy; a.hout = d_a_src;
   a.y = g; a.ldy = ldg; a.ybytes = nnz > 0 ? attn16_extent(m, k, ldg, 2u) : 0u;
   a.t0 = a_dst; a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn16_extent(m, heads, heads, 4u) : 0u;
   return gat16_run(dtype, GAT16_BW_COLS, a, entry, stream);
}
