// attention.hip -- row-softmax attention aggregation over the stored entries of a CSR matrix, forward and backward
// (include/isplib_hip.h: isplib_attention_csr_hip, isplib_attention_bw_rows_hip, isplib_attention_bw_cols_hip).  For every row i and
// stored entry e = (i, j), with x [m, k], y [n, k] and a scalar p:
//    s_e  = p <x_i, y_j>          a_e = exp(s_e - lse_i),  lse_i = log sum_e exp(s_e)          z_i = sum_e a_e y_j
// and for g = dL/dz
//    D_i  = <g_i, z_i>            t_e = <g_i, y_j>          ds_e = a_e (t_e - D_i)
//    dx_i = p sum_e ds_e y_j      dy_j = sum_{e -> j} (a_e g_i + p ds_e x_i).
// Stored values are not read; every stored entry is its own edge; an empty row has z_i = 0, lse_i = -inf, dx_i = 0, D_i = 0.
//
// Mapping: the row form of fusedmm_general.hip -- one wave per row (per column of A in the columns kernel), G = 64 / LPR edge slots, the
// wave's own row in registers, every gathered row fetched once with 16-byte buffer loads through one descriptor (lanes past k and dead
// edges carry an offset the descriptor answers with 0), the per-edge dot products reduced by the transposed butterfly of gather.h.
//
// The softmax is the online form: a slot carries (m, l, acc[.]) -- running maximum, denominator and weighted sum relative to it.  A
// step of U edges takes the step's maximum, rescales l and acc ONCE by exp(m_old - m_new) and adds exp(s - m_new) (* y_j).  The G slots
// are merged pairwise by the same rule at the end of the row.  A slot that saw no edge carries m = -FLT_MAX, a finite sentinel: it
// never forms -inf - (-inf), and exp(-FLT_MAX - m) is 0 for every m that matters.  fmaxf drops a NaN score from the maximum, so the
// NaN enters l through exp(NaN - m); a +inf score enters through exp(inf - inf): both make their own row NaN and nothing else.
//
// The backward stores nothing per edge: a_e is recomputed from the row's saved lse_i, so what autograd keeps is x, y, z and one scalar
// per row.  The rows kernel writes D_i beside dx; the columns kernel walks the transposed structure, gathers x_i and g_i as two
// streams and takes lse_i and D_i with the edge batch (one per lane, handed out by __shfl like the edge value of the generic kernel).
//
// No atomics and a fixed order of operations: two launches give equal bits.  Every output element is written, nothing is read from
// an output.  DESIGN.md 4.6b.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "attn_common.h"

namespace isplib {

constexpr float ATTN_NONE = -FLT_MAX;      // the running maximum of a slot that saw no edge

struct AttnArgs {
   int64_t rows, k;                        // rows: one wave each (rows of A; columns of A in the columns kernel)
   const int64_t *indx, *pntrb, *pntre;
   float p;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const float *own;                       // x (forward, rows) | y (columns)
   int64_t ldown;
   const float *g;                         // rows: dL/dz
   int64_t ldg;
   const float *zin;                       // rows: z of the forward
   int64_t ldzin;
   const float *lse, *dsum;                // rows: lse [rows]; columns: lse, D [gathered rows], one per edge
   float *out;                             // z | dx | dy
   int64_t ldout;
   float *lse_out, *dsum_out;              // forward: lse; rows: D
   // the gathered operands: y (forward, rows) | x and g (columns), each behind one descriptor
   const float *y;
   int64_t ldy;
   unsigned ybytes;
   const float *y2;
   int64_t ldy2;
   unsigned y2bytes;
};

template <int LPR, int NCH> struct AttnCols {
   unsigned cbyte[NCH], poison[NCH];       // this lane's 4 consecutive columns per chunk; past k: an offset the descriptor answers with 0
   bool ok[NCH][4];
   __device__ __forceinline__ AttnCols(int k, int lc) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const int c = (j * LPR + lc) * 4;
         cbyte[j] = (unsigned)c * 4u;
         poison[j] = c < k ? 0u : BUF_OOB;
#pragma unroll
         for (int v = 0; v < 4; v++) ok[j][v] = c + v < k;
      }
   }
};

// the U gathers of this slot for the edges [s0, s0 + G*U) of the batch (edge s0 + u*G + g); dead edges carry BUF_OOB: they read 0
template <int LPR, int NCH, int U>
__device__ __forceinline__ void attn_gather(const __amdgpu_buffer_rsrc_t rsrc, unsigned off_l, int s0, int g, const AttnCols<LPR, NCH> &cm,
                                            v4i_t (&t)[U][NCH]) {
   constexpr int G = 64 / LPR;
#pragma unroll
   for (int u = 0; u < U; u++) {
      const unsigned off = (unsigned)__shfl((int)off_l, (s0 + u * G + g) & 63);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const unsigned o = (off + cm.cbyte[j]) | cm.poison[j];      // off = BUF_OOB + cbyte (< 2^24) cannot wrap
         t[u][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
      }
   }
}

// <r, t> over this lane's columns; a 16-byte load may run into the next row, the mask drops what it brought
template <int LPR, int NCH>
__device__ __forceinline__ float attn_dot(const float (&r)[NCH][4], const v4i_t (&t)[NCH], const AttnCols<LPR, NCH> &cm) {
   float d = 0.0f;
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) d = fmaf(r[j][v], cm.ok[j][v] ? __int_as_float(t[j][v]) : 0.0f, d);
   return d;
}

template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention_fw_kernel(const AttnArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsrc = attn_rsrc(a.y, a.ybytes);
   const AttnCols<LPR, NCH> cm((int)a.k, lc);
   float xv[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, xv);

   float mrun = ATTN_NONE, l = 0.0f, acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const unsigned off_l = pos < ee ? (unsigned)a.indx[pos] * ldyb : BUF_OOB;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         attn_gather<LPR, NCH, U>(rsrc, off_l, s0, g, cm, yv);
         float part[U], sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) part[u] = attn_dot<LPR, NCH>(xv, yv[u], cm);
         int mine;
         const float sum = reduce_transposed<U, LPR>(part, lc, mine);
         float mnew = mrun;
#pragma unroll
         for (int u = 0; u < U; u++) {
            sc[u] = a.p * __shfl(sum, g * LPR + transposed_owner<U, LPR>(u));
            mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u]) : mnew;      // a NaN score is not a maximum; it enters through exp below
         }
         const float r = __expf(mrun - mnew);
         mrun = mnew;
         l *= r;
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 4; v++) acc[j][v] *= r;
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float w = (s0 + u * G + g < cnt) ? __expf(sc[u] - mnew) : 0.0f;
            l += w;
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(w, __int_as_float(yv[u][j][v]), acc[j][v]);
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
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 4; v++) acc[j][v] = acc[j][v] * ra + __shfl_xor(acc[j][v], o) * rb;
      mrun = mnew;
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++)
         if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = empty ? 0.0f : acc[j][v] / l;
   if (lc == 0) a.lse_out[row] = empty ? -INFINITY : mrun + logf(l);
}

template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention_bw_rows_kernel(const AttnArgs a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsrc = attn_rsrc(a.y, a.ybytes);
   const AttnCols<LPR, NCH> cm((int)a.k, lc);
   float xv[NCH][4], gv[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, xv);
   attn_own_row<LPR, NCH>(a.g, row, a.ldg, lc, cm.ok, gv);
   float dsum = 0.0f;                                  // D_i = <g_i, z_i>: every slot holds the row, so every lane ends with it
   {
      float zv[NCH][4];
      attn_own_row<LPR, NCH>(a.zin, row, a.ldzin, lc, cm.ok, zv);
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 4; v++) dsum = fmaf(gv[j][v], zv[j][v], dsum);
#pragma unroll
      for (int o = LPR / 2; o >= 1; o >>= 1) dsum += __shfl_xor(dsum, o);
   }
   const float lse = a.lse[row];

   float acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const unsigned off_l = pos < ee ? (unsigned)a.indx[pos] * ldyb : BUF_OOB;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t yv[U][NCH];
         attn_gather<LPR, NCH, U>(rsrc, off_l, s0, g, cm, yv);
         float part[2 * U];                            // both dot products of the step through one butterfly
#pragma unroll
         for (int u = 0; u < U; u++) {
            part[u] = attn_dot<LPR, NCH>(xv, yv[u], cm);
            part[U + u] = attn_dot<LPR, NCH>(gv, yv[u], cm);
         }
         int mine;
         const float sum = reduce_transposed<2 * U, LPR>(part, lc, mine);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float s = a.p * __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(u));
            const float t = __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(U + u));
            const float ds = (s0 + u * G + g < cnt) ? __expf(s - lse) * (t - dsum) : 0.0f;
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
               for (int v = 0; v < 4; v++) acc[j][v] = fmaf(ds, __int_as_float(yv[u][j][v]), acc[j][v]);
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
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++)
         if (cm.ok[j][v]) a.out[(size_t)row * (size_t)a.ldout + (size_t)((j * LPR + lc) * 4 + v)] = empty ? 0.0f : a.p * acc[j][v];
   if (lc == 0) a.dsum_out[row] = empty ? 0.0f : dsum;
}

// one wave per column j of A (a row of the transposed structure): y_j in registers, x_i and g_i gathered
template <int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention_bw_cols_kernel(const AttnArgs a) {
   constexpr int G = 64 / LPR, U = NCH >= 2 ? 2 : 4;   // two gather streams: half the edges per step where a lane holds two chunks
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsx = attn_rsrc(a.y, a.ybytes);
   __amdgpu_buffer_rsrc_t rsg = attn_rsrc(a.y2, a.y2bytes);
   const AttnCols<LPR, NCH> cm((int)a.k, lc);
   float yv[NCH][4];
   attn_own_row<LPR, NCH>(a.own, row, a.ldown, lc, cm.ok, yv);

   float acc[NCH][4];
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) acc[j][v] = 0.0f;

   const unsigned ldxb = (unsigned)a.ldy * 4u, ldgb = (unsigned)a.ldy2 * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      unsigned offx_l = BUF_OOB, offg_l = BUF_OOB;
      float lse_l = 0.0f, dsum_l = 0.0f;
      if (pos < ee) {
         const int64_t i = a.indx[pos];
         offx_l = (unsigned)i * ldxb;
         offg_l = (unsigned)i * ldgb;
         lse_l = a.lse[i];
         dsum_l = a.dsum[i];
      }
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t xg[U][NCH], gg[U][NCH];
         attn_gather<LPR, NCH, U>(rsx, offx_l, s0, g, cm, xg);
         attn_gather<LPR, NCH, U>(rsg, offg_l, s0, g, cm, gg);
         float part[2 * U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            part[u] = attn_dot<LPR, NCH>(yv, xg[u], cm);
            part[U + u] = attn_dot<LPR, NCH>(yv, gg[u], cm);
         }
         int mine;
         const float sum = reduce_transposed<2 * U, LPR>(part, lc, mine);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int src = (s0 + u * G + g) & 63;
            const bool live = s0 + u * G + g < cnt;
            const float s = a.p * __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(u));
            const float t = __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(U + u));
            const float lse = __shfl(lse_l, src), dsum = __shfl(dsum_l, src);      // every lane takes part: not under `live`
            const float ae = live ? __expf(s - lse) : 0.0f;
            const float pds = live ? a.p * (ae * (t - dsum)) : 0.0f;
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
               for (int v = 0; v < 4; v++)
                  acc[j][v] += fmaf(pds, __int_as_float(xg[u][j][v]), ae * __int_as_float(gg[u][j][v]));
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

enum { ATTN_FW = 0, ATTN_BW_ROWS = 1, ATTN_BW_COLS = 2 };

template <int LPR, int NCH>
static int launch_attention(int which, const AttnArgs &a, const char *entry, hipStream_t st) {
   constexpr int WAVES = 4;
   const int64_t nb = (a.rows + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block(WAVES * 64);
   if (which == ATTN_FW) hipLaunchKernelGGL((attention_fw_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   else if (which == ATTN_BW_ROWS) hipLaunchKernelGGL((attention_bw_rows_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((attention_bw_cols_kernel<LPR, NCH, WAVES>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the width ladder (attn_by_width)
static int attention_by_width(int which, const AttnArgs &a, const char *entry, hipStream_t st) {
   return attn_by_width(a.k, [&](auto lpr, auto nch) { return launch_attention<decltype(lpr)::value, decltype(nch)::value>(which, a, entry, st); });
}

static const char *const ATTN_DOMAIN = "outside isplib_attention_serves(rows_gathered, k, ld): 1 <= k <= 512, ld >= k, rows_gathered < 2^31, "
                                       "rows_gathered*ld*4 <= 3.5 GiB";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_attention_domain(int64_t rows_gathered, int64_t k, int64_t ld) { return isplib_attention_serves(rows_gathered, k, ld); }

extern "C" int isplib_attention_csr_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                        const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                        float *z, int64_t ldz, float *lse, void *stream) {
   const char *entry = "isplib_attention_csr_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !x || !z || !lse || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldx < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention_serves(n, k, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN_DOMAIN);
   AttnArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   a.own = x; a.ldown = ldx;
   a.out = z; a.ldout = ldz; a.lse_out = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   return attention_by_width(ATTN_FW, a, entry, (hipStream_t)stream);
}

extern "C" int isplib_attention_bw_rows_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                            const int64_t *pntre, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                            const float *g, int64_t ldg, const float *z, int64_t ldz, const float *lse, float *dx,
                                            int64_t lddx, float *dsum, void *stream) {
   const char *entry = "isplib_attention_bw_rows_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!pntrb || !pntre || !x || !g || !z || !lse || !dx || !dsum || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldx < k || ldg < k || ldz < k || lddx < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention_serves(n, k, ldy)) return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN_DOMAIN);
   AttnArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   a.own = x; a.ldown = ldx; a.g = g; a.ldg = ldg; a.zin = z; a.ldzin = ldz; a.lse = lse;
   a.out = dx; a.ldout = lddx; a.dsum_out = dsum;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn_extent(n, k, ldy) : 0u;
   return attention_by_width(ATTN_BW_ROWS, a, entry, (hipStream_t)stream);
}

extern "C" int isplib_attention_bw_cols_hip(int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                            const int64_t *cole, const float *x, int64_t ldx, const float *y, int64_t ldy, float scale,
                                            const float *g, int64_t ldg, const float *lse, const float *dsum, float *dy, int64_t lddy,
                                            void *stream) {
   const char *entry = "isplib_attention_bw_cols_hip";
   clear_error();
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (!colb || !cole || !y || !dy || (nnz > 0 && (!row_t || !x || !g || !lse || !dsum))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention_serves(m, k, ldx) || !isplib_attention_serves(m, k, ldg)) return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN_DOMAIN);
   AttnArgs a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.p = scale;
   a.own = y; a.ldown = ldy; a.lse = lse; a.dsum = dsum;
   a.out = dy; a.ldout = lddy;
   a.y = x; a.ldy = ldx; a.ybytes = nnz > 0 ? attn_extent(m, k, ldx) : 0u;
   a.y2 = g; a.ldy2 = ldg; a.y2bytes = nnz > 0 ? attn_extent(m, k, ldg) : 0u;
   return attention_by_width(ATTN_BW_COLS, a, entry, (hipStream_t)stream);
}
