// attention16.hip -- the row-softmax attention aggregation of attention.hip for dense operands of 16-bit elements (bf16, fp16), forward
// and backward (include/isplib_hip.h: isplib_attention16_csr_hip, isplib_attention16_bw_rows_hip, isplib_attention16_bw_cols_hip).
// For every row i and stored entry e = (i, j), with x [m, k], y [n, k], a scalar p and g = dL/dz:
//    s_e  = p <x_i, y_j>          a_e = exp(s_e - lse_i),  lse_i = log sum_e exp(s_e)          z_i = sum_e a_e y_j
//    D_i  = sum_e a_e t_e         t_e = <g_i, y_j>          ds_e = a_e (t_e - D_i)
//    dx_i = p sum_e ds_e y_j      dy_j = sum_{e -> j} (a_e g_i + p ds_e x_i).
// No operand is widened in memory: a gathered row is half the bytes of the fp32 kernels', and the operator is bound by gathered bytes.
//
// The 16-bit family's contract: x, y and g are 16-bit and widening is exact (half16.h: widen2); every product, sum,
// exponential and division is fp32; z, dx and dy are rounded ONCE, to nearest even (narrow2); lse and D stay fp32; nothing is clamped or
// flushed.  No atomics, no LDS, a fixed order of operations: two launches give equal bits.
//
// Mapping: attention.hip's -- one wave per row (per column of A in the columns kernel), G = 64 / LPR edge slots, the wave's own row(s)
// widened into registers by plain loads that touch nothing outside the row's k columns, every gathered row behind one buffer descriptor
// and fetched by ONE 16-byte load of EIGHT columns per lane and edge (dead edges and lanes past k carry an offset the descriptor
// answers with 0), the per-edge dot products through reduce_transposed.  Always one chunk per lane, so LPR = 4 / 8 / 16 / 32 / 64 for
// ceil(k / 8) up to 4 / 8 / 16 / 32 / 64: k <= 512.  reduce_transposed<U, LPR> needs LPR >= U, so the kernels of two dot products
// per edge take U = 2 gathers per step at LPR = 4 and U = 4 elsewhere.
//
// Ragged K (k % 8 != 0): the last vector of a row over-reads columns that are not the row's (the next row, or 0 past the descriptor,
// whose size is the extent a row-strided view owns).  Each gathered dword is SELECTED by a per-lane mask before it is widened (k is
// even, so a dword is inside the row or outside it), and the own rows hold 0 there: both factors are 0, never Inf * 0, and what was
// over-read enters neither a dot product nor an accumulator.
//
// The forward is the online softmax of attention.hip, with its finite sentinel -FLT_MAX and its special values: a NaN or +inf score
// makes its own row NaN and no other; a row of one entry has weight exp(0) = 1 and l = 1, so z_i is y_j's 16 bits.
//
// The backward does NOT read z: in 16 bits z is rounded, and D_i = <g_i, z16_i> would carry u * sum_c |g_ic z_ic| into every ds_e.
// The rows kernel forms D_i in fp32 from the row's own edges, in one pass: l = sum a_e, Dacc = sum a_e t_e, Z = sum a_e y_j,
// A1 = sum a_e t_e y_j per slot, the slots merged by plain sums, D_i = Dacc / l, dx_i = p (A1 - D_i Z).  Autograd keeps x, y and lse.
// DESIGN.md 4.6c.
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "half16.h"
#include "attn16_common.h"

namespace isplib {

constexpr float ATTN16_NONE = -FLT_MAX;      // the running maximum of a slot that saw no edge

struct Attn16Args {
   int64_t rows, k;                          // rows: one wave each (rows of A; columns of A in the columns kernel)
   const int64_t *indx, *pntrb, *pntre;
   float p;
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const unsigned short *own;                // x (forward, rows) | y (columns)
   int64_t ldown;
   const unsigned short *g;                  // rows: dL/dz
   int64_t ldg;
   const float *lse, *dsum;                  // rows: lse [rows]; columns: lse, D [gathered rows], one per edge
   unsigned short *out;                      // z | dx | dy
   int64_t ldout;
   float *lse_out, *dsum_out;                // forward: lse; rows: D
   // the gathered operands: y (forward, rows) | x and g (columns), each behind one descriptor
   const void *y;
   int64_t ldy;
   unsigned ybytes;
   const void *y2;
   int64_t ldy2;
   unsigned y2bytes;
};

// this lane's eight consecutive columns; ok[q]: the dword of columns (2q, 2q + 1) lies inside the row (k is even)
struct Attn16Cols {
   int col;
   unsigned cbyte, poison;                   // past k: an offset the descriptor answers with 0
   bool ok[4];
   __device__ __forceinline__ Attn16Cols(int k, int lc) {
      col = lc * 8;
      cbyte = (unsigned)col * 2u;
      poison = col < k ? 0u : BUF_OOB;
#pragma unroll
      for (int q = 0; q < 4; q++) ok[q] = col + 2 * q < k;
   }
};

// the U gathers of this slot for the edges [s0, s0 + G*U) of the batch (edge s0 + u*G + g); dead edges carry BUF_OOB: they read 0
template <int LPR, int U>
__device__ __forceinline__ void attn16_gather(const __amdgpu_buffer_rsrc_t rsrc, unsigned off_l, int s0, int g, const Attn16Cols &cm,
                                              v4i_t (&t)[U]) {
   constexpr int G = 64 / LPR;
#pragma unroll
   for (int u = 0; u < U; u++) {
      const unsigned off = (unsigned)__shfl((int)off_l, (s0 + u * G + g) & 63);
      const unsigned o = (off + cm.cbyte) | cm.poison;      // off = BUF_OOB + cbyte (< 2^10) cannot wrap
      t[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
   }
}

template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention16_fw_kernel(const Attn16Args a) {
   constexpr int G = 64 / LPR, U = 4;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsrc = attn16_desc(a.y, a.ybytes);
   const Attn16Cols cm((int)a.k, lc);
   float xv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, xv);

   float mrun = ATTN16_NONE, l = 0.0f, acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const unsigned off_l = pos < ee ? (unsigned)a.indx[pos] * ldyb : BUF_OOB;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t t[U];
         attn16_gather<LPR, U>(rsrc, off_l, s0, g, cm, t);
         float part[U], sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float yv[8];
            attn16_widen<ELT>(t[u], cm.ok, yv);
            part[u] = attn16_dot_part(xv, yv);
         }
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
         for (int v = 0; v < 8; v++) acc[v] *= r;
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float w = (s0 + u * G + g < cnt) ? __expf(sc[u] - mnew) : 0.0f;
            l += w;
            float yv[8];
            attn16_widen<ELT>(t[u], cm.ok, yv);
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] = fmaf(w, yv[v], acc[v]);
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
   if (lc == 0) a.lse_out[row] = empty ? -INFINITY : mrun + logf(l);
}

// the one-pass backward over the rows: no z, D_i from the row's own edges
template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention16_bw_rows_kernel(const Attn16Args a) {
   constexpr int G = 64 / LPR, U = LPR >= 8 ? 4 : 2;      // both dot products of a step through one butterfly: 2U <= LPR
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsrc = attn16_desc(a.y, a.ybytes);
   const Attn16Cols cm((int)a.k, lc);
   float xv[8], gv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, xv);
   attn16_own_row<ELT>(a.g, row, a.ldg, cm.col, cm.ok, gv);
   const float lse = a.lse[row];

   float l = 0.0f, dacc = 0.0f, zacc[8], a1[8];      // sum a_e, sum a_e t_e, sum a_e y_j, sum a_e t_e y_j
#pragma unroll
   for (int v = 0; v < 8; v++) zacc[v] = a1[v] = 0.0f;

   const unsigned ldyb = (unsigned)a.ldy * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const unsigned off_l = pos < ee ? (unsigned)a.indx[pos] * ldyb : BUF_OOB;
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t tv[U];
         attn16_gather<LPR, U>(rsrc, off_l, s0, g, cm, tv);
         float part[2 * U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float yv[8];
            attn16_widen<ELT>(tv[u], cm.ok, yv);
            part[u] = attn16_dot_part(xv, yv);
            part[U + u] = attn16_dot_part(gv, yv);
         }
         int mine;
         const float sum = reduce_transposed<2 * U, LPR>(part, lc, mine);
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float s = a.p * __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(u));
            const float t = __shfl(sum, g * LPR + transposed_owner<2 * U, LPR>(U + u));
            const bool live = s0 + u * G + g < cnt;
            const float ae = live ? __expf(s - lse) : 0.0f;
            const float at = live ? ae * t : 0.0f;
            l += ae;
            dacc += at;
            float yv[8];
            attn16_widen<ELT>(tv[u], cm.ok, yv);
#pragma unroll
            for (int v = 0; v < 8; v++) {
               zacc[v] = fmaf(ae, yv[v], zacc[v]);
               a1[v] = fmaf(at, yv[v], a1[v]);
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
         zacc[v] += __shfl_xor(zacc[v], o);
         a1[v] += __shfl_xor(a1[v], o);
      }
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
   const float dsum = empty ? 0.0f : dacc / l;
   float dxr[8];
#pragma unroll
   for (int v = 0; v < 8; v++) dxr[v] = empty ? 0.0f : a.p * (a1[v] - dsum * zacc[v]);
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, dxr);
   if (lc == 0) a.dsum_out[row] = dsum;
}

// one wave per column j of A (a row of the transposed structure): y_j in registers, x_i and g_i gathered as two 16-bit streams
template <int ELT, int LPR, int WAVES>
__global__ __launch_bounds__(WAVES * 64) void attention16_bw_cols_kernel(const Attn16Args a) {
   constexpr int G = 64 / LPR, U = LPR >= 8 ? 4 : 2;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   __amdgpu_buffer_rsrc_t rsx = attn16_desc(a.y, a.ybytes);
   __amdgpu_buffer_rsrc_t rsg = attn16_desc(a.y2, a.y2bytes);
   const Attn16Cols cm((int)a.k, lc);
   float yv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, yv);

   float acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldxb = (unsigned)a.ldy * 2u, ldgb = (unsigned)a.ldy2 * 2u;
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
         v4i_t xt[U], gt[U];
         attn16_gather<LPR, U>(rsx, offx_l, s0, g, cm, xt);
         attn16_gather<LPR, U>(rsg, offg_l, s0, g, cm, gt);
         float part[2 * U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float xg[8], gg[8];
            attn16_widen<ELT>(xt[u], cm.ok, xg);
            attn16_widen<ELT>(gt[u], cm.ok, gg);
            part[u] = attn16_dot_part(yv, xg);
            part[U + u] = attn16_dot_part(yv, gg);
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
            float xg[8], gg[8];
            attn16_widen<ELT>(xt[u], cm.ok, xg);
            attn16_widen<ELT>(gt[u], cm.ok, gg);
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] += fmaf(pds, xg[v], ae * gg[v]);
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

enum { ATTN16_FW = 0, ATTN16_BW_ROWS = 1, ATTN16_BW_COLS = 2 };

template <int ELT, int LPR>
static int launch_attention16(int which, const Attn16Args &a, const char *entry, hipStream_t st) {
   constexpr int WAVES = 4;
   const int64_t nb = (a.rows + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block(WAVES * 64);
   if (which == ATTN16_FW) hipLaunchKernelGGL((attention16_fw_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   else if (which == ATTN16_BW_ROWS) hipLaunchKernelGGL((attention16_bw_rows_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((attention16_bw_cols_kernel<ELT, LPR, WAVES>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the element type and the slot width (attn16_run)
static int attention16_run(int dtype, int which, const Attn16Args &a, const char *entry, void *stream) {
   return attn16_run(dtype, a.k, [&](auto elt, auto lpr) {
      return launch_attention16<decltype(elt)::value, decltype(lpr)::value>(which, a, entry, (hipStream_t)stream);
   });
}

static const char *const ATTN16_DOMAIN = "outside isplib_attention16_serves(rows_gathered, k, ld): 8 <= k <= 512, k and every pitch even, ld >= k, "
                                         "rows_gathered < 2^31, rows_gathered*ld*2 <= 3.5 GiB (convert the operands and use the fp32 entries)";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_attention16_domain(int64_t rows_gathered, int64_t k, int64_t ld) { return isplib_attention16_serves(rows_gathered, k, ld); }

extern "C" int isplib_attention16_auto(int64_t rows_gathered, int64_t ld) { return isplib_attention16_native_pays(rows_gathered, ld); }

// the refusals of the three entries come in one order: dtype, negative dimension, nothing to do, a pitch below k, the domain, a null
// operand, alignment -- all before any launch
extern "C" int isplib_attention16_csr_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                          const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy, float scale, void *z,
                                          int64_t ldz, float *lse, void *stream) {
   const char *entry = "isplib_attention16_csr_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldx < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention16_serves(n, k, ldy) || !attn16_even(ldx, ldz)) return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN16_DOMAIN);
   if (!pntrb || !pntre || !x || !z || !lse || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(x, y, z)) return fail(ISPLIB_FAIL, entry, "x, y and z must be 4-byte aligned");
   Attn16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   a.own = reinterpret_cast<const unsigned short *>(x); a.ldown = ldx;
   a.out = reinterpret_cast<unsigned short *>(z); a.ldout = ldz; a.lse_out = lse;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   return attention16_run(dtype, ATTN16_FW, a, entry, stream);
}

extern "C" int isplib_attention16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                              const int64_t *pntre, const void *x, int64_t ldx, const void *y, int64_t ldy, float scale,
                                              const void *g, int64_t ldg, const float *lse, void *dx, int64_t lddx, float *dsum, void *stream) {
   const char *entry = "isplib_attention16_bw_rows_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldx < k || ldg < k || lddx < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention16_serves(n, k, ldy) || !attn16_even(ldx, ldg, lddx)) return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN16_DOMAIN);
   if (!pntrb || !pntre || !x || !g || !lse || !dx || !dsum || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(x, y, g, dx)) return fail(ISPLIB_FAIL, entry, "x, y, g and dx must be 4-byte aligned");
   Attn16Args a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   a.own = reinterpret_cast<const unsigned short *>(x); a.ldown = ldx;
   a.g = reinterpret_cast<const unsigned short *>(g); a.ldg = ldg; a.lse = lse;
   a.out = reinterpret_cast<unsigned short *>(dx); a.ldout = lddx; a.dsum_out = dsum;
   a.y = y; a.ldy = ldy; a.ybytes = nnz > 0 ? attn16_extent(n, k, ldy, 2u) : 0u;
   return attention16_run(dtype, ATTN16_BW_ROWS, a, entry, stream);
}

extern "C" int isplib_attention16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                              const int64_t *cole, const void *x, int64_t ldx, const void *y, int64_t ldy, float scale,
                                              const void *g, int64_t ldg, const float *lse, const float *dsum, void *dy, int64_t lddy,
                                              void *stream) {
   const char *entry = "isplib_attention16_bw_cols_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldy < k || lddy < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_attention16_serves(m, k, ldx) || !isplib_attention16_serves(m, k, ldg) || !attn16_even(ldy, lddy))
      return fail(ISPLIB_NO_OPT_IMPL, entry, ATTN16_DOMAIN);
   if (!colb || !cole || !y || !dy || (nnz > 0 && (!row_t || !x || !g || !lse || !dsum))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(x, y, g, dy)) return fail(ISPLIB_FAIL, entry, "x, y, g and dy must be 4-byte aligned");
   Attn16Args a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.p = scale;
   a.own = reinterpret_cast<const unsigned short *>(y); a.ldown = ldy; a.lse = lse; a.dsum = dsum;
   a.out = reinterpret_cast<unsigned short *>(dy); a.ldout = lddy;
   a.y = x; a.ldy = ldx; a.ybytes = nnz > 0 ? attn16_extent(m, k, ldx, 2u) : 0u;
   a.y2 = g; a.ldy2 = ldg; a.y2bytes = nnz > 0 ? attn16_extent(m, k, ldg, 2u) : 0u;
   return attention16_run(dtype, ATTN16_BW_COLS, a, entry, stream);
}
