// spmm_rows16_epilogue.hip -- the 16-bit row kernel's unit-weight / column-scaled sum (spmm_rows16.hip) with an epilogue on the
// finished fp32 row: fusedMM_csr_rows16_epilogue_hip,
//    z[i,c] = round16( act( rs_i * ( sum_e cs[indx[e]] * y[indx[e],c] + ss_i * y[i,c] ) + bias[c] ) )
// -- the fused GCN layer relu(D^-1/2 (A + I) D^-1/2 X + b) of a bf16 / fp16 X with cs = ss = rs = D^-1/2: X is gathered as it lies (no
// pre-scaled copy, neither fp32 nor 16-bit), the self loop, the left D^-1/2, bias and ReLU are applied in registers, the row is
// rounded ONCE.  DESIGN.md 4.2e.
//
// Front end, mapping and edge loop are the family's (rows16_common.h, rows16_sum.h: W_COL, or W_UNIT when col_scale is null), so the
// sum has the bits of fusedMM_csr_rows16_colscale_hip / fusedMM_csr_rows16_hip.  The epilogue runs on the lanes that store (slot 0;
// long rows: wave 0 after the fixed-order LDS combine), in this order: one fmaf(ss_i, y[i,c], sum), * rs_i, + bias[c], v > 0 ? v : 0
// (the fp32 epilogue's ReLU: -0.0 and NaN become +0.0), store_tail16x8.  No atomics: two launches give equal bits, and any row order
// gives the bits of index order.
//
// What can go wrong here that cannot in the plain kernel:
//   * the self row is one more 16-byte load per storing lane, through y's own descriptor at row * ldy * 2 + the lane's column bytes:
//     self_scale needs m == n (checked before the launch), so row < n and the offset is below n*ldy*2 <= 3.5 GiB; it is 4-byte
//     aligned for the reason the gathers are.  With ragged K the lane's last vector is shifted back (rows16_column): its first
//     `vfirst` components belong to the neighbouring lane, are read (valid columns k-8 ..) and are not stored;
//   * the bias is read with plain loads at the lane's eight columns, all < k (the shifted vector: k-8 .. k-1, and k >= 8);
//   * an empty row (and nnz == 0) still gets its epilogue: the launch is never skipped for nnz == 0.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"
#include "half16.h"
#include "rows16_common.h"
#include "rows16_sum.h"

namespace isplib {

struct Rows16EpArgs {
   int64_t m, k;
   const float *val;            // W_COL: the column table (col_scale), one factor per column of the sparse operand; W_UNIT: null
   const int64_t *indx, *pntrb, *pntre;
   const void *y;               // n x ldy elements of 2 bytes
   int64_t ldy;
   unsigned short *z;           // m x ldz
   int64_t ldz;
   int long_row;                // rows with more edges are split across the workgroup
   unsigned nblk;               // number of row blocks
   unsigned ybytes;             // n*ldy*2: the descriptor's size
   unsigned sbytes;             // W_COL: n*4, the size of the table's descriptor (a column id outside [0, n) reads 0)
   const int32_t *row_order;    // position -> row, null = the identity
   const float *row_scale;      // m, or null (= 1)
   const float *self_scale;     // m (== n), or null: no self term
   const float *bias;           // k, or null
   int relu;
};

// one wave's edges [rb, re) on rows16_batches: the column's factor (W_COL) or nothing, rows16_step per step
template <int ELT, int WM, int LPR, int NCH, int U>
__device__ __forceinline__ void rows16_ep_edges(const Rows16EpArgs &a, const __amdgpu_buffer_rsrc_t rsrc, const __amdgpu_buffer_rsrc_t srsrc, int64_t rb,
                                                int64_t re, const int (&ccol)[NCH], const bool (&cok)[NCH], float (&acc)[NCH][8]) {
   rows16_batches<LPR, NCH, U>(
      a, rb, re, ccol, cok,
      [&](int64_t p) {
         // a valid id is < n < 2^28 (n*ldy*2 fits the descriptor and ldy >= 8), so id * 4 cannot wrap
         if (WM == W_COL) return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(srsrc, (int)((unsigned)a.indx[p] * 4u), 0, 0));
         return 0.0f;
      },
      [&](auto uu, auto, unsigned off_l, float v_l, int s, int, int64_t, int g, const unsigned (&cbyte)[NCH], const unsigned (&poison)[NCH]) {
         rows16_step<ELT, WM != W_UNIT, LPR, NCH, decltype(uu)::value>(rsrc, off_l, v_l, s, g, cbyte, poison, acc);
      });
}

// the finished fp32 sum of the storing lanes: self term, row scale, bias, ReLU, then rounded once and stored
template <int ELT, int NCH>
__device__ __forceinline__ void rows16_ep_write(const Rows16EpArgs &a, const __amdgpu_buffer_rsrc_t rsrc, int64_t row, const int (&ccol)[NCH],
                                                const bool (&cok)[NCH], const int (&vfirst)[NCH], float (&acc)[NCH][8]) {
   unsigned short *zr = a.z + (size_t)row * (size_t)a.ldz;
   const float ss = a.self_scale ? a.self_scale[row] : 0.0f;
   const float rs = a.row_scale ? a.row_scale[row] : 1.0f;
   const unsigned rbyte = (unsigned)row * ((unsigned)a.ldy * 2u);      // self term: row < n, so this is below ybytes
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (!cok[j]) continue;
      if (a.self_scale) {
         const v4i_t t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(rbyte + (unsigned)ccol[j] * 2u), 0, 0);
#pragma unroll
         for (int q = 0; q < 4; q++) {
            float lo, hi;
            widen2<ELT>((unsigned)t[q], lo, hi);
            acc[j][2 * q] = fmaf(ss, lo, acc[j][2 * q]);
            acc[j][2 * q + 1] = fmaf(ss, hi, acc[j][2 * q + 1]);
         }
      }
      if (a.row_scale) {
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] *= rs;
      }
      if (a.bias) {
         const float *br = a.bias + ccol[j];                            // columns ccol .. ccol + 7, all < k
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] += br[v];
      }
      if (a.relu) {
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = acc[j][v] > 0.0f ? acc[j][v] : 0.0f;
      }
      store_tail16x8<ELT>(zr + ccol[j], acc[j], vfirst[j]);
   }
}

template <int ELT, int WM, int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64, (rows16_min_blocks<NCH>())) void spmm_rows16_epilogue_kernel(const Rows16EpArgs a) {
   constexpr int U = rows16_unroll<NCH>();
   constexpr int PANEL = LPR * 8 * NCH;     // columns covered by one grid.y panel
   __shared__ float sh_val[WAVES][PANEL];

   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   __amdgpu_buffer_rsrc_t rsrc = rows16_desc(a.y, a.ybytes);
   __amdgpu_buffer_rsrc_t srsrc = WM == W_COL ? rows16_desc(a.val, a.sbytes) : rsrc;

   int ccol[NCH], vfirst[NCH];                     // the family's column map, block remap and chunk split: rows16_common.h
   bool cok[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) ccol[j] = rows16_column((int)blockIdx.y * PANEL + (j * LPR + lc) * 8, a.k, cok[j], vfirst[j]);
   const unsigned lb = rows16_block(a.nblk);

   const int64_t row0 = (int64_t)lb * WAVES;
   const int64_t row = (a.row_order && row0 + wave < a.m) ? (int64_t)a.row_order[row0 + wave] : row0 + wave;

   // phase 1: one row per wave (rows up to long_row edges)
   if (row0 + wave < a.m) {
      const int64_t b = a.pntrb[row], e = a.pntre[row];
      if (e - b <= a.long_row) {
         float acc[NCH][8];
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) acc[j][v] = 0.0f;
         rows16_ep_edges<ELT, WM, LPR, NCH, U>(a, rsrc, srsrc, b, e, ccol, cok, acc);
#pragma unroll
         for (int off = LPR; off < 64; off <<= 1)        // butterfly over the 64 / LPR edge slots, fp32
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
               for (int v = 0; v < 8; v++) acc[j][v] += __shfl_xor(acc[j][v], off);
         if (g == 0) rows16_ep_write<ELT, NCH>(a, rsrc, row, ccol, cok, vfirst, acc);
      }
   }

   // phase 2: long rows of this block, all waves on one row at a time (contiguous edge chunks, fixed-order LDS combine in fp32)
   for (int r = 0; r < WAVES; r++) {
      if (row0 + r >= a.m) break;                  // uniform over the block
      const int64_t lr = a.row_order ? (int64_t)a.row_order[row0 + r] : row0 + r;
      const int64_t b = a.pntrb[lr], e = a.pntre[lr];
      if (e - b <= a.long_row) continue;           // uniform over the block
      int64_t cb, ce;
      rows16_chunk(b, e, wave, cb, ce);
      float acc[NCH][8];
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = 0.0f;
      rows16_ep_edges<ELT, WM, LPR, NCH, U>(a, rsrc, srsrc, cb, ce, ccol, cok, acc);
#pragma unroll
      for (int off = LPR; off < 64; off <<= 1)
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) acc[j][v] += __shfl_xor(acc[j][v], off);
      if (g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) sh_val[wave][(j * LPR + lc) * 8 + v] = acc[j][v];
      }
      __syncthreads();
      if (wave == 0 && g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) {
               const int o = (j * LPR + lc) * 8 + v;
               float t = sh_val[0][o];
               for (int w = 1; w < WAVES; w++) t += sh_val[w][o];
               acc[j][v] = t;
            }
         rows16_ep_write<ELT, NCH>(a, rsrc, lr, ccol, cok, vfirst, acc);
      }
      __syncthreads();
   }
}

template <int ELT, int WM>
static int launch_rows16_epilogue(const char *entry, const Rows16EpArgs &a, hipStream_t st) {
   return rows16_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      return rows16_launch<LPR, NCH>(entry, "spmm_rows16_epilogue_kernel", spmm_rows16_epilogue_kernel<ELT, WM, LPR, NCH, ROWS16_WAVES>, a, st);
   });
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_rows16_gcn_auto(int64_t n, int64_t ldy, int ordered) { return isplib_rows16_gcn_native_pays(n, ldy, ordered); }

extern "C" int fusedMM_csr_rows16_epilogue_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *col_scale, const int64_t *indx,
                                               const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order, const void *y, int64_t ldy,
                                               void *z, int64_t ldz, const isplib_epilogue16 *ep, void *stream) {
   static const char *entry = "fusedMM_csr_rows16_epilogue_hip";
   Rows16EpArgs a;
   bool run;
   const int rc = rows16_check(entry, true, "", true, false, dtype, m, n, k, nnz, col_scale, indx, pntrb, pntre, row_order, y, ldy, z, ldz, a, &run);
   if (!run) return rc;
   if (ep && ep->self_scale && m != n) return fail(ISPLIB_FAIL, entry, "self_scale needs m == n (the self row of i is y[i,:])");
   if (ep && ep->self_scale && !y) return fail(ISPLIB_FAIL, entry, "null operand");      // (rows16_check asks for y only when there are edges)
   a.sbytes = col_scale ? (unsigned)((unsigned long long)n * 4ull) : 0u;      // inside the domain n*ldy*2 fits 32 bits and ldy >= 8
   a.row_scale = ep ? ep->row_scale : nullptr;
   a.self_scale = ep ? ep->self_scale : nullptr;
   a.bias = ep ? ep->bias : nullptr;
   a.relu = ep && ep->relu ? 1 : 0;
   hipStream_t st = (hipStream_t)stream;
   const bool bf = dtype == ISPLIB_DTYPE_BF16;
   if (col_scale) return bf ? launch_rows16_epilogue<ELT_BF16, W_COL>(entry, a, st) : launch_rows16_epilogue<ELT_F16, W_COL>(entry, a, st);
   return bf ? launch_rows16_epilogue<ELT_BF16, W_UNIT>(entry, a, st) : launch_rows16_epilogue<ELT_F16, W_UNIT>(entry, a, st);
}
