// spmm_rows16.hip -- the plain schedule of the SpMM (spmm.hip: one CSR row per wavefront) for dense operands of 16-bit elements
// (bf16, fp16): fusedMM_csr_rows16_hip, sum / mean.  The row kernel on operands beyond every cache is bound by the BYTES it gathers
// (DESIGN.md 4.2), and a 16-bit row is half the lines: a lane's gather stays 16 bytes and now holds EIGHT columns, so a slot of LPR
// lanes covers LPR * 8 columns and a row of K columns takes half as many gather instructions as in fp32.
//
// Mapping (its pieces shared with spmm_rows16_minmax.hip: rows16_common.h): spmm_csr_kernel's plain mode -- one row per wave,
// WAVES rows per workgroup, blockIdx remapped so that an XCD walks a contiguous range of positions, an optional row order
// (position -> row), rows over long_row edges taken by all waves of the workgroup with a fixed-order LDS combine in fp32.  No
// atomics: two launches give equal bits, and any row order gives the bits of index order.
//
// The contract (the 16-bit stream kernel's): the halves are widened in registers, products, sums and the mean's
// division are fp32, and the finished row is rounded ONCE, to nearest even -- NaN stays NaN, bf16 keeps subnormals, fp16 overflows
// to +-Inf.  An empty row is 0.  No max / min, no epilogue, no column-sliced form here.
//
// Three weight modes (W_UNIT, W_EDGE, W_COL): no weights, one fp32 weight per edge (val[p]), or one fp32 factor per COLUMN taken
// from an n-entry table (col_scale[indx[p]], fusedMM_csr_rows16_colscale_hip).  W_COL differs from W_EDGE only in where a lane's
// factor of its edge of the 64-edge batch comes from -- one 4-byte load that depends on the index load instead of one that does
// not -- so it computes, bit for bit, what W_EDGE computes on val[p] = col_scale[indx[p]], without the nnz-long weight stream.
// The modes and the edge step (rows16_step) are in rows16_sum.h, shared with spmm_rows16_epilogue.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"
#include "half16.h"
#include "rows16_common.h"
#include "rows16_sum.h"

namespace isplib {

struct Rows16Args {
   int64_t m, k;
   const float *val;            // fp32 weights, one per edge; null = unit weights.  W_COL: the table, one factor per column
   const int64_t *indx, *pntrb, *pntre;
   const void *y;               // n x ldy elements of 2 bytes
   int64_t ldy;
   unsigned short *z;           // m x ldz
   int64_t ldz;
   int mean;                    // divide by max(deg, 1)
   int long_row;                // rows with more edges are split across the workgroup
   unsigned nblk;               // number of row blocks
   unsigned ybytes;             // n*ldy*2: the descriptor's size
   unsigned sbytes;             // W_COL: n*4, the size of the table's descriptor (a column id outside [0, n) reads 0)
   const int32_t *row_order;    // position -> row, null = the identity
};

// one wave's edges [rb, re) on rows16_batches (rows16_common.h): the weight of an edge by mode, rows16_step per step
template <int ELT, int WM, int LPR, int NCH, int U>
__device__ __forceinline__ void rows16_edges(const Rows16Args &a, const __amdgpu_buffer_rsrc_t rsrc, const __amdgpu_buffer_rsrc_t srsrc, int64_t rb, int64_t re,
                                             const int (&ccol)[NCH], const bool (&cok)[NCH], float (&acc)[NCH][8]) {
   rows16_batches<LPR, NCH, U>(
      a, rb, re, ccol, cok,
      [&](int64_t p) {
         if (WM == W_EDGE) return a.val[p];
         // the column's factor: a valid id is < n < 2^28 (n*ldy*2 fits the descriptor and ldy >= 8), so id * 4 cannot wrap
         if (WM == W_COL) return __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(srsrc, (int)((unsigned)a.indx[p] * 4u), 0, 0));
         return 0.0f;
      },
      [&](auto uu, auto, unsigned off_l, float v_l, int s, int, int64_t, int g, const unsigned (&cbyte)[NCH], const unsigned (&poison)[NCH]) {
         rows16_step<ELT, WM != W_UNIT, LPR, NCH, decltype(uu)::value>(rsrc, off_l, v_l, s, g, cbyte, poison, acc);
      });
}

// the finished fp32 row of the g == 0 lanes: the mean's division, then rounded once and stored
template <int ELT, int NCH>
__device__ __forceinline__ void rows16_write(const Rows16Args &a, int64_t row, int64_t deg, const int (&ccol)[NCH],
                                             const bool (&cok)[NCH], const int (&vfirst)[NCH], float (&acc)[NCH][8]) {
   unsigned short *zr = a.z + (size_t)row * (size_t)a.ldz;
   if (a.mean) {
      const float d = (float)(deg > 1 ? deg : 1);
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = acc[j][v] / d;
   }
#pragma unroll
   for (int j = 0; j < NCH; j++)
      if (cok[j]) store_tail16x8<ELT>(zr + ccol[j], acc[j], vfirst[j]);
}

template <int ELT, int WM, int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64, (rows16_min_blocks<NCH>())) void spmm_rows16_kernel(const Rows16Args a) {
   constexpr int U = rows16_unroll<NCH>();
   constexpr int PANEL = LPR * 8 * NCH;     // columns covered by one grid.y panel
   __shared__ float sh_val[WAVES][PANEL];

   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   __amdgpu_buffer_rsrc_t rsrc = rows16_desc(a.y, a.ybytes);
   // W_COL: the table behind a descriptor of its own (kernel arguments only: wave-uniform); the other modes never read through it
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
      const int64_t deg = e - b;
      if (deg <= a.long_row) {
         float acc[NCH][8];
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) acc[j][v] = 0.0f;
         rows16_edges<ELT, WM, LPR, NCH, U>(a, rsrc, srsrc, b, e, ccol, cok, acc);
#pragma unroll
         for (int off = LPR; off < 64; off <<= 1)        // butterfly over the 64 / LPR edge slots, fp32
#pragma unroll
            for (int j = 0; j < NCH; j++)
#pragma unroll
               for (int v = 0; v < 8; v++) acc[j][v] += __shfl_xor(acc[j][v], off);
         if (g == 0) rows16_write<ELT, NCH>(a, row, deg, ccol, cok, vfirst, acc);
      }
   }

   // phase 2: long rows of this block, all waves on one row at a time (contiguous edge chunks, fixed-order LDS combine in fp32)
   for (int r = 0; r < WAVES; r++) {
      if (row0 + r >= a.m) break;                  // uniform over the block
      const int64_t lr = a.row_order ? (int64_t)a.row_order[row0 + r] : row0 + r;
      const int64_t b = a.pntrb[lr], e = a.pntre[lr];
      const int64_t deg = e - b;
      if (deg <= a.long_row) continue;             // uniform over the block
      int64_t cb, ce;
      rows16_chunk(b, e, wave, cb, ce);
      float acc[NCH][8];
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = 0.0f;
      rows16_edges<ELT, WM, LPR, NCH, U>(a, rsrc, srsrc, cb, ce, ccol, cok, acc);
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
         rows16_write<ELT, NCH>(a, lr, deg, ccol, cok, vfirst, acc);
      }
      __syncthreads();
   }
}

template <int ELT, int WM>
static int launch_rows16(const char *entry, const Rows16Args &a, hipStream_t st) {
   return rows16_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      return rows16_launch<LPR, NCH>(entry, "spmm_rows16_kernel", spmm_rows16_kernel<ELT, WM, LPR, NCH, ROWS16_WAVES>, a, st);
   });
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_rows16_auto(int64_t n, int64_t ldy, int ordered, int weighted) { return isplib_rows16_native_pays(n, ldy, ordered, weighted); }
extern "C" int isplib_rows16_domain(int64_t n, int64_t k, int64_t ldy, int64_t ldz) { return isplib_rows16_serves(n, k, ldy, ldz); }

// the checks (rows16_check) and the launch of both entries: `val` is the per-edge weights (wm = W_EDGE, or W_UNIT when null) or the
// per-column table (wm = W_COL)
static int rows16_entry(const char *entry, int wm, int32_t imessage, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                        const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order,
                        const void *y, int64_t ldy, void *z, int64_t ldz, void *stream) {
   Rows16Args a;
   bool run;
   const int rc = rows16_check(entry, imessage == ISPLIB_MSG_SPMM_SUM || imessage == ISPLIB_MSG_SPMM_MEAN,
                               "sum and mean only (max / min of a 16-bit operand: convert it and use fusedMM_csr_hip)", true,
                               wm == W_COL && nnz > 0 && !val, dtype, m, n, k, nnz, val, indx, pntrb, pntre, row_order, y, ldy, z, ldz, a, &run);
   if (!run) return rc;
   a.mean = imessage == ISPLIB_MSG_SPMM_MEAN ? 1 : 0;
   a.sbytes = wm == W_COL && val ? (unsigned)((unsigned long long)n * 4ull) : 0u;      // inside the domain n*ldy*2 fits 32 bits and ldy >= 8
   hipStream_t st = (hipStream_t)stream;
   const bool bf = dtype == ISPLIB_DTYPE_BF16;
   if (wm == W_COL) return bf ? launch_rows16<ELT_BF16, W_COL>(entry, a, st) : launch_rows16<ELT_F16, W_COL>(entry, a, st);
   if (val) return bf ? launch_rows16<ELT_BF16, W_EDGE>(entry, a, st) : launch_rows16<ELT_F16, W_EDGE>(entry, a, st);
   return bf ? launch_rows16<ELT_BF16, W_UNIT>(entry, a, st) : launch_rows16<ELT_F16, W_UNIT>(entry, a, st);
}

extern "C" int fusedMM_csr_rows16_hip(int32_t imessage, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                                      const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order,
                                      const void *y, int64_t ldy, void *z, int64_t ldz, void *stream) {
   return rows16_entry("fusedMM_csr_rows16_hip", val ? W_EDGE : W_UNIT, imessage, dtype, m, n, k, nnz, val, indx, pntrb, pntre, row_order, y, ldy, z,
                       ldz, stream);
}

extern "C" int isplib_rows16_colscale_auto(int64_t n, int64_t ldy, int ordered) { return isplib_rows16_colscale_native_pays(n, ldy, ordered); }

extern "C" int fusedMM_csr_rows16_colscale_hip(int32_t imessage, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *col_scale,
                                               const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order,
                                               const void *y, int64_t ldy, void *z, int64_t ldz, void *stream) {
   return rows16_entry("fusedMM_csr_rows16_colscale_hip", W_COL, imessage, dtype, m, n, k, nnz, col_scale, indx, pntrb, pntre, row_order, y, ldy, z,
                       ldz, stream);
}
