// sddmm_rows16.hip -- the value gradient of SpMM-sum / SpMM-mean (the SDDMM of backward.hip, sddmm_csr_kernel) for dense operands
// of 16-bit elements (bf16, fp16): isplib_sddmm_csr_rows16_hip,
//    dval[j] = <y[indx[j], :], g[i, :]> * (mean ? 1 / max(deg_i, 1) : 1)      for the edges j of row i.
// Neither operand is widened in memory: a gathered row of y is half the bytes of the fp32 kernel's, and the SDDMM is bound by the
// bytes that leave the L2.  DESIGN.md 4.2d describes this file.
//
// Mapping: the 16-bit row kernels' (rows16_common.h) -- one row per wave, ROWS16_WAVES rows per workgroup, blockIdx
// remapped so that an XCD walks a contiguous range of positions, an optional row order, y behind one descriptor, one 16-byte gather
// of EIGHT columns per lane and edge, edge metadata 64 per coalesced load, rows over long_row edges cut into one chunk per wave.
// dval is per edge, so a long row needs no LDS combine and no barrier, and a row wider than one slot cannot be cut into grid.y
// panels: two chunks per lane (k <= 1024) is the widest form.
//
// The dot product: g[row, :] sits in registers, widened, for the whole row (a lane's 8 x NCH columns, read once per row or per
// chunk of a long row); a step takes U gathers per slot, a lane multiplies its eight (sixteen) columns into one fp32 partial per
// edge, and the slot reduction and the hand-off are sddmm_edges' (backward.hip): reduce_transposed leaves edge u of slot g in one
// lane of the slot, lane l of the wave collects edge l of the 64-edge batch, and ONE 256-byte store follows the batch.
//
// The contract: widening is exact, products and sums are fp32 (fused multiply-adds), the mean multiplies the finished dot by the
// fp32 1.0f / deg as the fp32 kernel does, dval is fp32 -- nothing is rounded to 16 bits and nothing is flushed.  No atomics: two
// launches give equal bits and any row order gives the bits of index order.
//
// Ragged K (k % 8 != 0): rows16_column shifts a row's last 16-byte vector back to end at column k, so its first `vfirst` components
// are columns the neighbouring lane multiplies too.  The SpMM kernels do not store them; here they would be ADDED twice.  They are
// taken out of the gathered y (an AND with a per-lane dword mask: k is even, so vfirst is) AND out of g's registers: zeroing g
// alone would turn an Inf of y into Inf * 0 = NaN where the true product is Inf.  The mask sits behind the compile-time RAGGED
// flag; k % 8 == 0 pays nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"
#include "half16.h"
#include "rows16_common.h"

namespace isplib {

struct SddmmRows16Args {
   int64_t m, k;
   const int64_t *indx, *pntrb, *pntre;
   const void *y;               // n x ldy elements of 2 bytes
   int64_t ldy;
   const unsigned short *g;     // m x ldg elements of 2 bytes
   int64_t ldg;
   float *dval;                 // nnz, CSR order
   int mean;                    // multiply by 1 / max(deg, 1)
   int long_row;                // rows with more edges are split across the workgroup
   unsigned nblk;               // number of row blocks
   unsigned ybytes;             // n*ldy*2: the descriptor's size
   const int32_t *row_order;    // position -> row, null = the identity
};

// gathers issued back to back per slot: the fp32 kernels' (sddmm_edges, sddmm_task_kernel), a power of two for reduce_transposed.
// tests/sddmm_rows16_cases.py mirrors it and the slot widths of rows16_by_width
constexpr int SDDMM16_U = 4;

// the lane of the wave that holds, after reduce_transposed<UU, LPR>, the result of edge `e` of a step of G * UU edges (edge e is
// gather e / G of slot e % G)
template <int UU, int LPR> __device__ __forceinline__ int sddmm16_holder(int e) {
   constexpr int G = 64 / LPR;
   return (e % G) * LPR + transposed_owner<UU, LPR>(e / G);
}

// this lane's columns of g[row, :] as floats.  Plain loads, so nothing outside the row's k columns is read: a lane whose chunk
// lies beyond the row holds zeros, and so do the duplicated components of a shifted last vector
template <int ELT, int NCH>
__device__ __forceinline__ void sddmm16_load_g(const SddmmRows16Args &a, int64_t row, const int (&ccol)[NCH], const bool (&cok)[NCH],
                                               const int (&vfirst)[NCH], float (&gv)[NCH][8]) {
   const unsigned short *gr = a.g + (size_t)row * (size_t)a.ldg;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      unsigned w[4] = {0u, 0u, 0u, 0u};
      if (cok[j]) {
         const unsigned *p = reinterpret_cast<const unsigned *>(gr + ccol[j]);      // 4-byte aligned: base, ldg and the column are even
#pragma unroll
         for (int q = 0; q < 4; q++) w[q] = p[q];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
         if (2 * q < vfirst[j]) w[q] = 0u;
         widen2<ELT>(w[q], gv[j][2 * q], gv[j][2 * q + 1]);
      }
   }
}

// UU gathers per slot for the edges [s, s + G*UU) of the current 64-edge batch, their dot products with g[row, :], and the
// hand-off: lane l keeps the result of edge l in `res`
template <int ELT, bool RAGGED, int LPR, int NCH, int UU>
__device__ __forceinline__ void sddmm16_step(const __amdgpu_buffer_rsrc_t rsrc, unsigned off_l, int s, int g, const unsigned (&cbyte)[NCH],
                                             const unsigned (&poison)[NCH], const float (&gv)[NCH][8], const unsigned (&ymask)[4], int src,
                                             float &res) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   v4i_t t[UU][NCH];
#pragma unroll
   for (int u = 0; u < UU; u++) {
      const int ei = (s + u * G + g) & 63;
      const unsigned off = (unsigned)__shfl((int)off_l, ei);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         // masked edge: off = BUF_OOB, + cbyte (< 2^25) cannot wrap; masked column: OR-ed past the limit.  Both read zeros
         const unsigned o = (off + cbyte[j]) | poison[j];
         t[u][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
      }
   }
   float d[UU];
#pragma unroll
   for (int u = 0; u < UU; u++) {
      float acc = 0.0f;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
         for (int q = 0; q < 4; q++) {
            unsigned w = (unsigned)t[u][j][q];
            if (RAGGED && j == NCH - 1) w &= ymask[q];      // only a row's last chunk holds a shifted vector
            float lo, hi;
            widen2<ELT>(w, lo, hi);
            acc = fmaf(lo, gv[j][2 * q], acc);
            acc = fmaf(hi, gv[j][2 * q + 1], acc);
         }
      }
      d[u] = acc;
   }
   int mine;
   const float sum = reduce_transposed<UU, LPR>(d, lane % LPR, mine);
   const float got = __shfl(sum, src);
   res = ((unsigned)(lane - s) < (unsigned)(G * UU)) ? got : res;
}

// one wave, the edges [rb, re) of row `row`, on rows16_batches (rows16_common.h)
template <int ELT, bool RAGGED, int LPR, int NCH>
__device__ __forceinline__ void sddmm16_edges(const SddmmRows16Args &a, const __amdgpu_buffer_rsrc_t rsrc, int64_t row, int64_t rb, int64_t re,
                                              float scale, const int (&ccol)[NCH], const bool (&cok)[NCH], const int (&vfirst)[NCH]) {
   constexpr int G = 64 / LPR, U = SDDMM16_U, UT = U >= 4 ? 2 : 1;
   if (rb >= re) return;                           // wave-uniform (an empty chunk of a long row)
   const int lane = threadIdx.x & 63;
   float gv[NCH][8];
   sddmm16_load_g<ELT, NCH>(a, row, ccol, cok, vfirst, gv);
   unsigned ymask[4];
#pragma unroll
   for (int q = 0; q < 4; q++) ymask[q] = 2 * q < vfirst[NCH - 1] ? 0u : 0xFFFFFFFFu;
   // a full step starts at a multiple of G*U and a tail step at a multiple of G*UT, so the holder of this lane's edge is fixed
   const int src_full = sddmm16_holder<U, LPR>(lane % (G * U)), src_tail = sddmm16_holder<UT, LPR>(lane % (G * UT));
   float res = 0.0f;                               // lane l collects the result of edge l of the batch: one store per batch
   rows16_batches<LPR, NCH, U>(
      a, rb, re, ccol, cok, [](int64_t) { return 0.0f; },
      [&](auto uu, auto tail, unsigned off_l, float, int s, int cnt, int64_t base, int g, const unsigned (&cbyte)[NCH], const unsigned (&poison)[NCH]) {
         constexpr int UU = decltype(uu)::value;
         sddmm16_step<ELT, RAGGED, LPR, NCH, UU>(rsrc, off_l, s, g, cbyte, poison, gv, ymask, decltype(tail)::value ? src_tail : src_full, res);
         // the batch's last step (wave-uniform): every lane below cnt has collected its edge
         if (s + G * UU >= cnt && lane < cnt) a.dval[base + lane] = res * scale;
      });
}

template <int ELT, bool RAGGED, int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64, NCH == 1 ? 8 : 1) void sddmm_rows16_kernel(const SddmmRows16Args a) {
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int lc = lane % LPR;
   __amdgpu_buffer_rsrc_t rsrc = rows16_desc(a.y, a.ybytes);

   int ccol[NCH], vfirst[NCH];                     // the family's column map, block remap and chunk split: rows16_common.h
   bool cok[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) ccol[j] = rows16_column((j * LPR + lc) * 8, a.k, cok[j], vfirst[j]);
   const unsigned lb = rows16_block(a.nblk);

   const int64_t row0 = (int64_t)lb * WAVES;
   const int64_t row = (a.row_order && row0 + wave < a.m) ? (int64_t)a.row_order[row0 + wave] : row0 + wave;

   // phase 1: one row per wave (rows up to long_row edges)
   if (row0 + wave < a.m) {
      const int64_t b = a.pntrb[row], e = a.pntre[row];
      const int64_t deg = e - b;
      if (deg > 0 && deg <= a.long_row) {
         const float scale = a.mean ? 1.0f / (float)deg : 1.0f;
         sddmm16_edges<ELT, RAGGED, LPR, NCH>(a, rsrc, row, b, e, scale, ccol, cok, vfirst);
      }
   }

   // phase 2: long rows of this block, all waves on one row at a time (contiguous edge chunks; dval is per edge: nothing to combine)
   for (int r = 0; r < WAVES; r++) {
      if (row0 + r >= a.m) break;                  // uniform over the block
      const int64_t lr = a.row_order ? (int64_t)a.row_order[row0 + r] : row0 + r;
      const int64_t b = a.pntrb[lr], e = a.pntre[lr];
      const int64_t deg = e - b;
      if (deg <= a.long_row) continue;             // uniform over the block
      int64_t cb, ce;
      rows16_chunk(b, e, wave, cb, ce);
      const float scale = a.mean ? 1.0f / (float)deg : 1.0f;
      sddmm16_edges<ELT, RAGGED, LPR, NCH>(a, rsrc, lr, cb, ce, scale, ccol, cok, vfirst);
   }
}

// one workgroup of ROWS16_WAVES waves per ROWS16_WAVES positions (rows16_launch without its column panels)
template <int ELT, bool RAGGED>
static int launch_sddmm_rows16(const char *entry, SddmmRows16Args a, hipStream_t st) {
   const int64_t nb = (a.m + ROWS16_WAVES - 1) / ROWS16_WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many row blocks for one launch");
   a.nblk = (unsigned)nb;
   return rows16_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      hipLaunchKernelGGL((sddmm_rows16_kernel<ELT, RAGGED, LPR, NCH, ROWS16_WAVES>), dim3((unsigned)nb, 1, 1), dim3(ROWS16_WAVES * 64, 1, 1), 0, st, a);
      return check_launch("sddmm_rows16_kernel");
   });
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_sddmm_rows16_auto(int64_t n, int64_t ldy, int ordered) { return isplib_sddmm_rows16_native_pays(n, ldy, ordered); }

// the refusals come in rows16_check's order and wording (rows16_common.h), with g in the place of the 16-bit output
extern "C" int isplib_sddmm_csr_rows16_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                           const int64_t *pntre, const int32_t *row_order, const void *y, int64_t ldy, const void *g, int64_t ldg,
                                           int mean, float *dval, void *stream) {
   const char *entry = "isplib_sddmm_csr_rows16_hip";
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, "dtype must be ISPLIB_DTYPE_BF16 or ISPLIB_DTYPE_F16");
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0 || nnz == 0) return ISPLIB_SUCCESS;
   if (ldy < k || ldg < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_sddmm_rows16_serves(n, k, ldy, ldg))
      return fail(ISPLIB_FAIL, entry, "outside isplib_sddmm_rows16_serves(n, k, ldy, ldg): 8 <= k <= 1024, k / ldy / ldg even, n < 2^31, "
                                      "n*ldy*2 <= 3.5 GiB (convert the operands and use isplib_sddmm_csr_hip)");
   if (row_order && m >= (1LL << 31)) return fail(ISPLIB_FAIL, entry, "m must be < 2^31 (32-bit row order)");
   if (!pntrb || !pntre || !dval || !indx || !y || !g) return fail(ISPLIB_FAIL, entry, "null operand");
   if ((((uintptr_t)y | (uintptr_t)g) & 3) != 0) return fail(ISPLIB_FAIL, entry, "y and g must be 4-byte aligned");
   SddmmRows16Args a;
   a.m = m; a.k = k;
   a.indx = indx; a.pntrb = pntrb; a.pntre = pntre;
   a.y = y; a.ldy = ldy; a.g = reinterpret_cast<const unsigned short *>(g); a.ldg = ldg;
   a.dval = dval;
   a.mean = mean ? 1 : 0;
   a.long_row = 2048;
   a.nblk = 0;
   a.ybytes = (unsigned)((unsigned long long)n * (unsigned long long)ldy * 2ull);      // inside the domain it fits 32 bits
   a.row_order = row_order;
   hipStream_t st = (hipStream_t)stream;
   const bool bf = dtype == ISPLIB_DTYPE_BF16;
   if (k % 8 != 0) return bf ? launch_sddmm_rows16<ELT_BF16, true>(entry, a, st) : launch_sddmm_rows16<ELT_F16, true>(entry, a, st);
   return bf ? launch_sddmm_rows16<ELT_BF16, false>(entry, a, st) : launch_sddmm_rows16<ELT_F16, false>(entry, a, st);
}
