// spmm_rows16_minmax.hip -- max / min of the SpMM on the plain schedule (one CSR row per wavefront) for dense operands of 16-bit
// elements (bf16, fp16): fusedMM_csr_rows16_minmax_hip.  spmm_rows16.hip's mapping (its pieces: rows16_common.h) -- a lane's 16-byte gather holds EIGHT columns,
// a slot of LPR lanes covers LPR * 8 columns, WAVES rows per workgroup, blockIdx remapped so that an XCD walks a contiguous range of
// positions, an optional row order, rows over long_row edges taken by all waves of the workgroup -- with the arithmetic of the fp32
// kernel's max / min (gather.h, buf_step): the halves are widened in registers, the candidate of an edge is val * y (ONE fp32
// multiply; unit weights: y itself), it replaces the running value only if STRICTLY better, and the row-relative id of the winning
// edge travels with the value (INT_MAX = none).  Slots, waves and the LDS combine merge (value, id) pairs with better<OP>.
//
// Why the result equals the conversion route's bit for bit, values and positions, on any data: widening is exact, every compare is
// an fp32 compare of the same fp32 candidates, and "strictly better, else the lower edge id" picks the same edge however a row's
// edges are dealt to slots and waves -- the first edge among equal candidates (+0 and -0 are equal), never a NaN.  The finished fp32
// winner is then rounded ONCE, to nearest even, which is what converting the fp32 kernel's output does.  (Packed 16-bit max / min
// instructions order +-0 and NaN differently and are not used.)
//
// z_arg == NULL runs the values-only instances: no id registers, selects or stores.  Without ids a slot still keeps its own first
// edge among equals (its edges come in ascending order), and equal candidates have equal bits except +0 / -0: only a cross-slot tie
// of +0 against -0 needs to know which came first.  The butterfly marks such elements, and a marked element whose result is zero is
// settled by mm16_first_zero, a walk along the wave's edges up to the first zero candidate -- a path real data hardly ever takes.
//
// No atomics: two launches give equal bits, and any row order gives the bits of index order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"
#include "half16.h"
#include "rows16_common.h"

namespace isplib {

struct Rows16MMArgs {
   int64_t m, k, nnz;
   const float *val;            // fp32 weights; null = unit weights
   const int64_t *indx, *pntrb, *pntre;
   const void *y;               // n x ldy elements of 2 bytes
   int64_t ldy;
   unsigned short *z;           // m x ldz
   int64_t ldz;
   int64_t *z_arg;              // m x ldarg CSR positions; null = values only
   int64_t ldarg;
   int empty_init;              // an empty row holds the identity (-+FLT_MAX, rounded: -+Inf) instead of 0
   int long_row;                // rows with more edges are split across the workgroup
   unsigned nblk;               // number of row blocks
   unsigned ybytes;             // n*ldy*2: the descriptor's size
   const int32_t *row_order;    // position -> row, null = the identity
};

// gathers issued back to back per slot, and the occupancy the allocator is held to: 8 waves per SIMD (64 VGPRs) for every
// single-chunk kernel, as in spmm_rows16.hip.  A chunk's state is 8 values + 8 ids where the fp32 kernel has 4 + 4 and the 16-bit sum
// kernel 8 sums, a gather in flight is four VGPRs and a weighted step keeps its weights: the deepest step of each form that the
// compiler fits into 64 VGPRs WITHOUT scratch (one deeper spills 12-76 bytes per lane; DESIGN.md 4.2b has the counts)
template <bool HAS_VAL, bool ARG, int NCH> constexpr int mm16_unroll() {
   if (NCH > 1) return 2;
   if (ARG) return HAS_VAL ? 2 : 3;
   return HAS_VAL ? 3 : 6;
}
template <int NCH> constexpr int mm16_min_blocks() { return NCH == 1 ? 8 : 1; }

// buf_step's max / min branch (gather.h) at eight 16-bit columns per 16-byte gather: UU gathers per slot back to back for the
// edges [s, s + G*UU) of the current 64-edge batch, consumed in ascending edge order.  TAIL: the step may pass the end of the batch
// (edges >= cnt read zeros past the descriptor and must not compete); a full step needs no such test
template <int ELT, int OP, bool HAS_VAL, bool ARG, bool TAIL, int LPR, int NCH, int UU>
__device__ __forceinline__ void mm16_step(const __amdgpu_buffer_rsrc_t rsrc, unsigned off_l, float v_l, int s, int cnt, int rel0, int g,
                                          const unsigned (&cbyte)[NCH], const unsigned (&poison)[NCH], float (&acc)[NCH][8],
                                          int (&bi)[NCH][ARG ? 8 : 1]) {
   constexpr int G = 64 / LPR;
   v4i_t t[UU][NCH];
   float vv[UU];
#pragma unroll
   for (int u = 0; u < UU; u++) {
      const int ei = (s + u * G + g) & 63;
      const unsigned off = (unsigned)__shfl((int)off_l, ei);
      if (HAS_VAL) vv[u] = __shfl(v_l, ei);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         // masked edge: off = BUF_OOB, + cbyte (< 2^25) cannot wrap; masked column: OR-ed past the limit
         const unsigned o = (off + cbyte[j]) | poison[j];
         t[u][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
      }
   }
#pragma unroll
   for (int u = 0; u < UU; u++) {
      const int ei = s + u * G + g;
      const bool ok = !TAIL || ei < cnt;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
         for (int q = 0; q < 4; q++) {
            float x[2];
            widen2<ELT>((unsigned)t[u][j][q], x[0], x[1]);
#pragma unroll
            for (int h = 0; h < 2; h++) {
               const int v = 2 * q + h;
               const float tt = HAS_VAL ? vv[u] * x[h] : x[h];
               const bool win = ok && (OP == OP_MAX ? tt > acc[j][v] : tt < acc[j][v]);
               acc[j][v] = win ? tt : acc[j][v];
               if (ARG) bi[j][v] = win ? rel0 + ei : bi[j][v];
            }
         }
      }
   }
}

// one wave's edges [rb, re) of a row that starts at CSR position row_b, on rows16_batches (rows16_common.h): mm16_step per step
template <int ELT, int OP, bool HAS_VAL, bool ARG, int LPR, int NCH, int U>
__device__ __forceinline__ void mm16_edges(const Rows16MMArgs &a, const __amdgpu_buffer_rsrc_t rsrc, int64_t row_b, int64_t rb, int64_t re,
                                           const int (&ccol)[NCH], const bool (&cok)[NCH], float (&acc)[NCH][8],
                                           int (&bi)[NCH][ARG ? 8 : 1]) {
   rows16_batches<LPR, NCH, U>(
      a, rb, re, ccol, cok, [&](int64_t p) { return HAS_VAL ? a.val[p] : 0.0f; },
      [&](auto uu, auto tail, unsigned off_l, float v_l, int s, int cnt, int64_t base, int g, const unsigned (&cbyte)[NCH],
          const unsigned (&poison)[NCH]) {
         mm16_step<ELT, OP, HAS_VAL, ARG, decltype(tail)::value, LPR, NCH, decltype(uu)::value>(rsrc, off_l, v_l, s, cnt, (int)(base - row_b), g, cbyte,
                                                                                               poison, acc, bi);
      });
}

// the values-only butterfly over the 64 / LPR edge slots: the strictly better value.  Equal values have equal bits unless they are
// +0 and -0; such a tie is marked in `amb` (bit j * 8 + v; the marks of both partners travel on), because without ids nobody knows
// which of the two came first
template <int OP, int LPR, int NCH>
__device__ __forceinline__ unsigned mm16_slot_reduce_values(float (&acc)[NCH][8]) {
   unsigned amb = 0u;
#pragma unroll
   for (int off = LPR; off < 64; off <<= 1) {
      amb |= (unsigned)__shfl_xor((int)amb, off);
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
         for (int v = 0; v < 8; v++) {
            const float ot = __shfl_xor(acc[j][v], off);
            const bool take = OP == OP_MAX ? ot > acc[j][v] : ot < acc[j][v];
            if (ot == acc[j][v] && __float_as_uint(ot) != __float_as_uint(acc[j][v])) amb |= 1u << (j * 8 + v);
            acc[j][v] = take ? ot : acc[j][v];
         }
      }
   }
   return amb;
}

// settles the marked elements of the g == 0 lanes whose result is zero: the winner is the FIRST zero candidate among the wave's edges
// [rb, re) (every candidate before it lost to it or was NaN, none after it is strictly better), found by walking them in order with
// the main loop's own arithmetic.  The whole wave walks (the trip count is wave-uniform); lanes with nothing to settle only ride along
template <int ELT, bool HAS_VAL, int NCH>
__device__ __forceinline__ void mm16_first_zero(const Rows16MMArgs &a, const __amdgpu_buffer_rsrc_t rsrc, int64_t rb, int64_t re,
                                             const int (&ccol)[NCH], const bool (&cok)[NCH], unsigned pend, float (&acc)[NCH][8]) {
   const unsigned ldyb = (unsigned)a.ldy * 2u;
   for (int64_t p = rb; p < re && __any((int)(pend != 0u)); p++) {
      const unsigned off = (unsigned)a.indx[p] * ldyb;
      const float w = HAS_VAL ? a.val[p] : 1.0f;
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const unsigned o = (off + (unsigned)ccol[j] * 2u) | (cok[j] ? 0u : BUF_OOB);
         const v4i_t t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
#pragma unroll
         for (int q = 0; q < 4; q++) {
            float x[2];
            widen2<ELT>((unsigned)t[q], x[0], x[1]);
#pragma unroll
            for (int h = 0; h < 2; h++) {
               const unsigned bit = 1u << (j * 8 + 2 * q + h);
               const float tt = HAS_VAL ? w * x[h] : x[h];
               if ((pend & bit) != 0u && tt == 0.0f) {
                  acc[j][2 * q + h] = tt;
                  pend &= ~bit;
               }
            }
         }
      }
   }
}

// the cross-slot reduction of a wave's edges [rb, re); afterwards the g == 0 lanes hold the wave's (value, id) pairs
template <int ELT, int OP, bool HAS_VAL, bool ARG, int LPR, int NCH>
__device__ __forceinline__ void mm16_slots(const Rows16MMArgs &a, const __amdgpu_buffer_rsrc_t rsrc, int64_t rb, int64_t re, int g,
                                           const int (&ccol)[NCH], const bool (&cok)[NCH], float (&acc)[NCH][8],
                                           int (&bi)[NCH][ARG ? 8 : 1]) {
   if constexpr (ARG) {
      slot_reduce<OP, 8, LPR, NCH>(acc, bi);
   } else if constexpr (LPR < 64) {
      unsigned pend = mm16_slot_reduce_values<OP, LPR, NCH>(acc);
      unsigned zero = 0u;
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 8; v++) zero |= (cok[j] && acc[j][v] == 0.0f) ? 1u << (j * 8 + v) : 0u;
      pend = g == 0 ? (pend & zero) : 0u;
      if (__any((int)(pend != 0u))) mm16_first_zero<ELT, HAS_VAL, NCH>(a, rsrc, rb, re, ccol, cok, pend, acc);
   }
}

// the finished fp32 winners of the g == 0 lanes: the empty row's value, rounded once and stored; positions as CSR positions
template <int ELT, int OP, bool ARG, int NCH>
__device__ __forceinline__ void mm16_write(const Rows16MMArgs &a, int64_t row, int64_t row_b, int64_t deg, const int (&ccol)[NCH],
                                           const bool (&cok)[NCH], const int (&vfirst)[NCH], float (&acc)[NCH][8],
                                           const int (&bi)[NCH][ARG ? 8 : 1]) {
   unsigned short *zr = a.z + (size_t)row * (size_t)a.ldz;
   if (deg <= 0) {
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = a.empty_init ? identity<OP>() : 0.0f;
   }
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (!cok[j]) continue;
      store_tail16x8<ELT>(zr + ccol[j], acc[j], vfirst[j]);
      if constexpr (ARG) {
         int64_t *ar = a.z_arg + (size_t)row * (size_t)a.ldarg + ccol[j];
         int64_t pos[8];
#pragma unroll
         for (int v = 0; v < 8; v++) pos[v] = bi[j][v] == INT_MAX ? a.nnz : row_b + (int64_t)bi[j][v];
         if (vfirst[j] == 0 && ((uintptr_t)ar & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 4; q++) reinterpret_cast<longlong2 *>(ar)[q] = make_longlong2(pos[2 * q], pos[2 * q + 1]);
         } else {
#pragma unroll
            for (int v = 0; v < 8; v++)
               if (v >= vfirst[j]) ar[v] = pos[v];
         }
      }
   }
}

template <int ELT, int OP, bool HAS_VAL, bool ARG, int LPR, int NCH, int WAVES>
__global__ __launch_bounds__(WAVES * 64, (mm16_min_blocks<NCH>())) void spmm_rows16_minmax_kernel(const Rows16MMArgs a) {
   constexpr int U = mm16_unroll<HAS_VAL, ARG, NCH>();
   constexpr int PANEL = LPR * 8 * NCH;     // columns covered by one grid.y panel
   constexpr int NB = ARG ? 8 : 1;
   __shared__ float sh_val[WAVES][PANEL];
   __shared__ int sh_idx[ARG ? WAVES : 1][ARG ? PANEL : 1];

   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   __amdgpu_buffer_rsrc_t rsrc = rows16_desc(a.y, a.ybytes);

   const unsigned lb = rows16_block(a.nblk);
   int ccol[NCH], vfirst[NCH];
   bool cok[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) ccol[j] = rows16_column((int)blockIdx.y * PANEL + (j * LPR + lc) * 8, a.k, cok[j], vfirst[j]);

   const int64_t row0 = (int64_t)lb * WAVES;
   const int64_t row = (a.row_order && row0 + wave < a.m) ? (int64_t)a.row_order[row0 + wave] : row0 + wave;

   // phase 1: one row per wave (rows up to long_row edges)
   if (row0 + wave < a.m) {
      const int64_t b = a.pntrb[row], e = a.pntre[row];
      const int64_t deg = e - b;
      if (deg <= a.long_row) {
         float acc[NCH][8];
         int bi[NCH][NB];
#pragma unroll
         for (int j = 0; j < NCH; j++) {
#pragma unroll
            for (int v = 0; v < 8; v++) acc[j][v] = identity<OP>();
#pragma unroll
            for (int v = 0; v < NB; v++) bi[j][v] = INT_MAX;
         }
         mm16_edges<ELT, OP, HAS_VAL, ARG, LPR, NCH, U>(a, rsrc, b, b, e, ccol, cok, acc, bi);
         mm16_slots<ELT, OP, HAS_VAL, ARG, LPR, NCH>(a, rsrc, b, e, g, ccol, cok, acc, bi);
         if (g == 0) mm16_write<ELT, OP, ARG, NCH>(a, row, b, deg, ccol, cok, vfirst, acc, bi);
      }
   }

   // phase 2: long rows of this block, all waves on one row at a time (contiguous edge chunks in wave order, LDS combine with
   // better<OP> in wave order; values only: the strictly better value, so among equals the earlier chunk's stays)
   for (int r = 0; r < WAVES; r++) {
      if (row0 + r >= a.m) break;                  // uniform over the block
      const int64_t lr = a.row_order ? (int64_t)a.row_order[row0 + r] : row0 + r;
      const int64_t b = a.pntrb[lr], e = a.pntre[lr];
      const int64_t deg = e - b;
      if (deg <= a.long_row) continue;             // uniform over the block
      int64_t cb, ce;
      rows16_chunk(b, e, wave, cb, ce);
      float acc[NCH][8];
      int bi[NCH][NB];
#pragma unroll
      for (int j = 0; j < NCH; j++) {
#pragma unroll
         for (int v = 0; v < 8; v++) acc[j][v] = identity<OP>();
#pragma unroll
         for (int v = 0; v < NB; v++) bi[j][v] = INT_MAX;
      }
      mm16_edges<ELT, OP, HAS_VAL, ARG, LPR, NCH, U>(a, rsrc, b, cb, ce, ccol, cok, acc, bi);
      mm16_slots<ELT, OP, HAS_VAL, ARG, LPR, NCH>(a, rsrc, cb, ce, g, ccol, cok, acc, bi);
      if (g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) {
               sh_val[wave][(j * LPR + lc) * 8 + v] = acc[j][v];
               if constexpr (ARG) sh_idx[wave][(j * LPR + lc) * 8 + v] = bi[j][v];
            }
      }
      __syncthreads();
      if (wave == 0 && g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < 8; v++) {
               const int o = (j * LPR + lc) * 8 + v;
               float t = sh_val[0][o];
               int ti = ARG ? sh_idx[0][o] : 0;
               for (int w = 1; w < WAVES; w++) {
                  const float ot = sh_val[w][o];
                  if constexpr (ARG) {
                     const int oi = sh_idx[w][o];
                     if (better<OP>(ot, oi, t, ti)) { t = ot; ti = oi; }
                  } else {
                     if (OP == OP_MAX ? ot > t : ot < t) t = ot;
                  }
               }
               acc[j][v] = t;
               if constexpr (ARG) bi[j][v] = ti;
            }
         mm16_write<ELT, OP, ARG, NCH>(a, lr, b, deg, ccol, cok, vfirst, acc, bi);
      }
      __syncthreads();
   }
}

template <int ELT, int OP, bool HAS_VAL, bool ARG>
static int launch_mm16_width(const Rows16MMArgs &a, hipStream_t st) {
   return rows16_by_width(a.k, [&](auto lpr, auto nch) {
      constexpr int LPR = decltype(lpr)::value, NCH = decltype(nch)::value;
      return rows16_launch<LPR, NCH>("fusedMM_csr_rows16_minmax_hip", "spmm_rows16_minmax_kernel",
                                     spmm_rows16_minmax_kernel<ELT, OP, HAS_VAL, ARG, LPR, NCH, ROWS16_WAVES>, a, st);
   });
}

template <int ELT, int OP>
static int launch_mm16(const Rows16MMArgs &a, hipStream_t st) {
   if (a.z_arg) return a.val ? launch_mm16_width<ELT, OP, true, true>(a, st) : launch_mm16_width<ELT, OP, false, true>(a, st);
   return a.val ? launch_mm16_width<ELT, OP, true, false>(a, st) : launch_mm16_width<ELT, OP, false, false>(a, st);
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_rows16_minmax_auto(int64_t n, int64_t ldy, int ordered, int weighted, int want_arg) {
   return isplib_rows16_minmax_native_pays(n, ldy, ordered, weighted, want_arg);
}

extern "C" int fusedMM_csr_rows16_minmax_hip(int32_t imessage, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                                             const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order,
                                             const void *y, int64_t ldy, void *z, int64_t ldz, int64_t *z_arg, int64_t ldarg,
                                             void *stream) {
   Rows16MMArgs a;
   bool run;
   const int rc = rows16_check("fusedMM_csr_rows16_minmax_hip", imessage == ISPLIB_MSG_SPMM_MAX || imessage == ISPLIB_MSG_SPMM_MIN,
                               "max and min only (sum / mean of a 16-bit operand: fusedMM_csr_rows16_hip)", !z_arg || ldarg >= k, false, dtype, m,
                               n, k, nnz, val, indx, pntrb, pntre, row_order, y, ldy, z, ldz, a, &run);
   if (!run) return rc;
   a.nnz = nnz;
   a.z_arg = z_arg; a.ldarg = ldarg;
   a.empty_init = empty_row_init();
   hipStream_t st = (hipStream_t)stream;
   const bool mx = imessage == ISPLIB_MSG_SPMM_MAX;
   if (dtype == ISPLIB_DTYPE_BF16) return mx ? launch_mm16<ELT_BF16, OP_MAX>(a, st) : launch_mm16<ELT_BF16, OP_MIN>(a, st);
   return mx ? launch_mm16<ELT_F16, OP_MAX>(a, st) : launch_mm16<ELT_F16, OP_MIN>(a, st);
}
