// rows16_sum.h -- the edge step of the 16-bit row kernels that SUM (spmm_rows16.hip: sum / mean; spmm_rows16_epilogue.hip: the sum
// with an epilogue on the finished row), with the weight modes and the unroll / occupancy both kernels are held to.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gather.h"
#include "half16.h"

namespace isplib {

enum { W_UNIT = 0, W_EDGE = 1, W_COL = 2 };

// gathers issued back to back per slot, and the occupancy the allocator is held to -- the fp32 plain kernel's 8 waves per SIMD
// (gather.h, min_waves_of).  Four VGPRs per gather in flight as there, but eight accumulators per chunk instead of four and eight
// widened values: at U = 8 the unit-weight bf16 kernels spill (12-28 bytes of scratch per lane), at U = 6 every single-chunk
// kernel fits 64 VGPRs without scratch (DESIGN.md 4.2a has the counts)
template <int NCH> constexpr int rows16_unroll() { return NCH > 1 ? 4 : 6; }
template <int NCH> constexpr int rows16_min_blocks() { return NCH == 1 ? 8 : 1; }

// buf_step (gather.h) at eight 16-bit columns per 16-byte gather: UU gathers per slot back to back for the edges [s, s + G*UU) of
// the current 64-edge batch; their values are summed among themselves first and enter the running sum as ONE term
template <int ELT, bool HAS_VAL, int LPR, int NCH, int UU>
__device__ __forceinline__ void rows16_step(const __amdgpu_buffer_rsrc_t rsrc, unsigned off_l, float v_l, int s, int g,
                                            const unsigned (&cbyte)[NCH], const unsigned (&poison)[NCH], float (&acc)[NCH][8]) {
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
   for (int j = 0; j < NCH; j++) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
         float lo, hi;
         widen2<ELT>((unsigned)t[0][j][q], lo, hi);
         float p0 = HAS_VAL ? vv[0] * lo : lo, p1 = HAS_VAL ? vv[0] * hi : hi;
#pragma unroll
         for (int u = 1; u < UU; u++) {
            widen2<ELT>((unsigned)t[u][j][q], lo, hi);
            p0 = HAS_VAL ? fmaf(vv[u], lo, p0) : p0 + lo;
            p1 = HAS_VAL ? fmaf(vv[u], hi, p1) : p1 + hi;
         }
         acc[j][2 * q] += p0;
         acc[j][2 * q + 1] += p1;
      }
   }
}

}  // namespace isplib
