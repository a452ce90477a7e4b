// half16.h -- the two conversions every kernel of 16-bit dense operands (bf16, fp16) shares: a gathered dword widened to two
// floats, and two finished floats rounded once, to nearest even, into a dword (spmm_stream16.hip, spmm_rows16.hip,
// spmm_rows16_minmax.hip); and the row kernels' store of a lane's eight finished columns.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isplib_hip.h"

namespace isplib {

enum { ELT_BF16 = ISPLIB_DTYPE_BF16, ELT_F16 = ISPLIB_DTYPE_F16 };

// two 16-bit elements of a gathered dword as floats (lo: the lower address).  bf16 is the top half of an fp32: a shift and a mask
template <int ELT> __device__ __forceinline__ void widen2(unsigned w, float &lo, float &hi) {
   if (ELT == ELT_BF16) {
      lo = __uint_as_float(w << 16);
      hi = __uint_as_float(w & 0xFFFF0000u);
   } else {
      lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xFFFFu));
      hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16));
   }
}

// two finished floats as one dword of two 16-bit elements, round to nearest even (the casts: v_cvt_pk_bf16_f32 / v_cvt_f16_f32 in
// the default rounding mode -- not the packed fp16 conversion, which rounds towards zero)
template <int ELT> __device__ __forceinline__ unsigned narrow2(float lo, float hi) {
   unsigned short a, b;
   if (ELT == ELT_BF16) {
      a = __builtin_bit_cast(unsigned short, (__bf16)lo);
      b = __builtin_bit_cast(unsigned short, (__bf16)hi);
   } else {
      a = __builtin_bit_cast(unsigned short, (_Float16)lo);
      b = __builtin_bit_cast(unsigned short, (_Float16)hi);
   }
   return (unsigned)a | ((unsigned)b << 16);
}

// the eight finished columns of a lane as 16 bytes at p (4-byte aligned: k, the pitch and the columns are even); the first `vfirst`
// components (even) belong to the neighbouring lane -- the last vector of a row is shifted back to end at column k -- and are skipped
template <int ELT> __device__ __forceinline__ void store_tail16x8(unsigned short *p, const float (&r)[8], int vfirst) {
   unsigned d[4];
#pragma unroll
   for (int q = 0; q < 4; q++) d[q] = narrow2<ELT>(r[2 * q], r[2 * q + 1]);
   if (vfirst == 0 && ((uintptr_t)p & 15) == 0) {
      *reinterpret_cast<uint4 *>(p) = make_uint4(d[0], d[1], d[2], d[3]);
   } else {
#pragma unroll
      for (int q = 0; q < 4; q++)
         if (2 * q >= vfirst) reinterpret_cast<unsigned *>(p)[q] = d[q];
   }
}

}  // namespace isplib
