// rows16_common.h -- what the 16-bit row kernels (spmm_rows16.hip: sum / mean in three weight modes, spmm_rows16_epilogue.hip: the sum
// with an epilogue on the finished row, spmm_rows16_minmax.hip: max / min with or without positions) decide alike, written once.
// DESIGN.md 4.2a describes the mapping; the summing kernels' edge step is rows16_sum.h.
//   host    rows16_check     the refusals of every entry of the family and the argument fields all its kernels share
//           rows16_by_width  the slot width / chunks per lane by K
//           rows16_launch    the launch geometry and its two refusals
//   device  rows16_desc      the gather descriptor
//           rows16_block     the XCD remap of blockIdx.x
//           rows16_column    a lane's columns of a chunk, with the shifted last vector of a ragged K
//           rows16_chunk     a long row's split into wave chunks
//           rows16_batches   a wave's edges in batches of 64: a lane's byte offset, then the full / tail step ladder
// Each kernel keeps its own two phases (a row per wave; long rows across the workgroup through LDS) around these calls: one walk
// templated over a reduction policy compiled the two-chunk sum kernels to other register counts, and rows16_column is per chunk
// because a helper over all chunks regrouped the kernel-argument loads (scripts/rows16_isa_table.py is the check to repeat after a
// change here; profiles/rows16_frontend_isa.txt is its table).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"

namespace isplib {

constexpr int ROWS16_WAVES = 4;      // rows per workgroup, and the waves a long row is split across

// The shared code is generic over a kernel's argument struct `Args`, which holds under these names
//    int64_t m, k;  const float *val;  const int64_t *indx, *pntrb, *pntre;  const void *y;  int64_t ldy;
//    unsigned short *z;  int64_t ldz;  int long_row;  unsigned nblk, ybytes;  const int32_t *row_order;
// (val: fp32 weights, null = unit; y: n x ldy elements of 2 bytes; z: m x ldz; long_row: rows with more edges are split across the
// workgroup; nblk: row blocks; ybytes: n*ldy*2, the descriptor's size; row_order: position -> row, null = the identity) in an order
// of its own (the order decides how the compiler groups the kernel-argument loads); ROWS16_ARGS_OK states it to the compiler.
#define ROWS16_FIELD(A, f, T) std::is_same<decltype(A::f), T>::value
#define ROWS16_ARGS_OK(A)                                                                                                              \
   (ROWS16_FIELD(A, m, int64_t) && ROWS16_FIELD(A, k, int64_t) && ROWS16_FIELD(A, val, const float *) &&                             \
    ROWS16_FIELD(A, indx, const int64_t *) && ROWS16_FIELD(A, pntrb, const int64_t *) && ROWS16_FIELD(A, pntre, const int64_t *) && \
    ROWS16_FIELD(A, y, const void *) && ROWS16_FIELD(A, ldy, int64_t) && ROWS16_FIELD(A, z, unsigned short *) &&                     \
    ROWS16_FIELD(A, ldz, int64_t) && ROWS16_FIELD(A, long_row, int) && ROWS16_FIELD(A, nblk, unsigned) &&                            \
    ROWS16_FIELD(A, ybytes, unsigned) && ROWS16_FIELD(A, row_order, const int32_t *))

template <int V> using rows16_int = std::integral_constant<int, V>;

// The checks of every entry of the family, in one order, and the common fields of its arguments.  `msg_ok` / `msg_text`: the
// entry's own reductions; `ld_ok`: its further leading dimensions; `null_table`: a column table that is needed and missing.
// *run = false with ISPLIB_SUCCESS: nothing to compute
template <class Args>
inline int rows16_check(const char *entry, bool msg_ok, const char *msg_text, bool ld_ok, bool null_table, int dtype, int64_t m, int64_t n, int64_t k,
                        int64_t nnz, const float *val, const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const int32_t *row_order,
                        const void *y, int64_t ldy, void *z, int64_t ldz, Args &a, bool *run) {
   static_assert(ROWS16_ARGS_OK(Args), "the argument struct of a 16-bit row kernel must hold the family's fields");
   clear_error();
   *run = false;
   if (!msg_ok) return fail(ISPLIB_NO_OPT_IMPL, entry, msg_text);
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, "dtype must be ISPLIB_DTYPE_BF16 or ISPLIB_DTYPE_F16");
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldy < k || ldz < k || !ld_ok) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (!isplib_rows16_serves(n, k, ldy, ldz))
      return fail(ISPLIB_FAIL, entry, "outside isplib_rows16_serves(n, k, ldy, ldz): 8 <= k < 2^24, k / ldy / ldz even, n < 2^31, "
                                      "n*ldy*2 <= 3.5 GiB (convert the operand and use fusedMM_csr_hip)");
   if (row_order && m >= (1LL << 31)) return fail(ISPLIB_FAIL, entry, "m must be < 2^31 (32-bit row order)");
   if (!pntrb || !pntre || !z || (nnz > 0 && (!indx || !y))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (null_table) return fail(ISPLIB_FAIL, entry, "null col_scale (unit weights: fusedMM_csr_rows16_hip with val = NULL)");
   if ((((uintptr_t)y | (uintptr_t)z) & 3) != 0) return fail(ISPLIB_FAIL, entry, "y and z must be 4-byte aligned");
   a.m = m; a.k = k;
   a.val = val; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre;
   a.y = y; a.ldy = ldy; a.z = reinterpret_cast<unsigned short *>(z); a.ldz = ldz;
   a.long_row = 2048;
   a.nblk = 0;
   a.ybytes = (unsigned)((unsigned long long)n * (unsigned long long)ldy * 2ull);      // inside the domain it fits 32 bits
   a.row_order = row_order;
   *run = true;
   return ISPLIB_SUCCESS;
}

// slot width by K (a slot is LPR lanes x 8 columns): 8 / 4 / 2 / 1 rows per gather instruction up to 64 / 128 / 256 / 512 columns,
// two chunks per lane up to 1024, and 1024-column grid.y panels beyond.  f(LPR, NCH) takes both as rows16_int constants
template <class F>
static int rows16_by_width(int64_t k, F f) {
   const int64_t width = (k + 7) / 8;     // 16-byte vectors per row (ragged K: the last one is shifted back)
   if (width <= 8) return f(rows16_int<8>(), rows16_int<1>());
   if (width <= 16) return f(rows16_int<16>(), rows16_int<1>());
   if (width <= 32) return f(rows16_int<32>(), rows16_int<1>());
   if (width <= 64) return f(rows16_int<64>(), rows16_int<1>());
   return f(rows16_int<64>(), rows16_int<2>());
}

// one workgroup of ROWS16_WAVES waves per ROWS16_WAVES positions, one grid.y panel per LPR * 8 * NCH columns
template <int LPR, int NCH, class Args>
static int rows16_launch(const char *entry, const char *kernel_name, void (*kernel)(const Args), Args a, hipStream_t st) {
   constexpr int PANEL = LPR * 8 * NCH;
   const int64_t nb = (a.m + ROWS16_WAVES - 1) / ROWS16_WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many row blocks for one launch");
   a.nblk = (unsigned)nb;
   const int64_t ny = (a.k + PANEL - 1) / PANEL;
   if (ny > 65535) return fail(ISPLIB_FAIL, entry, "too many column panels for one launch");
   hipLaunchKernelGGL(kernel, dim3((unsigned)nb, (unsigned)ny, 1), dim3(ROWS16_WAVES * 64, 1, 1), 0, st, a);
   return check_launch(kernel_name);
}

// the dense operand (or a table) behind a descriptor of `bytes` bytes: a read past it returns zeros (kernel arguments only: wave-uniform)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rows16_desc(const void *p, unsigned bytes) {
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

// XCD-aware remap (spmm_csr_kernel, plain): blocks pb, pb + 8, ... share one XCD, which walks a contiguous range of row blocks
__device__ __forceinline__ unsigned rows16_block(unsigned nb) {
   const unsigned pb = blockIdx.x;
   const unsigned xcd = pb & 7u, within = pb >> 3;
   const unsigned per = nb >> 3, rem = nb & 7u;
   return xcd * per + (xcd < rem ? xcd : rem) + within;
}

// a lane's eight columns of one chunk, nominally from `col`; ragged K (k % 8 != 0): the last 16-byte vector of a row is shifted back
// to end at column k, its first `vfirst` components duplicate the neighbouring lane's work and are not stored.  Returns the first
// column the lane gathers; ok = false: the chunk lies beyond the row
__device__ __forceinline__ int rows16_column(int col, int64_t k, bool &ok, int &vfirst) {
   ok = col < k;
   vfirst = 0;
   if (ok && col + 8 > (int)k) {
      vfirst = col + 8 - (int)k;
      col = (int)k - 8;
   }
   return col;
}

// a long row's edges [b, e) in ROWS16_WAVES contiguous chunks of whole 64-edge batches: wave `wave` takes [cb, ce)
__device__ __forceinline__ void rows16_chunk(int64_t b, int64_t e, int wave, int64_t &cb, int64_t &ce) {
   int64_t chunk = (e - b + ROWS16_WAVES - 1) / ROWS16_WAVES;
   chunk = (chunk + 63) & ~(int64_t)63;
   cb = b + (int64_t)wave * chunk, ce = cb + chunk;
   if (cb > e) cb = e;
   if (ce > e) ce = e;
}

// wave_edges_buf (gather.h) for the family: one wave walks edges [rb, re); edge metadata comes 64 per coalesced load, one 32-bit
// multiply per edge (col * ldy * 2), handed off per step.  weight(p) is the lane's factor of edge p (the caller's source: val[p], a
// table, or nothing); step(UU, TAIL, off_l, v_l, s, cnt, base, g, cbyte, poison) takes UU gathers per slot for the edges
// [s, s + G*UU) of the batch that starts at `base` -- U deep while they fit, then UT deep (TAIL: the step may pass the batch's last
// edge, cnt - 1).  The lane's slot g is handed to the step as a value: captured by reference in the caller's lambda, the lane numbers
// of a step's shuffles are formed ahead of the loop and the unit-weight kernels take ten more VGPRs
template <int LPR, int NCH, int U, class Args, class Weight, class Step>
__device__ __forceinline__ void rows16_batches(const Args &a, int64_t rb, int64_t re, const int (&ccol)[NCH], const bool (&cok)[NCH],
                                               Weight weight, Step step) {
   constexpr int G = 64 / LPR;
   constexpr int UT = U >= 4 ? 2 : 1;   // tail granularity (U is a multiple of UT, so a step never passes edge 63 of its batch)
   static_assert(U % UT == 0 && 64 % (G * UT) == 0, "a tail step must end inside the batch");
   const int lane = threadIdx.x & 63;
   const int g = lane / LPR;
   const unsigned ldyb = (unsigned)a.ldy * 2u;
   unsigned cbyte[NCH], poison[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      cbyte[j] = (unsigned)ccol[j] * 2u;
      poison[j] = cok[j] ? 0u : BUF_OOB;
   }
   for (int64_t base = rb; base < re; base += 64) {
      const int64_t p = base + lane;
      unsigned off_l = BUF_OOB;
      float v_l = 0.0f;
      if (p < re) {
         off_l = (unsigned)a.indx[p] * ldyb;
         v_l = weight(p);
      }
      const int64_t left = re - base;
      const int cnt = left < 64 ? (int)left : 64;
      int s = 0;
      for (; s + G * U <= cnt; s += G * U) step(rows16_int<U>(), std::false_type(), off_l, v_l, s, cnt, base, g, cbyte, poison);
      for (; s < cnt; s += G * UT) step(rows16_int<UT>(), std::true_type(), off_l, v_l, s, cnt, base, g, cbyte, poison);
   }
}

}  // namespace isplib
