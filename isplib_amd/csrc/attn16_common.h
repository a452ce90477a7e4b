// attn16_common.h -- what the 16-bit attention families (attention16.hip: row softmax; gat16.hip, gatv2_16.hip, mha16.hip: multi-head;
// bf16 / fp16 operands, fp32 arithmetic) decide alike, written once.  DESIGN.md 4.6n states the mapping: one wave per row, G = 64 / LPR
// edge slots, a lane holds the 8 consecutive columns from lc * 8 (one 16-byte gather, always one chunk), one head is summed by a DPP /
// ds_bpermute butterfly over its `hlanes` lanes, dead edges and lanes past k carry BUF_OOB, which every descriptor answers with 0.
//   host    attn16_extent         what a descriptor over a row-strided view may answer
//           attn16_head_geometry  hshift / hlanes / hmask of a launch
//           attn16_even / attn16_aligned / ATTN16_DTYPE   the pitch and pointer checks of the entries, and the dtype message
//           attn16_run            the dtype dispatch and the width ladder: (ELT, LPR) by dtype and k
//   device  Attn16HeadCols        the column map: col, head, cbyte, hbyte, poison, ok, first
//           attn16_desc           the descriptor of a gathered table
//           attn16_off            the byte offset of an edge's gathered row; a dead edge: BUF_OOB
//           attn16_own_row / attn16_store_row   a lane's columns of the wave's own row, widened / rounded once
//           attn16_own_head       a lane's entry of the wave's own row of an fp32 [rows, H] table
//           attn16_load_wide / attn16_load_head / attn16_widen   the gathers and a gathered vector as eight floats
//           attn16_head_sum       the N-wide butterfly over a head (gat16.hip's single sum is N = 1)
//           attn16_dot_part       a lane's part of <r, t>_h
// The helpers take the scalars they need (k, hshift, hmask, hlanes), never a kernel's argument struct: the structs, their field order,
// the kernels and their template parameters are the families' own.  What stays in the kernel files, and why:
//   attention16.hip  has no heads: it keeps its column map (Attn16Cols) and attn16_gather / attn16_dot, which reduce a whole slot by the
//                    transposed butterfly of gather.h; what it shares takes `col` and `ok`, which both maps hold
//   gat16.hip        gat16_edge (both offsets of an edge from one shuffle) and gat16_head_dot (dot product and sum in one call)
//   every family     its constants (*_NONE, *_WAVES, the U choices, the ISPLIB_MHA16_*_U macros), its score (gat16_score,
//                    gatv2_16_leaky / gatv2_16_score_part, gatv2_16_own_att), the per-wave and per-batch preambles, and the pairwise
//                    merge of the G slots at the end of a row: each kernel merges a state of its own shape, and with one helper for
//                    the online-softmax form the forward kernels of all four files compiled to other listings (attn_common.h)
// scripts/rows16_isa_table.py is the check to repeat after a change here; profiles/attn_common_isa.txt is its table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "common.h"
#include "gather.h"
#include "half16.h"

namespace isplib {

template <int V> using attn16_int = std::integral_constant<int, V>;

// what a descriptor over `rows` rows of k elements of `size` bytes at pitch ld may answer: the extent a row-strided view owns, not
// rows * ld
static unsigned attn16_extent(int64_t rows, int64_t k, int64_t ld, unsigned size) {
   return rows <= 0 ? 0u : (unsigned)(((unsigned long long)(rows - 1) * (unsigned long long)ld + (unsigned long long)k) * size);
}

// the head geometry of a launch; the family's domain has been checked: H == 1, or d a power of two >= 8
//    hshift: head of column c = c >> hshift (H == 1: 31, every column is head 0)      hlanes: lanes that share a head, d / 8
//    hmask:  c & hmask == 0 opens a head (H == 1: only column 0)
static void attn16_head_geometry(int64_t heads, int64_t d, int &nheads, int &hshift, int &hlanes, unsigned &hmask) {
   nheads = (int)heads;
   if (heads == 1) {
      hshift = 31; hlanes = 64; hmask = 0x7fffffffu;
   } else {
      int sh = 0;
      while ((1LL << sh) < d) sh++;
      hshift = sh; hlanes = (int)(d / 8); hmask = (unsigned)(d - 1);
   }
}

static const char *const ATTN16_DTYPE = "dtype must be ISPLIB_DTYPE_BF16 or ISPLIB_DTYPE_F16";

// every pitch even; every operand 4-byte aligned (a null pointer is aligned)
static bool attn16_even(int64_t a, int64_t b, int64_t c = 0, int64_t d = 0) { return ((a | b | c | d) & 1) == 0; }
static bool attn16_aligned(const void *a, const void *b, const void *c = nullptr, const void *d = nullptr, const void *e = nullptr,
                           const void *f = nullptr) {
   return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d | (uintptr_t)e | (uintptr_t)f) & 3) == 0;
}

// the element type by dtype (checked by the entry), then the slot width by ceil(k / 8) 16-byte vectors per row: 16 / 8 / 4 / 2 / 1 rows
// per gather instruction up to 32 / 64 / 128 / 256 / 512 columns, always one chunk per lane.  f(ELT, LPR) takes both as attn16_int
// constants
template <int ELT, class F> static int attn16_by_width(int64_t k, F f) {
   const int64_t w = (k + 7) / 8;
   if (w <= 4) return f(attn16_int<ELT>(), attn16_int<4>());
   if (w <= 8) return f(attn16_int<ELT>(), attn16_int<8>());
   if (w <= 16) return f(attn16_int<ELT>(), attn16_int<16>());
   if (w <= 32) return f(attn16_int<ELT>(), attn16_int<32>());
   return f(attn16_int<ELT>(), attn16_int<64>());
}

template <class F> static int attn16_run(int dtype, int64_t k, F f) {
   return dtype == ISPLIB_DTYPE_BF16 ? attn16_by_width<ELT_BF16>(k, f) : attn16_by_width<ELT_F16>(k, f);
}

// this lane's eight consecutive columns and their head; ok[q]: the dword of columns (2q, 2q + 1) lies inside the row (k is even)
struct Attn16HeadCols {
   int col, head;
   unsigned cbyte, hbyte, poison;            // past k: an offset the descriptors answer with 0
   bool ok[4], first;                        // first: this lane opens a head (and lies inside k)
   // the three kernel arguments by reference: each is read where it is used, as the families' own maps read them
   __device__ __forceinline__ Attn16HeadCols(const int64_t &k, const int &hshift, const unsigned &hmask, int lc) {
      col = lc * 8;
      cbyte = (unsigned)col * 2u;
      poison = col < (int)k ? 0u : BUF_OOB;
      head = col >> hshift;
      hbyte = (unsigned)head * 4u;
      first = col < (int)k && ((unsigned)col & hmask) == 0u;
#pragma unroll
      for (int q = 0; q < 4; q++) ok[q] = col + 2 * q < (int)k;
   }
};

// a gathered table behind a descriptor of exactly the extent it owns (attn16_extent): a read past it returns zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t attn16_desc(const void *p, unsigned bytes) {
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(p), 0, (int)bytes, 0x00020000);
}

// byte offset of the gathered row of edge `id` at a pitch of `pitch_bytes`; a dead edge: BUF_OOB
__device__ __forceinline__ unsigned attn16_off(int id, unsigned pitch_bytes) {
   return id < 0 ? BUF_OOB : (unsigned)id * pitch_bytes;     // BUF_OOB + cbyte / hbyte (< 2^10) cannot wrap
}

// the lane's columns [col, col + 8) of row `row` of a dense 16-bit operand as floats; plain dword loads (base, pitch and column are
// even), nothing outside the row's k columns is read
template <int ELT>
__device__ __forceinline__ void attn16_own_row(const unsigned short *base, int64_t row, int64_t ld, int col, const bool (&ok)[4], float (&r)[8]) {
   const unsigned *p = reinterpret_cast<const unsigned *>(base + (size_t)row * (size_t)ld + (size_t)col);
#pragma unroll
   for (int q = 0; q < 4; q++) {
      unsigned w = 0u;
      if (ok[q]) w = p[q];
      widen2<ELT>(w, r[2 * q], r[2 * q + 1]);
   }
}

// the lane's eight finished columns, rounded once; only the dwords inside the row are written (ok[0]: the lane lies inside k)
template <int ELT>
__device__ __forceinline__ void attn16_store_row(unsigned short *base, int64_t row, int64_t ld, int col, const bool (&ok)[4], const float (&r)[8]) {
   if (!ok[0]) return;
   unsigned *p = reinterpret_cast<unsigned *>(base + (size_t)row * (size_t)ld + (size_t)col);
   unsigned d[4];
#pragma unroll
   for (int q = 0; q < 4; q++) d[q] = narrow2<ELT>(r[2 * q], r[2 * q + 1]);
   if (ok[3] && ((uintptr_t)p & 15) == 0) {
      *reinterpret_cast<uint4 *>(p) = make_uint4(d[0], d[1], d[2], d[3]);
   } else {
#pragma unroll
      for (int q = 0; q < 4; q++)
         if (ok[q]) p[q] = d[q];
   }
}

// entry [row, this lane's head] of a dense fp32 [rows, H] table; a lane past k reads nothing
__device__ __forceinline__ float attn16_own_head(const float *base, int64_t row, int heads, const Attn16HeadCols &cm) {
   return cm.poison == 0u ? base[(size_t)row * (size_t)heads + (size_t)cm.head] : 0.0f;
}

__device__ __forceinline__ v4i_t attn16_load_wide(const __amdgpu_buffer_rsrc_t rsrc, unsigned off, const Attn16HeadCols &cm) {
   return __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((off + cm.cbyte) | cm.poison), 0, 0);
}

__device__ __forceinline__ float attn16_load_head(const __amdgpu_buffer_rsrc_t rsrc, unsigned offh, const Attn16HeadCols &cm) {
   return __int_as_float((int)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)((offh + cm.hbyte) | cm.poison), 0, 0));
}

// a gathered vector as eight floats; a dword the 16-byte load brought from outside the row is dropped by a select, not a multiply
template <int ELT> __device__ __forceinline__ void attn16_widen(const v4i_t &t, const bool (&ok)[4], float (&y)[8]) {
#pragma unroll
   for (int q = 0; q < 4; q++) widen2<ELT>(ok[q] ? (unsigned)t[q] : 0u, y[2 * q], y[2 * q + 1]);
}

// N sums over the lanes that share a head (an aligned group of `hlanes` lanes, a power of two; H == 1: the whole slot), level by level
// together; every lane of the group ends with the same bits (each level adds the same two numbers on both sides).  Partners 1, 2, 4, 8
// by DPP moves inside the 16-lane row (gather.h), wider ones by ds_bpermute.  hlanes == 1: no cross-lane step is taken
template <int LPR, int N, int O = 1> __device__ __forceinline__ void attn16_head_sum(float (&v)[N], int hlanes) {
   if constexpr (O < LPR) {
      float w[N];
#pragma unroll
      for (int i = 0; i < N; i++) w[i] = lane_xor<O>(v[i]);
#pragma unroll
      for (int i = 0; i < N; i++) v[i] = O < hlanes ? v[i] + w[i] : v[i];
      attn16_head_sum<LPR, N, 2 * O>(v, hlanes);
   }
}

// this lane's part of <r, t>_h: one fma chain over its eight columns; a column past k has r = t = 0
__device__ __forceinline__ float attn16_dot_part(const float (&r)[8], const float (&t)[8]) {
   float p = 0.0f;
#pragma unroll
   for (int v = 0; v < 8; v++) p = fmaf(r[v], t[v], p);
   return p;
}

}  // namespace isplib
