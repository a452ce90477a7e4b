// attn_common.h -- what the fp32 attention families (attention.hip: row softmax; gat.hip, gatv2.hip, mha.hip: multi-head, with their
// EDGE / DROP forms) decide alike, written once.  DESIGN.md 4.6n states the mapping: one wave per row, G = 64 / LPR edge slots, a lane
// holds NCH chunks of 4 consecutive columns (column (j * LPR + lc) * 4 of chunk j), one head is summed by a DPP / ds_bpermute butterfly
// over its `hlanes` lanes, dead edges and columns past k carry BUF_OOB, which every descriptor answers with 0.
//   host    attn_extent         what a descriptor over a row-strided view may answer
//           attn_head_geometry  hshift / hlanes / hmask / whole of a launch
//           AttnDrop            the dropout of one call, attn_drop_refusal, attn_set_drop
//           attn_by_width       the width ladder: (LPR, NCH) by k
//   device  AttnHeadCols        the <LPR, NCH> column map: cbyte, poison, hbyte, head, ok, first
//           attn_rsrc           the descriptor of a gathered table
//           attn_off            the byte offset of an edge's gathered row; a dead edge: BUF_OOB
//           attn_own_row / attn_store_row    a lane's columns of the wave's own row, plain loads / stores
//           attn_own_head       a lane's entries of the wave's own row of a [rows, H] table
//           attn_load_wide / attn_load_head  the gathers: 16 bytes per chunk / the chunk's head of a [., H] table
//           attn_head_sum / attn_head_reduce the N-wide butterfly over a head / the P x NCH dot products of a step through it
//           attn_dot_part       a lane's part of <r, t>_h for one chunk
//           attn_drop_heads     DROP: the per-lane constant of each chunk's head (gat_dropout.h)
// The helpers take the scalars they need (k, hshift, hmask, whole, hlanes, seed_hi), never a kernel's argument struct: the structs,
// their field order, the kernels and their template parameters are the families' own.  What stays in the kernel files, and why:
//   attention.hip  has no heads: it keeps its column map (AttnCols) and attn_gather / attn_dot, which reduce a whole slot by the
//                  transposed butterfly of gather.h; it takes attn_extent, attn_by_width, attn_rsrc and attn_own_row
//   gat.hip        gat_head_sum / gat_head_dot (one scalar through the butterfly: the score is a table lookup, only t_e is a dot
//                  product), gat_edge (both offsets of an edge from one shuffle), gat_rsrc_uniform (the per-batch a_edge window),
//                  gat_drop_ok (its entries refuse a bad scale ahead of everything else, in words of their own)
//   every family   its constants (*_NONE, *_WAVES, the U choices), its score (gat_score*, gatv2_leaky / gatv2_score_part), the stores
//                  that finish a row while they write it, the per-wave and per-batch preambles, and the pairwise merge of the G slots
//                  at the end of a row (online softmax in a forward kernel, plain sums in a backward one): each kernel merges a state
//                  of its own shape, and with one helper per form (here and in attn16_common.h) 62 of the 277 kernels, forward
//                  kernels of every family among them, compiled to other instruction orders and register counts
//   gat.hip, too   gat_head_sum through attn_head_sum: the N-wide form walks both chunks of a lane through a level together, gat.hip's
//                  adds chunk after chunk; its 24 two-chunk kernels compiled to other listings
// scripts/rows16_isa_table.py is the check to repeat after a change here; profiles/attn_common_isa.txt is its table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cfloat>
#include <type_traits>

#include "common.h"
#include "gather.h"
#include "gat_dropout.h"

namespace isplib {

template <int V> using attn_int = std::integral_constant<int, V>;

// what a descriptor over `rows` rows of k floats at pitch ld may answer: the extent a row-strided view owns, not rows * ld (the last
// row of the last head view of a wider tensor ends with the tensor)
static unsigned attn_extent(int64_t rows, int64_t k, int64_t ld) {
   return rows <= 0 ? 0u : (unsigned)(((unsigned long long)(rows - 1) * (unsigned long long)ld + (unsigned long long)k) * 4ull);
}

// the head geometry of a launch; the family's domain has been checked: H == 1, or d a power of two >= 4
//    hshift: head of column c = c >> hshift (H == 1: 31, every column is head 0)      hlanes: lanes of one chunk that share a head, d / 4
//    hmask:  c & hmask == 0 opens a head (H == 1: only column 0)                      whole:  H == 1, the head spans both chunks of a lane
static void attn_head_geometry(int64_t heads, int64_t d, int &nheads, int &hshift, int &hlanes, unsigned &hmask, int &whole) {
   nheads = (int)heads;
   if (heads == 1) {
      hshift = 31; hlanes = 64; hmask = 0x7fffffffu; whole = 1;
   } else {
      int sh = 0;
      while ((1LL << sh) < d) sh++;
      hshift = sh; hlanes = (int)(d / 4); hmask = (unsigned)(d - 1); whole = 0;
   }
}

// the dropout of one call: the threshold T(p), c = float32(1 / (1 - p)) and the seed; none: the entries without it
struct AttnDrop {
   bool on;
   uint32_t threshold;
   float keep_scale;
   uint64_t seed;
};
static const AttnDrop ATTN_NO_DROP = {false, 0u, 1.0f, 0ull};

// what the dropout entries refuse before a launch: a keep scale that is no positive finite number would poison every row (`bad_scale`:
// the entry's words for it), and the keep bit is a function of a position below 2^31
static const char *attn_drop_refusal(const AttnDrop &dr, int64_t nnz, const char *bad_scale) {
   if (!dr.on) return nullptr;
   if (!(dr.keep_scale > 0.0f && dr.keep_scale <= FLT_MAX)) return bad_scale;
   if (nnz >= (1LL << 31)) return "nnz must be below 2^31";
   return nullptr;
}

static void attn_set_drop(const AttnDrop &dr, unsigned &seed_lo, unsigned &seed_hi, unsigned &T, float &c) {
   seed_lo = (unsigned)dr.seed; seed_hi = (unsigned)(dr.seed >> 32); T = dr.threshold; c = dr.keep_scale;
}

// slot width by ceil(k / 4) 16-byte vectors per row: 8 / 4 / 2 / 1 rows per gather instruction up to 32 / 64 / 128 / 256 columns, two
// chunks per lane beyond.  f(LPR, NCH) takes both as attn_int constants
template <class F> static int attn_by_width(int64_t k, F f) {
   const int64_t w = (k + 3) / 4;
   if (w <= 8) return f(attn_int<8>(), attn_int<1>());
   if (w <= 16) return f(attn_int<16>(), attn_int<1>());
   if (w <= 32) return f(attn_int<32>(), attn_int<1>());
   if (w <= 64) return f(attn_int<64>(), attn_int<1>());
   return f(attn_int<64>(), attn_int<2>());
}

template <int LPR, int NCH> struct AttnHeadCols {
   unsigned cbyte[NCH], poison[NCH];       // this lane's 4 consecutive columns per chunk; past k: an offset the descriptor answers with 0
   unsigned hbyte[NCH];                    // byte offset of the chunk's head inside a row of a [., H] table
   int head[NCH];
   bool ok[NCH][4], first[NCH];            // first: this lane's chunk opens a head (and lies inside k)
   // the three kernel arguments by reference: each is read where it is used, as the families' own maps read them; taken by value,
   // the rows kernels of gat.hip and gatv2.hip compile to other instruction orders
   __device__ __forceinline__ AttnHeadCols(const int64_t &k, const int &hshift, const unsigned &hmask, int lc) {
#pragma unroll
      for (int j = 0; j < NCH; j++) {
         const int c = (j * LPR + lc) * 4;
         cbyte[j] = (unsigned)c * 4u;
         poison[j] = c < (int)k ? 0u : BUF_OOB;
         head[j] = c >> hshift;
         hbyte[j] = (unsigned)head[j] * 4u;
         first[j] = c < (int)k && ((unsigned)c & hmask) == 0u;
#pragma unroll
         for (int v = 0; v < 4; v++) ok[j][v] = c + v < (int)k;
      }
   }
};

// a gathered table behind a descriptor of exactly the extent it owns (attn_extent): a read past it returns zeros
__device__ __forceinline__ __amdgpu_buffer_rsrc_t attn_rsrc(const float *p, unsigned bytes) {
   return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p), 0, (int)bytes, 0x00020000);
}

// byte offset of the gathered row of edge `id` of the batch; a dead edge: -1
__device__ __forceinline__ unsigned attn_off(int id, unsigned pitch_bytes) {
   return id < 0 ? BUF_OOB : (unsigned)id * pitch_bytes;     // BUF_OOB + cbyte / hbyte (< 2^24) cannot wrap
}

// this lane's columns of row `row` of a dense operand; plain loads, nothing outside the row's k columns is read
template <int LPR, int NCH>
__device__ __forceinline__ void attn_own_row(const float *base, int64_t row, int64_t ld, int lc, const bool (&ok)[NCH][4], float (&r)[NCH][4]) {
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++) r[j][v] = ok[j][v] ? base[(size_t)row * (size_t)ld + (size_t)((j * LPR + lc) * 4 + v)] : 0.0f;
}

// this lane's columns of a row, stored; nothing outside the row's k columns is written
template <int LPR, int NCH>
__device__ __forceinline__ void attn_store_row(float *base, int64_t row, int64_t ld, int lc, const bool (&ok)[NCH][4], const float (&r)[NCH][4]) {
#pragma unroll
   for (int j = 0; j < NCH; j++)
#pragma unroll
      for (int v = 0; v < 4; v++)
         if (ok[j][v]) base[(size_t)row * (size_t)ld + (size_t)((j * LPR + lc) * 4 + v)] = r[j][v];
}

// entry [row, head of chunk j] of a dense [rows, H] table, per chunk; a chunk past k reads nothing
template <int LPR, int NCH>
__device__ __forceinline__ void attn_own_head(const float *base, int64_t row, int heads, const AttnHeadCols<LPR, NCH> &cm, float (&r)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) r[j] = cm.ok[j][0] ? base[(size_t)row * (size_t)heads + (size_t)cm.head[j]] : 0.0f;
}

template <int LPR, int NCH>
__device__ __forceinline__ void attn_load_wide(const __amdgpu_buffer_rsrc_t rsrc, unsigned off, const AttnHeadCols<LPR, NCH> &cm, v4i_t (&t)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) t[j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)((off + cm.cbyte[j]) | cm.poison[j]), 0, 0);
}

template <int LPR, int NCH>
__device__ __forceinline__ void attn_load_head(const __amdgpu_buffer_rsrc_t rsrc, unsigned offh, const AttnHeadCols<LPR, NCH> &cm, float (&t)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++)
      t[j] = __int_as_float((int)__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)((offh + cm.hbyte[j]) | cm.poison[j]), 0, 0));
}

// N sums over the lanes that share a head (an aligned group of `hlanes` lanes, a power of two <= LPR), level by level together; every
// lane of the group ends with the same bits (each level adds the same two numbers on both sides).  Partners 1, 2, 4, 8 by DPP moves
// inside the 16-lane row (gather.h), wider ones by ds_bpermute.
template <int LPR, int N, int O = 1> __device__ __forceinline__ void attn_head_sum(float (&v)[N], int hlanes) {
   if constexpr (O < LPR) {
      float w[N];
#pragma unroll
      for (int i = 0; i < N; i++) w[i] = lane_xor<O>(v[i]);
#pragma unroll
      for (int i = 0; i < N; i++) v[i] = O < hlanes ? v[i] + w[i] : v[i];
      attn_head_sum<LPR, N, 2 * O>(v, hlanes);
   }
}

// the per-lane parts p[.][chunk] of P dot products per head -> the dot products, in every lane of the head (both chunks where the head
// is the whole row)
template <int LPR, int NCH, int P>
__device__ __forceinline__ void attn_head_reduce(float (&p)[P][NCH], int whole, int hlanes) {
   if (NCH == 2 && whole) {
      float w[P];
#pragma unroll
      for (int i = 0; i < P; i++) w[i] = p[i][0] + p[i][NCH - 1];
      attn_head_sum<LPR, P>(w, hlanes);
#pragma unroll
      for (int i = 0; i < P; i++) p[i][0] = p[i][NCH - 1] = w[i];
   } else {
      float w[P * NCH];
#pragma unroll
      for (int i = 0; i < P; i++)
#pragma unroll
         for (int j = 0; j < NCH; j++) w[i * NCH + j] = p[i][j];
      attn_head_sum<LPR, P * NCH>(w, hlanes);
#pragma unroll
      for (int i = 0; i < P; i++)
#pragma unroll
         for (int j = 0; j < NCH; j++) p[i][j] = w[i * NCH + j];
   }
}

// this lane's part of <r, t>_h for one chunk; a 16-byte load may run into the next row, the mask drops what it brought
__device__ __forceinline__ float attn_dot_part(const float (&r)[4], const v4i_t &t, const bool (&ok)[4]) {
   float p = 0.0f;
#pragma unroll
   for (int v = 0; v < 4; v++) p = fmaf(r[v], ok[v] ? __int_as_float(t[v]) : 0.0f, p);
   return p;
}

// DROP: the per-lane constant of each chunk's head (gat_dropout.h)
template <int LPR, int NCH>
__device__ __forceinline__ void attn_drop_heads(unsigned seed_hi, const AttnHeadCols<LPR, NCH> &cm, unsigned (&hk)[NCH]) {
#pragma unroll
   for (int j = 0; j < NCH; j++) hk[j] = gat_drop_head(seed_hi, (unsigned)cm.head[j]);
}

}  // namespace isplib
