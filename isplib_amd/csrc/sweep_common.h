// sweep_common.h -- what the kernels of the row-resident schedules share: the launch arguments, the finish of a row, the
// fold of hub rows' partial rows, the device side of the stream front end, the compile-time geometry and the entries' host side.  Included by spmm_sweep.hip (the stream schedule: the
// default of sum / mean / max / min), fusedmm_stream.hip (the generic FusedMM words on the same front end) and
// experimental/experimental.hip (the sweep, hybrid and stream-SDDMM forms: measured, slower, kept out of the default library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>
#include <type_traits>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"

// geometry of the 64-column stream kernel (compile-time: rows per wave, 64-word batch registers per lane, workgroups per CU)
#ifndef ISPLIB_STREAM_NV4
#define ISPLIB_STREAM_NV4 64
#endif
#ifndef ISPLIB_STREAM_NBW4
#define ISPLIB_STREAM_NBW4 2
#endif
#ifndef ISPLIB_STREAM_WGS4
#define ISPLIB_STREAM_WGS4 2
#endif
// cache-policy bits of the stream kernel's gathers (experiment: sc0 = 1, nt = 2, sc1 = 16; every setting measured no faster)
#ifndef ISPLIB_EXP_GATHER_AUX
#define ISPLIB_EXP_GATHER_AUX 0
#endif
// geometry of the hybrid kernel (hot rows of y in LDS): rows per wave, batch registers, table rows (the last one zero),
// hot-word registers, for 64-column slots (streams = 4) and 32-column slots (streams = 8)
#ifndef ISPLIB_HYB4_NV
#define ISPLIB_HYB4_NV 64
#endif
#ifndef ISPLIB_HYB4_NBW
#define ISPLIB_HYB4_NBW 2
#endif
#ifndef ISPLIB_HYB4_HT
#define ISPLIB_HYB4_HT 128
#endif
#ifndef ISPLIB_HYB4_HWR
#define ISPLIB_HYB4_HWR 4
#endif
#ifndef ISPLIB_HYB8_NV
#define ISPLIB_HYB8_NV 128
#endif
#ifndef ISPLIB_HYB8_NBW
#define ISPLIB_HYB8_NBW 4
#endif
#ifndef ISPLIB_HYB8_HT
#define ISPLIB_HYB8_HT 256
#endif
#ifndef ISPLIB_HYB8_HWR
#define ISPLIB_HYB8_HWR 8
#endif
// the same for the 32-column stream kernel (8-lane slots, k <= 32).  Round 3: 128 rows per wave x 2 workgroups per CU hold
// the Reddit shape's 246 K (virtual) rows in ONE generation of 2,048 waves -- one dispatch per pass instead of two -- with
// 32 gathers in flight per wave: K=32 0.715 ms against 0.813 with 64 rows / 16 in flight / 3 workgroups per CU (128 rows
// with 16 or 24 in flight: 0.760 / 0.729; 96 rows: 0.778)
#ifndef ISPLIB_STREAM_NV8
#define ISPLIB_STREAM_NV8 128
#endif
#ifndef ISPLIB_STREAM_NBW8
#define ISPLIB_STREAM_NBW8 4
#endif
#ifndef ISPLIB_STREAM_WGS8
#define ISPLIB_STREAM_WGS8 2
#endif
// the same for max / min (a second LDS plane holds the winners' positions: half the rows per wave of the sum kernel);
// 64-column slots, and 32-column slots (k <= 32: eight rows per gather, 32 gathers in flight from four batch registers)
#ifndef ISPLIB_STREAM_MM_NV
#define ISPLIB_STREAM_MM_NV 32
#endif
#ifndef ISPLIB_STREAM_MM_NBW
#define ISPLIB_STREAM_MM_NBW 2
#endif
#ifndef ISPLIB_STREAM_MM_WGS
#define ISPLIB_STREAM_MM_WGS 2
#endif
#ifndef ISPLIB_STREAM_MM8_NV
#define ISPLIB_STREAM_MM8_NV 64
#endif
#ifndef ISPLIB_STREAM_MM8_NBW
#define ISPLIB_STREAM_MM8_NBW 4
#endif
#ifndef ISPLIB_STREAM_MM8_WGS
#define ISPLIB_STREAM_MM8_WGS 2
#endif

namespace isplib {

struct SweepArgs {
   int64_t k, nnz;
   const float *val;
   const int64_t *indx, *pntrb, *pntre;
   const int32_t *indx32;
   const float *y;
   int64_t ldy;
   unsigned ybytes;
   float *z;
   int64_t ldz;
   int64_t *z_arg;
   int mean;
   int empty_init;                 // max / min: an empty row holds the launcher's init value (-+FLT_MAX) instead of 0
   const int32_t *wave_row;        // [waves][NVMAX] row of the slot, -1 = unused slot
   const int32_t *wave_part;       // [waves][NVMAX] -1: the slot is a whole row (written to z); else index of its partial row
   const int64_t *wave_task_off;   // [waves + 1]
   const int64_t *task_b;          // [n_tasks] first CSR position
   const int32_t *task_meta;       // [n_tasks] (slot << 24) | edges
   int wave_base, wave_count;      // waves of this launch (one generation): [wave_base, wave_base + wave_count)
   // stream form (spmm_stream_kernel): the plan's own copy of the edges, in the order the waves walk them
   const int32_t *words;           // [steps][G] (local row << 24) | column; padding = (the slot's first row << 24) | n
   const float *vals;              // [steps][G] weights in the same order, or null (unit weights)
   const int64_t *wave_step_off;   // [waves + 1] first step of a wave
   unsigned null_word;
   const int32_t *ids;             // stream form, max / min: [steps][G] CSR position of every word (the plan's perm), -1 = padding
   int abs_ids;                    // part_idx holds absolute CSR positions (stream form) instead of row-relative ones
   // hybrid form (spmm_hybrid_kernel): the hottest rows of y of every column slice are served from an LDS table
   const int32_t *hot_rows;        // [slices][HT] column id of every table row of a slice; n = unused / the all-zero last row
   const int32_t *hot_words;       // [hot steps][G] (local row << 24) | table row, per (wave, slice) chunk
   const int64_t *hot_step_off;    // [waves * slices + 1] first hot step of a (wave, slice) chunk
   int slices;
   // SDDMM over the stream plan (sddmm_stream_kernel): dval[perm[word]] (+)= <y[col], g[row]>
   const float *g;                 // [m][ldg] the other dense operand (grad_out)
   int64_t ldg;
   float *dval;                    // [nnz]
   unsigned long long *dbg;        // the TIMED stream kernel (calibration, scripts/exp_wave_times.py), else null: [wave][5] s_memtime at start / loop entry / loop exit / end, and where the wave ran
   float *part_val;                // [n_parts][k]
   int *part_idx;                  // [n_parts][k] row-relative edge ids (max/min)
   const int32_t *hub_row, *hub_off;
   int64_t n_hub;
   const float *ep_row_scale, *ep_self, *ep_bias;
   int64_t ep_ld_self;
   int ep_relu;
   // packed word stream (include/isplib_hip.h; the PACKED instance of spmm_stream_kernel): the plan's packed copy of `words`, or null
   const uint32_t *packed;
   unsigned pack_width;            // the plan's slice width, ceil(n / slices)
};

// finished value of a whole row: mean scale / epilogue (sum, mean), empty-row value and absolute arg (max, min),
// of the VEC columns from c on (4 everywhere but in the single-column hub fold)
template <int OP, int VEC>
__device__ __forceinline__ void finish_row(const SweepArgs &a, int row, int c, float (&v)[VEC], int (&bi)[VEC], int64_t (&arg)[VEC]) {
   const int64_t rb = a.pntrb[row];
   const int64_t deg = a.pntre[row] - rb;
   if (OP == OP_ADD) {
      if (a.mean) {
         const float d = (float)(deg > 1 ? deg : 1);
#pragma unroll
         for (int i = 0; i < VEC; i++) v[i] = v[i] / d;
      }
      if (a.ep_self) {
         const float *sr = a.ep_self + (size_t)row * (size_t)a.ep_ld_self + c;
#pragma unroll
         for (int i = 0; i < VEC; i++) v[i] += sr[i];
      }
      if (a.ep_row_scale) {
         const float rs = a.ep_row_scale[row];
#pragma unroll
         for (int i = 0; i < VEC; i++) v[i] *= rs;
      }
      if (a.ep_bias) {
#pragma unroll
         for (int i = 0; i < VEC; i++) v[i] += a.ep_bias[c + i];
      }
      if (a.ep_relu) {
#pragma unroll
         for (int i = 0; i < VEC; i++) v[i] = v[i] > 0.0f ? v[i] : 0.0f;
      }
   } else {
#pragma unroll
      for (int i = 0; i < VEC; i++) {
         if (deg <= 0) v[i] = a.empty_init ? identity<OP>() : 0.0f;
         arg[i] = bi[i] == INT_MAX ? a.nnz : (a.abs_ids ? (int64_t)bi[i] : rb + (int64_t)bi[i]);
      }
   }
}

// rows cut into several virtual rows: fold their partial rows in chunk order (= ascending CSR position); VEC = 1 serves
// panels whose width is not a multiple of 4 (stream schedule at ragged k)
template <int OP, int VEC>
__global__ __launch_bounds__(256) void sweep_hub_fold_kernel(const SweepArgs a) {
   const int64_t kv = a.k / VEC;
   const int64_t total = a.n_hub * kv;
   const int64_t stride = (int64_t)gridDim.x * blockDim.x;
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t h = i / kv;
      const int c = (int)(i - h * kv) * VEC;
      float v[VEC];
      int bi[VEC];
#pragma unroll
      for (int q = 0; q < VEC; q++) { v[q] = identity<OP>(); bi[q] = INT_MAX; }
      const int p1 = a.hub_off[h + 1];
      for (int p = a.hub_off[h]; p < p1; p++) {
         const size_t po = (size_t)p * (size_t)a.k + c;
         float t[VEC];
         load_vec<VEC>(a.part_val + po, t);
#pragma unroll
         for (int q = 0; q < VEC; q++) {
            if (OP == OP_ADD) {
               v[q] += t[q];
            } else {
               // a values-only launch (z_arg == NULL) never wrote part_idx: the chunk's ordinal stands in for its position --
               // chunks are in CSR order, so among equal values the earliest chunk stays, exactly as with real positions
               const int oi = a.z_arg ? a.part_idx[po + q] : p;
               const bool take = better<OP>(t[q], oi, v[q], bi[q]);
               v[q] = take ? t[q] : v[q];
               bi[q] = take ? oi : bi[q];
            }
         }
      }
      const int row = a.hub_row[h];
      int64_t arg[VEC];
      finish_row<OP, VEC>(a, row, c, v, bi, arg);
      store_vec<VEC>(a.z + (size_t)row * (size_t)a.ldz + c, v);
      if (OP != OP_ADD && a.z_arg) {
         int64_t *ar = a.z_arg + (size_t)row * (size_t)a.ldz + c;
#pragma unroll
         for (int q = 0; q < VEC; q++) ar[q] = arg[q];
      }
   }
}

// ---- device side of a kernel on the stream front end ----------------------------------------------------
// What the stream kernels share: who a wave is, which columns a lane holds, the wave's word stream, the batch registers and the
// gathers in flight.  What a kernel does with a gathered row -- its loop body -- is the kernel's own.
// The position of a wave: G = 64 / LPR row slots of LPR lanes x 4 floats (one panel row each); a batch is NBW registers of 64
// words = U steps, a step is one word per slot = one full 1-KiB gather; slot q owns the local rows [q * PER, (q + 1) * PER).
template <int LPR_, int NVMAX_, int NBW_, int WAVES_ = 4>
struct StreamWave {
   static constexpr int LPR = LPR_, NVMAX = NVMAX_, NBW = NBW_, WAVES = WAVES_;
   static constexpr int G = 64 / LPR, PANEL = LPR * 4, U = 64 * NBW / G, PER = NVMAX / G;
   int lane, wave, g, lc;             // lane of the wave; wave of the workgroup (uniform); slot; lane of the slot
   int wl;                            // the wave's index in the launch ...
   int64_t w;                         // ... and in the plan
   bool cok;                          // the lane holds columns of the panel
   int ccol, vfirst;                  // the first of its four; leading components of its vector that are the neighbour's
   unsigned cbyte, poison;            // column term of a gather's byte offset; what throws the offset out of range
   int64_t s0, nwords;                // first step and number of words of the wave's stream
   const int32_t *wp;                 // the stream
   unsigned ldyb;                     // row pitch of y in bytes
};

// who the wave is; false: past the last wave of the launch (a kernel without barriers returns)
template <class SW> __device__ __forceinline__ bool stream_wave_id(const SweepArgs &a, SW &sw) {
   sw.lane = threadIdx.x & 63;
   sw.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   sw.g = sw.lane / SW::LPR;
   sw.lc = sw.lane % SW::LPR;
   sw.wl = (int)blockIdx.x * SW::WAVES + sw.wave;
   sw.w = (int64_t)a.wave_base + sw.wl;
   return sw.wl < a.wave_count;
}

// a lane holds columns lc*4 .. lc*4+3 of the panel; when k is not a multiple of 4 (RAGGED: the entry admits that) the last
// lane's vector is shifted back to END at column k (its first `vfirst` components repeat the neighbour's columns and are never
// stored), so no load reaches past a row and rows need only 4-byte alignment (the GCN's K = 41 runs here instead of the task
// list).  Lanes beyond column k gather nothing: `poison` is OR-ed into their offsets
template <bool RAGGED, class SW> __device__ __forceinline__ void stream_columns(const SweepArgs &a, SW &sw) {
   sw.cok = sw.lc * 4 < a.k;
   sw.ccol = sw.lc * 4;
   sw.vfirst = 0;
   if (RAGGED && sw.cok && sw.ccol + 4 > (int)a.k) { sw.vfirst = sw.ccol + 4 - (int)a.k; sw.ccol = (int)a.k - 4; }
   sw.cbyte = (unsigned)sw.ccol * 4u;
   sw.poison = sw.cok ? 0u : BUF_OOB;
}

// the wave's stream: steps [s0, s1) of G words each
template <class SW> __device__ __forceinline__ void stream_bounds(const SweepArgs &a, SW &sw) {
   sw.s0 = a.wave_step_off[sw.w];
   const int64_t s1 = a.wave_step_off[sw.w + 1];
   sw.nwords = (s1 - sw.s0) * SW::G;
   sw.wp = a.words + sw.s0 * SW::G;
   sw.ldyb = (unsigned)a.ldy * 4u;
}

// the word past the end of a wave's stream, and of the plan's padding: column n (the gather reads 0 through the range check) in
// one of the slot's own rows (to which 0 is added), or in the spare row NVMAX of the plans whose kernels keep one (max / min,
// where 0 would beat negative values; FusedMM)
template <class SW> __device__ __forceinline__ unsigned stream_pad_own_row(const SweepArgs &a, const SW &sw) {
   return ((unsigned)((sw.lane % SW::G) * SW::PER) << 24) | a.null_word;
}
template <class SW> __device__ __forceinline__ unsigned stream_pad_spare_row(const SweepArgs &a, const SW &) {
   return ((unsigned)SW::NVMAX << 24) | a.null_word;
}

// one batch of a per-word array of the wave (src: its first element -- words, weights, CSR positions): lane i of batch register
// q holds element first + q*64 + i = (step (q*64 + i) / G, slot i % G); past the end of the wave: pad.
// Three batches of words are on the way at any time: while batch b is consumed, every gather taken is replaced by the same step
// of batch b + 1 (the kernels' w1); w2 holds the words of batch b + 2, loaded a whole batch before the first of them is handed
// out.  What is needed only when a gather is CONSUMED (the weights; the SDDMM's CSR positions) is needed one batch later than its
// word, so it is loaded one batch later.  (The order of these loads stays spelled out in each kernel: it decides the register
// allocation of the whole loop -- the weighted 128-column sum kernel went from 226 registers to 256 and four spills with the
// weights of batches 0 and 1 loaded after the words of batch 2 instead of beside their own.)
template <class SW, class S, class T>
__device__ __forceinline__ void stream_load_batch(const SW &sw, const S *src, int64_t first, T pad, T (&reg)[SW::NBW]) {
#pragma unroll
   for (int q = 0; q < SW::NBW; q++) {
      const int64_t i = first + q * 64 + sw.lane;
      reg[q] = i < sw.nwords ? (T)src[i] : pad;
   }
}

// The same batch of WORDS out of the plan's packed stream (include/isplib_hip.h, PACKED WORD STREAM): 304 bytes instead of 512.
// The load and the decode are apart by a whole batch, like the load of w2 and its move to w1: decoding where the batch is loaded
// would wait for the load, and with it for every gather issued before it.  stream_load_packed: 76 dwords, one per lane and 12 more;
// a batch past the wave's last loads nothing and holds 0, which decodes to padding (a header that says "no entry is real").
template <class SW>
__device__ __forceinline__ void stream_load_packed(const SW &sw, const uint32_t *wave_packed, int64_t batch, int64_t nbatches, unsigned (&raw)[2]) {
   static_assert(SW::NBW == 2 && SW::G == 4 && SW::PER == 16, "the packed stream is the 64-column sum geometry's: 128 words a batch, 16 rows a slot");
   const uint32_t *p = wave_packed + batch * ISPLIB_STREAM_PACK_DWORDS;
   const bool in = batch < nbatches;
   raw[0] = in ? p[sw.lane] : 0u;
   raw[1] = in && sw.lane < ISPLIB_STREAM_PACK_DWORDS - 64 ? p[64 + sw.lane] : 0u;
}
// what of a lane's place in the packed batch does not change from batch to batch
struct StreamPackLane {
   unsigned row_hi;                // the slot's first local row as the top byte of a word
   unsigned mask_lo, mask_hi;      // the lanes of this lane's slot up to and including itself
   unsigned slot_lanes;            // the lanes of the slot among any 32 (the same pattern in both halves of the wave)
   int nib_addr, hdr_addr;         // ds_bpermute addresses: the lane that holds this lane's second local row; its slot's header
   unsigned nib_shift, step;       // where that row is in the dword; this lane's step in the batch's first register
};
template <class SW> __device__ __forceinline__ StreamPackLane stream_pack_lane(const SW &sw) {
   StreamPackLane pl;
   const unsigned t = (unsigned)sw.lane >> 2, slot = (unsigned)sw.lane & 3u;
   pl.row_hi = (slot * (unsigned)SW::PER) << 24;
   pl.slot_lanes = 0x11111111u << slot;
   pl.mask_lo = pl.slot_lanes & (sw.lane < 32 ? (2u << sw.lane) - 1u : 0xFFFFFFFFu);
   pl.mask_hi = sw.lane < 32 ? 0u : pl.slot_lanes & ((2u << (sw.lane - 32)) - 1u);
   pl.nib_addr = (int)(slot * 2u + (t >> 3)) * 4;
   pl.hdr_addr = (int)(8u + slot) * 4;
   pl.nib_shift = (t & 7u) * 4u;
   pl.step = t;
   return pl;
}
// raw (loaded a batch ago) -> the two batch registers, exactly what stream_load_batch reads from `words`
template <class SW>
__device__ __forceinline__ void stream_decode_packed(const StreamPackLane &pl, unsigned width, unsigned pad_word, const unsigned (&raw)[2], unsigned (&reg)[2]) {
   const unsigned d = raw[0];
   const unsigned rows1 = (unsigned)__builtin_amdgcn_ds_bpermute(pl.nib_addr, (int)raw[1]);
   const unsigned hdr = (unsigned)__builtin_amdgcn_ds_bpermute(pl.hdr_addr, (int)raw[1]);
   const unsigned long long f0 = __ballot((d & 0x40000000u) != 0u), f1 = __ballot((int)d < 0);
   const unsigned f0lo = (unsigned)f0, f0hi = (unsigned)(f0 >> 32), f1lo = (unsigned)f1, f1hi = (unsigned)(f1 >> 32);
   // advance flags of the slot's entries up to and including this lane's: of the first register, and of the second (after all of the first)
   const unsigned c0 = __popc(f0lo & pl.mask_lo) + __popc(f0hi & pl.mask_hi);
   const unsigned c1 = __popc(f0lo & pl.slot_lanes) + __popc(f0hi & pl.slot_lanes) + __popc(f1lo & pl.mask_lo) + __popc(f1hi & pl.mask_hi);
   const unsigned base = hdr & 0xFFFu, real = (hdr >> 12) & 0x3Fu;
   constexpr unsigned CM = (1u << ISPLIB_STREAM_PACK_COL_BITS) - 1u;
   const unsigned w0 = __umul24(base + c0, width) + (d & CM) + (pl.row_hi + (((d >> 26) & 15u) << 24));
   const unsigned w1 = __umul24(base + c1, width) + ((d >> ISPLIB_STREAM_PACK_COL_BITS) & CM) + (pl.row_hi + (((rows1 >> pl.nib_shift) & 15u) << 24));
   reg[0] = pl.step < real ? w0 : pad_word;
   reg[1] = pl.step + 16u < real ? w1 : pad_word;
}

// the gather of step u of a batch.  One cross-lane read (ds_bpermute) hands a slot its word of the step (the LDS pipe is otherwise
// idle; picking it with v_readlane + v_cndmask cost 16 vector instructions per step); column * row pitch is a 24-bit multiply
// (n < 2^24, pitch < 2^24, product < 2^32: checked by the entry).  la: the LDS offset of the word's local row.  AUX: cache-policy
// bits of the load (ISPLIB_EXP_GATHER_AUX)
template <int AUX, class SW>
__device__ __forceinline__ void stream_issue(const SW &sw, __amdgpu_buffer_rsrc_t rsrc, const unsigned (&word_l)[SW::NBW], int u, unsigned &la, v4i_t &t) {
   const unsigned word = (unsigned)__shfl((int)word_l[(u * SW::G) / 64], (u * SW::G) % 64 + sw.g);
   const unsigned o = (__umul24(word & 0xFFFFFFu, sw.ldyb) + sw.cbyte) | sw.poison;
   la = (word >> 24) * (unsigned)SW::PANEL;
   t = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, AUX);
}

// The row a slot is working on keeps its running sum in registers; it moves to the slot's LDS row when the stream turns to
// another row (every ~deg / slices edges) and is picked up again from there when the stream comes back in the next slice.
// Plain read-add-write by the only lanes that ever touch that LDS row: LDS float atomics (one ds_add_f32 per gathered
// float) ran 25x slower than the gathers they were meant to keep up with.
__device__ __forceinline__ void stream_flush(float *lds_row, const float (&acc)[4]) {
   float4 *p = reinterpret_cast<float4 *>(lds_row);
   float4 o = *p;
   o.x += acc[0]; o.y += acc[1]; o.z += acc[2]; o.w += acc[3];
   *p = o;
}
// (The fetch of a slot's row ids ahead of the write-out stays in each kernel too: as a function its loads are merged and speculated
// -- the 144 global_load_dword of the six sum kernels become 48 wider ones -- at two more SGPRs in every one of them.)

// Geometry of the stream kernels.  Persistent waves only stay on the same column slices while FEW of them share a SIMD:
// a SIMD's memory instructions go to its oldest ready wave first, so with 8 waves per SIMD the waves of a CU finish
// one after the other (L2 hit rate 48 % at 32 slices; 67-75 % with 4; the compulsory misses only with 2).  The bytes
// in flight that keep a CU's address pipeline busy (~256 KB) therefore come from depth, not from occupancy:
// WGS workgroups (of 4 waves, one per SIMD) per CU, each wave with U = 64 * NBW / G gathers of 1 KiB in flight.
//
// The one geometry per (plan family, slot width) that the entries launch, check plans against and report: lanes per row slot
// (64 / streams), rows per wave, 64-word batch registers, workgroups per CU, and whether a wave keeps two LDS planes of its rows
// plus the spare row that padding words point at (max / min: values and positions; FusedMM: x_i and the accumulator).  Sum / mean
// measured on the Reddit shape, K = 128 in 64-column panels.  nvmax 0: the family has no kernel for that
// slot width.  The hybrid's row is its cold stream (its LDS -- 8 waves and the hot table -- is its own: experimental.hip).
enum StreamFamily { STREAM_SUM = 0, STREAM_MINMAX, STREAM_FUSEDMM, STREAM_HYBRID, STREAM_FAMILIES };
struct StreamGeom { int lpr, nvmax, nbw, wgs; bool two_planes; };
constexpr StreamGeom STREAM_GEOMS[STREAM_FAMILIES][3] = {      // [family][streams = 2, 4, 8]
   // sum / mean (and the SDDMM over their plans)
   {{32, 32, 1, 2, false},                  // 128-column panels: U = 32 gathers of 1 KiB per wave
    {16, ISPLIB_STREAM_NV4, ISPLIB_STREAM_NBW4, ISPLIB_STREAM_WGS4, false},
    {8, ISPLIB_STREAM_NV8, ISPLIB_STREAM_NBW8, ISPLIB_STREAM_WGS8, false}},
   // max / min
   {{32, 0, 0, 0, true},
    {16, ISPLIB_STREAM_MM_NV, ISPLIB_STREAM_MM_NBW, ISPLIB_STREAM_MM_WGS, true},
    {8, ISPLIB_STREAM_MM8_NV, ISPLIB_STREAM_MM8_NBW, ISPLIB_STREAM_MM8_WGS, true}},
   // the FusedMM words
   {{32, 16, 1, 2, true},                   // 128-column slots: 2 rows per gather, 32 gathers in flight
    {16, 32, 2, 2, true},
    {8, 64, 4, 2, true}},
   // the cold stream of the hybrid
   {{32, 0, 0, 0, false},
    {16, ISPLIB_HYB4_NV, ISPLIB_HYB4_NBW, 1, false},
    {8, ISPLIB_HYB8_NV, ISPLIB_HYB8_NBW, 1, false}},
};
constexpr bool stream_count_ok(int streams) { return streams == 2 || streams == 4 || streams == 8; }
constexpr StreamGeom stream_geom(int family, int streams) { return STREAM_GEOMS[family][streams == 2 ? 0 : (streams == 4 ? 1 : 2)]; }

// a plan's `streams` as a template argument: f(std::integral_constant<int, streams>()), the launcher of a family's kernel for
// that slot width.  Only the widths the family has a kernel for are instantiated (the entries refuse a plan of any other width
// before anything is launched: check_stream_call)
template <int FAMILY, class F>
static inline int with_streams(int streams, F f) {
   if constexpr (stream_geom(FAMILY, 2).nvmax != 0) {
      if (streams == 2) return f(std::integral_constant<int, 2>());
   }
   if constexpr (stream_geom(FAMILY, 4).nvmax != 0) {
      if (streams == 4) return f(std::integral_constant<int, 4>());
   }
   return f(std::integral_constant<int, 8>());
}

// LDS of a workgroup (4 waves x rows x one panel row of LPR lanes x 4 floats), the workgroups of a CU that its 160 KB and
// the geometry's cap admit -- the kernels' launch bound -- and the waves of a launch that are resident together
constexpr int CU_LDS_BYTES = 163840;
constexpr int stream_lds_bytes(int lpr, int rows) { return 4 * rows * lpr * 4 * 4; }
constexpr int stream_lds_rows(const StreamGeom &ge) { return ge.two_planes ? 2 * (ge.nvmax + 1) : ge.nvmax; }
constexpr int lds_wgs_per_cu(int lds_bytes, int cap) { return CU_LDS_BYTES / lds_bytes < cap ? CU_LDS_BYTES / lds_bytes : cap; }
template <int LPR, int ROWS, int WGS> constexpr int stream_wgs_per_cu() { return lds_wgs_per_cu(stream_lds_bytes(LPR, ROWS), WGS); }
constexpr int stream_resident_waves(const StreamGeom &ge, int cus) {
   return cus * lds_wgs_per_cu(stream_lds_bytes(ge.lpr, stream_lds_rows(ge)), ge.wgs) * 4;
}

static inline int device_cus() {
   int dev = 0, cus = 0;
   if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
      (void)hipGetLastError();
      cus = 256;                                          // MI355X
   }
   return cus;
}

// isplib_spmm_stream_geometry, isplib_spmm_stream_minmax_geometry, isplib_fusedmm_stream_geometry
static inline int stream_geometry(const char *entry, int family, int streams, int *rows_per_wave, int *waves_resident) {
   clear_error();
   if (!stream_count_ok(streams) || !stream_geom(family, streams).nvmax)
      return fail(ISPLIB_FAIL, entry, stream_geom(family, 2).nvmax ? "streams must be 2, 4 or 8" : "streams must be 4 (64-column slots) or 8 (32-column slots)");
   const StreamGeom ge = stream_geom(family, streams);
   if (rows_per_wave) *rows_per_wave = ge.nvmax;
   if (waves_resident) *waves_resident = stream_resident_waves(ge, device_cus());
   return ISPLIB_SUCCESS;
}

// The isplib_suggest_*stream* rules offer a shape the stream schedule only when (a) its entry and plan builder would serve
// it -- isplib_stream_serves (include/isplib_hip.h) with ldy = k, a contiguous dense operand; callers with a padded leading
// dimension ask it again with theirs -- so that a shape outside the domain runs on the task list or the plain kernel as
// before the stream schedule existed instead of being offered and then refused with an error, and (b) the graph has work
// for the whole chip: at least this many stored entries (a measured rule, not an address domain).
constexpr int64_t STREAM_MIN_NNZ = 4 * 1048576;

// (c) every generation of waves sweeps the whole dense operand once per XCD, so the rows a generation holds must reuse each
// row of it often: edges per generation and XCD >= 3 x rows of y.  Then: slices of `slice_bytes` of a panel of y, and rows
// longer than 1 / chunk_div of a stream's share of the edges dealt to several virtual rows.
static inline int suggest_stream_geom(int64_t m, int64_t n, int64_t nnz, int st, int rpw, int resident, double slice_bytes, double chunk_div,
                                      int *slices, int *chunk) {
   const int64_t per_gen = (int64_t)rpw * resident;
   const int64_t gens = (m + per_gen - 1) / per_gen;
   if ((double)nnz / (double)gens / 8.0 < 3.0 * (double)n) return 0;
   const double panel_bytes = 1024.0 / st;
   int sl = (int)((double)n * panel_bytes / slice_bytes + 0.5);
   sl = sl < 1 ? 1 : (sl > 512 ? 512 : sl);
   int64_t ch = (int64_t)((double)nnz / ((double)gens * resident * st) / chunk_div);
   ch = ch < 256 ? 256 : (ch > (1 << 20) ? (1 << 20) : ch);
   if (slices) *slices = sl;
   if (chunk) *chunk = (int)ch;
   return 1;
}

// ---- host side of an entry on the stream front end: one check, one fill, one driver ------------------------------------
// What an entry was called with, as far as all of them are alike.
struct StreamCall {
   const char *entry;                     // its name: the prefix of every message
   const char *instead;                   // the entry that serves what this one refuses for k or size
   int family;                            // whose plans it runs
   int64_t m, n, k, nnz;
   bool empty;                            // nothing to compute: success before the plan is looked at
   const int64_t *pntrb, *pntre;
   const isplib_stream_plan *plan;
   const float *y;
   int64_t ldy;
   int64_t ld_other;                      // the entry's other leading dimension (z; the SDDMM's g)
   bool others;                           // the entry's other operands are all there
   bool hub_fold;                         // hub rows leave partial rows in the workspace (not the SDDMM: it writes per edge)
   void *workspace;
   size_t workspace_bytes, workspace_need;
   int elt_bytes = 4;                     // bytes per element of y (2: the 16-bit entry, spmm_stream16.hip)
};

// Every refusal the entries share that is decided before anything is launched.  *done: nothing (more) to do, the entry returns
// the status.  What is an entry's own (its message words before this; limits of its kernel after it) stays with the entry,
// and the workspace comes last: a plan that is refused is refused whatever the workspace.
static inline int check_stream_call(const StreamCall &c, bool *done) {
   const isplib_stream_plan *plan = c.plan;
   auto use_instead = [&](const char *what) {          // "<what> (use <the entry that serves it>)"
      char msg[256];
      snprintf(msg, sizeof msg, "%s (use %s)", what, c.instead);
      return fail(ISPLIB_FAIL, c.entry, msg);
   };
   *done = true;
   if (c.m < 0 || c.n < 0 || c.k < 0 || c.nnz < 0) return fail(ISPLIB_FAIL, c.entry, "negative dimension");
   if (c.empty) return ISPLIB_SUCCESS;
   if (!plan) return fail(ISPLIB_FAIL, c.entry, "plan is required");
   if (plan->rows != c.m || plan->cols != c.n) return fail(ISPLIB_FAIL, c.entry, "the plan was built for another shape");
   if (c.n >= ISPLIB_STREAM_N_END || c.ldy >= ISPLIB_STREAM_LDY_END) return fail(ISPLIB_FAIL, c.entry, "n must be < 2^24 and ldy < 2^22 (24-bit address arithmetic)");
   if (!stream_count_ok(plan->streams)) return fail(ISPLIB_FAIL, c.entry, "bad plan geometry (streams 2, 4 or 8)");
   if (!stream_geom(c.family, plan->streams).nvmax) return fail(ISPLIB_FAIL, c.entry, "bad plan geometry (this entry runs on 4- or 8-stream plans)");
   if (plan->gens < 1 || plan->waves_per_gen < 1 || plan->rows_per_wave != stream_geom(c.family, plan->streams).nvmax)
      return fail(ISPLIB_FAIL, c.entry, "bad plan geometry (rows_per_wave must be what the geometry entry of this plan family reports)");
   if (c.k < ISPLIB_K_MIN) return use_instead("k >= 4 required");
   if (c.ldy < c.k || c.ld_other < c.k) return fail(ISPLIB_FAIL, c.entry, "leading dimension smaller than k");
   if (!isplib_rows_within(c.n, c.ldy, (uint64_t)ISPLIB_DENSE_BYTES_MAX * 4u / (uint64_t)c.elt_bytes)) return use_instead("dense operand larger than 3.5 GiB");
   if (!c.pntrb || !c.pntre || !c.y || !c.others || !plan->wave_row || !plan->wave_step_off || (plan->n_steps > 0 && !plan->words) ||
       (c.hub_fold && (!plan->wave_part || (plan->n_hub > 0 && (!plan->hub_row || !plan->hub_off)))))
      return fail(ISPLIB_FAIL, c.entry, "null operand");
   *done = false;
   return ISPLIB_SUCCESS;
}

static inline int check_stream_workspace(const StreamCall &c) {
   if (c.plan->n_parts <= 0) return ISPLIB_SUCCESS;
   if (!c.workspace || c.workspace_bytes < c.workspace_need) return fail(ISPLIB_NOT_ENOUGH_MEM, c.entry, "workspace too small");
   if (((uintptr_t)c.workspace & 255) != 0) return fail(ISPLIB_FAIL, c.entry, "workspace must be 256-byte aligned");
   return ISPLIB_SUCCESS;
}

// the kernel arguments every stream kernel reads from the plan and the dense operands (the entry adds what is its own)
static inline SweepArgs stream_args(const StreamCall &c, float *z, int64_t ldz) {
   const isplib_stream_plan *plan = c.plan;
   SweepArgs a = {};
   a.empty_init = empty_row_init();
   a.k = c.k; a.nnz = c.nnz; a.pntrb = c.pntrb; a.pntre = c.pntre;
   a.y = c.y; a.ldy = c.ldy; a.ybytes = (unsigned)((unsigned long long)c.n * (unsigned long long)c.ldy * 4ull); a.z = z; a.ldz = ldz;
   a.ids = plan->perm; a.abs_ids = 1;
   a.wave_row = plan->wave_row; a.wave_part = plan->wave_part;
   a.words = plan->words; a.vals = plan->vals; a.wave_step_off = plan->wave_step_off; a.null_word = (unsigned)c.n;
   a.hub_row = plan->hub_row; a.hub_off = plan->hub_off; a.n_hub = plan->n_hub;
   a.part_val = (float *)c.workspace;
   a.packed = nullptr;              // the sum / mean entry alone attaches the packed stream (spmm_sweep.hip)
   return a;
}

static inline int set_epilogue(const char *entry, const isplib_epilogue *ep, SweepArgs &a) {
   if (!ep) return ISPLIB_SUCCESS;
   if (ep->self && ep->ld_self < a.k) return fail(ISPLIB_FAIL, entry, "ld_self smaller than k");
   a.ep_row_scale = ep->row_scale; a.ep_self = ep->self; a.ep_ld_self = ep->ld_self; a.ep_bias = ep->bias;
   a.ep_relu = ep->relu ? 1 : 0;
   return ISPLIB_SUCCESS;
}

// the fold of the hub rows' partial rows of one panel.  RAGGED: the entry admits panels that are not whole, 16-byte aligned
// float4 columns (they are folded one column per thread); the others fold four columns per thread, always.
template <int OP, bool RAGGED>
static inline int launch_hub_fold(const SweepArgs &p, hipStream_t st) {
   if (p.n_hub <= 0) return ISPLIB_SUCCESS;
   const bool v4 = !RAGGED || ((p.k % 4) == 0 && (p.ldz % 4) == 0 && ((uintptr_t)p.z & 15) == 0 &&
                               (!p.ep_self || ((p.ep_ld_self % 4) == 0 && ((uintptr_t)p.ep_self & 15) == 0)));
   int64_t blocks = (p.n_hub * (v4 ? p.k / 4 : p.k) + 255) / 256;
   if (blocks > 4096) blocks = 4096;
   if (v4) hipLaunchKernelGGL((sweep_hub_fold_kernel<OP, 4>), dim3((unsigned)blocks), dim3(256), 0, st, p);
   else if constexpr (RAGGED) hipLaunchKernelGGL((sweep_hub_fold_kernel<OP, 1>), dim3((unsigned)blocks), dim3(256), 0, st, p);
   return check_launch("sweep_hub_fold_kernel");
}

// one dispatch per generation of resident waves (all in one launch: measured slower, 2.73 against 2.68 ms)
template <class Launch>
static inline int run_generations(int gens, int waves_per_gen, SweepArgs &p, Launch launch) {
   for (int gen = 0; gen < gens; gen++) {
      p.wave_base = gen * waves_per_gen;
      p.wave_count = waves_per_gen;
      const int rc = launch(p);
      if (rc) return rc;
   }
   return ISPLIB_SUCCESS;
}

// the partial rows of the hub rows, at the start of every stream entry's workspace (what isplib_spmm_stream_workspace_bytes was
// before it grew the staging area; max / min keep a second plane of the same size behind it)
static inline size_t stream_parts_bytes(const isplib_stream_plan *plan) {
   if (!plan || plan->n_parts <= 0) return 256;
   const size_t pk = (size_t)(256 / (plan->streams > 0 ? plan->streams : 4));
   return ((size_t)plan->n_parts * pk * sizeof(float) + 255) & ~(size_t)255;
}

// an entry that never stages a panel (max / min, the hybrid) passes this to run_stream_panels
struct NoStage { int operator()(SweepArgs &, int64_t) const { return ISPLIB_SUCCESS; } };

// column panels of the plan's slot width (a slot is 64 / streams lanes x 4 floats): every generation, then the hub fold, per panel.
// stage(p, c0) runs before the panel's first dispatch, on the panel's arguments: the sum / mean entry's launches a copy of a panel
// whose lines sit in a slow address class (isplib_stream_stage_panel, include/isplib_hip.h) and points p.y / p.ldy / p.ybytes at
// the copy -- rows n and beyond are still outside the descriptor, so padding words still read 0; the kernel, z, the epilogue's
// operands and the fold see no difference.
template <class Launch, class Fold, class Stage>
static inline int run_stream_panels(const isplib_stream_plan *plan, const SweepArgs &a, Launch launch, Fold fold, Stage stage) {
   const int64_t k = a.k, pw = 256 / plan->streams;
   for (int64_t c0 = 0; c0 < k; c0 += pw) {
      SweepArgs p = a;
      p.k = (k - c0) < pw ? (k - c0) : pw;
      if (p.k < 4) {                              // a sliver of 1-3 columns: widen it backwards (the overlap is rewritten identically)
         p.k = 4;
         c0 = k - 4;
      }
      p.y = a.y + c0;
      p.z = a.z + c0;
      p.ep_self = a.ep_self ? a.ep_self + c0 : nullptr;
      p.ep_bias = a.ep_bias ? a.ep_bias + c0 : nullptr;
      p.z_arg = a.z_arg ? a.z_arg + c0 : nullptr;
      p.ybytes = a.ybytes - (unsigned)c0 * 4u;
      int rc = stage(p, c0);
      if (!rc) rc = run_generations(plan->gens, plan->waves_per_gen, p, launch);
      if (!rc) rc = fold(p);
      if (rc) return rc;
   }
   return ISPLIB_SUCCESS;
}

}  // namespace isplib
