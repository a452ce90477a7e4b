// spmm.hip -- SpMM (sum / mean / max / min) forward for gfx950 (MI355X, CDNA4): the plain and the
// column-sliced schedules, and the entry points fusedMM_csr_hip / fusedMM_csr_sliced{,_phase}_hip.
//
// Replaces the body behind fusedMM_csr (reference csrc/fusedMM.h:77-99, called at csrc/fusedmm.cpp:198)
// for device-resident operands.  Written for wave64.  The gather loop itself lives in gather.h; the
// task-list schedule (the default fast path) in spmm_tasks.hip.
//
// Mapping of this file's kernel (spmm_csr_kernel)
//   * plain : one CSR row -> one wavefront, WAVES rows -> one workgroup; blockIdx is remapped so that each
//     XCD (blocks b, b+8, ... share one) walks a contiguous range of rows (neighbouring rows of a real graph
//     share neighbours, and then share that XCD's 4 MiB L2).  Speed only.
//   * sliced: one (row, column-slice) segment -> one wavefront; each XCD walks ALL rows of its own slice(s),
//     so its L2 only ever sees a fraction of the rows of y; per-slice partials go to a workspace and
//     combine_slices_kernel folds them in slice order.
//   * rows / segments longer than long_row edges are processed by all WAVES waves of the workgroup together
//     (contiguous edge chunks, fixed-order LDS combine), so a hub row never serialises on one wave.
//   * no atomics anywhere: results are bitwise reproducible run to run; max/min carry (value, row-relative
//     edge id) pairs whose comparator makes the result independent of the slot / wave / slice split.
//
// Roofline: gather-bound (L1->L2 request rate when sliced, Infinity-Cache rate when not); see DESIGN.md 5.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <float.h>
#include <limits.h>

#include "../../include/isplib_hip.h"
#include "common.h"
#include "gather.h"

namespace isplib {

struct SpmmArgs {
   int64_t m, k, nnz;
   const float *val;       // may be null (unit weights)
   const int64_t *indx;
   const int32_t *indx32;  // packed copy of indx (task entries only; null here)
   const int64_t *pntrb;
   const int64_t *pntre;
   const float *y;
   int64_t ldy;
   float *z;
   int64_t ldz;
   int64_t *z_arg;         // may be null
   int mean;               // OP_ADD only: divide by max(deg,1)
   int empty_init;         // max / min: an empty row holds the launcher's init value (-+FLT_MAX) instead of 0
   int auto_panels;        // plain mode, index order, dense operand beyond the Infinity Cache: 128-column panels (launch_vec)
   int long_row;           // rows with more edges are split across the workgroup
   unsigned nblk;          // number of row blocks
   unsigned ybytes;        // n*ldy*4 when it fits the buffer-descriptor path, else 0
   // column-sliced mode (fusedMM_csr_sliced_hip): row i's edges with column in slice s are
   // [sliceptr[i*(slices+1)+s], sliceptr[i*(slices+1)+s+1]); this launch walks slices
   // [slice_first, slice_first + slice_count), dealt over the 8 XCDs (see the kernel)
   const int64_t *sliceptr;
   int slices, slice_first, slice_count, combine;
   float *part_val;        // [slices][m][k] partial results
   int *part_idx;          // [slices][m][k] row-relative edge ids (max/min), INT_MAX = none
   // plain mode only (fusedMM_csr_ordered_hip): position -> row, a permutation of [0, m); the workgroups of an XCD walk
   // a contiguous range of POSITIONS, so rows that share neighbours and sit next to each other in the order share that
   // XCD's L2 while they are worked on.  Every row is still computed by the same code in the same edge order: any
   // order gives the same bits.  Null = the identity.
   const int32_t *row_order;
};

template <int OP, int VEC, int NCH>
__device__ __forceinline__ void write_row(const SpmmArgs &a, int64_t row, int64_t row_b, int64_t deg,
                                          const int (&ccol)[NCH], const bool (&cok)[NCH], const int (&vfirst)[NCH],
                                          float (&acc)[NCH][VEC], const int (&bi)[NCH][VEC]) {
   float *zr = a.z + (size_t)row * (size_t)a.ldz;
   if (OP == OP_ADD) {
      if (a.mean) {
         const float d = (float)(deg > 1 ? deg : 1);
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[j][v] = acc[j][v] / d;
      }
   } else if (deg <= 0) {
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < VEC; v++) acc[j][v] = a.empty_init ? identity<OP>() : 0.0f;
   }
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (!cok[j]) continue;
      store_tail<VEC>(zr + ccol[j], acc[j], vfirst[j]);
      if (OP != OP_ADD && a.z_arg) {
         int64_t *ar = a.z_arg + (size_t)row * (size_t)a.ldz + ccol[j];
#pragma unroll
         for (int v = 0; v < VEC; v++)
            if (v >= vfirst[j]) ar[v] = bi[j][v] == INT_MAX ? a.nnz : row_b + (int64_t)bi[j][v];
      }
   }
}

// sliced mode: raw partial of (slice, row); finished by combine_slices_kernel
template <int OP, int VEC, int NCH>
__device__ __forceinline__ void write_partial(const SpmmArgs &a, int slice, int64_t row, const int (&ccol)[NCH],
                                              const bool (&cok)[NCH], const int (&vfirst)[NCH],
                                              const float (&acc)[NCH][VEC], const int (&bi)[NCH][VEC]) {
   const size_t off = ((size_t)slice * (size_t)a.m + (size_t)row) * (size_t)a.k;
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      if (!cok[j]) continue;
      store_tail<VEC>(a.part_val + off + ccol[j], acc[j], vfirst[j]);
      if (OP != OP_ADD) {
#pragma unroll
         for (int v = 0; v < VEC; v++)
            if (v >= vfirst[j]) a.part_idx[off + ccol[j] + v] = bi[j][v];
      }
   }
}

// ADDR: 0 = 64-bit addresses (any size, any VEC); 1 / 2 = buffer descriptor, unit weights / weighted (VEC = 4)
template <int OP, int VEC, int LPR, int NCH, int WAVES, bool SLICED, int ADDR>
__global__ __launch_bounds__(WAVES * 64, (min_waves_of<OP, LPR, NCH, ADDR>())) void spmm_csr_kernel(const SpmmArgs a) {
   constexpr int U = unroll_of<OP, NCH, ADDR>();
   constexpr int PANEL = LPR * VEC * NCH;   // columns covered by one grid.y slice
   __shared__ float sh_val[WAVES][PANEL];
   __shared__ int sh_idx[OP == OP_ADD ? 1 : WAVES][OP == OP_ADD ? 1 : PANEL];

   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave-uniform: task/row bookkeeping lives in SGPRs
   const int g = lane / LPR, lc = lane % LPR;
   __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
       const_cast<float *>(a.y), 0, ADDR ? (int)a.ybytes : 0, 0x00020000);   // kernarg-only: provably wave-uniform

   // XCD-aware remap: physical blocks pb, pb+8, ... share one XCD (speed only, never correctness).
   //  plain : each XCD walks a contiguous range of row blocks.
   //  sliced: each XCD walks the row blocks of its own column slice(s), so its L2 only ever sees a
   //          fraction of the rows of y.
   const unsigned pb = blockIdx.x, nb = a.nblk;
   const unsigned xcd = pb & 7u, within = pb >> 3;
   unsigned lb;
   int slice = 0;
   if (SLICED) {
      // the (slice, row block) items of this launch, slice-major, are cut into 8 equal contiguous runs, one per
      // XCD: an XCD walks at most a few slices one after the other (L2 affinity) and every XCD gets the same
      // number of items whatever the slice count (16 -> two slices each, 2 -> a quarter of a slice each, 14 ->
      // 1.75 each).  Slices wrap around modulo `slices`, so "all but my own" is one launch.
      const uint64_t items = (uint64_t)a.slice_count * nb;
      const uint64_t per_x = (items + 7u) / 8u;
      const uint64_t item = (uint64_t)xcd * per_x + within;
      if (within >= per_x || item >= items) return;
      lb = (unsigned)(item % nb);
      slice = (int)(((uint64_t)a.slice_first + item / nb) % (uint64_t)a.slices);
   } else {
      const unsigned per = nb >> 3, rem = nb & 7u;
      lb = xcd * per + (xcd < rem ? xcd : rem) + within;
   }

   int ccol[NCH];
   bool cok[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      ccol[j] = (int)blockIdx.y * PANEL + (j * LPR + lc) * VEC;
      cok[j] = ccol[j] < a.k;
   }
   // ragged K (k % 4 != 0, buffer path only): the last 16-byte vector of a row is shifted back so
   // that it ends at column k; its first vfirst components duplicate the neighbouring lane's work
   // and are simply not stored.  Rows then need only 4-byte alignment.
   int vfirst[NCH];
#pragma unroll
   for (int j = 0; j < NCH; j++) {
      vfirst[j] = 0;
      if (VEC == 4 && ADDR != 0 && cok[j] && ccol[j] + 4 > (int)a.k) {
         vfirst[j] = ccol[j] + 4 - (int)a.k;
         ccol[j] = (int)a.k - 4;
      }
   }

   const int64_t row0 = (int64_t)lb * WAVES;
   const int64_t row = (!SLICED && a.row_order && row0 + wave < a.m) ? (int64_t)a.row_order[row0 + wave] : row0 + wave;

   // phase 1: one row per wave (rows up to long_row edges)
   if (row0 + wave < a.m) {
      int64_t b, e, row_b;
      if (SLICED) {
         const int64_t *sp = a.sliceptr + (size_t)row * (size_t)(a.slices + 1) + slice;
         b = sp[0]; e = sp[1];
         row_b = OP == OP_ADD ? b : a.pntrb[row];
      } else {
         b = a.pntrb[row]; e = a.pntre[row]; row_b = b;
      }
      const int64_t deg = e - b;
      if (deg <= a.long_row) {
         float acc[NCH][VEC];
         int bi[NCH][VEC];
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < VEC; v++) { acc[j][v] = identity<OP>(); bi[j][v] = INT_MAX; }
         if constexpr (ADDR != 0) wave_edges_buf<OP, ADDR == 2, LPR, NCH, U>(a, rsrc, row_b, b, e, ccol, cok, acc, bi);
         else wave_edges<OP, VEC, LPR, NCH, U>(a, row_b, b, e, ccol, cok, acc, bi);
         slot_reduce<OP, VEC, LPR, NCH>(acc, bi);
         if (g == 0) {
            if (SLICED) write_partial<OP, VEC, NCH>(a, slice, row, ccol, cok, vfirst, acc, bi);
            else write_row<OP, VEC, NCH>(a, row, b, deg, ccol, cok, vfirst, acc, bi);
         }
      }
   }

   // phase 2: long rows of this block, all waves on one row at a time
   for (int r = 0; r < WAVES; r++) {
      if (row0 + r >= a.m) break;                  // uniform over the block
      const int64_t lr = (!SLICED && a.row_order) ? (int64_t)a.row_order[row0 + r] : row0 + r;
      int64_t b, e, row_b;
      if (SLICED) {
         const int64_t *sp = a.sliceptr + (size_t)lr * (size_t)(a.slices + 1) + slice;
         b = sp[0]; e = sp[1];
         row_b = OP == OP_ADD ? b : a.pntrb[lr];
      } else {
         b = a.pntrb[lr]; e = a.pntre[lr]; row_b = b;
      }
      const int64_t deg = e - b;
      if (deg <= a.long_row) continue;             // uniform over the block
      int64_t chunk = (deg + WAVES - 1) / WAVES;
      chunk = (chunk + 63) & ~(int64_t)63;
      int64_t cb = b + (int64_t)wave * chunk, ce = cb + chunk;
      if (cb > e) cb = e;
      if (ce > e) ce = e;
      float acc[NCH][VEC];
      int bi[NCH][VEC];
#pragma unroll
      for (int j = 0; j < NCH; j++)
#pragma unroll
         for (int v = 0; v < VEC; v++) { acc[j][v] = identity<OP>(); bi[j][v] = INT_MAX; }
      if constexpr (ADDR != 0) wave_edges_buf<OP, ADDR == 2, LPR, NCH, U>(a, rsrc, row_b, cb, ce, ccol, cok, acc, bi);
      else wave_edges<OP, VEC, LPR, NCH, U>(a, row_b, cb, ce, ccol, cok, acc, bi);
      slot_reduce<OP, VEC, LPR, NCH>(acc, bi);
      if (g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < VEC; v++) {
               sh_val[wave][(j * LPR + lc) * VEC + v] = acc[j][v];
               if (OP != OP_ADD) sh_idx[wave][(j * LPR + lc) * VEC + v] = bi[j][v];
            }
      }
      __syncthreads();
      if (wave == 0 && g == 0) {
#pragma unroll
         for (int j = 0; j < NCH; j++)
#pragma unroll
            for (int v = 0; v < VEC; v++) {
               const int o = (j * LPR + lc) * VEC + v;
               float t = sh_val[0][o];
               int ti = OP == OP_ADD ? 0 : sh_idx[0][o];
               for (int w = 1; w < WAVES; w++) {
                  const float ot = sh_val[w][o];
                  if (OP == OP_ADD) {
                     t += ot;
                  } else {
                     const int oi = sh_idx[w][o];
                     if (better<OP>(ot, oi, t, ti)) { t = ot; ti = oi; }
                  }
               }
               acc[j][v] = t;
               bi[j][v] = ti;
            }
         if (SLICED) write_partial<OP, VEC, NCH>(a, slice, lr, ccol, cok, vfirst, acc, bi);
         else write_row<OP, VEC, NCH>(a, lr, b, deg, ccol, cok, vfirst, acc, bi);
      }
      __syncthreads();
   }
}

// Finishes the sliced mode: folds the per-slice partials of one output row in slice order
// (ascending column = ascending CSR position, so the fold order is fixed and ties resolve
// to the lowest edge id), then applies what write_row applies: mean scale, empty-row value,
// absolute arg positions.  One thread per VEC output columns; coalesced along K.
template <int OP, int VEC>
__global__ __launch_bounds__(256) void combine_slices_kernel(const SpmmArgs a) {
   const int64_t kv = a.k / VEC;
   const int64_t total = a.m * kv;
   const int64_t stride = (int64_t)gridDim.x * blockDim.x;
   const size_t plane = (size_t)a.m * (size_t)a.k;
   for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
      const int64_t row = t / kv;
      const int c = (int)(t - row * kv) * VEC;
      const size_t off = (size_t)row * (size_t)a.k + c;
      float acc[VEC];
      int bi[VEC];
      load_vec<VEC>(a.part_val + off, acc);
      if (OP != OP_ADD) {
#pragma unroll
         for (int v = 0; v < VEC; v++) bi[v] = a.part_idx[off + v];
      }
      for (int s = 1; s < a.slices; s++) {
         float p[VEC];
         load_vec<VEC>(a.part_val + s * plane + off, p);
#pragma unroll
         for (int v = 0; v < VEC; v++) {
            if (OP == OP_ADD) {
               acc[v] += p[v];
            } else {
               const int oi = a.part_idx[s * plane + off + v];
               const bool take = better<OP>(p[v], oi, acc[v], bi[v]);
               acc[v] = take ? p[v] : acc[v];
               bi[v] = take ? oi : bi[v];
            }
         }
      }
      const int64_t rb = a.pntrb[row];
      const int64_t deg = a.pntre[row] - rb;
      if (OP == OP_ADD) {
         if (a.mean) {
            const float d = (float)(deg > 1 ? deg : 1);
#pragma unroll
            for (int v = 0; v < VEC; v++) acc[v] = acc[v] / d;
         }
      } else if (deg <= 0) {
#pragma unroll
         for (int v = 0; v < VEC; v++) acc[v] = a.empty_init ? identity<OP>() : 0.0f;
      }
      store_vec<VEC>(a.z + (size_t)row * (size_t)a.ldz + c, acc);
      if (OP != OP_ADD && a.z_arg) {
         int64_t *ar = a.z_arg + (size_t)row * (size_t)a.ldz + c;
#pragma unroll
         for (int v = 0; v < VEC; v++) ar[v] = bi[v] == INT_MAX ? a.nnz : rb + (int64_t)bi[v];
      }
   }
}

__global__ void dummy_kernel(int64_t flag) { (void)flag; }

template <int OP, int VEC, int LPR, int NCH, int ADDR>
static int launch_addr(const SpmmArgs &a0, hipStream_t st);

template <int OP, int CV>
static int launch_combine_vec(const SpmmArgs &a, hipStream_t st) {
   int64_t blocks = (a.m * (a.k / CV) + 255) / 256;
   if (blocks > 256 * 32) blocks = 256 * 32;
   hipLaunchKernelGGL((combine_slices_kernel<OP, CV>), dim3((unsigned)blocks), dim3(256), 0, st, a);
   return check_launch("combine_slices_kernel");
}

template <int OP>
static int launch_combine(const SpmmArgs &a, hipStream_t st) {   // vector width by the alignment of z and the planes
   const uintptr_t al = (uintptr_t)a.z;
   if (a.k % 4 == 0 && a.ldz % 4 == 0 && (al & 15) == 0) return launch_combine_vec<OP, 4>(a, st);
   if (a.k % 2 == 0 && a.ldz % 2 == 0 && (al & 7) == 0) return launch_combine_vec<OP, 2>(a, st);
   return launch_combine_vec<OP, 1>(a, st);
}

template <int OP, int VEC, int LPR, int NCH>
static int launch_cfg(const SpmmArgs &a, hipStream_t st) {
   if constexpr (VEC == 4) {
      if (a.ybytes != 0) return a.val ? launch_addr<OP, VEC, LPR, NCH, 2>(a, st) : launch_addr<OP, VEC, LPR, NCH, 1>(a, st);
   }
   return launch_addr<OP, VEC, LPR, NCH, 0>(a, st);
}

template <int OP, int VEC, int LPR, int NCH, int ADDR>
static int launch_addr(const SpmmArgs &a0, hipStream_t st) {
   constexpr int WAVES = 4;
   SpmmArgs a = a0;
   const int64_t nb = (a.m + WAVES - 1) / WAVES;
   if (nb > 0x7fffffffLL) return ISPLIB_FAIL;
   a.nblk = (unsigned)nb;
   constexpr int PANEL = LPR * VEC * NCH;
   const unsigned ny = (unsigned)((a.k + PANEL - 1) / PANEL);
   if (a.sliceptr) {
      if (a.slice_count > 0) {
         const int64_t gx = 8 * (((int64_t)a.slice_count * nb + 7) / 8);
         if (gx > 0x7fffffffLL) return ISPLIB_FAIL;
         hipLaunchKernelGGL((spmm_csr_kernel<OP, VEC, LPR, NCH, WAVES, true, ADDR>), dim3((unsigned)gx, ny, 1),
                            dim3(WAVES * 64, 1, 1), 0, st, a);
         int rc = check_launch("spmm_csr_kernel<sliced>");
         if (rc) return rc;
      }
      return a.combine ? launch_combine<OP>(a, st) : ISPLIB_SUCCESS;
   }
   hipLaunchKernelGGL((spmm_csr_kernel<OP, VEC, LPR, NCH, WAVES, false, ADDR>), dim3((unsigned)nb, ny, 1),
                      dim3(WAVES * 64, 1, 1), 0, st, a);
   return check_launch("spmm_csr_kernel");
}

int g_force_lpr = 0;   // tuning knob (isplib_hip_tune): lanes per row slot, 0 = by K
int g_addr_mode = 1;   // tuning knob: 0 = always 64-bit addressing, 1 = buffer descriptors when they fit
int g_tasks_per_wave = 0;   // tuning knob: consecutive tasks handled by one wave of the task kernel (0 = 2 for the pipelined variants, else 1)
int g_one_pass_kib = 9216;     // per-slice footprint of whole rows (KiB) up to which a plan runs in one pass (isplib_hip_tune(8, kib))
int g_panel_cols_minmax = 64;   // the same for max / min (isplib_hip_tune(5, w))
int g_panel_cols = 64;      // column-panel width of the task schedule for wide K (isplib_hip_tune(4, w); 0 = one pass)

template <int OP, int VEC>
static int launch_vec(const SpmmArgs &a, hipStream_t st) {
   int64_t width = (a.k + VEC - 1) / VEC;   // vector columns (ragged K: the last one is shifted back)
   if (g_force_lpr > 0 && g_force_lpr < width) width = g_force_lpr;   // narrower slots: K swept in grid.y panels
   // Operands beyond every cache, rows in index order (no community order was given or found): two rows per gather instruction
   // in 128-column panels instead of one 256-column row -- round 5, ogbn-products shape, K=256: Chung-Lu 19.5 -> 17.8 ms, SBM twin
   // in index order 18.4 -> 17.8 (64-column panels: the same again).  NOT when the rows come in a community order: the panels
   // then halve what a community's rows of y keep of the L2 per byte of index stream (8.94 -> 9.73 ms).  The panel form sums a
   // row's edges over two slots, so its last bits differ from the one-pass form's: isplib_hip_tune(0, 64) keeps one pass.
   else if (VEC == 4 && g_force_lpr == 0 && a.auto_panels && width > 32) width = 32;      // (measured on 16-byte lanes only)
   if (width <= 8) return launch_cfg<OP, VEC, 8, 1>(a, st);
   if (width <= 16) return launch_cfg<OP, VEC, 16, 1>(a, st);
   if (width <= 32) return launch_cfg<OP, VEC, 32, 1>(a, st);
   if (width <= 64) return launch_cfg<OP, VEC, 64, 1>(a, st);
   if (width <= 128) return launch_cfg<OP, VEC, 64, 2>(a, st);
   return launch_cfg<OP, VEC, 64, 4>(a, st);
}

template <int OP>
static int launch_op(const SpmmArgs &a, hipStream_t st) {
   const uintptr_t al = (uintptr_t)a.y | (uintptr_t)a.z;
   if (a.k % 4 == 0 && a.ldy % 4 == 0 && a.ldz % 4 == 0 && (al & 15) == 0) return launch_vec<OP, 4>(a, st);
   if (a.ybytes != 0 && a.k >= 4 && g_addr_mode == 1) return launch_vec<OP, 4>(a, st);   // ragged / dword-aligned rows
   if (a.k % 2 == 0 && a.ldy % 2 == 0 && a.ldz % 2 == 0 && (al & 7) == 0) return launch_vec<OP, 2>(a, st);
   return launch_vec<OP, 1>(a, st);
}

}  // namespace isplib

using namespace isplib;

// The index-order launch runs K > 128 in 128-column panels (launch_vec) when the dense operand is beyond the Infinity Cache.
extern "C" int isplib_plain_panels(int64_t n, int64_t ldy) {
   return (n > 0 && ldy > 0 && (double)n * (double)ldy * 4.0 > 256.0 * 1048576.0) ? 1 : 0;
}

static int spmm_entry(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                      const int64_t *indx, const int64_t *pntrb, const int64_t *pntre, const float *y, int64_t ldy,
                      float beta, float *z, int64_t ldz, int64_t *z_arg, const int64_t *sliceptr, int slices,
                      int slice_first, int slice_count, int combine, void *workspace, size_t workspace_bytes,
                      void *stream, const int32_t *row_order = nullptr) {
   clear_error();
   const int32_t vop = imessage & 0xF, rop = imessage & 0xF0, sop = imessage & 0xF00, vsc = imessage & 0xF000,
                 aop = imessage & 0xF0000;
   if (vop != ISPLIB_VOP_COPY_RHS || rop != ISPLIB_ROP_NOOP || sop != ISPLIB_SOP_COPY)
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_hip: only VOP_COPY_RHS|ROP_NOOP|SOP_COPY messages (SpMM) are implemented");
   if (vsc != ISPLIB_VSC_MUL && vsc != ISPLIB_VSC_MEAN)
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_hip: VSC must be MUL or MEAN");
   if (aop != ISPLIB_AOP_ADD && aop != ISPLIB_AOP_MAX && aop != ISPLIB_AOP_MIN)
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_hip: AOP must be ADD, MAX or MIN");
   if (vsc == ISPLIB_VSC_MEAN && aop != ISPLIB_AOP_ADD)
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_hip: VSC_MEAN is only defined with AOP_ADD");
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, "fusedMM_csr_hip: negative dimension");
   if (n > 0x7fffffffLL) return fail(ISPLIB_FAIL, "fusedMM_csr_hip: n must be < 2^31");
   if (beta != 0.0f) return fail(ISPLIB_FAIL, "fusedMM_csr_hip: beta must be 0 (z is write-only)");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldy < k || ldz < k) return fail(ISPLIB_FAIL, "fusedMM_csr_hip: leading dimension smaller than k");
   if (!pntrb || !pntre || !z || (nnz > 0 && (!indx || !y)))
      return fail(ISPLIB_FAIL, "fusedMM_csr_hip: null operand");

   SpmmArgs a;
   a.m = m; a.k = k; a.nnz = nnz;
   a.val = val; a.indx = indx; a.indx32 = nullptr; a.pntrb = pntrb; a.pntre = pntre;
   a.y = y; a.ldy = ldy; a.z = z; a.ldz = ldz; a.z_arg = z_arg;
   a.mean = (vsc == ISPLIB_VSC_MEAN) ? 1 : 0;
   a.empty_init = empty_row_init();
   a.long_row = 2048;
   a.nblk = 0;
   {
      const unsigned long long yb = (unsigned long long)n * (unsigned long long)ldy * 4ull;
      a.ybytes = (isplib_dense_in_descriptor(n, ldy) && g_addr_mode != 0) ? (unsigned)yb : 0u;
   }
   a.sliceptr = nullptr; a.slices = 1; a.slice_first = 0; a.slice_count = 0; a.combine = 0;
   a.part_val = nullptr; a.part_idx = nullptr;
   a.row_order = row_order;
   a.auto_panels = (!row_order && !sliceptr && isplib_plain_panels(n, ldy)) ? 1 : 0;
   if (sliceptr) {
      if (slices < 1 || slices > ISPLIB_MAX_SLICES) return fail(ISPLIB_FAIL, "fusedMM_csr_sliced_hip: slices must be in [1, 4096]");
      const size_t need = isplib_spmm_sliced_workspace_bytes(imessage, m, k, slices);
      if (!workspace || workspace_bytes < need) return fail(ISPLIB_NOT_ENOUGH_MEM, "fusedMM_csr_sliced_hip: workspace too small");
      if (((uintptr_t)workspace & 255) != 0) return fail(ISPLIB_FAIL, "fusedMM_csr_sliced_hip: workspace must be 256-byte aligned");
      if (slice_first < 0 || slice_first >= slices || slice_count < 0 || slice_count > slices)
         return fail(ISPLIB_FAIL, "fusedMM_csr_sliced_phase_hip: slice range outside [0, slices)");
      a.sliceptr = sliceptr; a.slices = slices;
      a.slice_first = slice_first; a.slice_count = slice_count; a.combine = combine ? 1 : 0;
      a.part_val = (float *)workspace;
      const size_t plane = ((size_t)slices * (size_t)m * (size_t)k * sizeof(float) + 255) & ~(size_t)255;
      a.part_idx = aop == ISPLIB_AOP_ADD ? nullptr : (int *)((char *)workspace + plane);
   }
   hipStream_t st = (hipStream_t)stream;
   if (aop == ISPLIB_AOP_ADD) return launch_op<OP_ADD>(a, st);
   if (aop == ISPLIB_AOP_MAX) return launch_op<OP_MAX>(a, st);
   return launch_op<OP_MIN>(a, st);
}

extern "C" int fusedMM_csr_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, float alpha, int64_t nnz,
                               int64_t rows, int64_t cols, const float *val, const int64_t *indx,
                               const int64_t *pntrb, const int64_t *pntre, const float *x, int64_t ldx,
                               const float *y, int64_t ldy, float beta, float *z, int64_t ldz, int64_t *z_arg,
                               void *stream) {
   const int32_t head = imessage & 0xFFF, vsc = imessage & 0xF000;
   const bool spmm_word = head == (ISPLIB_VOP_COPY_RHS | ISPLIB_ROP_NOOP | ISPLIB_SOP_COPY) &&
                          (vsc == ISPLIB_VSC_MUL || vsc == ISPLIB_VSC_MEAN) && (imessage >> 20) == 0;
   if (!spmm_word)      // SDDMM-fused words: the generic pipeline (no user function: *_UDEF stages are refused there)
      return fusedMM_csr_udef_hip(imessage, m, n, k, alpha, nnz, rows, cols, val, indx, pntrb, pntre, x, ldx, y, ldy, beta,
                                  z, ldz, z_arg, ISPLIB_SOP_NONE, 0.0f, stream);
   return spmm_entry(imessage, m, n, k, nnz, val, indx, pntrb, pntre, y, ldy, beta, z, ldz, z_arg, nullptr, 1, 0, 0, 0,
                     nullptr, 0, stream);
}

extern "C" int fusedMM_csr_ordered_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz, const float *val,
                                       const int64_t *indx, const int64_t *pntrb, const int64_t *pntre,
                                       const int32_t *row_order, const float *y, int64_t ldy, float *z, int64_t ldz,
                                       int64_t *z_arg, void *stream) {
   if (m >= (1LL << 31)) {
      clear_error();
      return fail(ISPLIB_FAIL, "fusedMM_csr_ordered_hip: m must be < 2^31 (32-bit row order)");
   }
   return spmm_entry(imessage, m, n, k, nnz, val, indx, pntrb, pntre, y, ldy, 0.0f, z, ldz, z_arg, nullptr, 1, 0, 0, 0,
                     nullptr, 0, stream, row_order);
}

extern "C" size_t isplib_spmm_sliced_workspace_bytes(int32_t imessage, int64_t m, int64_t k, int slices) {
   if (m <= 0 || k <= 0 || slices <= 0) return 256;
   const size_t plane = ((size_t)slices * (size_t)m * (size_t)k * sizeof(float) + 255) & ~(size_t)255;
   const bool minmax = (imessage & 0xF0000) != ISPLIB_AOP_ADD;
   return plane * (minmax ? 2 : 1);
}

extern "C" int fusedMM_csr_sliced_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                      const float *val, const int64_t *indx, const int64_t *pntrb,
                                      const int64_t *pntre, const int64_t *sliceptr, int slices, const float *y,
                                      int64_t ldy, float *z, int64_t ldz, int64_t *z_arg, void *workspace,
                                      size_t workspace_bytes, void *stream) {
   if (!sliceptr) {
      clear_error();
      return fail(ISPLIB_FAIL, "fusedMM_csr_sliced_hip: sliceptr is required");
   }
   return spmm_entry(imessage, m, n, k, nnz, val, indx, pntrb, pntre, y, ldy, 0.0f, z, ldz, z_arg, sliceptr, slices, 0,
                     slices, 1, workspace, workspace_bytes, stream);
}

extern "C" int fusedMM_csr_sliced_phase_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                            const float *val, const int64_t *indx, const int64_t *pntrb,
                                            const int64_t *pntre, const int64_t *sliceptr, int slices,
                                            int slice_first, int slice_count, int combine, const float *y,
                                            int64_t ldy, float *z, int64_t ldz, int64_t *z_arg, void *workspace,
                                            size_t workspace_bytes, void *stream) {
   if (!sliceptr) {
      clear_error();
      return fail(ISPLIB_FAIL, "fusedMM_csr_sliced_phase_hip: sliceptr is required");
   }
   return spmm_entry(imessage, m, n, k, nnz, val, indx, pntrb, pntre, y, ldy, 0.0f, z, ldz, z_arg, sliceptr, slices,
                     slice_first, slice_count, combine, workspace, workspace_bytes, stream);
}


extern "C" int isplib_hip_tune(int key, int value) {
   if (key == 0) { g_force_lpr = value; return ISPLIB_SUCCESS; }
   if (key == 1) { g_addr_mode = value; return ISPLIB_SUCCESS; }
   if (key == 2) { g_tasks_per_wave = value; return ISPLIB_SUCCESS; }
   if (key == 4) { g_panel_cols = value; return ISPLIB_SUCCESS; }
   if (key == 5) { g_panel_cols_minmax = value; return ISPLIB_SUCCESS; }
   if (key == 8 && value >= 0) { g_one_pass_kib = value; return ISPLIB_SUCCESS; }
   return ISPLIB_FAIL;      // (9 and 12: isplib_hip_tune_experimental, include/isplib_hip_experimental.h; 10 and 11 are gone)
}

// not in include/isplib_hip.h: the experimental library's knob 12 (column panels of the task-list SDDMM, measured slower)
extern "C" int isplib_internal_set_sddmm_panel_cols(int cols) {
   if (cols < 0) return ISPLIB_FAIL;
   g_sddmm_panel_cols = cols;
   return ISPLIB_SUCCESS;
}

extern "C" void performDummySpMM_hip(int64_t flag, void *stream) {
   clear_error();
   hipLaunchKernelGGL(dummy_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flag);
   (void)check_launch("dummy_kernel");
}
