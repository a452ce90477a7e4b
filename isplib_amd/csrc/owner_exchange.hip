// owner_exchange.hip -- the sender's half of the owner-bucketed exchange of the partitioned max / min backward
// (isplib_minmax_bw_bucket_hip; the receiver's half, isplib_scatter_keys_det_hip, lives with the run sums in backward_det.hip).
//
// A rank's m x k winners become (key, value) pairs and are split by the rank that owns the destination row: a STABLE multi-way
// split, so every owner's segment keeps ascending t = i*k + c and the owner, laying the segments side by side in source-rank
// order, holds its pairs in ascending global row order -- the order isplib_scatter_rows_det_hip adds them up in.
//   1. count    a block owns a tile of BUCKET_TILE consecutive pairs, read striped (item j * 256 + tid: coalesced, and iteration,
//               then wave, then lane is ascending t); per wave and bucket ONE lane (the lowest of the bucket) adds the bucket's
//               lane count to the wave's LDS row (an LDS integer add: the counts commute, no placement hangs on their order);
//               the block's histogram goes to hist[bucket][block]
//   2. scan     one exclusive scan over that bucket-major table: the global write position of every (bucket, block)
//   3. scatter  the same walk; position = block base + pairs of earlier (iteration, wave) steps of the block (an LDS table,
//               scanned by one thread per bucket) + lower lanes of the same bucket in the wave
// A lane's bucket mates are found with ceil(log2(world + 1)) ballots over the bits of the bucket id (bucket `world` = no winner /
// dropped: counted like any other, so that every lane takes part, and written nowhere).  No atomic decides a placement.
// The scatter pass recomputes indx[arg] instead of reading it back from a plane the count pass would write: both passes then
// need no scratch beyond the histogram, and the second gather hits the L2 the first one filled.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/isplib_hip.h"
#include "common.h"

#include "prims.h"

namespace isplib {

constexpr int BUCKET_THREADS = 256, BUCKET_WAVES = BUCKET_THREADS / 64, BUCKET_ITEMS = 8;
constexpr int BUCKET_TILE = BUCKET_THREADS * BUCKET_ITEMS;                      // 2,048 pairs per block
constexpr int BUCKET_SLOTS = ISPLIB_OWNER_WORLD_MAX + 1;                        // the owners + "no winner"
constexpr int BUCKET_STEPS = BUCKET_ITEMS * BUCKET_WAVES;                       // (iteration, wave) steps of a block, in order of t

struct OwnerCuts {
   int64_t c[ISPLIB_OWNER_WORLD_MAX + 1];                                       // by value: no device copy, nothing to keep alive
};

struct Pair {
   int bucket;
   uint32_t key;
   float value;
};

// the pair of element t (bucket == world: none); cuts: the block's LDS copy
template <bool WITH_VALUE>
__device__ __forceinline__ Pair owner_pair(int64_t t, int64_t total, uint32_t k, int64_t nnz, int64_t edge0, int world, const int64_t *cuts,
                                           const int64_t *__restrict__ arg, const int64_t *__restrict__ indx,
                                           const float *__restrict__ val, const float *__restrict__ grad_out) {
   Pair p = {world, 0u, 0.0f};
   if (t >= total) return p;
   const int64_t a = arg[t] - edge0;
   if (a < 0 || a >= nnz) return p;
   const int64_t d = indx[a];
   if (d < cuts[0] || d >= cuts[world]) return p;
   int lo = 0, hi = world - 1;                                                  // the owner: cuts[lo] <= d < cuts[lo + 1]
   while (lo < hi) {                                                            // (an empty shard, cuts[p] == cuts[p+1], owns nothing)
      const int mid = (lo + hi) >> 1;
      if (cuts[mid + 1] <= d) lo = mid + 1;
      else hi = mid;
   }
   p.bucket = lo;
   p.key = (uint32_t)(d - cuts[lo]) * k + (uint32_t)t % k;
   if (WITH_VALUE) p.value = (val ? val[a] : 1.0f) * grad_out[t];
   return p;
}

// the lanes of this wave whose bucket equals this lane's (every lane of the wave takes part)
__device__ __forceinline__ uint64_t bucket_mates(int bucket, int id_bits) {
   uint64_t mates = ~0ull;
   for (int b = 0; b < id_bits; b++) {
      const bool bit = (bucket >> b) & 1;
      const uint64_t with = __ballot(bit);
      mates &= bit ? with : ~with;
   }
   return mates;
}

__device__ __forceinline__ int lanes_below(uint64_t mask) {                     // set bits of mask below this lane
   return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

__global__ __launch_bounds__(BUCKET_THREADS) void owner_count_kernel(int64_t total, uint32_t k, int64_t nnz, int64_t edge0, int world, int id_bits,
                                                                     OwnerCuts cuts_arg, const int64_t *__restrict__ arg,
                                                                     const int64_t *__restrict__ indx, int64_t *__restrict__ hist) {
   __shared__ int64_t cuts[BUCKET_SLOTS];
   __shared__ int count[BUCKET_WAVES][BUCKET_SLOTS];
   const int tid = (int)threadIdx.x, wave = tid >> 6;
   if (tid <= world) cuts[tid] = cuts_arg.c[tid];
   for (int e = tid; e < BUCKET_WAVES * BUCKET_SLOTS; e += BUCKET_THREADS) (&count[0][0])[e] = 0;
   __syncthreads();
   const int64_t base = (int64_t)blockIdx.x * BUCKET_TILE;
#pragma unroll
   for (int j = 0; j < BUCKET_ITEMS; j++) {
      const Pair p = owner_pair<false>(base + j * BUCKET_THREADS + tid, total, k, nnz, edge0, world, cuts, arg, indx, nullptr, nullptr);
      const uint64_t mates = bucket_mates(p.bucket, id_bits);
      if (lanes_below(mates) == 0) atomicAdd(&count[wave][p.bucket], __popcll(mates));   // one lane per bucket and step; integer counts: any order, one sum
   }
   __syncthreads();
   if (tid <= world) {
      int sum = 0;
      for (int w = 0; w < BUCKET_WAVES; w++) sum += count[w][tid];
      hist[(int64_t)tid * gridDim.x + blockIdx.x] = sum;
   }
}

__global__ __launch_bounds__(BUCKET_THREADS) void owner_scatter_kernel(int64_t total, uint32_t k, int64_t nnz, int64_t edge0, int world, int id_bits,
                                                                       OwnerCuts cuts_arg, const int64_t *__restrict__ arg,
                                                                       const int64_t *__restrict__ indx, const float *__restrict__ val,
                                                                       const float *__restrict__ grad_out, const int64_t *__restrict__ offs,
                                                                       uint32_t *__restrict__ keys, float *__restrict__ vals,
                                                                       int64_t *__restrict__ seg_off) {
   __shared__ int64_t cuts[BUCKET_SLOTS];
   __shared__ int64_t block_base[BUCKET_SLOTS];
   __shared__ int step[BUCKET_STEPS][BUCKET_SLOTS];                               // pairs of a bucket in one (iteration, wave) step, then their prefix
   const int tid = (int)threadIdx.x, wave = tid >> 6;
   if (tid <= world) {
      cuts[tid] = cuts_arg.c[tid];
      block_base[tid] = offs[(int64_t)tid * gridDim.x + blockIdx.x];
      if (blockIdx.x == 0) seg_off[tid] = block_base[tid];                       // bucket-major: a bucket's first block starts its segment
   }
   for (int e = tid; e < BUCKET_STEPS * BUCKET_SLOTS; e += BUCKET_THREADS) (&step[0][0])[e] = 0;
   __syncthreads();
   const int64_t base = (int64_t)blockIdx.x * BUCKET_TILE;
   Pair pairs[BUCKET_ITEMS];
   int below[BUCKET_ITEMS];
#pragma unroll
   for (int j = 0; j < BUCKET_ITEMS; j++) {
      pairs[j] = owner_pair<true>(base + j * BUCKET_THREADS + tid, total, k, nnz, edge0, world, cuts, arg, indx, val, grad_out);
      const uint64_t mates = bucket_mates(pairs[j].bucket, id_bits);
      below[j] = lanes_below(mates);
      if (below[j] == 0) step[j * BUCKET_WAVES + wave][pairs[j].bucket] = __popcll(mates);
   }
   __syncthreads();
   if (tid < world) {                                                           // exclusive prefix over the steps, in the order of t
      int run = 0;
      for (int s = 0; s < BUCKET_STEPS; s++) {
         const int c = step[s][tid];
         step[s][tid] = run;
         run += c;
      }
   }
   __syncthreads();
#pragma unroll
   for (int j = 0; j < BUCKET_ITEMS; j++) {
      const int b = pairs[j].bucket;
      if (b < world) {
         const int64_t at = block_base[b] + step[j * BUCKET_WAVES + wave][b] + below[j];
         keys[at] = pairs[j].key;
         vals[at] = pairs[j].value;
      }
   }
}

__global__ void owner_no_pairs_kernel(int world, int64_t *__restrict__ seg_off) {       // m*k == 0: every segment is empty
   if ((int)threadIdx.x <= world) seg_off[threadIdx.x] = 0;
}

static inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

static inline int64_t bucket_blocks(int64_t total) { return (total + BUCKET_TILE - 1) / BUCKET_TILE; }

}  // namespace isplib

using namespace isplib;

extern "C" size_t isplib_minmax_bw_bucket_workspace_bytes(int64_t m, int64_t k, int world) {
   if (world < 1 || world > ISPLIB_OWNER_WORLD_MAX || m < 0 || k < 0) return 0;
   if (!isplib_product_within(m, k, ISPLIB_MINMAX_BW_PAIRS_END - 1u)) return 0;
   if (m == 0 || k == 0) return 256;
   const size_t cells = (size_t)bucket_blocks(m * k) * (size_t)(world + 1);
   size_t temp = 0;
   if (scan_exclusive_i64(nullptr, temp, nullptr, nullptr, cells, (hipStream_t)0) != hipSuccess) { (void)hipGetLastError(); return 0; }
   return 2 * up256(cells * 8) + up256(temp) + 256;
}

extern "C" int isplib_minmax_bw_bucket_hip(int64_t m, int64_t k, int64_t nnz, int64_t edge0, const int64_t *arg, const int64_t *indx,
                                           const float *val, const float *grad_out, int world, const int64_t *cuts_host, uint32_t *keys,
                                           float *vals, int64_t *seg_off, void *workspace, size_t workspace_bytes, void *stream) {
   clear_error();
   const char *const me = "isplib_minmax_bw_bucket_hip";
   if (m < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, me, "negative dimension");
   if (world < 1 || world > ISPLIB_OWNER_WORLD_MAX) return fail(ISPLIB_FAIL, me, "world outside 1..ISPLIB_OWNER_WORLD_MAX");
   if (!cuts_host || !seg_off) return fail(ISPLIB_FAIL, me, "null operand");
   for (int p = 0; p < world; p++)
      if (cuts_host[p + 1] < cuts_host[p]) return fail(ISPLIB_FAIL, me, "cuts must ascend");
   if (!isplib_owner_exchange_serves(m, k, world, cuts_host))
      return fail(ISPLIB_NO_OPT_IMPL, me, "m*k or an owner's rows*k beyond 32-bit keys (isplib_owner_exchange_serves)");
   hipStream_t st = (hipStream_t)stream;
   const int64_t total = m * k;
   if (total == 0) {                                                             // no pair: every segment is empty
      hipLaunchKernelGGL(owner_no_pairs_kernel, dim3(1), dim3(128), 0, st, world, seg_off);   // (a kernel, not a memset: see zero_f32_kernel)
      return check_launch("owner_no_pairs_kernel");
   }
   if (!arg || !grad_out || !keys || !vals || (nnz > 0 && !indx)) return fail(ISPLIB_FAIL, me, "null operand");
   const size_t need = isplib_minmax_bw_bucket_workspace_bytes(m, k, world);
   if (need == 0) return fail(ISPLIB_NO_OPT_IMPL, me, "not served");
   if (!workspace || workspace_bytes < need) return fail(ISPLIB_NOT_ENOUGH_MEM, me, "workspace too small");
   if (((uintptr_t)workspace & 255) != 0) return fail(ISPLIB_FAIL, me, "workspace must be 256-byte aligned");
   const int64_t blocks = bucket_blocks(total);
   const size_t cells = (size_t)blocks * (size_t)(world + 1);
   char *w = (char *)workspace;
   int64_t *hist = (int64_t *)w, *offs = (int64_t *)(w + up256(cells * 8));
   void *temp = w + 2 * up256(cells * 8);
   size_t temp_bytes = 0;
   ISPLIB_HIP_TRY(scan_exclusive_i64(nullptr, temp_bytes, nullptr, nullptr, cells, (hipStream_t)0));
   OwnerCuts cuts;
   for (int p = 0; p <= ISPLIB_OWNER_WORLD_MAX; p++) cuts.c[p] = cuts_host[p <= world ? p : world];
   int id_bits = 0;
   while ((1 << id_bits) < world + 1) id_bits++;
   hipLaunchKernelGGL(owner_count_kernel, dim3((unsigned)blocks), dim3(BUCKET_THREADS), 0, st, total, (uint32_t)k, nnz, edge0, world, id_bits, cuts,
                      arg, indx, hist);
   int rc = check_launch("owner_count_kernel");
   if (rc) return rc;
   ISPLIB_HIP_TRY(scan_exclusive_i64(temp, temp_bytes, hist, offs, cells, st));
   hipLaunchKernelGGL(owner_scatter_kernel, dim3((unsigned)blocks), dim3(BUCKET_THREADS), 0, st, total, (uint32_t)k, nnz, edge0, world, id_bits, cuts,
                      arg, indx, val, grad_out, offs, keys, vals, seg_off);
   return check_launch("owner_scatter_kernel");
}
