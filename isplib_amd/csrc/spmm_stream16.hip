// spmm_stream16.hip -- the stream schedule of the SpMM (spmm_sweep.hip) for dense operands of 16-bit elements
// (bf16, fp16): fusedMM_csr_stream16_hip, sum / mean.  Same plans, same geometry table, same front end (sweep_common.h) as the fp32
// kernel: a lane owns the same four columns of its slot's panel row, but its gather is 8 bytes instead of 16 -- a 64-column panel
// row is ONE 128-byte line instead of two, and the loop is charged per line.  The four halves are widened in
// registers; everything after that is the fp32 kernel's: the running sum in fp32 registers, the fp32 LDS rows, the word rotation
// with the weights (fp32, the plan's own) one batch behind.  A finished row is rounded ONCE, to nearest even, when it is written:
// hub rows cut into virtual rows keep their partial rows in fp32 in the workspace and round in the fold.
//
// The contract: the result equals the fp32 computation on the widened operand, rounded once to the operand's type -- NaN stays
// NaN, bf16 keeps subnormals, fp16 overflows to +-Inf.  No epilogue, no staged panels, no max / min here.
#include "sweep_common.h"
#include "half16.h"

namespace isplib {

typedef unsigned v2u_t __attribute__((ext_vector_type(2)));

// (widen2 / narrow2, the conversions between a gathered dword and two floats: half16.h)

// the four finished columns of a lane as 8 bytes at p (4-byte aligned: k, the pitch and the columns are even); the first `vfirst`
// components belong to the neighbouring lane (the last vector of a ragged panel is shifted back to end at column k) and are skipped
template <int ELT> __device__ __forceinline__ void store_tail16(unsigned short *p, const float (&r)[4], int vfirst) {
   const unsigned d0 = narrow2<ELT>(r[0], r[1]), d1 = narrow2<ELT>(r[2], r[3]);
   if (vfirst == 0) {
      if (((uintptr_t)p & 7) == 0) {
         *reinterpret_cast<uint2 *>(p) = make_uint2(d0, d1);
      } else {
         reinterpret_cast<unsigned *>(p)[0] = d0;
         reinterpret_cast<unsigned *>(p)[1] = d1;
      }
   } else if (vfirst == 2) {
      reinterpret_cast<unsigned *>(p)[1] = d1;
   } else {                                               // odd: not reachable from the entry (k even); kept whole
      if (vfirst <= 1) p[1] = (unsigned short)(d0 >> 16);
      if (vfirst <= 1) p[2] = (unsigned short)(d1 & 0xFFFFu);
      p[3] = (unsigned short)(d1 >> 16);
   }
}

// stream_columns / stream_bounds / stream_issue of sweep_common.h at two bytes per element
template <class SW> __device__ __forceinline__ void stream_columns16(const SweepArgs &a, SW &sw) {
   stream_columns<true>(a, sw);
   sw.cbyte = (unsigned)sw.ccol * 2u;
}
template <class SW> __device__ __forceinline__ void stream_bounds16(const SweepArgs &a, SW &sw) {
   stream_bounds(a, sw);
   sw.ldyb = (unsigned)a.ldy * 2u;
}
template <class SW>
__device__ __forceinline__ void stream_issue16(const SW &sw, __amdgpu_buffer_rsrc_t rsrc, const unsigned (&word_l)[SW::NBW], int u, unsigned &la, v2u_t &t) {
   const unsigned word = (unsigned)__shfl((int)word_l[(u * SW::G) / 64], (u * SW::G) % 64 + sw.g);
   const unsigned o = (__umul24(word & 0xFFFFFFu, sw.ldyb) + sw.cbyte) | sw.poison;
   la = (word >> 24) * (unsigned)SW::PANEL;
   t = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)o, 0, 0);
}

// spmm_stream_kernel (spmm_sweep.hip) with 8-byte gathers; the order of the batch loads is that kernel's (sweep_common.h: it
// decides the register allocation of the loop)
template <int ELT, int LPR, bool HAS_VAL, int NVMAX, int NBW, int WGS>
__global__ __launch_bounds__(256, (stream_wgs_per_cu<LPR, NVMAX, WGS>())) void spmm_stream16_kernel(const SweepArgs a) {
   using Wave = StreamWave<LPR, NVMAX, NBW>;
   constexpr int WAVES = Wave::WAVES, G = Wave::G, PANEL = Wave::PANEL, U = Wave::U, PER = Wave::PER;
   constexpr int WAVE_FLOATS = NVMAX * PANEL;
   static_assert(NVMAX <= 256 && NVMAX % G == 0, "the local row is the top byte of a word");
   __shared__ __attribute__((aligned(16))) float s_all[WAVES * WAVE_FLOATS];
   Wave sw;
   if (!stream_wave_id(a, sw)) return;                   // no barrier anywhere below
   const int lane = sw.lane;
   float *my = s_all + sw.wave * WAVE_FLOATS;
   for (int i = lane * 4; i < WAVE_FLOATS; i += 256)
      *reinterpret_cast<float4 *>(my + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   __amdgpu_buffer_rsrc_t rsrc = dense_rsrc(a);
   stream_columns16(a, sw);
   float *lane_base = my + sw.lc * 4;                     // a lane's four columns of a row are contiguous
   stream_bounds16(a, sw);
   const float *vp = HAS_VAL ? a.vals + sw.s0 * G : nullptr;
   unsigned w1[NBW], w2[NBW];                             // the words of the next batch and of the one after it
   float v0[NBW] = {}, v1[NBW] = {};                      // the weights of the batch being consumed and of the next
   v2u_t t[U];
   unsigned la[U];
   const unsigned pad_word = stream_pad_own_row(a, sw);
   stream_load_batch(sw, sw.wp, 0, pad_word, w1);
   if (HAS_VAL) stream_load_batch(sw, vp, 0, 0.0f, v0);
#pragma unroll
   for (int u = 0; u < U; u++) stream_issue16(sw, rsrc, w1, u, la[u], t[u]);
   stream_load_batch(sw, sw.wp, 64 * NBW, pad_word, w1);
   if (HAS_VAL) stream_load_batch(sw, vp, 64 * NBW, 0.0f, v1);
   stream_load_batch(sw, sw.wp, 128 * NBW, pad_word, w2);
   unsigned cur = (unsigned)(sw.g * PER * PANEL);         // the row whose running sum the registers hold (stream_flush)
   float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
   const int64_t nb = (sw.nwords + 64 * NBW - 1) / (64 * NBW);
   for (int64_t b = 0; b < nb; b++) {
      // the U gathers of batch b are in flight; each one consumed is replaced by the same step of batch b + 1
      float vnext = HAS_VAL ? __shfl(v0[0], sw.g) : 0.0f;
#pragma unroll
      for (int u = 0; u < U; u++) {
         const float vcur = vnext;
         if (HAS_VAL && u + 1 < U) vnext = __shfl(v0[((u + 1) * G) / 64], ((u + 1) * G) % 64 + sw.g);
         if (la[u] != cur) {                             // per lane: the slots of a wave change rows at different steps
            stream_flush(lane_base + cur, acc);
            cur = la[u];
            acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
         }
         float x[4];
         widen2<ELT>(t[u][0], x[0], x[1]);
         widen2<ELT>(t[u][1], x[2], x[3]);
#pragma unroll
         for (int v = 0; v < 4; v++) acc[v] = HAS_VAL ? fmaf(vcur, x[v], acc[v]) : acc[v] + x[v];
         stream_issue16(sw, rsrc, w1, u, la[u], t[u]);
      }
#pragma unroll
      for (int q = 0; q < NBW; q++) { w1[q] = w2[q]; v0[q] = v1[q]; }
      stream_load_batch(sw, sw.wp, (b + 3) * 64 * NBW, pad_word, w2);
      if (HAS_VAL) stream_load_batch(sw, vp, (b + 2) * 64 * NBW, 0.0f, v1);
   }
   stream_flush(lane_base + cur, acc);
   // write-out, as in the fp32 kernel: the slot's row ids first, the rows then four at a time.  A partial row of a hub row goes to
   // the workspace as it is, in fp32; a whole row is finished in fp32 (the mean's division) and rounded here, once
   int row_[PER], part_[PER];
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      row_[jj] = sw.cok ? a.wave_row[(size_t)sw.w * NVMAX + sw.g * PER + jj] : -1;
      part_[jj] = a.wave_part[(size_t)sw.w * NVMAX + sw.g * PER + jj];
   }
   unsigned short *z16 = reinterpret_cast<unsigned short *>(a.z);
#pragma unroll 4
   for (int jj = 0; jj < PER; jj++) {
      const int lrow = sw.g * PER + jj;
      const int row = row_[jj];
      if (row < 0) continue;
      const int part = part_[jj];
      const float4 t4 = *reinterpret_cast<const float4 *>(lane_base + lrow * PANEL);
      float v[4] = {t4.x, t4.y, t4.z, t4.w};
      int bi[4] = {INT_MAX, INT_MAX, INT_MAX, INT_MAX};
      const int c = sw.ccol;
      if (part >= 0) {
         store_tail<4>(a.part_val + (size_t)part * (size_t)a.k + c, v, sw.vfirst);
         continue;
      }
      int64_t arg[4];
      finish_row<OP_ADD>(a, row, c, v, bi, arg);
      store_tail16<ELT>(z16 + (size_t)row * (size_t)a.ldz + c, v, sw.vfirst);
   }
}

// sweep_hub_fold_kernel for a 16-bit output: the fp32 partial rows of a hub row are added in chunk order, the row is finished in
// fp32 and rounded once.  Two columns per thread (k, ldz even: one aligned 4-byte store; the partial rows' pairs are 8-byte aligned)
template <int ELT>
__global__ __launch_bounds__(256) void sweep_hub_fold16_kernel(const SweepArgs a) {
   const int64_t kv = a.k / 2;
   const int64_t total = a.n_hub * kv;
   const int64_t stride = (int64_t)gridDim.x * blockDim.x;
   unsigned short *z16 = reinterpret_cast<unsigned short *>(a.z);
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t h = i / kv;
      const int c = (int)(i - h * kv) * 2;
      float v[2] = {0.0f, 0.0f};
      int bi[2] = {INT_MAX, INT_MAX};
      const int p1 = a.hub_off[h + 1];
      for (int p = a.hub_off[h]; p < p1; p++) {
         float t[2];
         load_vec<2>(a.part_val + (size_t)p * (size_t)a.k + c, t);
         v[0] += t[0];
         v[1] += t[1];
      }
      const int row = a.hub_row[h];
      int64_t arg[2];
      finish_row<OP_ADD, 2>(a, row, c, v, bi, arg);
      *reinterpret_cast<unsigned *>(z16 + (size_t)row * (size_t)a.ldz + c) = narrow2<ELT>(v[0], v[1]);
   }
}

template <int ELT, int STREAMS, bool HAS_VAL>
static int launch_stream16(const SweepArgs &a, hipStream_t st) {
   constexpr StreamGeom ge = stream_geom(STREAM_SUM, STREAMS);
   const unsigned blocks = (unsigned)((a.wave_count + 3) / 4);
   if (blocks == 0) return ISPLIB_SUCCESS;
   hipLaunchKernelGGL((spmm_stream16_kernel<ELT, ge.lpr, HAS_VAL, ge.nvmax, ge.nbw, ge.wgs>), dim3(blocks), dim3(256), 0, st, a);
   return check_launch("spmm_stream16_kernel");
}

template <int ELT>
static int launch_hub_fold16(const SweepArgs &p, hipStream_t st) {
   if (p.n_hub <= 0) return ISPLIB_SUCCESS;
   int64_t blocks = (p.n_hub * (p.k / 2) + 255) / 256;
   if (blocks > 4096) blocks = 4096;
   hipLaunchKernelGGL((sweep_hub_fold16_kernel<ELT>), dim3((unsigned)blocks), dim3(256), 0, st, p);
   return check_launch("sweep_hub_fold16_kernel");
}

// run_stream_panels (sweep_common.h) with the panel's column offset counted in 2-byte elements: every generation, then the hub
// fold, per panel of the plan's slot width.  A sliver of 2 columns is widened backwards to 4 (the overlap is rewritten identically)
template <int ELT>
static int run_stream16(const isplib_stream_plan *plan, const SweepArgs &a, hipStream_t st) {
   const int64_t k = a.k, pw = 256 / plan->streams;
   const bool has_val = plan->vals != nullptr;
   for (int64_t c0 = 0; c0 < k; c0 += pw) {
      SweepArgs p = a;
      p.k = (k - c0) < pw ? (k - c0) : pw;
      if (p.k < 4) {
         p.k = 4;
         c0 = k - 4;
      }
      p.y = reinterpret_cast<const float *>(reinterpret_cast<const unsigned short *>(a.y) + c0);
      p.z = reinterpret_cast<float *>(reinterpret_cast<unsigned short *>(a.z) + c0);
      p.ybytes = a.ybytes - (unsigned)c0 * 2u;            // row n, the padding words' column, stays outside the descriptor
      int rc = run_generations(plan->gens, plan->waves_per_gen, p, [&](const SweepArgs &q) {
         return with_streams<STREAM_SUM>(plan->streams, [&](auto s) {
            return has_val ? launch_stream16<ELT, s(), true>(q, st) : launch_stream16<ELT, s(), false>(q, st);
         });
      });
      if (!rc) rc = launch_hub_fold16<ELT>(p, st);
      if (rc) return rc;
   }
   return ISPLIB_SUCCESS;
}

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_stream16_auto(int streams, int weighted) { return isplib_stream16_native_pays(streams, weighted); }

extern "C" int fusedMM_csr_stream16_hip(int32_t imessage, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                        const int64_t *pntrb, const int64_t *pntre, const isplib_stream_plan *plan,
                                        const void *y, int64_t ldy, void *z, int64_t ldz, void *workspace,
                                        size_t workspace_bytes, void *stream) {
   clear_error();
   const char *entry = "fusedMM_csr_stream16_hip";
   if (imessage != ISPLIB_MSG_SPMM_SUM && imessage != ISPLIB_MSG_SPMM_MEAN)
      return fail(ISPLIB_NO_OPT_IMPL, entry, "sum and mean only (max / min of a 16-bit operand: convert it and use fusedMM_csr_stream_minmax_hip)");
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, "dtype must be ISPLIB_DTYPE_BF16 or ISPLIB_DTYPE_F16");
   const bool empty = m == 0 || k == 0;
   if (m >= 0 && n >= 0 && k >= 0 && nnz >= 0 && !empty && !isplib_stream16_serves(n, k, ldy, ldz, nnz))
      return fail(ISPLIB_FAIL, entry, "outside isplib_stream16_serves(n, k, ldy, ldz, nnz): k >= 4, k / ldy / ldz even, n < 2^24, ldy < 2^22, "
                                      "n*ldy*2 <= 3.5 GiB, nnz < 2^31 (convert the operand and use fusedMM_csr_stream_hip)");
   StreamCall c = {entry, "fusedMM_csr_stream_hip on the converted operand", STREAM_SUM, m, n, k, nnz, empty, pntrb, pntre, plan,
                   reinterpret_cast<const float *>(y), ldy, /* ld_other */ ldz, /* others */ z != nullptr, /* hub_fold */ true,
                   workspace, workspace_bytes, stream_parts_bytes(plan)};
   c.elt_bytes = 2;
   bool done;
   int rc = check_stream_call(c, &done);
   if (done) return rc;
   if ((((uintptr_t)y | (uintptr_t)z) & 3) != 0) return fail(ISPLIB_FAIL, entry, "y and z must be 4-byte aligned");
   if ((rc = check_stream_workspace(c)) != ISPLIB_SUCCESS) return rc;
   SweepArgs a = stream_args(c, reinterpret_cast<float *>(z), ldz);
   a.ybytes = (unsigned)((unsigned long long)n * (unsigned long long)ldy * 2ull);
   a.mean = imessage == ISPLIB_MSG_SPMM_MEAN ? 1 : 0;
   hipStream_t st = (hipStream_t)stream;
   return dtype == ISPLIB_DTYPE_BF16 ? run_stream16<ELT_BF16>(plan, a, st) : run_stream16<ELT_F16>(plan, a, st);
}
