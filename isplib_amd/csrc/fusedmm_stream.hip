// fusedmm_stream.hip -- the SDDMM-fused FusedMM words on the stream front end (fusedMM_csr_udef_stream_hip).
//
// The generic pipeline z_i = AOP_j VSC(SOP(ROP(VOP(x_i, y_j)))) (csrc/fusedMM.h:18-74) gathers the same rows of y over the same
// edges as the SpMM; on the task list (fusedmm_general.hip) its two hot shapes -- the sigmoid / attention family
// COPY_RHS|DOT|UDEF|MUL|ADD and the t-distribution family SUBR|NORMR|UDEF|MUL|ADD of the FusedMM paper's graph-embedding
// kernels -- took 6.3 ms at K=128 on the Reddit shape where the SpMM that gathers the same rows takes 2.7.  Here they run
// on the stream schedule's front end (spmm_sweep.hip): word streams, one full 1-KiB gather per step, 32 gathers in flight
// per wave, two waves per SIMD, rows resident in LDS.  What differs from the SpMM:
//   * the reduce stage needs the WHOLE row of y before anything can be accumulated, so a slot spans the full width (k <= 128:
//     32-lane slots, two rows per gather; k <= 64: 16-lane; k <= 32: 8-lane) and there are no column panels;
//   * two LDS planes per row: x_i (read when the slot's stream turns to the row) and the accumulator z_i -- the max / min
//     kernel's LDS budget, so plans have its shape: half the rows per wave of a sum plan plus the spare row that padding
//     words point at (x = 0, gathered y = 0: whatever a padding step computes lands in a row nobody writes out);
//   * four steps at a time: their four partial dot products (or squared distances) are summed over the slot's lanes by ONE
//     transposed butterfly (gather.h), the scalar stage runs once on the lanes that end up owning a sum (reciprocals by v_rcp_f32),
//     four cross-lane reads
//     hand every lane its step's scalar, and only then are the four gathered rows scaled into the accumulator and their
//     gathers re-issued (28-32 in flight instead of 32).
// Every row is accumulated by the one wave that owns it, in stream order: no atomics, bitwise reproducible.  Hub rows cut
// into virtual rows leave partial rows that sweep_hub_fold_kernel adds up, as for the SpMM.
#include "sweep_common.h"

namespace isplib {

// (reciprocals by v_rcp_f32, 1 ulp: an IEEE division is ten vector instructions in a loop that is bound by them -- the ISA of the
// first form of this kernel had 39 per step against the SpMM's 13.  What that costs in accuracy is measured, not assumed:
// profiles/fusedmm_sop_accuracy.txt, and DESIGN.md 4.6a for the per-element contract the results are held to)
__device__ __forceinline__ float sop_menu(int kind, float s, float p) {
   switch (kind) {
      case ISPLIB_SOP_SIGMOID: return __builtin_amdgcn_rcpf(1.0f + __expf(-s));
      case ISPLIB_SOP_ONE_MINUS_SIGMOID: return 1.0f - __builtin_amdgcn_rcpf(1.0f + __expf(-s));
      case ISPLIB_SOP_TDIST: return __builtin_amdgcn_rcpf(1.0f + s);
      case ISPLIB_SOP_SCALE: return p * s;
      case ISPLIB_SOP_EXP: return __expf(s);
      case ISPLIB_SOP_LEAKY_EXP: return __expf(s > 0.0f ? s : p * s);
      default: return s;
   }
}

// PAT 1: T = y_j, s = f(<x_i, y_j>);   PAT 2: T = y_j - x_i, s = f(|T|^2);   z_i += s * T
template <int PAT, int LPR, int NVMAX, int NBW, int WGS>
__global__ __launch_bounds__(256, (stream_wgs_per_cu<LPR, 2 * (NVMAX + 1), WGS>())) void fusedmm_stream_kernel(const SweepArgs a, const int sop_udef,
                                                                                                             const float sop_param) {
   using Wave = StreamWave<LPR, NVMAX, NBW>;
   constexpr int WAVES = Wave::WAVES, G = Wave::G, PANEL = Wave::PANEL, U = Wave::U, PER = Wave::PER;
   constexpr int ROWS = NVMAX + 1, WAVE_FLOATS = 2 * ROWS * PANEL, Z0 = ROWS * PANEL;
   static_assert(U % 4 == 0 && ROWS <= 256 && NVMAX % G == 0, "four steps per butterfly; the local row is the top byte of a word");
   __shared__ __attribute__((aligned(16))) float s_all[WAVES * WAVE_FLOATS];
   Wave sw;
   if (!stream_wave_id(a, sw)) return;                   // no barrier anywhere below
   float *my = s_all + sw.wave * WAVE_FLOATS;
   stream_columns<false>(a, sw);                          // k % 4 == 0 (entry): a lane's four columns are all inside or all outside
   float *lane_x = my + sw.lc * 4;                        // a lane's four columns of a row of x ...
   float *lane_z = my + Z0 + sw.lc * 4;                   // ... and of its accumulator
   // the wave's rows of x into the first plane (unused local rows and the spare row: 0), zeros into the second
#pragma unroll 1
   for (int jj = 0; jj <= PER; jj++) {
      const int lrow = jj < PER ? sw.g * PER + jj : NVMAX;
      const int row = jj < PER ? a.wave_row[(size_t)sw.w * NVMAX + lrow] : -1;
      float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (row >= 0 && sw.cok) v = *reinterpret_cast<const float4 *>(a.g + (size_t)row * (size_t)a.ldg + sw.ccol);
      *reinterpret_cast<float4 *>(lane_x + lrow * PANEL) = v;
      *reinterpret_cast<float4 *>(lane_z + lrow * PANEL) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   }
   __amdgpu_buffer_rsrc_t rsrc = dense_rsrc(a);
   stream_bounds(a, sw);
   const unsigned pad_word = stream_pad_spare_row(a, sw);      // past the end of the wave: the spare row
   unsigned w1[NBW], w2[NBW];
   v4i_t t[U];
   unsigned la[U];
   stream_load_batch(sw, sw.wp, 0, pad_word, w1);
#pragma unroll
   for (int u = 0; u < U; u++) stream_issue<0>(sw, rsrc, w1, u, la[u], t[u]);
   stream_load_batch(sw, sw.wp, 64 * NBW, pad_word, w1);
   stream_load_batch(sw, sw.wp, 128 * NBW, pad_word, w2);
   unsigned curz = (unsigned)(sw.g * PER * PANEL);        // the row whose accumulator the registers hold
   float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
   const int64_t nb = (sw.nwords + 64 * NBW - 1) / (64 * NBW);
   for (int64_t b = 0; b < nb; b++) {
#pragma unroll
      for (int u0 = 0; u0 < U; u0 += 4) {
         float d[4];
         // x_i of each of the four steps straight from its LDS row (one ds_read_b128 per step, issued together: the LDS pipe is
         // otherwise idle).  Keeping the row in registers and re-reading it when the stream turns to another row -- what the
         // accumulator does below -- cost a compare, a branch and four register copies per step here; the read costs none.
         float4 xq[4];
#pragma unroll
         for (int q = 0; q < 4; q++) xq[q] = *reinterpret_cast<const float4 *>(lane_x + la[u0 + q]);
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const int u = u0 + q;
            const float4 xv = xq[q];
            float y0 = __int_as_float(t[u][0]), y1 = __int_as_float(t[u][1]), y2 = __int_as_float(t[u][2]), y3 = __int_as_float(t[u][3]);
            if (PAT == 2) {                               // T = y - x replaces y in the registers of the gather
               y0 -= xv.x; y1 -= xv.y; y2 -= xv.z; y3 -= xv.w;
               t[u][0] = __float_as_int(y0); t[u][1] = __float_as_int(y1); t[u][2] = __float_as_int(y2); t[u][3] = __float_as_int(y3);
               d[q] = fmaf(y0, y0, fmaf(y1, y1, fmaf(y2, y2, y3 * y3)));
            } else {
               d[q] = fmaf(y0, xv.x, fmaf(y1, xv.y, fmaf(y2, xv.z, y3 * xv.w)));
            }
         }
         int mine;
         const float sum = reduce_transposed<4, LPR>(d, sw.lc, mine);
         const float sown = sop_menu(sop_udef, sum, sop_param);      // meaningful on the lanes that own a step's sum
         float s[4];
#pragma unroll
         for (int q = 0; q < 4; q++) s[q] = __shfl(sown, sw.g * LPR + transposed_owner<4, LPR>(q));
#pragma unroll
         for (int q = 0; q < 4; q++) {
            const int u = u0 + q;
            if (la[u] != curz) {
               stream_flush(lane_z + curz, acc);
               curz = la[u];
               acc[0] = acc[1] = acc[2] = acc[3] = 0.0f;
            }
#pragma unroll
            for (int v = 0; v < 4; v++) acc[v] = fmaf(s[q], __int_as_float(t[u][v]), acc[v]);
         }
#pragma unroll
         for (int q = 0; q < 4; q++) stream_issue<0>(sw, rsrc, w1, u0 + q, la[u0 + q], t[u0 + q]);
      }
#pragma unroll
      for (int q = 0; q < NBW; q++) w1[q] = w2[q];
      stream_load_batch(sw, sw.wp, (b + 3) * 64 * NBW, pad_word, w2);
   }
   stream_flush(lane_z + curz, acc);
   // write-out: slot q owns the local rows [q * PER, (q + 1) * PER); its LPR lanes hold one row
   int row_[PER], part_[PER];
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      row_[jj] = sw.cok ? a.wave_row[(size_t)sw.w * NVMAX + sw.g * PER + jj] : -1;
      part_[jj] = a.wave_part[(size_t)sw.w * NVMAX + sw.g * PER + jj];
   }
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      if (row_[jj] < 0) continue;
      const float4 v = *reinterpret_cast<const float4 *>(lane_z + (sw.g * PER + jj) * PANEL);
      float *dst = part_[jj] >= 0 ? a.part_val + (size_t)part_[jj] * (size_t)a.k + sw.ccol : a.z + (size_t)row_[jj] * (size_t)a.ldz + sw.ccol;
      *reinterpret_cast<float4 *>(dst) = v;
   }
}

template <int PAT, int STREAMS>
static int launch_fusedmm_stream(const SweepArgs &a, int sop_udef, float sop_param, hipStream_t st) {
   constexpr StreamGeom ge = stream_geom(STREAM_FUSEDMM, STREAMS);
   const unsigned blocks = (unsigned)((a.wave_count + 3) / 4);
   if (blocks == 0) return ISPLIB_SUCCESS;
   hipLaunchKernelGGL((fusedmm_stream_kernel<PAT, ge.lpr, ge.nvmax, ge.nbw, ge.wgs>), dim3(blocks), dim3(256), 0, st, a, sop_udef, sop_param);
   return check_launch("fusedmm_stream_kernel");
}

template <int PAT>
static int launch_fusedmm_stream(const SweepArgs &a, int streams, int sop_udef, float sop_param, hipStream_t st) {
   return with_streams<STREAM_FUSEDMM>(streams, [&](auto s) { return launch_fusedmm_stream<PAT, s()>(a, sop_udef, sop_param, st); });
}

}  // namespace isplib

using namespace isplib;

// the two words this front end serves (enum values of csrc/fusedMM.h:18-74): everything else stays on fusedMM_csr_udef(_tasks)_hip
static int stream_pattern(int32_t imessage) {
   if (imessage == (0x2 | 0x10 | 0xF00 | 0x1000 | 0x10000)) return 1;      // COPY_RHS | DOT   | UDEF | MUL | ADD
   if (imessage == (0x5 | 0x50 | 0xF00 | 0x1000 | 0x10000)) return 2;      // SUBR     | NORMR | UDEF | MUL | ADD
   return 0;
}

extern "C" int isplib_fusedmm_stream_geometry(int streams, int *rows_per_wave, int *waves_resident) {
   return stream_geometry("isplib_fusedmm_stream_geometry", STREAM_FUSEDMM, streams, rows_per_wave, waves_resident);
}

extern "C" int isplib_suggest_fusedmm_stream(int32_t imessage, int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk) {
   // the SpMM's reuse rule on this kernel's geometry (half the rows per wave of a sum plan: twice the generations, each sweeping y
   // once per XCD): edges per generation and XCD >= 3 x rows of y.  Slices of ~2.6 MB of y on 128-column slots, ~3.8 MB on the
   // narrower ones; rows cut at ~0.4 of a stream's share.  Reddit shape, round 5, sigmoid word, ms (task list: 5.55 / 2.74 / 1.52):
   //   K=128: 7 / 15 / 31 / 46 / 62 slices 4.89 / 4.14 / 3.94 / 3.79 / 3.85; chunk 1457 / 2914 / 5828 (31 slices): 3.78 / 3.94 / 4.14
   //   K=64 : 4 / 8 / 16 / 24 / 32 slices 2.10 / 1.91 / 1.88 / 1.92 / 1.96;  chunk 1457 / 2914 / 5828: 1.87 / 1.88 / 2.17
   //   K=32 : 2 / 4 / 8 / 12 / 16 slices 1.08 / 1.04 / 1.04 / 1.07 / 1.08;   chunk 1457 / 2914 / 5828: 1.02 / 1.04 / 1.31
   clear_error();
   if (!stream_pattern(imessage) || m <= 0 || n <= 0 || nnz < STREAM_MIN_NNZ || k > 128 || (k % 4) != 0) return 0;
   if (!isplib_stream_serves(n, k, k, nnz, 0)) return 0;
   const int st = k <= 32 ? 8 : (k <= 64 ? 4 : 2);
   int rpw = 0, resident = 0;
   if (isplib_fusedmm_stream_geometry(st, &rpw, &resident) != ISPLIB_SUCCESS) return 0;
   if (!suggest_stream_geom(m, n, nnz, st, rpw, resident, st == 2 ? 2.6e6 : 3.8e6, 2.4, slices, chunk)) return 0;
   if (streams) *streams = st;
   return 1;
}

extern "C" int fusedMM_csr_udef_stream_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *pntrb,
                                           const int64_t *pntre, const isplib_stream_plan *plan, const float *x, int64_t ldx,
                                           const float *y, int64_t ldy, float *z, int64_t ldz, int sop_udef, float sop_param,
                                           void *workspace, size_t workspace_bytes, void *stream) {
   clear_error();
   const char *entry = "fusedMM_csr_udef_stream_hip";
   const int pat = stream_pattern(imessage);
   if (!pat) return fail(ISPLIB_NO_OPT_IMPL, entry, "COPY_RHS|DOT|UDEF|MUL|ADD and SUBR|NORMR|UDEF|MUL|ADD only (other words: fusedMM_csr_udef_hip)");
   if (sop_udef < ISPLIB_SOP_SIGMOID || sop_udef > ISPLIB_SOP_LEAKY_EXP)
      return fail(ISPLIB_UNDEFINED_USER_FUNCTION, entry, "SOP_UDEF needs a built-in function (enum isplib_sop_udef)");
   const StreamCall c = {entry, "fusedMM_csr_udef_tasks_hip", STREAM_FUSEDMM, m, n, k, nnz, /* empty */ m == 0 || k == 0, pntrb, pntre, plan, y, ldy,
                         /* ld_other */ ldz, /* others */ x && z, /* hub_fold */ true, workspace, workspace_bytes, (size_t)(plan ? plan->n_parts : 0) * (size_t)k * sizeof(float)};
   bool done;
   int rc = check_stream_call(c, &done);
   if (done) return rc;
   if ((k % 4) != 0 || k > 256 / plan->streams)
      return fail(ISPLIB_FAIL, entry, "k must be a multiple of 4 within the plan's slot width (256 / streams columns); use fusedMM_csr_udef_tasks_hip");
   if (ldx < k || (ldx % 4) != 0 || (ldz % 4) != 0 || ((uintptr_t)x & 15) != 0 || ((uintptr_t)z & 15) != 0)
      return fail(ISPLIB_FAIL, entry, "ldx, ldz multiples of 4 and >= k, x and z 16-byte aligned");
   if ((rc = check_stream_workspace(c)) != ISPLIB_SUCCESS) return rc;
   SweepArgs a = stream_args(c, z, ldz);
   a.g = x; a.ldg = ldx;
   hipStream_t st = (hipStream_t)stream;
   rc = run_generations(plan->gens, plan->waves_per_gen, a, [&](const SweepArgs &p) {
      return pat == 1 ? launch_fusedmm_stream<1>(p, plan->streams, sop_udef, sop_param, st) : launch_fusedmm_stream<2>(p, plan->streams, sop_udef, sop_param, st);
   });
   return rc ? rc : launch_hub_fold<OP_ADD, false>(a, st);
}
