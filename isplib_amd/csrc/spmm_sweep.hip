// spmm_sweep.hip -- the STREAM schedule of the SpMM (fusedMM_csr_stream_hip, fusedMM_csr_stream_minmax_hip: the default of
// sum / mean / max / min on graphs with work for the whole chip): see include/isplib_hip.h and DESIGN.md 4.3-4.4.
//
// The task-list schedule (spmm_tasks.hip) gets its L2 locality from the ORDER in which the hardware hands out
// workgroups (slice-major task list), and pays for it with one partial row per task, written to HBM and folded by a
// second kernel.  Here the locality comes from TIME instead: a launch holds only as many waves as are resident at
// once, every wave owns a fixed set of (virtual) rows whose running sums live in LDS, and all waves walk the column
// slices 0, 1, 2, ... of their own rows together.  Equal edge mass per wave (plan) keeps them in step, so at any
// moment an XCD's L2 serves one or two slices -- which can therefore be as small as the L2 -- and nothing but the
// finished rows ever leaves the CU: no partial rows (but for hub rows cut into virtual rows), no fold, z written once.
// (The file keeps its name from the round-2 "sweep" schedule, the first of this family; that kernel, the LDS hot-row hybrid
// and the stream-plan SDDMM -- all measured slower than what is here -- live in experimental/experimental.hip.)
#include <vector>

#include "sweep_common.h"

extern "C" void isplib_debug_wave_times(unsigned long long *buf);

namespace isplib {

// ---- stream form ------------------------------------------------------------------------------------------------
// The round-2 sweep (experimental/experimental.hip) pays one latency chain per (row, slice) segment -- and with L2-sized
// slices a segment is 15 edges.  Here a wave does not see segments at all.  The plan gives each of the G = 64 / LPR slots of a wave its
// own STREAM: the edges of the slot's NVMAX / G rows, slice by slice, as 4-byte words (local row << 24 | column) in
// the plan's own copy of the index array.  Step i of a wave gathers word i of each of its G streams -- one 1-KiB
// buffer load, always full -- and every lane adds the four floats it receives to the running sum of the row its
// slot is on (registers), which moves to and from the slot's LDS row when the stream changes rows.  The slots of a
// wave own disjoint rows and a wave's LDS operations execute in order, so every sum is formed in one fixed order.
// U gathers are in flight per wave at all times, across row and slice boundaries alike; there is no butterfly, no
// masked tail, no per-segment bookkeeping.  Sum / mean only.
// TIMED (the calibration of the levelled deal, isplib_stream_capacities_hip, and scripts/exp_wave_times.py): the same kernel, and
// every wave also reports when it started, entered and left its loop and finished (s_memtime), and where it ran.
// PACKED (64-column geometry, not TIMED): the words come out of the plan's packed stream (include/isplib_hip.h, PACKED WORD STREAM) --
// 304 bytes a batch from beyond the L2 instead of 512.  Only the batch loader differs: where the other instances load a batch of
// words into w2 and move it to w1 a batch later, this one loads the packed batch into two registers and DECODES it into w1 a
// batch later (two cross-lane reads, two ballots); the loads keep their places and the 32 steps that follow are the same instructions.
template <int LPR, bool HAS_VAL, int NVMAX, int NBW, int WGS, bool TIMED = false, bool PACKED = false>
__global__ __launch_bounds__(256, (stream_wgs_per_cu<LPR, NVMAX, WGS>())) void spmm_stream_kernel(const SweepArgs a) {
   using Wave = StreamWave<LPR, NVMAX, NBW>;
   constexpr int WAVES = Wave::WAVES, G = Wave::G, PANEL = Wave::PANEL, U = Wave::U, PER = Wave::PER;
   constexpr int WAVE_FLOATS = NVMAX * PANEL;
   static_assert(NVMAX <= 256 && NVMAX % G == 0, "the local row is the top byte of a word");
   __shared__ __attribute__((aligned(16))) float s_all[WAVES * WAVE_FLOATS];
   Wave sw;
   if (!stream_wave_id(a, sw)) return;                   // no barrier anywhere below
   const int lane = sw.lane;
   unsigned long long t_start = 0, t_loop = 0, t_loop_end = 0;
   if constexpr (TIMED) t_start = __builtin_amdgcn_s_memtime();
   float *my = s_all + sw.wave * WAVE_FLOATS;
   for (int i = lane * 4; i < WAVE_FLOATS; i += 256)
      *reinterpret_cast<float4 *>(my + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
   __amdgpu_buffer_rsrc_t rsrc = dense_rsrc(a);
   stream_columns<true>(a, sw);
   float *lane_base = my + sw.lc * 4;                     // a lane's four columns of a row are contiguous
   stream_bounds(a, sw);
   const float *vp = HAS_VAL ? a.vals + sw.s0 * G : nullptr;
   unsigned w1[NBW], w2[NBW];                             // the words of the next batch and of the one after it
   float v0[NBW] = {}, v1[NBW] = {};                      // the weights of the batch being consumed and of the next
   v4i_t t[U];
   unsigned la[U];
   // (a weight is fetched from its batch register when its gather is consumed, one step ahead: a ring of U weights
   // beside the U gathers in flight costs 30 registers)
   const unsigned pad_word = stream_pad_own_row(a, sw);
   const int64_t nb = (sw.nwords + 64 * NBW - 1) / (64 * NBW);
   // PACKED: the wave's first packed batch follows from its position alone; w2 holds a packed batch, not words
   [[maybe_unused]] const uint32_t *pk = nullptr;
   [[maybe_unused]] StreamPackLane pl;
   if constexpr (PACKED) {
      static_assert(!TIMED, "the TIMED instance reads the words");
      pk = a.packed + ((sw.s0 * G) / (64 * NBW) + sw.w) * ISPLIB_STREAM_PACK_DWORDS;
      pl = stream_pack_lane(sw);
      stream_load_packed(sw, pk, 0, nb, w2);
      stream_decode_packed<Wave>(pl, a.pack_width, pad_word, w2, w1);
   } else {
      stream_load_batch(sw, sw.wp, 0, pad_word, w1);
   }
   if (HAS_VAL) stream_load_batch(sw, vp, 0, 0.0f, v0);
#pragma unroll
   for (int u = 0; u < U; u++) stream_issue<ISPLIB_EXP_GATHER_AUX>(sw, rsrc, w1, u, la[u], t[u]);
   if constexpr (PACKED) {
      stream_load_packed(sw, pk, 1, nb, w2);
      stream_decode_packed<Wave>(pl, a.pack_width, pad_word, w2, w1);
   } else {
      stream_load_batch(sw, sw.wp, 64 * NBW, pad_word, w1);
   }
   if (HAS_VAL) stream_load_batch(sw, vp, 64 * NBW, 0.0f, v1);
   if constexpr (PACKED) stream_load_packed(sw, pk, 2, nb, w2);
   else stream_load_batch(sw, sw.wp, 128 * NBW, pad_word, w2);
   unsigned cur = (unsigned)(sw.g * PER * PANEL);         // the row whose running sum the registers hold (stream_flush)
   float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
   if constexpr (TIMED) t_loop = __builtin_amdgcn_s_memtime();
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
#pragma unroll
         for (int v = 0; v < 4; v++) {
            const float x = __int_as_float(t[u][v]);
            acc[v] = HAS_VAL ? fmaf(vcur, x, acc[v]) : acc[v] + x;
         }
         stream_issue<ISPLIB_EXP_GATHER_AUX>(sw, rsrc, w1, u, la[u], t[u]);
      }
#pragma unroll
      for (int q = 0; q < NBW; q++) v0[q] = v1[q];
      if constexpr (PACKED) {
         stream_decode_packed<Wave>(pl, a.pack_width, pad_word, w2, w1);      // batch b + 2, loaded a batch ago
         stream_load_packed(sw, pk, b + 3, nb, w2);
      } else {
#pragma unroll
         for (int q = 0; q < NBW; q++) w1[q] = w2[q];
         stream_load_batch(sw, sw.wp, (b + 3) * 64 * NBW, pad_word, w2);
      }
      if (HAS_VAL) stream_load_batch(sw, vp, (b + 2) * 64 * NBW, 0.0f, v1);
   }
   stream_flush(lane_base + cur, acc);
   if constexpr (TIMED) t_loop_end = __builtin_amdgcn_s_memtime();
   // write-out: slot q owns the local rows [q * PER, (q + 1) * PER); its LPR lanes hold one row of the panel.  The rows' ids
   // (two dependent global loads per row) are fetched for the whole slot first and the rows then go out four at a time: a
   // row-at-a-time loop pays every row's memory latencies one after the other (2 % of a dispatch, scripts/exp_wave_times.py)
   int row_[PER], part_[PER];
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      row_[jj] = sw.cok ? a.wave_row[(size_t)sw.w * NVMAX + sw.g * PER + jj] : -1;
      part_[jj] = a.wave_part[(size_t)sw.w * NVMAX + sw.g * PER + jj];
   }
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
      store_tail<4>(a.z + (size_t)row * (size_t)a.ldz + c, v, sw.vfirst);
   }
   if constexpr (TIMED) if (a.dbg && lane == 0) {
      a.dbg[(size_t)sw.wl * 5 + 0] = t_start;
      a.dbg[(size_t)sw.wl * 5 + 1] = t_loop;
      a.dbg[(size_t)sw.wl * 5 + 2] = t_loop_end;
      a.dbg[(size_t)sw.wl * 5 + 3] = __builtin_amdgcn_s_memtime();
      // where the wave ran: (XCC id << 24) | bits 8..23 of HW_ID (CU, SH, SE); s_getreg operand = id | (bits - 1) << 11
      a.dbg[(size_t)sw.wl * 5 + 4] = (__builtin_amdgcn_s_getreg(20u | (3u << 11)) << 24) | ((__builtin_amdgcn_s_getreg(4u | (31u << 11)) >> 8) & 0xFFFFu);
   }
}

// max / min on the stream schedule.  The running sum becomes the best value so far and the WORD INDEX (position in the
// wave's stream) at which it was met; a second LDS plane keeps those indices beside the values.  "Strictly better
// wins" in stream order: the plan walks the edges of a row slice by slice and, inside a slice, in CSR order, so for rows
// whose columns ascend the stream order of a row IS its CSR order and the first of equal candidates -- the lowest CSR
// position, the reference's tie rule -- is the one that stays (the plan builders refuse graphs with unsorted rows for
// this kernel).  No position travels with the gathers: the word index is arithmetic (batch, step, slot), and only the
// M x K winners are translated to CSR positions, through the plan's `perm`, when a row is written out.
//
// Round 4: the registers CARRY the row's pair.  Rounds 2-3 started every visit of a row from the identity and merged
// the visit's winners into the row's LDS pair when the stream left it (read both planes, four compare-selects, write both
// planes, reset eight registers: ~20 vector instructions per change of row on top of ~25 per step -- the ISA showed 40-45
// vector instructions per step against 13 for the sum kernel, i.e. more vector-ALU cycles per step than the 26 the
// address pipeline needs for the gather: the kernel was ALU-bound and wanted FEW changes of row, 8 slices of 7.5 MB,
// 67 % L2 hits).  Now a change of row is a SWAP: the pair in the registers is stored to the row it belongs to, the pair
// of the new row is loaded and the compare simply goes on -- two 16-byte LDS writes and two reads, no vector ALU work at
// all -- so the row's best so far meets every later candidate directly ("strictly better" against the EARLIER stream
// position keeps the tie rule), and the slices can be as small as the sum kernel's.  Padding words (column n: the gather
// returns 0, which would beat negative values) carry the local row NVMAX, a spare LDS row of the wave that is never
// written out: the plan builders emit it for max / min plans, so the loop neither tests for padding nor masks the column.
// (Also built in round 4 and dropped: 16-bit row-relative ORDINALS in place of the 32-bit word indices -- 388 bytes of LDS per
// row instead of 512, 48 rows per wave, three generations on the Reddit shape instead of four, no permutation lookup at
// write-out; bit-exact, and slower: K=64 weighted 1.89 against 1.81 ms, unit 1.63 against 1.61 -- the swap then packs and
// unpacks and moves a per-row word count as well, which costs what the saved dispatch gave.)
typedef float v2f_t __attribute__((ext_vector_type(2)));

// ARG = false (z_arg == NULL: values only, e.g. the aggregation of an inference pass, where no backward will ask which edge
// won): the index registers, their selects -- four of the 16-18 vector instructions of a step, in a loop that is bound by
// them (profiles/r04_experiments.txt) --, the index plane and the permutation lookups at write-out all drop out; same plan,
// same values bit for bit.  K=64 on the Reddit shape: 1.80 -> 1.6 ms with U(0,1) weights, 1.61 -> 1.4 with unit weights.
template <int OP, int LPR, bool HAS_VAL, int NVMAX, int NBW, int WGS, bool ARG>
__global__ __launch_bounds__(256, (stream_wgs_per_cu<LPR, 2 * (NVMAX + 1), WGS>())) void spmm_stream_minmax_kernel(const SweepArgs a) {
   using Wave = StreamWave<LPR, NVMAX, NBW>;
   constexpr int WAVES = Wave::WAVES, G = Wave::G, PANEL = Wave::PANEL, U = Wave::U, PER = Wave::PER;
   constexpr int ROWS = NVMAX + 1;                        // + the spare row of the padding words
   constexpr int WAVE_DWORDS = 2 * ROWS * PANEL;          // a wave's block: the values, then their indices
   constexpr int IDX0 = ROWS * PANEL;
   constexpr int NONE = INT_MAX;                          // "no winner yet"
   static_assert(ROWS <= 256 && NVMAX % G == 0, "the local row (and the spare row) is the top byte of a word");
   __shared__ __attribute__((aligned(16))) float s_all[WAVES * WAVE_DWORDS];
   Wave sw;
   if (!stream_wave_id(a, sw)) return;                   // no barrier anywhere below
   const int lane = sw.lane;
   float *my = s_all + sw.wave * WAVE_DWORDS;
   for (int i = lane * 4; i < ROWS * PANEL; i += 256)
      *reinterpret_cast<float4 *>(my + i) = make_float4(identity<OP>(), identity<OP>(), identity<OP>(), identity<OP>());
   if (ARG)
      for (int i = lane * 4; i < ROWS * PANEL; i += 256)
         *reinterpret_cast<int4 *>(my + IDX0 + i) = make_int4(INT_MAX, INT_MAX, INT_MAX, INT_MAX);
   __amdgpu_buffer_rsrc_t rsrc = dense_rsrc(a);
   stream_columns<true>(a, sw);
   // lanes beyond column k gather nothing: their column term is 2^31, past the end of the descriptor (the entry admits dense
   // operands under 2 GiB only, so row offset + 2^31 neither stays inside the descriptor nor wraps) -- no OR in the loop
   const unsigned cbyte = sw.cok ? sw.cbyte : 0x80000000u;
   float *lane_base = my + sw.lc * 4;                     // a lane's four values of a row ...
   int *lane_idx = reinterpret_cast<int *>(my + IDX0) + sw.lc * 4;   // ... and their indices
   stream_bounds(a, sw);
   const float *vp = HAS_VAL ? a.vals + sw.s0 * G : nullptr;
   const unsigned pad_word = stream_pad_spare_row(a, sw);     // past the end of the wave: the spare row too
   const int g4 = sw.g * 4;                               // byte address of lane g for ds_bpermute
   unsigned w1[NBW], w2[NBW];
   float v0[NBW] = {}, v1[NBW] = {};                     // the weights of the batch being consumed and of the next: a weight is
                                                         // needed one batch later than its word, so it is loaded one batch later
   v4i_t t[U];
   unsigned la[U];
   // (a weight is fetched from its batch register when its gather is consumed, one step ahead -- a ring of U weights
   // beside the U gathers in flight does not fit the register file).  The 24-bit multiply reads the column straight out
   // of the word: its top byte, the local row, is outside the bits the instruction looks at.
   // the slot's word of step u of a batch register set: lane (u * G) % 64 + g of register (u * G) / 64
   auto fetch = [&](int u, const unsigned (&word_l)[NBW]) {
      return (unsigned)__builtin_amdgcn_ds_bpermute(g4 + (int)(((u * G) % 64) * 4), (int)word_l[(u * G) / 64]);
   };
   // la[u] keeps the WORD of step u as it is: its top byte, the local row, is compared byte against byte when the gather is
   // consumed (one SDWA compare) and only becomes an LDS offset inside the rare change of row -- no shift per step
   auto issue = [&](int u, unsigned word) {
      const unsigned o = __umul24(word, sw.ldyb) + cbyte;
      la[u] = word;
      t[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)o, 0, 0);
   };
   stream_load_batch(sw, sw.wp, 0, pad_word, w1);
   if (HAS_VAL) stream_load_batch(sw, vp, 0, 0.0f, v0);
#pragma unroll
   for (int u = 0; u < U; u++) issue(u, fetch(u, w1));
   stream_load_batch(sw, sw.wp, 64 * NBW, pad_word, w1);
   if (HAS_VAL) stream_load_batch(sw, vp, 64 * NBW, 0.0f, v1);
   stream_load_batch(sw, sw.wp, 128 * NBW, pad_word, w2);
   unsigned cur = (unsigned)(sw.g * PER * PANEL);         // LDS offset of the row the registers hold ...
   unsigned curw = (unsigned)(sw.g * PER) << 24;          // ... and that row as the top byte of a word
   float acc[4];
   int bi[4];
#pragma unroll
   for (int v = 0; v < 4; v++) { acc[v] = identity<OP>(); bi[v] = NONE; }
   // change of row: the pair held goes to the row it belongs to, the new row's pair comes in.  The slots of a wave own
   // disjoint rows (the spare row is written by all and read back by nobody who cares) and a wave's LDS operations execute
   // in order, so a later visit of a row reads what the last one stored.
   // (reads first: the wave then waits for the loads only -- the stores just have to be issued)
   auto swap_to = [&](unsigned nxt_word) {
      asm volatile("" : "+v"(nxt_word));                 // keeps the LDS address arithmetic inside the branch (one vector instruction per step otherwise)
      const unsigned nxt = (nxt_word >> 24) * (unsigned)PANEL;
      curw = nxt_word;
      const float4 o = *reinterpret_cast<const float4 *>(lane_base + nxt);
      if constexpr (ARG) {
         const int4 oi = *reinterpret_cast<const int4 *>(lane_idx + nxt);
         *reinterpret_cast<float4 *>(lane_base + cur) = make_float4(acc[0], acc[1], acc[2], acc[3]);
         *reinterpret_cast<int4 *>(lane_idx + cur) = make_int4(bi[0], bi[1], bi[2], bi[3]);
         bi[0] = oi.x; bi[1] = oi.y; bi[2] = oi.z; bi[3] = oi.w;
      } else {
         *reinterpret_cast<float4 *>(lane_base + cur) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      }
      acc[0] = o.x; acc[1] = o.y; acc[2] = o.z; acc[3] = o.w;
      cur = nxt;
   };
   const int64_t nb = (sw.nwords + 64 * NBW - 1) / (64 * NBW);
   for (int64_t b = 0; b < nb; b++) {
      const int widx0 = (int)(b * (64 * NBW)) + sw.g;        // word index of this lane's slot at step 0 of the batch
      float vnext = HAS_VAL ? __int_as_float(__builtin_amdgcn_ds_bpermute(g4, __float_as_int(v0[0]))) : 0.0f;
      // the word of the gather that REPLACES step u's is fetched one step ahead: the cross-lane read then has a whole step
      // (the row check and the compares) to land instead of being waited for straight away
      unsigned wnext = fetch(0, w1);
#pragma unroll
      for (int u = 0; u < U; u++) {
         const float vcur = vnext;
         const unsigned wcur = wnext;
         if (HAS_VAL && u + 1 < U)
            vnext = __int_as_float(__builtin_amdgcn_ds_bpermute(g4 + (int)((((u + 1) * G) % 64) * 4), __float_as_int(v0[((u + 1) * G) / 64])));
         if (u + 1 < U) wnext = fetch(u + 1, w1);
         // per lane: the slots of a wave change rows at different steps.  ONE vector instruction: the top bytes of the two words
         // compared in place (SDWA), the lane mask handed to the branch as it is -- written in C++ the test becomes xor + compare,
         // and with the row offset kept per step, shift + compare (round 4, second session: 18 -> 17 instructions per step)
         unsigned long long row_changes;
         asm("v_cmp_ne_u32_sdwa %0, %1, %2 src0_sel:BYTE_3 src1_sel:BYTE_3" : "=s"(row_changes) : "v"(la[u]), "v"(curw));
         if (__builtin_amdgcn_inverse_ballot_w64(row_changes)) swap_to(la[u]);
         const int mark = widx0 + u * G;                 // what a winner of this step is remembered by: its word index
         v2f_t x01 = {__int_as_float(t[u][0]), __int_as_float(t[u][1])};
         v2f_t x23 = {__int_as_float(t[u][2]), __int_as_float(t[u][3])};
         if (HAS_VAL) {                                  // two packed multiplies instead of four
            const v2f_t vv = {vcur, vcur};
            x01 *= vv;
            x23 *= vv;
         }
         const float tt[4] = {x01.x, x01.y, x23.x, x23.y};
#pragma unroll
         for (int v = 0; v < 4; v++) {
            const bool win = OP == OP_MAX ? tt[v] > acc[v] : tt[v] < acc[v];      // NaN never wins, as in the oracle
            acc[v] = win ? tt[v] : acc[v];
            if (ARG) bi[v] = win ? mark : bi[v];
         }
         issue(u, wcur);
      }
#pragma unroll
      for (int q = 0; q < NBW; q++) { w1[q] = w2[q]; v0[q] = v1[q]; }
      stream_load_batch(sw, sw.wp, (b + 3) * 64 * NBW, pad_word, w2);
      if (HAS_VAL) stream_load_batch(sw, vp, (b + 2) * 64 * NBW, 0.0f, v1);
   }
   *reinterpret_cast<float4 *>(lane_base + cur) = make_float4(acc[0], acc[1], acc[2], acc[3]);
   if (ARG) *reinterpret_cast<int4 *>(lane_idx + cur) = make_int4(bi[0], bi[1], bi[2], bi[3]);
   // write-out, ALL rows of the slot at once: the winners' word indices become CSR positions through the plan's permutation --
   // four dependent loads per row and lane, which a row-at-a-time loop waits for PER times over (the gather registers are free
   // by now: every load of the slot's PER rows is in flight before the first one is needed)
   const int32_t *ids = a.ids + sw.s0 * G;
   int row_[PER], part_[PER], best_[PER][4];
   float val_[PER][4];
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      const int lrow = sw.g * PER + jj;
      row_[jj] = sw.cok ? a.wave_row[(size_t)sw.w * NVMAX + lrow] : -1;
      part_[jj] = a.wave_part[(size_t)sw.w * NVMAX + lrow];
      const float4 t4 = *reinterpret_cast<const float4 *>(lane_base + lrow * PANEL);
      val_[jj][0] = t4.x; val_[jj][1] = t4.y; val_[jj][2] = t4.z; val_[jj][3] = t4.w;
      if constexpr (ARG) {
         const int4 i4 = *reinterpret_cast<const int4 *>(lane_idx + lrow * PANEL);
         best_[jj][0] = i4.x; best_[jj][1] = i4.y; best_[jj][2] = i4.z; best_[jj][3] = i4.w;
      } else {
         best_[jj][0] = best_[jj][1] = best_[jj][2] = best_[jj][3] = INT_MAX;
      }
   }
   if constexpr (ARG) {
#pragma unroll
      for (int jj = 0; jj < PER; jj++)
#pragma unroll
         for (int i = 0; i < 4; i++)   // (a word index outside the wave's stream -- INT_MAX = no winner -- never reaches the subscript)
            best_[jj][i] = (row_[jj] >= 0 && (unsigned)best_[jj][i] < (unsigned)sw.nwords) ? ids[best_[jj][i]] : INT_MAX;
   }
#pragma unroll
   for (int jj = 0; jj < PER; jj++) {
      const int row = row_[jj];
      if (row < 0) continue;
      const int c = sw.ccol;
      if (part_[jj] >= 0) {
         const size_t po = (size_t)part_[jj] * (size_t)a.k + c;
         store_tail<4>(a.part_val + po, val_[jj], sw.vfirst);
         if constexpr (ARG) {
#pragma unroll
            for (int i = 0; i < 4; i++) if (i >= sw.vfirst) a.part_idx[po + i] = best_[jj][i];
         }
         continue;
      }
      int64_t arg[4];
      finish_row<OP>(a, row, c, val_[jj], best_[jj], arg);
      store_tail<4>(a.z + (size_t)row * (size_t)a.ldz + c, val_[jj], sw.vfirst);
      if (a.z_arg) {
         int64_t *ar = a.z_arg + (size_t)row * (size_t)a.ldz + c;
#pragma unroll
         for (int i = 0; i < 4; i++) if (i >= sw.vfirst) ar[i] = arg[i];
      }
   }
}


// Staged column panel (include/isplib_hip.h, isplib_stream_stage_panel): dst[r * 128 + j] = y[r * ldy + j] for the 64 columns from
// y on, i.e. rows at a 512-byte pitch with the data in bytes 0..255 -- the address pattern of the FIRST panel of a contiguous
// K = 128 operand, whose lines are all in fast classes (profiles/line_classes.txt).  16 lanes x 16 bytes per row, rows of both
// sides fully coalesced; y 16-byte aligned (the rule asks 256) and ldy a multiple of 4.
__global__ __launch_bounds__(256) void stream_stage_copy_kernel(const float *__restrict__ y, int64_t ldy, int64_t n, float *__restrict__ dst) {
   const int64_t total = n * 16;
   const int64_t stride = (int64_t)gridDim.x * blockDim.x;
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
      const int64_t r = i >> 4;
      const int j = (int)(i & 15) * 4;
      *reinterpret_cast<float4 *>(dst + r * (ISPLIB_STREAM_STAGE_PITCH / 4) + j) = *reinterpret_cast<const float4 *>(y + r * ldy + j);
   }
}

static int launch_stage_copy(const float *y, int64_t ldy, int64_t n, float *dst, hipStream_t st) {
   int64_t blocks = (n * 16 + 255) / 256;
   if (blocks > 4096) blocks = 4096;
   if (blocks <= 0) return ISPLIB_SUCCESS;
   hipLaunchKernelGGL(stream_stage_copy_kernel, dim3((unsigned)blocks), dim3(256), 0, st, y, ldy, n, dst);
   return check_launch("stream_stage_copy_kernel");
}

// set by isplib_debug_wave_times, for the calling thread's launches: [dispatch % 4][wave][5], the TIMED kernel's stamps
static thread_local unsigned long long *g_dbg = nullptr;
static thread_local int g_dbg_launch = 0;
template <int STREAMS, bool HAS_VAL>
static int launch_stream(const SweepArgs &a_in, hipStream_t st) {
   constexpr StreamGeom ge = stream_geom(STREAM_SUM, STREAMS);
   SweepArgs a = a_in;
   const unsigned blocks = (unsigned)((a.wave_count + 3) / 4);
   if (blocks == 0) return ISPLIB_SUCCESS;
   // the TIMED instance exists for unit-weight plans only: what the calibration and the experiment scripts launch
   if constexpr (!HAS_VAL) {
      if (g_dbg) {
         a.dbg = g_dbg + (size_t)(g_dbg_launch++ % 4) * (size_t)a.wave_count * 5;
         hipLaunchKernelGGL((spmm_stream_kernel<ge.lpr, false, ge.nvmax, ge.nbw, ge.wgs, true>), dim3(blocks), dim3(256), 0, st, a);
         return check_launch("spmm_stream_kernel");
      }
   }
   // the plan's packed word stream (the entry attached it): the 64-column geometry's PACKED instance
   if constexpr (STREAMS == 4 && ge.nbw == 2 && ge.nvmax == 64) {
      if (a.packed) {
         hipLaunchKernelGGL((spmm_stream_kernel<ge.lpr, HAS_VAL, ge.nvmax, ge.nbw, ge.wgs, false, true>), dim3(blocks), dim3(256), 0, st, a);
         return check_launch("spmm_stream_kernel");
      }
   }
   hipLaunchKernelGGL((spmm_stream_kernel<ge.lpr, HAS_VAL, ge.nvmax, ge.nbw, ge.wgs>), dim3(blocks), dim3(256), 0, st, a);
   return check_launch("spmm_stream_kernel");
}

template <int OP, int STREAMS, bool HAS_VAL, bool ARG>
static void launch_minmax_kernel(const SweepArgs &a, unsigned blocks, hipStream_t st) {
   constexpr StreamGeom ge = stream_geom(STREAM_MINMAX, STREAMS);
   hipLaunchKernelGGL((spmm_stream_minmax_kernel<OP, ge.lpr, HAS_VAL, ge.nvmax, ge.nbw, ge.wgs, ARG>), dim3(blocks), dim3(256), 0, st, a);
}

template <int OP, bool HAS_VAL>
static int launch_stream_minmax(const SweepArgs &a, hipStream_t st, int streams) {
   const unsigned blocks = (unsigned)((a.wave_count + 3) / 4);
   if (blocks == 0) return ISPLIB_SUCCESS;
   return with_streams<STREAM_MINMAX>(streams, [&](auto s) {
      if (a.z_arg) launch_minmax_kernel<OP, s(), HAS_VAL, true>(a, blocks, st);
      else launch_minmax_kernel<OP, s(), HAS_VAL, false>(a, blocks, st);      // values only
      return check_launch("spmm_stream_minmax_kernel");
   });
}

}  // namespace isplib

using namespace isplib;


// ---- stream form: entry ---------------------------------------------------------------------------------------------
extern "C" int isplib_spmm_stream_geometry(int streams, int *rows_per_wave, int *waves_resident) {
   return stream_geometry("isplib_spmm_stream_geometry", STREAM_SUM, streams, rows_per_wave, waves_resident);
}

extern "C" int isplib_spmm_stream_minmax_geometry(int streams, int *rows_per_wave, int *waves_resident) {
   return stream_geometry("isplib_spmm_stream_minmax_geometry", STREAM_MINMAX, streams, rows_per_wave, waves_resident);
}

extern "C" int isplib_suggest_stream_weighted(int64_t m, int64_t n, int64_t nnz, int64_t k, int weighted, int *streams, int *slices, int *chunk) {
   // When does the stream schedule pay, and with which plan?  Measured on MI355X:
   //   * slots of 8 lanes (32-column panels) up to k = 32, of 16 lanes (64-column panels) up to 64 and from 128 on, of
   //     32 lanes (one 128-column pass) in between -- 64 + 36 columns in two passes cost K=100 3.23 ms, one pass 2.63
   //     (task list 3.17); K=72: 2.92 / 2.30 (2.42); K=96: 2.51 / 2.30 (2.56); K=160 wants 64 + 64 + 32: 3.85 / 4.97 (4.15);
   //   * WEIGHTED graphs at whole multiples of 128 columns: 128-column slots as well -- a pass reads the plan's weight stream
   //     (4 bytes per edge, as large as the word stream) once per panel, and half as many panels halve that: round 4, same
   //     box, alternating: K=128 2.90 -> 2.82 ms (63 slices; 72: 2.87), K=256 5.89 -> 5.74; with unit weights the two
   //     geometries tie (2.69-2.72 against 2.69-2.70), so those stay on 64-column slots;
   //   * a column slice of ~1.9 MB of the panel (Reddit shape: 32 slices at 64 columns, 16 at 32);
   //   * every generation of waves sweeps the whole dense operand once per XCD, so the rows a generation holds must
   //     reuse each row of it often: edges per generation and XCD >= 3 x rows of y (Reddit shape: 31; one rank's shard
   //     of it at 8 / 16 / 32 ranks: 7.7 / 3.9 / 1.9 -- stream 0.37 / 0.22-0.24 / 0.16-0.18 ms against 0.43 / 0.24 /
   //     0.16-0.19 ms on the task list, scripts/exp_shard_schedule.py; the ogbn-products shape, mean degree 50 over 2.4 M
   //     rows: 0.3 -- such graphs stay on the plain kernel);
   //   * rows longer than ~0.3 of a stream's share of the edges are dealt to several virtual rows (chunk).
   clear_error();
   if (m <= 0 || n <= 0 || nnz < STREAM_MIN_NNZ) return 0;
   if (!isplib_stream_serves(n, k, k, nnz, 0)) return 0;         // what the entry and the plan builder would refuse: not offered
   int st = k <= 32 ? 8 : (k <= 64 ? 4 : (k < 128 ? 2 : 4));
   if (weighted && k >= 128 && (k % 128) == 0) st = 2;
   int rpw = 0, resident = 0;
   if (isplib_spmm_stream_geometry(st, &rpw, &resident) != ISPLIB_SUCCESS || rpw <= 0 || resident <= 0) return 0;
   if (!suggest_stream_geom(m, n, nnz, st, rpw, resident, 1.9e6, 3.4, slices, chunk)) {
      if (st != 2 || k < 128) return 0;
      st = 4;                                          // (fewer rows per wave on the wide slots: the reuse rule may still accept the narrow ones)
      if (isplib_spmm_stream_geometry(st, &rpw, &resident) != ISPLIB_SUCCESS || rpw <= 0 || resident <= 0) return 0;
      if (!suggest_stream_geom(m, n, nnz, st, rpw, resident, 1.9e6, 3.4, slices, chunk)) return 0;
   }
   if (streams) *streams = st;
   return 1;
}

extern "C" int isplib_suggest_stream(int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk) {
   return isplib_suggest_stream_weighted(m, n, nnz, k, 0, streams, slices, chunk);      // unit weights
}

extern "C" int isplib_suggest_stream_minmax(int64_t m, int64_t n, int64_t nnz, int64_t k, int *streams, int *slices, int *chunk) {
   // max / min: 32-column slots up to k = 32, 64-column slots above; the same reuse rule; rows must be column-sorted.
   // Round 4 (the row's pair rides in registers, a change of row is an LDS swap without vector-ALU work), Reddit shape,
   // K = 64, U(0,1) weights / unit weights, ms: 8 slices 1.97 / 1.73, 12: 1.85 / 1.68, 16: 1.81 / 1.63, 20: 1.82 / 1.61,
   // 24: 1.84 / 1.63, 31: 1.92 / 1.73, 48: 2.01 / 1.82 -- slices of ~3.3 MB of the panel (rounds 2-3, when every change of
   // row cost a read-compare-write of both planes: 7.5 MB, 2.04 / 1.82); K = 32 on 32-column slots: 8-16 slices 0.87-0.89,
   // 24: 0.94.  Rows cut at ~0.85 of a stream's share on 64-column slots (chunk 3000: 1.81, 2057: 1.84, 1028: 1.91), ~0.6
   // on 32-column ones (2057: 0.873, 3000: 0.890).  Task list: 2.35 / 1.96 (K=128 weighted 3.71 against 4.54).
   clear_error();
   if (m <= 0 || n <= 0 || nnz < STREAM_MIN_NNZ) return 0;
   if (!isplib_stream_serves(n, k, k, nnz, 1)) return 0;         // the max / min entry: under 2 GiB
   const int st = k <= 32 ? 8 : 4;
   int rpw = 0, resident = 0;
   if (isplib_spmm_stream_minmax_geometry(st, &rpw, &resident) != ISPLIB_SUCCESS || rpw <= 0 || resident <= 0) return 0;
   if (!suggest_stream_geom(m, n, nnz, st, rpw, resident, 3.3e6, st == 8 ? 1.7 : 1.17, slices, chunk)) return 0;
   if (streams) *streams = st;
   return 1;
}

// the partial rows, then (4-stream plans: the 64-column slots of sum / mean) room for one staged column panel of any call on
// this plan -- plan->cols rows at a 512-byte pitch, + 512 to start on a 512-byte boundary (isplib_stream_stage_panel).  The
// function is not told k, and a call whose workspace ends before the staging area runs unstaged.
extern "C" size_t isplib_spmm_stream_workspace_bytes(const isplib_stream_plan *plan) {
   size_t bytes = stream_parts_bytes(plan);
   if (plan && plan->streams == 4 && plan->cols > 0 && (uint64_t)plan->cols <= (ISPLIB_STREAM_STAGE_BYTES_MAX - ISPLIB_STREAM_STAGE_PITCH) / ISPLIB_STREAM_STAGE_PITCH)
      bytes += (size_t)plan->cols * ISPLIB_STREAM_STAGE_PITCH + ISPLIB_STREAM_STAGE_PITCH;
   return bytes;
}

extern "C" size_t isplib_spmm_stream_minmax_workspace_bytes(const isplib_stream_plan *plan) {
   return 2 * stream_parts_bytes(plan);   // values, then CSR positions (max / min never stage)
}

static int stream_run(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *pntrb, const int64_t *pntre,
                      const isplib_stream_plan *plan, const float *y, int64_t ldy, float *z, int64_t ldz, int64_t *z_arg,
                      void *workspace, size_t workspace_bytes, const isplib_epilogue *ep, void *stream) {
   clear_error();
   const char *entry = "fusedMM_csr_stream_hip";
   const bool mm = imessage == ISPLIB_MSG_SPMM_MAX || imessage == ISPLIB_MSG_SPMM_MIN;
   if (imessage != ISPLIB_MSG_SPMM_SUM && imessage != ISPLIB_MSG_SPMM_MEAN && !mm) return fail(ISPLIB_NO_OPT_IMPL, entry, "message outside the SpMM set");
   const StreamCall c = {entry, "fusedMM_csr_hip", mm ? STREAM_MINMAX : STREAM_SUM, m, n, k, nnz, /* empty */ m == 0 || k == 0, pntrb, pntre, plan, y, ldy,
                         /* ld_other */ ldz, /* others */ z != nullptr, /* hub_fold */ true, workspace, workspace_bytes, (mm ? 2 : 1) * stream_parts_bytes(plan)};
   bool done;
   int rc = check_stream_call(c, &done);
   if (done) return rc;
   if (mm && plan->n_steps > 0 && !plan->perm) return fail(ISPLIB_FAIL, entry, "max / min need the plan's perm array (the winners' CSR positions)");
   if (mm && nnz >= ISPLIB_STREAM_NNZ_END) return fail(ISPLIB_FAIL, entry, "max / min need nnz < 2^31");
   if (mm && !isplib_rows_within(n, ldy, ISPLIB_STREAM_MINMAX_BYTES_END - 1u))
      return fail(ISPLIB_FAIL, "fusedMM_csr_stream_minmax_hip", "dense operand of 2 GiB or more (use fusedMM_csr_tasks_hip)");
   if ((rc = check_stream_workspace(c)) != ISPLIB_SUCCESS) return rc;
   SweepArgs a = stream_args(c, z, ldz);
   a.z_arg = z_arg;
   a.mean = imessage == ISPLIB_MSG_SPMM_MEAN ? 1 : 0;
   a.part_idx = mm && workspace ? (int *)((char *)workspace + stream_parts_bytes(plan)) : nullptr;
   if ((rc = set_epilogue(entry, ep, a)) != ISPLIB_SUCCESS) return rc;
   hipStream_t st = (hipStream_t)stream;
   const bool has_val = plan->vals != nullptr;
   // sum / mean on a plan that carries a packed word stream (4-stream plans of the kernel's own geometry: the builders pack no
   // other), where ISPLIB_STREAM_PACK allows it: 0 never, 1 always, auto from the size on where the stream schedule is offered
   const int pack_mode = mm ? ISPLIB_PACK_OFF : stream_pack_mode();
   const bool packed = pack_mode != ISPLIB_PACK_OFF && plan->has_packed && plan->packed && plan->streams == 4 && plan->slices >= 1 &&
                       (pack_mode == ISPLIB_PACK_FORCE || nnz >= ISPLIB_STREAM_PACK_MIN_WORDS);
   if (packed) {
      a.packed = plan->packed;
      a.pack_width = (unsigned)((plan->cols + plan->slices - 1) / plan->slices);
   }
   if (!mm) stream_pack_report(packed ? 1 : 0);
   // sum / mean: the staging area follows the partial rows, from the first 512-byte boundary on; a workspace without one (sized
   // by the partial rows alone, or NULL for a plan without hub rows) leaves every panel where it is
   const int stage_mode = mm ? ISPLIB_STAGE_OFF : stream_stage_mode();
   float *stage_base = nullptr;
   uint64_t stage_room = 0;
   if (stage_mode != ISPLIB_STAGE_OFF && workspace) {
      const uintptr_t lo = ((uintptr_t)workspace + stream_parts_bytes(plan) + (ISPLIB_STREAM_STAGE_PITCH - 1)) & ~(uintptr_t)(ISPLIB_STREAM_STAGE_PITCH - 1);
      const uintptr_t hi = (uintptr_t)workspace + workspace_bytes;
      if (lo < hi) { stage_base = (float *)lo; stage_room = hi - lo; }
   }
   unsigned staged = 0;
   auto stage = [&](SweepArgs &p, int64_t c0) {
      if (!isplib_stream_stage_panel((uint64_t)(uintptr_t)y, ldy, c0, k, plan->streams, n, nnz, stage_room, stage_mode)) return (int)ISPLIB_SUCCESS;
      const int rc = launch_stage_copy(p.y, ldy, n, stage_base, st);
      if (rc) return rc;
      p.y = stage_base;
      p.ldy = ISPLIB_STREAM_STAGE_PITCH / 4;
      p.ybytes = (unsigned)((uint64_t)n * ISPLIB_STREAM_STAGE_PITCH);      // <= 1 GiB (the rule); row n, the padding words' column, is outside
      staged |= 1u << ((c0 / 64) & 31);
      return (int)ISPLIB_SUCCESS;
   };
   const int rc_run = run_stream_panels(plan, a,
      [&](const SweepArgs &p) {
         if (imessage == ISPLIB_MSG_SPMM_MAX) return has_val ? launch_stream_minmax<OP_MAX, true>(p, st, plan->streams) : launch_stream_minmax<OP_MAX, false>(p, st, plan->streams);
         if (imessage == ISPLIB_MSG_SPMM_MIN) return has_val ? launch_stream_minmax<OP_MIN, true>(p, st, plan->streams) : launch_stream_minmax<OP_MIN, false>(p, st, plan->streams);
         return with_streams<STREAM_SUM>(plan->streams, [&](auto s) { return has_val ? launch_stream<s(), true>(p, st) : launch_stream<s(), false>(p, st); });
      },
      [&](const SweepArgs &p) {
         return imessage == ISPLIB_MSG_SPMM_MAX ? launch_hub_fold<OP_MAX, true>(p, st)
              : imessage == ISPLIB_MSG_SPMM_MIN ? launch_hub_fold<OP_MIN, true>(p, st) : launch_hub_fold<OP_ADD, true>(p, st);
      }, stage);
   if (!mm) stream_stage_report(staged);
   return rc_run;
}

extern "C" int fusedMM_csr_stream_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                      const int64_t *pntrb, const int64_t *pntre, const isplib_stream_plan *plan,
                                      const float *y, int64_t ldy, float *z, int64_t ldz, void *workspace,
                                      size_t workspace_bytes, const isplib_epilogue *ep, void *stream) {
   if (imessage != ISPLIB_MSG_SPMM_SUM && imessage != ISPLIB_MSG_SPMM_MEAN) {
      clear_error();
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_stream_hip: sum and mean only (max / min: fusedMM_csr_stream_minmax_hip)");
   }
   return stream_run(imessage, m, n, k, nnz, pntrb, pntre, plan, y, ldy, z, ldz, nullptr, workspace, workspace_bytes, ep, stream);
}

extern "C" int fusedMM_csr_stream_minmax_hip(int32_t imessage, int64_t m, int64_t n, int64_t k, int64_t nnz,
                                             const int64_t *pntrb, const int64_t *pntre, const isplib_stream_plan *plan,
                                             const float *y, int64_t ldy, float *z, int64_t ldz, int64_t *z_arg,
                                             void *workspace, size_t workspace_bytes, void *stream) {
   if (imessage != ISPLIB_MSG_SPMM_MAX && imessage != ISPLIB_MSG_SPMM_MIN) {
      clear_error();
      return fail(ISPLIB_NO_OPT_IMPL, "fusedMM_csr_stream_minmax_hip: max and min only");
   }
   return stream_run(imessage, m, n, k, nnz, pntrb, pntre, plan, y, ldy, z, ldz, z_arg, workspace, workspace_bytes, nullptr, stream);
}

// ---- the calibration of the levelled deal (isplib_stream_capacities_hip, stream_plan.hip) ---------------------------------------
// One generation of the stream kernel, TIMED, on a synthetic graph: waves_per_gen * rows_per_wave rows of `degree` stored entries
// each in pseudo-random columns of a matrix with col_mult times as many columns, one column panel, the plan built with equal
// capacities -- every wave the same work, in L2-sized slices like a real launch's.  What differs between the waves' loop times is
// then where and when they ran.  ~11 ms and 2.7 GB of device memory at its peak at 512 entries per row; once per (device, geometry) and process, never inside a call.
namespace isplib {
__global__ __launch_bounds__(256) void stream_calib_graph_kernel(int64_t n, int64_t ncols, int64_t degree, int64_t *__restrict__ rowptr, int64_t *__restrict__ col) {
   const int64_t stride = (int64_t)gridDim.x * blockDim.x, nnz = n * degree;
   for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += stride) rowptr[i] = i * degree;
   for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += stride) {
      uint64_t h = (uint64_t)e * 0x9E3779B97F4A7C15ull;
      h ^= h >> 29; h *= 0xBF58476D1CE4E5B9ull; h ^= h >> 32;
      col[e] = (int64_t)(h % (uint64_t)ncols);
   }
}

int stream_kernel_calibrate(int streams, int waves_per_gen, int launches, int degree, int col_mult, double *wave_ticks, hipStream_t st) {
   int rpw = 0, resident = 0;
   if (isplib_spmm_stream_geometry(streams, &rpw, &resident) != ISPLIB_SUCCESS) return ISPLIB_FAIL;
   if (waves_per_gen < 4 || waves_per_gen % 4 != 0 || waves_per_gen > resident || launches < 1 || launches > 16 || degree < 1 || degree > 1024 ||
       col_mult < 1 || col_mult > 8)
      return fail(ISPLIB_FAIL, "stream calibration: whole workgroups of one resident generation, 1..16 launches");
   const int64_t n = (int64_t)waves_per_gen * rpw, ncols = n * col_mult, nnz = n * degree, k = 256 / streams;
   struct Temps {
      std::vector<void *> p;
      isplib_stream_plan plan;
      unsigned long long *callers_dbg = g_dbg;                // a buffer the caller holds (an experiment script) is put back
      Temps() { memset(&plan, 0, sizeof(plan)); }
      ~Temps() { isplib_debug_wave_times(callers_dbg); isplib_stream_plan_free(&plan); for (void *q : p) (void)hipFree(q); }
      void *get(size_t bytes) { void *q = nullptr; if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; } p.push_back(q); return q; }
   } T;
   int64_t *rowptr = (int64_t *)T.get((size_t)(n + 1) * 8), *col = (int64_t *)T.get((size_t)nnz * 8);
   float *y = (float *)T.get((size_t)ncols * k * 4), *z = (float *)T.get((size_t)n * k * 4);
   unsigned long long *dbg = (unsigned long long *)T.get((size_t)4 * waves_per_gen * 5 * 8);
   if (!rowptr || !col || !y || !z || !dbg) return fail(ISPLIB_NOT_ENOUGH_MEM, "stream calibration: device allocation failed");
   hipLaunchKernelGGL(stream_calib_graph_kernel, dim3(4096), dim3(256), 0, st, n, ncols, (int64_t)degree, rowptr, col);
   int rc = check_launch("stream_calib_graph_kernel");
   if (rc) return rc;
   ISPLIB_HIP_TRY(hipMemsetAsync(y, 0, (size_t)ncols * k * 4, st));
   int slices = (int)((ncols * k * 4 + 1900000 - 1) / 1900000);
   if (slices < 1) slices = 1;
   if ((rc = isplib_stream_plan_build_caps_hip(n, ncols, nnz, rowptr, col, nullptr, streams, slices, 4 * degree, waves_per_gen, nullptr, &T.plan, st)) != ISPLIB_SUCCESS) return rc;
   if (T.plan.gens != 1 || T.plan.n_hub != 0) return fail(ISPLIB_FAIL, "stream calibration: internal: the synthetic plan is not one generation");
   std::vector<unsigned long long> h((size_t)waves_per_gen * 5);
   for (int w = 0; w < waves_per_gen; w++) wave_ticks[w] = 0.0;
   for (int l = 0; l <= launches; l++) {
      isplib_debug_wave_times(l ? dbg : nullptr);            // (the first launch is not counted)
      rc = fusedMM_csr_stream_hip(ISPLIB_MSG_SPMM_SUM, n, ncols, k, nnz, rowptr, rowptr + 1, &T.plan, y, k, z, k, nullptr, 0, nullptr, st);
      isplib_debug_wave_times(nullptr);                      // (and nothing else of this thread's is timed into dbg)
      if (rc) return rc;
      if (!l) continue;
      ISPLIB_HIP_TRY(hipMemcpyAsync(h.data(), dbg, h.size() * 8, hipMemcpyDeviceToHost, st));
      ISPLIB_HIP_TRY(hipStreamSynchronize(st));
      for (int w = 0; w < waves_per_gen; w++) wave_ticks[w] += (double)(h[(size_t)w * 5 + 2] - h[(size_t)w * 5 + 1]) / launches;
   }
   return ISPLIB_SUCCESS;
}
}  // namespace isplib

// experiments (scripts/exp_wave_times.py, scripts/exp_stream_level.py; not declared in include/isplib_hip.h): while buf is set, the
// unit-weight sum / mean dispatches of THIS THREAD run the TIMED kernel and write their stamps to it.  The contract of buf: device
// memory of 4 x W x 5 unsigned 64-bit words, W = the largest wave count of a dispatch launched meanwhile (the plan's
// waves_per_gen); dispatch number d since the call writes slab d % 4, wave w of it the five words at (d % 4) * wave_count * 5 +
// w * 5: s_memtime at start / loop entry / loop exit / end, then (XCC id << 24) | HW_ID bits 8..23.  Nothing checks the size: the
// caller sizes it by the plan it launches.  NULL ends it.  A calibration that runs meanwhile puts the buffer back when it is done.
extern "C" void isplib_debug_wave_times(unsigned long long *buf) { isplib::g_dbg = buf; isplib::g_dbg_launch = 0; }
