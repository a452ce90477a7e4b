// mha16.hip -- the sparse multi-head dot-product attention of mha.hip (separate keys and values) for dense operands of 16-bit elements
// (bf16, fp16), all heads in one launch, forward and backward (include/isplib_hip_mha16.h: isplib_qkv16_csr_hip,
// isplib_qkv16_bw_rows_hip, isplib_qkv16_bw_cols_hip).  The mathematics is mha.hip's, stated in its header: for every row i, stored
// entry e = (i, j) and head h, with q [m, k], key [n, k], v [n, k], k = H*d, a scalar scale p and g = dL/dz:
//    s_e  = p <q_i, key_j>_h     a_e = exp(s_e - lse[i,h]),  lse[i,h] = log sum_e exp(s_e)     z_i[head h] = sum_e a_e v_j[head h]
//    D[i,h] = sum_e a_e t_e      t_e = <g_i, v_j>_h          ds_e = a_e (t_e - D[i,h])
//    dq_i[head h]   = p sum_e ds_e key_j[head h]
//    dkey_j[head h] = p sum_{e -> j} ds_e q_i[head h]
//    dv_j[head h]   = sum_{e -> j} a_e g_i[head h].
// No wide operand is widened in memory: a gathered row of key, v, q or g is half the bytes of the fp32 kernels', and the operator is
// bound by gathered bytes -- two wide rows per edge in every kernel.
//
// The 16-bit family's contract: q, key, v, g, z, dq, dkey and dv are 16-bit and widening is exact (half16.h: widen2);
// every product, sum, exponential and division is fp32; each wide output is rounded ONCE, to nearest even (narrow2).  lse and D stay
// fp32.  p multiplies the finished dot product, in all three kernels alike, and the finished rows of dq and dkey.
//
// Mapping: gatv2_16.hip's -- one wave per row (per column of A in the columns kernel), ONE 16-byte buffer load of EIGHT columns per
// lane, edge and gathered table, one chunk per lane, LPR = 4 / 8 / 16 / 32 / 64 for ceil(k / 8) up to 4 / 8 / 16 / 32 / 64 and
// G = 64 / LPR edge slots.  With H > 1, d is a power of two >= 8: a lane's eight columns never straddle heads and a head is an aligned
// group of d / 8 lanes.  With H == 1 the head is the whole slot and k may be any even width >= 8; the ragged last vector (k % 8 != 0)
// over-reads, and each over-read dword is dropped by a per-dword select before it is widened, never by a multiply.  The dot products
// of a step (U scores in the forward, U scores and U <g_i, v_j>_h in the backward kernels) go through the levels of ONE butterfly
// together.  Every gathered table sits behind a buffer descriptor of exactly the extent it owns (2 bytes per element for the wide
// tables, 4 for lse / D); dead edges and lanes past k carry BUF_OOB, which the descriptor answers with 0.  No atomics, no LDS, a fixed
// order of operations: two launches give equal bits.
//
// The forward is the online softmax per lane: (m, l, acc[8]), one rescale per step of U edges, -FLT_MAX for "no edge yet", the slots
// merged pairwise.  A row of one entry has weight exp(0) = 1 and l = 1: z_i is v_j's 16 bits.  fmaxf drops a NaN score from the
// maximum, so it enters l through exp(NaN - m): a NaN in key[j,c] makes the head of c NaN in the rows that reference j, a NaN in
// v[j,c] column c of those rows, and nothing else.
//
// The backward over the rows does NOT read z: in 16 bits z is rounded, and D = <g_i, z16_i>_h would carry u * sum_c |g_ic z_ic| into
// every ds_e.  One pass over the row's edges accumulates, per head and slot, l = sum a_e and
// Dacc = sum a_e t_e and, per column, P_c = sum a_e t_e key_jc and Q_c = sum a_e key_jc; the slots merge by plain sums; D = Dacc / l
// and dq_ic = p (P_c - D Q_c).  The columns kernel walks the transposed structure with key_j and v_j (widened) in registers, gathers
// q_i and g_i (16 bytes each) and lse, D of [i, head] (4 bytes each, two tables, each behind its own descriptor), and writes dkey and
// dv, each rounded once, each at its own pitch.  The column map, the descriptor, the gathers, the widening and the butterfly are those
// of attn16_common.h, shared with gat16.hip and gatv2_16.hip.  DESIGN.md 4.6l, 4.6n.
//
// Attention dropout (include/isplib_hip_mha16_drop.h: isplib_qkv_half_drop_*_hip): the three kernels are templates on
// DROP, with the mathematics of mha.hip's DROP kernels under this family's contract.  Every stored entry e and head h has the keep bit
// q_e,h = word(seed, CSR position of e, h) >= T of gat_dropout.h, a pure function recomputed in all three kernels, and with
// c = float32(1 / (1 - p)):
//    z_i = c sum_e q_e a_e v_j      t_e = q_e c <g_i, v_j>_h      dv_j = sum_{e -> j} q_e c a_e g_i
//    a_e, lse, s_e and the form of ds_e unchanged
// m, l and lse do not see the mask; the value accumulation takes q_e ? w : 0 and the finished row is (acc / l) * c, then the one
// rounding.  The rows kernel stays one pass and does not read z: t_e takes the mask after the butterfly, Dacc = sum a_e t_e and
// P_c = sum a_e t_e key_jc carry it, l and Q_c = sum a_e key_jc do not, so a dropped edge still gives -a_e D.  A lane's eight columns
// lie in ONE head: the head's part of the word is a single per-lane constant.  The lane that loads an entry's index hashes the entry's
// position (base + lane in the forward and the rows kernel; csr2csc[pos] in the columns kernel) and hands the word across with the
// index, by the same __shfl and slot; per edge one add, one fmix32, one compare and one select remain.  T = 0 and c = 1 give the bits
// of DROP = false, and DROP = false is the code it was (profiles/mha16_dropout_isa.txt).
#include <cfloat>
#include <cmath>

#include "common.h"
#include "gather.h"
#include "half16.h"
#include "gat_dropout.h"
#include "attn_common.h"          // AttnDrop, attn_drop_refusal, attn_set_drop
#include "attn16_common.h"

// edges per slot and step, per kernel: measured among {2, 4}; an experiment build may override them (make EXTRA=-D...)
#ifndef ISPLIB_MHA16_FW_U
#define ISPLIB_MHA16_FW_U 2
#endif
#ifndef ISPLIB_MHA16_ROWS_U
#define ISPLIB_MHA16_ROWS_U 2
#endif
#ifndef ISPLIB_MHA16_COLS_U
#define ISPLIB_MHA16_COLS_U 2
#endif

namespace isplib {

constexpr float MHA16_NONE = -FLT_MAX;       // the running maximum of a lane that saw no edge
constexpr int MHA16_WAVES = 4;               // rows per block
constexpr int MHA16_FW_U = ISPLIB_MHA16_FW_U;
constexpr int MHA16_ROWS_U = ISPLIB_MHA16_ROWS_U;
constexpr int MHA16_COLS_U = ISPLIB_MHA16_COLS_U;

struct Mha16Args {
   int64_t rows, k;                          // rows: one wave each (rows of A; columns of A in the columns kernel)
   int heads;
   int hshift;                               // head of column c: c >> hshift (H == 1: 31, every column is head 0)
   int hlanes;                               // lanes that share a head: d / 8 (H == 1: 64, the whole slot)
   unsigned hmask;                           // c & hmask == 0: the first column of a head (H == 1: only column 0)
   const int64_t *indx, *pntrb, *pntre;
   float p;                                  // the scale of the scores
   // the row-resident operands (plain loads of the wave's own row) and the outputs
   const unsigned short *own;                // forward, rows: q | columns: key
   int64_t ldown;
   const unsigned short *own2;               // columns: v
   int64_t ldown2;
   const unsigned short *g;                  // rows: dL/dz
   int64_t ldg;
   const float *lse_in;                      // rows: lse [rows, H]
   unsigned short *out;                      // z | dq | dkey
   int64_t ldout;
   unsigned short *out2;                     // columns: dv
   int64_t ldout2;
   float *hout;                              // [rows, H]: forward lse | rows: D
   // the gathered operands, each behind one descriptor
   const void *ga;                           // forward, rows: key | columns: q
   int64_t ldga;
   unsigned gabytes;
   const void *gb;                           // forward, rows: v | columns: g
   int64_t ldgb;
   unsigned gbbytes;
   const float *t1, *t2;                     // columns: lse, D; both [gathered rows, H]
   unsigned tbytes;
};

// DROP only: the dropout fields, appended to the end of Mha16Args.  They are appended by derivation, not written into Mha16Args itself:
// the kernels without dropout take Mha16Args as it was, because a kernel argument beyond 240 bytes (232 + these 24) changes the
// compiler's register allocation and block layout in 16 of the 30 kernels that were there (profiles/mha16_dropout_isa.txt), whatever
// the kernels do with the new bytes.  The host fills one Mha16DropArgs per call; a launch without dropout passes its Mha16Args part.
struct Mha16DropArgs : Mha16Args {
   unsigned seed_lo, seed_hi;                // the two halves of the seed
   unsigned T;                               // keep: word >= T
   float c;                                  // float32(1 / (1 - p))
   const int64_t *epos;                      // columns: csr2csc [nnz], the CSR position of every entry of the transposed structure
};
template <bool DROP> struct Mha16KernelArgs { using type = Mha16Args; };
template <> struct Mha16KernelArgs<true> { using type = Mha16DropArgs; };

template <int ELT, int LPR, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha16_fw_kernel(const typename Mha16KernelArgs<DROP>::type a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsk = attn16_desc(a.ga, a.gabytes), rsv = attn16_desc(a.gb, a.gbbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float qv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, qv);
   [[maybe_unused]] unsigned hk = 0u;                   // DROP: the head's part of the word, one constant per lane
   if constexpr (DROP) hk = gat_drop_head(a.seed_hi, (unsigned)cm.head);

   float mrun = MHA16_NONE, l = 0.0f, acc[8];
#pragma unroll
   for (int v = 0; v < 8; v++) acc[v] = 0.0f;

   const unsigned ldkb = (unsigned)a.ldga * 2u, ldvb = (unsigned)a.ldgb * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t kv[U], vv[U];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            kv[u] = attn16_load_wide(rsk, attn16_off(id, ldkb), cm);
            vv[u] = attn16_load_wide(rsv, attn16_off(id, ldvb), cm);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float sc[U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float k8[8];
            attn16_widen<ELT>(kv[u], cm.ok, k8);
            sc[u] = attn16_dot_part(qv, k8);
         }
         attn16_head_sum<LPR, U>(sc, a.hlanes);
         float mnew = mrun;
#pragma unroll
         for (int u = 0; u < U; u++) {
            sc[u] *= a.p;
            mnew = (s0 + u * G + g < cnt) ? fmaxf(mnew, sc[u]) : mnew;      // a NaN score is not a maximum; it enters through exp below
         }
         const float r = __expf(mrun - mnew);
         mrun = mnew;
         l *= r;
#pragma unroll
         for (int v = 0; v < 8; v++) acc[v] *= r;
#pragma unroll
         for (int u = 0; u < U; u++) {
            const float w = (s0 + u * G + g < cnt) ? __expf(sc[u] - mnew) : 0.0f;
            float v8[8];
            attn16_widen<ELT>(vv[u], cm.ok, v8);
            l += w;                                       // the softmax runs over every stored entry: the mask reaches the values only
            float wk = w;
            if constexpr (DROP) wk = gat_drop_mix(hw[u], hk) >= a.T ? w : 0.0f;
#pragma unroll
            for (int v = 0; v < 8; v++) acc[v] = fmaf(wk, v8[v], acc[v]);
         }
      }
   }
   // merge the G slots pairwise, by the rule of a step
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      const float mo = __shfl_xor(mrun, o), lo = __shfl_xor(l, o);
      const float mnew = fmaxf(mrun, mo);
      const float ra = __expf(mrun - mnew), rb = __expf(mo - mnew);
      l = l * ra + lo * rb;
#pragma unroll
      for (int v = 0; v < 8; v++) acc[v] = acc[v] * ra + __shfl_xor(acc[v], o) * rb;
      mrun = mnew;
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
   float zr[8];
#pragma unroll
   for (int v = 0; v < 8; v++) {
      zr[v] = empty ? 0.0f : acc[v] / l;
      if constexpr (DROP) zr[v] *= a.c;
   }
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, zr);
   if (cm.first) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = empty ? -INFINITY : mrun + logf(l);
}

// the one-pass backward over the rows: no z, D[i,h] from the row's own edges
template <int ELT, int LPR, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha16_bw_rows_kernel(const typename Mha16KernelArgs<DROP>::type a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsk = attn16_desc(a.ga, a.gabytes), rsv = attn16_desc(a.gb, a.gbbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float qv[8], gv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, qv);
   attn16_own_row<ELT>(a.g, row, a.ldg, cm.col, cm.ok, gv);
   const float lse = attn16_own_head(a.lse_in, row, a.heads, cm);
   [[maybe_unused]] unsigned hk = 0u;                   // DROP: the head's part of the word, one constant per lane
   if constexpr (DROP) hk = gat_drop_head(a.seed_hi, (unsigned)cm.head);

   float l = 0.0f, dacc = 0.0f;                        // per head: sum a_e, sum a_e t_e
   float pc[8], qc[8];                                 // per column: sum a_e t_e key_jc, sum a_e key_jc
#pragma unroll
   for (int v = 0; v < 8; v++) pc[v] = qc[v] = 0.0f;

   const unsigned ldkb = (unsigned)a.ldga * 2u, ldvb = (unsigned)a.ldgb * 2u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, handed across lanes like the column id
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, (unsigned)pos);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t kv[U], vv[U];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            kv[u] = attn16_load_wide(rsk, attn16_off(id, ldkb), cm);
            vv[u] = attn16_load_wide(rsv, attn16_off(id, ldvb), cm);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float part[2 * U];                            // <q_i, key_j>_h and t_e of the step through one butterfly
#pragma unroll
         for (int u = 0; u < U; u++) {
            float k8[8], v8[8];
            attn16_widen<ELT>(kv[u], cm.ok, k8);
            attn16_widen<ELT>(vv[u], cm.ok, v8);
            part[u] = attn16_dot_part(qv, k8);
            part[U + u] = attn16_dot_part(gv, v8);
         }
         attn16_head_sum<LPR, 2 * U>(part, a.hlanes);         // every lane takes part: not under `live`
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
            if constexpr (DROP) part[U + u] *= gat_drop_mix(hw[u], hk) >= a.T ? a.c : 0.0f;      // t_e = q_e c <g_i, v_j>_h
            const float ae = live ? __expf(part[u] * a.p - lse) : 0.0f;
            const float aet = live ? ae * part[U + u] : 0.0f;
            l += ae;
            dacc += aet;
            float k8[8];
            attn16_widen<ELT>(kv[u], cm.ok, k8);
#pragma unroll
            for (int v = 0; v < 8; v++) {
               pc[v] = fmaf(aet, k8[v], pc[v]);
               qc[v] = fmaf(ae, k8[v], qc[v]);
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1) {
      l += __shfl_xor(l, o);
      dacc += __shfl_xor(dacc, o);
#pragma unroll
      for (int v = 0; v < 8; v++) {
         pc[v] += __shfl_xor(pc[v], o);
         qc[v] += __shfl_xor(qc[v], o);
      }
   }
   if (g != 0) return;
   const bool empty = ee <= eb;
   const float dsum = (empty || cm.poison != 0u) ? 0.0f : dacc / l;      // a lane past k saw no weight: l = 0
   float dq[8];
#pragma unroll
   for (int v = 0; v < 8; v++) dq[v] = empty ? 0.0f : a.p * (pc[v] - dsum * qc[v]);
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, dq);
   if (cm.first) a.hout[(size_t)row * (size_t)a.heads + (size_t)cm.head] = dsum;
}

// one wave per column j of A (a row of the transposed structure): key_j and v_j in registers; q_i, g_i and lse, D of [i, head] gathered
template <int ELT, int LPR, int WAVES, int U, bool DROP>
__global__ __launch_bounds__(WAVES * 64) void mha16_bw_cols_kernel(const typename Mha16KernelArgs<DROP>::type a) {
   constexpr int G = 64 / LPR;
   const int lane = threadIdx.x & 63;
   const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int g = lane / LPR, lc = lane % LPR;
   const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
   if (row >= a.rows) return;
   const int64_t eb = a.pntrb[row], ee = a.pntre[row];
   const __amdgpu_buffer_rsrc_t rsq = attn16_desc(a.ga, a.gabytes), rsg = attn16_desc(a.gb, a.gbbytes);
   const __amdgpu_buffer_rsrc_t rs1 = attn16_desc(a.t1, a.tbytes), rs2 = attn16_desc(a.t2, a.tbytes);
   const Attn16HeadCols cm(a.k, a.hshift, a.hmask, lc);
   float kv[8], vv[8];
   attn16_own_row<ELT>(a.own, row, a.ldown, cm.col, cm.ok, kv);
   attn16_own_row<ELT>(a.own2, row, a.ldown2, cm.col, cm.ok, vv);
   [[maybe_unused]] unsigned hk = 0u;                   // DROP: the head's part of the word, one constant per lane
   if constexpr (DROP) hk = gat_drop_head(a.seed_hi, (unsigned)cm.head);

   float dk[8], dv[8];
#pragma unroll
   for (int v = 0; v < 8; v++) dk[v] = dv[v] = 0.0f;

   const unsigned ldqb = (unsigned)a.ldga * 2u, ldgb = (unsigned)a.ldgb * 2u, hb = (unsigned)a.heads * 4u;
   for (int64_t base = eb; base < ee; base += 64) {
      const int64_t pos = base + lane;
      const int id_l = pos < ee ? (int)a.indx[pos] : -1;
      [[maybe_unused]] unsigned hw_l = 0u;               // DROP: the entry's part of the word, of its CSR position (nnz < 2^31)
      if constexpr (DROP) hw_l = gat_drop_entry(a.seed_lo, pos < ee ? (unsigned)a.epos[pos] : 0u);
      const int64_t left = ee - base;
      const int cnt = left < 64 ? (int)left : 64;
#pragma unroll 1
      for (int s0 = 0; s0 < cnt; s0 += G * U) {
         v4i_t qg[U], gg[U];
         float ls[U], dd[U];
         [[maybe_unused]] unsigned hw[DROP ? U : 1];
#pragma unroll
         for (int u = 0; u < U; u++) {
            const int id = __shfl(id_l, (s0 + u * G + g) & 63);
            qg[u] = attn16_load_wide(rsq, attn16_off(id, ldqb), cm);
            gg[u] = attn16_load_wide(rsg, attn16_off(id, ldgb), cm);
            ls[u] = attn16_load_head(rs1, attn16_off(id, hb), cm);
            dd[u] = attn16_load_head(rs2, attn16_off(id, hb), cm);
            if constexpr (DROP) hw[u] = (unsigned)__shfl((int)hw_l, (s0 + u * G + g) & 63);
         }
         float part[2 * U];
#pragma unroll
         for (int u = 0; u < U; u++) {
            float q8[8], g8[8];
            attn16_widen<ELT>(qg[u], cm.ok, q8);
            attn16_widen<ELT>(gg[u], cm.ok, g8);
            part[u] = attn16_dot_part(q8, kv);             // the products commute bit for bit: the rows kernel's score
            part[U + u] = attn16_dot_part(g8, vv);
         }
         attn16_head_sum<LPR, 2 * U>(part, a.hlanes);         // every lane takes part: not under `live`
#pragma unroll
         for (int u = 0; u < U; u++) {
            const bool live = s0 + u * G + g < cnt;
            const float ae = live ? __expf(part[u] * a.p - ls[u]) : 0.0f;
            float aev = ae;                               // the value coefficient: q_e c a_e
            if constexpr (DROP) {
               const bool keep = gat_drop_mix(hw[u], hk) >= a.T;
               part[U + u] *= keep ? a.c : 0.0f;          // t_e = q_e c <g_i, v_j>_h
               aev = keep ? ae * a.c : 0.0f;
            }
            const float ds = live ? ae * (part[U + u] - dd[u]) : 0.0f;
            float q8[8], g8[8];
            attn16_widen<ELT>(qg[u], cm.ok, q8);
            attn16_widen<ELT>(gg[u], cm.ok, g8);
#pragma unroll
            for (int v = 0; v < 8; v++) {
               dk[v] = fmaf(ds, q8[v], dk[v]);
               dv[v] = fmaf(aev, g8[v], dv[v]);
            }
         }
      }
   }
#pragma unroll
   for (int o = LPR; o < 64; o <<= 1)
#pragma unroll
      for (int v = 0; v < 8; v++) {
         dk[v] += __shfl_xor(dk[v], o);
         dv[v] += __shfl_xor(dv[v], o);
      }
   if (g != 0) return;
#pragma unroll
   for (int v = 0; v < 8; v++) dk[v] *= a.p;          // no incoming entry: 0
   attn16_store_row<ELT>(a.out, row, a.ldout, cm.col, cm.ok, dk);
   attn16_store_row<ELT>(a.out2, row, a.ldout2, cm.col, cm.ok, dv);
}

enum { MHA16_FW = 0, MHA16_BW_ROWS = 1, MHA16_BW_COLS = 2 };

template <int ELT, int LPR, bool DROP>
static int launch_mha16(int which, const Mha16DropArgs &full, const char *entry, hipStream_t st) {
   const typename Mha16KernelArgs<DROP>::type &a = full;
   const int64_t nb = (a.rows + MHA16_WAVES - 1) / MHA16_WAVES;
   if (nb > 0x7fffffffLL) return fail(ISPLIB_FAIL, entry, "too many rows for one launch");
   const dim3 grid((unsigned)nb), block((unsigned)MHA16_WAVES * 64u);
   if (which == MHA16_FW) hipLaunchKernelGGL((mha16_fw_kernel<ELT, LPR, MHA16_WAVES, MHA16_FW_U, DROP>), grid, block, 0, st, a);
   else if (which == MHA16_BW_ROWS) hipLaunchKernelGGL((mha16_bw_rows_kernel<ELT, LPR, MHA16_WAVES, MHA16_ROWS_U, DROP>), grid, block, 0, st, a);
   else hipLaunchKernelGGL((mha16_bw_cols_kernel<ELT, LPR, MHA16_WAVES, MHA16_COLS_U, DROP>), grid, block, 0, st, a);
   return check_launch(entry);
}

// the element type and the slot width (attn16_run); drop: the kernels with attention dropout
static int mha16_run(int dtype, int which, const Mha16DropArgs &a, bool drop, const char *entry, void *stream) {
   return attn16_run(dtype, a.k, [&](auto elt, auto lpr) {
      constexpr int ELT = decltype(elt)::value, LPR = decltype(lpr)::value;
      return drop ? launch_mha16<ELT, LPR, true>(which, a, entry, (hipStream_t)stream)
                  : launch_mha16<ELT, LPR, false>(which, a, entry, (hipStream_t)stream);
   });
}

// what the dropout entries (isplib_qkv_half_drop_*_hip) refuse AFTER the refusals of the entries without dropout, in the order of the
// fp32 dropout entries: attn_drop_refusal, then a seed of 2^63 or more
static const char *mha16_drop_refusal(const AttnDrop &dr, int64_t nnz) {
   if (const char *why = attn_drop_refusal(dr, nnz, "keep_scale must be a positive finite number")) return why;
   return dr.on && dr.seed >= (1ull << 63) ? "seed must be below 2^63" : nullptr;
}

static const char *const MHA16_DOMAIN = "outside isplib_qkv16_serves(rows_gathered, heads, d, ld) = isplib_gat16_serves: 1 <= heads, "
                                        "8 <= heads*d <= 512, heads == 1 with d even or d a power of two >= 8, every pitch even, "
                                        "ld >= heads*d, rows_gathered < 2^31, rows_gathered*ld*2 <= 3.5 GiB (convert the operands and "
                                        "use the fp32 entries)";

}  // namespace isplib

using namespace isplib;

extern "C" int isplib_qkv16_domain(int64_t rows_gathered, int64_t heads, int64_t d, int64_t ld) {
   return isplib_qkv16_serves(rows_gathered, heads, d, ld);
}

extern "C" int isplib_qkv16_auto(int64_t rows_gathered, int64_t ld) { return isplib_qkv16_native_pays(rows_gathered, ld); }

extern "C" int isplib_qkv_half_drop_auto(int64_t rows_gathered, int64_t ld) { return isplib_qkv_half_drop_native_pays(rows_gathered, ld); }

// The three entries, with and without attention dropout.  Their refusals come in one order: dtype, negative dimension, nothing to do, a
// pitch below k, k % heads, the scale, the domain, a null operand, alignment; then, with dropout, the keep scale, nnz >= 2^31, the seed
// and (columns) a null csr2csc -- all before any launch
static int mha16_forward(const char *entry, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                         const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale, const void *q, int64_t ldq,
                         const void *key, int64_t ldk, const void *v, int64_t ldv, void *z, int64_t ldz, float *lse, void *stream,
                         const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldq < k || ldz < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (heads < 1 || !isplib_qkv16_serves(n, heads, k / heads, ldk) || !isplib_qkv16_serves(n, heads, k / heads, ldv) ||
       !attn16_even(ldq, ldz))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA16_DOMAIN);
   if (!pntrb || !pntre || !q || !z || !lse || (nnz > 0 && (!indx || !key || !v))) return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(q, key, v, z)) return fail(ISPLIB_FAIL, entry, "q, key, v and z must be 4-byte aligned");
   if (const char *why = mha16_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   Mha16DropArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(q); a.ldown = ldq;
   a.out = reinterpret_cast<unsigned short *>(z); a.ldout = ldz; a.hout = lse;
   a.ga = key; a.ldga = ldk; a.gabytes = nnz > 0 ? attn16_extent(n, k, ldk, 2u) : 0u;
   a.gb = v; a.ldgb = ldv; a.gbbytes = nnz > 0 ? attn16_extent(n, k, ldv, 2u) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha16_run(dtype, MHA16_FW, a, dr.on, entry, stream);
}

static int mha16_backward_rows(const char *entry, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                               const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale, const void *q, int64_t ldq,
                               const void *key, int64_t ldk, const void *v, int64_t ldv, const void *g, int64_t ldg, const float *lse,
                               void *dq, int64_t lddq, float *dsum, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (m == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldq < k || ldg < k || lddq < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (heads < 1 || !isplib_qkv16_serves(n, heads, k / heads, ldk) || !isplib_qkv16_serves(n, heads, k / heads, ldv) ||
       !attn16_even(ldq, ldg, lddq))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA16_DOMAIN);
   if (!pntrb || !pntre || !q || !g || !lse || !dq || !dsum || (nnz > 0 && (!indx || !key || !v)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(q, key, v, g, dq)) return fail(ISPLIB_FAIL, entry, "q, key, v, g and dq must be 4-byte aligned");
   if (const char *why = mha16_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   Mha16DropArgs a = {};
   a.rows = m; a.k = k; a.indx = indx; a.pntrb = pntrb; a.pntre = pntre; a.p = scale;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(q); a.ldown = ldq;
   a.g = reinterpret_cast<const unsigned short *>(g); a.ldg = ldg; a.lse_in = lse;
   a.out = reinterpret_cast<unsigned short *>(dq); a.ldout = lddq; a.hout = dsum;
   a.ga = key; a.ldga = ldk; a.gabytes = nnz > 0 ? attn16_extent(n, k, ldk, 2u) : 0u;
   a.gb = v; a.ldgb = ldv; a.gbbytes = nnz > 0 ? attn16_extent(n, k, ldv, 2u) : 0u;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha16_run(dtype, MHA16_BW_ROWS, a, dr.on, entry, stream);
}

static int mha16_backward_cols(const char *entry, int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t,
                               const int64_t *colb, const int64_t *cole, const int64_t *csr2csc, int64_t heads, float scale,
                               const void *q, int64_t ldq, const void *g, int64_t ldg, const float *lse, const float *dsum,
                               const void *key, int64_t ldk, const void *v, int64_t ldv, void *dkey, int64_t lddk, void *dv,
                               int64_t lddv, void *stream, const AttnDrop &dr = ATTN_NO_DROP) {
   clear_error();
   if (dtype != ISPLIB_DTYPE_BF16 && dtype != ISPLIB_DTYPE_F16) return fail(ISPLIB_FAIL, entry, ATTN16_DTYPE);
   if (m < 0 || n < 0 || k < 0 || nnz < 0) return fail(ISPLIB_FAIL, entry, "negative dimension");
   if (n == 0 || k == 0) return ISPLIB_SUCCESS;
   if (ldk < k || ldv < k || lddk < k || lddv < k) return fail(ISPLIB_FAIL, entry, "leading dimension smaller than k");
   if (heads >= 1 && k % heads != 0) return fail(ISPLIB_FAIL, entry, "k is not a multiple of heads");
   if (!std::isfinite(scale)) return fail(ISPLIB_FAIL, entry, "scale must be a finite number");
   if (heads < 1 || !isplib_qkv16_serves(m, heads, k / heads, ldq) || !isplib_qkv16_serves(m, heads, k / heads, ldg) ||
       !attn16_even(ldk, ldv, lddk, lddv))
      return fail(ISPLIB_NO_OPT_IMPL, entry, MHA16_DOMAIN);
   if (!colb || !cole || !key || !v || !dkey || !dv || (nnz > 0 && (!row_t || !q || !g || !lse || !dsum)))
      return fail(ISPLIB_FAIL, entry, "null operand");
   if (!attn16_aligned(q, g, key, v, dkey, dv)) return fail(ISPLIB_FAIL, entry, "q, g, key, v, dkey and dv must be 4-byte aligned");
   if (const char *why = mha16_drop_refusal(dr, nnz)) return fail(ISPLIB_FAIL, entry, why);
   if (dr.on && nnz > 0 && !csr2csc) return fail(ISPLIB_FAIL, entry, "null csr2csc: the keep bit is a function of the CSR position");
   Mha16DropArgs a = {};
   a.rows = n; a.k = k; a.indx = row_t; a.pntrb = colb; a.pntre = cole; a.p = scale;
   attn16_head_geometry(heads, k / heads, a.heads, a.hshift, a.hlanes, a.hmask);
   a.own = reinterpret_cast<const unsigned short *>(key); a.ldown = ldk;
   a.own2 = reinterpret_cast<const unsigned short *>(v); a.ldown2 = ldv;
   a.out = reinterpret_cast<unsigned short *>(dkey); a.ldout = lddk;
   a.out2 = reinterpret_cast<unsigned short *>(dv); a.ldout2 = lddv;
   a.ga = q; a.ldga = ldq; a.gabytes = nnz > 0 ? attn16_extent(m, k, ldq, 2u) : 0u;
   a.gb = g; a.ldgb = ldg; a.gbbytes = nnz > 0 ? attn16_extent(m, k, ldg, 2u) : 0u;
   a.t1 = lse; a.t2 = dsum; a.tbytes = nnz > 0 ? attn16_extent(m, heads, heads, 4u) : 0u;
   if (dr.on) a.epos = csr2csc;
   attn_set_drop(dr, a.seed_lo, a.seed_hi, a.T, a.c);
   return mha16_run(dtype, MHA16_BW_COLS, a, dr.on, entry, stream);
}

extern "C" int isplib_qkv16_csr_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                    const int64_t *pntre, int64_t heads, float scale, const void *q, int64_t ldq, const void *key,
                                    int64_t ldk, const void *v, int64_t ldv, void *z, int64_t ldz, float *lse, void *stream) {
   return mha16_forward("isplib_qkv16_csr_hip", dtype, m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, z, ldz,
                        lse, stream);
}

extern "C" int isplib_qkv16_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx, const int64_t *pntrb,
                                        const int64_t *pntre, int64_t heads, float scale, const void *q, int64_t ldq, const void *key,
                                        int64_t ldk, const void *v, int64_t ldv, const void *g, int64_t ldg, const float *lse, void *dq,
                                        int64_t lddq, float *dsum, void *stream) {
   return mha16_backward_rows("isplib_qkv16_bw_rows_hip", dtype, m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv,
                              g, ldg, lse, dq, lddq, dsum, stream);
}

extern "C" int isplib_qkv16_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t, const int64_t *colb,
                                        const int64_t *cole, int64_t heads, float scale, const void *q, int64_t ldq, const void *g,
                                        int64_t ldg, const float *lse, const float *dsum, const void *key, int64_t ldk, const void *v,
                                        int64_t ldv, void *dkey, int64_t lddk, void *dv, int64_t lddv, void *stream) {
   return mha16_backward_cols("isplib_qkv16_bw_cols_hip", dtype, m, n, k, nnz, row_t, colb, cole, nullptr, heads, scale, q, ldq, g, ldg,
                              lse, dsum, key, ldk, v, ldv, dkey, lddk, dv, lddv, stream);
}

// attention dropout: the argument lists of the entries above (the columns entry with csr2csc after cole), then threshold, keep_scale, seed
extern "C" int isplib_qkv_half_drop_csr_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                                            const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale, const void *q,
                                            int64_t ldq, const void *key, int64_t ldk, const void *v, int64_t ldv, void *z, int64_t ldz,
                                            float *lse, void *stream, uint32_t threshold, float keep_scale, uint64_t seed) {
   return mha16_forward("isplib_qkv_half_drop_csr_hip", dtype, m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk, v, ldv, z,
                        ldz, lse, stream, AttnDrop{true, threshold, keep_scale, seed});
}

extern "C" int isplib_qkv_half_drop_bw_rows_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *indx,
                                                const int64_t *pntrb, const int64_t *pntre, int64_t heads, float scale, const void *q,
                                                int64_t ldq, const void *key, int64_t ldk, const void *v, int64_t ldv, const void *g,
                                                int64_t ldg, const float *lse, void *dq, int64_t lddq, float *dsum, void *stream,
                                                uint32_t threshold, float keep_scale, uint64_t seed) {
   return mha16_backward_rows("isplib_qkv_half_drop_bw_rows_hip", dtype, m, n, k, nnz, indx, pntrb, pntre, heads, scale, q, ldq, key, ldk,
                              v, ldv, g, ldg, lse, dq, lddq, dsum, stream, AttnDrop{true, threshold, keep_scale, seed});
}

extern "C" int isplib_qkv_half_drop_bw_cols_hip(int dtype, int64_t m, int64_t n, int64_t k, int64_t nnz, const int64_t *row_t,
                                                const int64_t *colb, const int64_t *cole, const int64_t *csr2csc, int64_t heads,
                                                float scale, const void *q, int64_t ldq, const void *g, int64_t ldg, const float *lse,
                                                const float *dsum, const void *key, int64_t ldk, const void *v, int64_t ldv, void *dkey,
                                                int64_t lddk, void *dv, int64_t lddv, void *stream, uint32_t threshold, float keep_scale,
                                                uint64_t seed) {
   return mha16_backward_cols("isplib_qkv_half_drop_bw_cols_hip", dtype, m, n, k, nnz, row_t, colb, cole, csr2csc, heads, scale, q, ldq, g,
                              ldg, lse, dsum, key, ldk, v, ldv, dkey, lddk, dv, lddv, stream, AttnDrop{true, threshold, keep_scale, seed});
}
