// gat_dropout.h -- the keep bit of the GAT aggregation's attention dropout (gat.hip, DROP kernels), stated once for the
// kernels and the host.  For a stored entry at CSR position pos (< 2^31), a head h and a non-negative 64-bit seed:
//    fmix32(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16                    (uint32 arithmetic)
//    word(seed, pos, h) = fmix32( fmix32(uint32(pos) ^ uint32(seed)) + uint32(h) * 0x9E3779B9 + uint32(seed >> 32) )
//    T(p) = min(2^32 - 1, floor(p * 2^32))   in double        keep = word >= T                                 T(0) = 0 keeps everything
// The inner fmix32 depends on the entry alone (the lane that loads the entry's index hashes it and hands the word across with the
// index); what is left per edge and chunk is one add of a per-lane constant, one fmix32 and one compare.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ISPLIB_HD __host__ __device__
#else
#define ISPLIB_HD
#endif

namespace isplib {

ISPLIB_HD inline uint32_t gat_fmix32(uint32_t x) {
   x ^= x >> 16;
   x *= 0x85ebca6bu;
   x ^= x >> 13;
   x *= 0xc2b2ae35u;
   x ^= x >> 16;
   return x;
}

// the part of the word that depends on the entry alone
ISPLIB_HD inline uint32_t gat_drop_entry(uint32_t seed_lo, uint32_t pos) { return gat_fmix32(pos ^ seed_lo); }

// the part that depends on the head alone: a per-lane constant of a launch
ISPLIB_HD inline uint32_t gat_drop_head(uint32_t seed_hi, uint32_t head) { return head * 0x9E3779B9u + seed_hi; }

ISPLIB_HD inline uint32_t gat_drop_mix(uint32_t entry, uint32_t headk) { return gat_fmix32(entry + headk); }

ISPLIB_HD inline uint32_t gat_drop_word(uint64_t seed, int64_t pos, int64_t head) {
   return gat_drop_mix(gat_drop_entry((uint32_t)seed, (uint32_t)pos), gat_drop_head((uint32_t)(seed >> 32), (uint32_t)head));
}

// T(p); p <= 0 (and NaN) gives 0, p >= 1 - 2^-32 gives 2^32 - 1
inline uint32_t gat_drop_threshold(double p) {
   const double v = std::floor(p * 4294967296.0);
   if (!(v > 0.0)) return 0u;
   return v >= 4294967295.0 ? 0xffffffffu : (uint32_t)v;
}

}  // namespace isplib
