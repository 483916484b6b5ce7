// The order of fp32 scores in the metrics (AUC, GAUC, isotonic fit): one definition for the host
// (cpu/kernels.cpp) and for the gfx950 kernels (hip/metric_common.hip, hip/isotonic.hip).
//
// Scores compare as IEEE fp32 values through an order-preserving 32-bit key of their bit pattern (negatives:
// all bits flipped; the others: sign bit set).  -0.0 is folded onto +0.0 by its bit pattern; no arithmetic
// touches the score, so denormals keep their order; +-inf are ordinary values; NaN scores are counted apart.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FM_SCORE_HD __host__ __device__ inline
#else
#define FM_SCORE_HD inline
#endif

namespace fm {

FM_SCORE_HD uint32_t score_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0u;  // -0.0 == +0.0
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// The fp32 bit pattern of a key (of +0.0 for either zero).
FM_SCORE_HD uint32_t score_key_bits(uint32_t key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

FM_SCORE_HD bool score_is_nan(uint32_t bits) { return (bits & 0x7fffffffu) > 0x7f800000u; }

}  // namespace fm
