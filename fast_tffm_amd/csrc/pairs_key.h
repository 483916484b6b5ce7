// Definitions shared by the pair-interaction kernel (hip/fm_pairs.hip) and its CPU twin (cpu/kernels.cpp):
// the limits and the 64-bit selection key.  The dot product's column order is topk_order.h's pi(Kp).  Both
// sides include this file, so they cannot drift apart; the results are required to agree bit for bit.
#pragma once
#include <cstdint>

#include "topk_order.h"

namespace fm {
namespace pairs {

constexpr int kMaxTop = 64;    // pairs returned per example
constexpr int kMaxN = 4096;    // occurrences per example: the pair index j * kMaxN + l stays below 2^24

// ---- the selection key ----------------------------------------------------------------------------
// 64 bits: the bit image of |p| above [0xFFFFFF - (j * kMaxN + l)] above p's sign bit.  Greater key =
// greater |p| (a NaN above every number), equal |p| by ascending (j, l) whatever the signs (-0 == +0: the
// sign sits below the pair index and no two candidates share one).  The `top` greatest keys are the answer.
// j < l < kMaxN, so the index field is at least 1 and every key of a real pair is nonzero: 0 marks an
// empty place.
FM_TOPK_HD inline uint64_t make_key(uint32_t p_bits, int j, int l) {
  const uint32_t idx = (uint32_t)j * (uint32_t)kMaxN + (uint32_t)l;
  return ((uint64_t)(p_bits & 0x7FFFFFFFu) << 32) | (uint64_t)(((0xFFFFFFu - idx) << 1) | (p_bits >> 31));
}
FM_TOPK_HD inline int key_first(uint64_t key) { return key ? (int)((0xFFFFFFu - ((uint32_t)key >> 1)) / kMaxN) : -1; }
FM_TOPK_HD inline int key_second(uint64_t key) { return key ? (int)((0xFFFFFFu - ((uint32_t)key >> 1)) % kMaxN) : -1; }
FM_TOPK_HD inline uint32_t key_value_bits(uint64_t key) {  // the signed p; +0 for an empty place
  return (uint32_t)(key >> 32) | ((uint32_t)key << 31);
}

}  // namespace pairs
}  // namespace fm
