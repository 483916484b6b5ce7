// Definitions shared by the top-k ranking kernel (hip/fm_topk.hip) and its CPU twin (cpu/kernels.cpp):
// the column order of the dot product, the selection key and the slab plan.  Both sides include this
// file, so they cannot drift apart; the results are required to agree bit for bit.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FM_TOPK_HD __host__ __device__
#else
#define FM_TOPK_HD
#endif

namespace fm {
namespace topk {

constexpr int kMaxK = 128;    // results per query
constexpr int kMaxKp = 256;   // profile width
constexpr int kTile = 16;     // queries / candidates per matrix-core tile (v_mfma_f32_16x16x4_f32)

// ---- the column order pi(Kp) --------------------------------------------------------------------
// dot = 0; for i in 0 .. Kp-1 (ascending): dot = fmaf(Q[col(i)], C[col(i)], dot), with
//   col = 16 g + 4 h + e,   the loops nested g (outer), e, h (inner); columns >= Kp are skipped.
// On the GPU lane (r, h) of a wave loads the 16 bytes at columns 16 g + 4 h .. + 3 of row r; element e
// of that load is the lane's operand of the 16x16x4 matrix instruction number 4 g + e, whose k index is
// h: the instruction is a fmaf chain over k = 0 .. 3 in that order.  A group cut short by Kp feeds zeros,
// and fmaf(0, 0, dot) == dot (dot starts at +0 and never becomes -0), which is the same as skipping.
constexpr int kGroup = 16;  // columns per 16-byte-load group
FM_TOPK_HD inline int groups(int Kp) { return (Kp + kGroup - 1) / kGroup; }
FM_TOPK_HD inline int col(int g, int e, int h) { return kGroup * g + 4 * h + e; }

// f(column) for every column of pi(Kp) in order (the CPU twin's loop; Kp a multiple of 4)
template <typename F>
inline void for_each_col(int Kp, F&& f) {
  for (int g = 0; g < groups(Kp); ++g)
    for (int e = 0; e < 4; ++e)
      for (int h = 0; h < 4; ++h)
        if (col(g, 0, h) < Kp) f(col(g, e, h));
}

// ---- the selection key ----------------------------------------------------------------------------
// 64 bits: the score's order-preserving image (negatives with all bits flipped, the
// others with the sign bit set) above 0xFFFFFFFF - candidate.  Greater key = greater score, equal scores
// by ascending candidate; the k greatest keys are the answer.  Every key of a real candidate (< 2^31) is
// nonzero, so 0 marks an empty place.
FM_TOPK_HD inline uint32_t order_u32(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
FM_TOPK_HD inline uint32_t unorder_u32(uint32_t k) { return (k & 0x80000000u) ? (k ^ 0x80000000u) : ~k; }
FM_TOPK_HD inline uint64_t make_key(uint32_t score_bits, uint32_t c) {
  return ((uint64_t)order_u32(score_bits) << 32) | (uint64_t)(0xFFFFFFFFu - c);
}
FM_TOPK_HD inline int key_index(uint64_t key) { return key ? (int)(0xFFFFFFFFu - (uint32_t)key) : -1; }
FM_TOPK_HD inline uint32_t key_score_bits(uint64_t key) {
  return key ? unorder_u32((uint32_t)(key >> 32)) : 0xFF800000u;  // empty: -inf
}

// ---- the slab plan -------------------------------------------------------------------------------
// The candidates are cut into `parts` slabs of `slab` candidates (the last one shorter); one wave ranks
// one 16-query tile against one slab and leaves its k best keys, phase 2 merges a query's `parts` lists.
// Enough (tile, slab) pairs to fill the chip whatever nq is (a single query against 2^20 candidates: 512
// waves), at most kMaxParts lists per query, and slabs of at least kMinSlab candidates (a multiple of 32:
// two candidate tiles are in flight) so that the selection's warm-up stays a small share of a slab
// (measured: 2048 slabs of 512 instead of 512 of 2048 made 64 queries against 2^20 candidates 1.6x slower).
constexpr int kTargetWaves = 2048;
constexpr int kMaxParts = 512;
constexpr int kMinSlab = 256;
struct Plan { long long slab; int parts; };
inline Plan plan(long long nq, long long nc, int /*k*/) {
  const long long qt = nq > 0 ? (nq + kTile - 1) / kTile : 1;
  long long want = (kTargetWaves + qt - 1) / qt;
  if (want < 1) want = 1;
  if (want > kMaxParts) want = kMaxParts;
  long long slab = nc > 0 ? (nc + want - 1) / want : 1;
  slab = (slab + 31) / 32 * 32;
  if (slab < kMinSlab) slab = kMinSlab;
  long long parts = nc > 0 ? (nc + slab - 1) / slab : 1;
  return Plan{slab, (int)parts};
}

}  // namespace topk
}  // namespace fm
