// Definitions shared by the place kernel (hip/fm_place.hip) and its CPU twin (cpu/kernels.cpp): the slab plan,
// the record layout and the metric terms of one context.  The score and its column order are topk_order.h's,
// the discount and harmonic sums rank_table.h's; both sides include this file, so they cannot drift apart.
#pragma once
#include <cstdint>
#include "rank_table.h"
#include "topk_order.h"

namespace fm {
namespace place {

constexpr int kWaves = 4;                              // waves per workgroup, one 16-query tile each
constexpr int kQueryBlock = kWaves * topk::kTile;      // queries per workgroup
constexpr int kMetricTile = 1024;                      // contexts per fp64 partial of the reduce pass

// ---- the slab plan --------------------------------------------------------------------------------
// The candidates are cut into `parts` slabs of `slab` candidates (the last one shorter); one workgroup counts
// one 64-query block against one slab and leaves (greater, equal) per query.  There is no selection to warm up,
// so a slab only has to be a whole number of staged chunks (kSlabUnit, the longest chunk): about kTargetGroups
// workgroups whatever nq is, at most kMaxParts partial counts per query.
constexpr int kTargetGroups = 1024;
constexpr int kMaxParts = 1024;
constexpr int kSlabUnit = 128;
struct Plan { long long slab; int parts; };
inline Plan plan(long long nq, long long nc) {
  const long long qb = nq > 0 ? (nq + kQueryBlock - 1) / kQueryBlock : 1;
  long long want = (kTargetGroups + qb - 1) / qb;
  if (want > kMaxParts) want = kMaxParts;
  long long slab = nc > 0 ? (nc + want - 1) / want : 1;
  slab = (slab + kSlabUnit - 1) / kSlabUnit * kSlabUnit;
  const long long parts = nc > 0 ? (nc + slab - 1) / slab : 1;
  return Plan{slab, (int)parts};
}

// ---- the record -----------------------------------------------------------------------------------
// 2 + 3 nk 64-bit words: [ranked contexts (int64), sum of a + b over them (int64: twice mean_place's numerator),
// then per cutoff the sums of hit, ndcg, mrr (fp64)].
FM_TOPK_HD inline int rec_words(int nk) { return 2 + 3 * nk; }

// The terms of one ranked context (equal >= 1): the target holds the places a = greater + 1 .. b = greater +
// equal, and a metric with the position weights c(j), C(r) = sum_{j <= min(r, k)} c(j), is (C(b) - C(a - 1)) /
// equal -- the expectation under uniform tie-breaking.  out[3 i .. 3 i + 2] = hit, ndcg, mrr at cutoff k[i];
// D / H: rank_dcg_table / rank_harmonic_table.  Returns a + b.
FM_TOPK_HD inline long long terms(int greater, int equal, const int* k, int nk, const double* D, const double* H,
                                  double* out) {
  const long long lo_r = greater, hi_r = (long long)greater + equal;
  const double len = (double)equal;
  for (int i = 0; i < nk; ++i) {
    const int lo = lo_r < k[i] ? (int)lo_r : k[i], hi = hi_r < k[i] ? (int)hi_r : k[i];
    out[3 * i] = (double)(hi - lo) / len;
    out[3 * i + 1] = (D[hi] - D[lo]) / len;
    out[3 * i + 2] = (H[hi] - H[lo]) / len;
  }
  return lo_r + hi_r + 1;
}

// ---- several targets per context (hip/fm_place_multi.hip) -------------------------------------------
// A context's ascending target list is cut into segments of at most kSegment entries; one row of the count pass is
// one (context, segment), so T targets own ceil(T / kSegment) rows and at most nq + nnz / kSegment rows exist.
constexpr int kSegment = 32;
FM_TOPK_HD inline long long segments(long long T) { return (T + kSegment - 1) / kSegment; }
inline long long multi_rows_max(long long nq, long long nnz) { return nq + nnz / kSegment; }

// The record: 3 + 3 nk 64-bit words: [ranked contexts, entries, sum of a + b over the entries (int64); then per
// cutoff the sums of recall, ndcg, precision over the ranked contexts (fp64)].
FM_TOPK_HD inline int multi_rec_words(int nk) { return 3 + 3 * nk; }

// The terms of one ranked context from its T >= 1 (greater, equal) pairs in ascending target order: entry t holds
// the places a = greater + 1 .. b = greater + equal, the context's hits and DCG at k are the sums over its entries
// of (min(b, k) - min(a - 1, k)) / equal and (D[min(b, k)] - D[min(a - 1, k)]) / equal -- rank_metrics' expectation
// under uniform tie-breaking with label 1 on the targets -- added in fp64 in entry order.  out[3 i .. 3 i + 2] =
// recall, ndcg, precision at k[i].  Returns the sum of a + b.
FM_TOPK_HD inline long long multi_terms(const int* counts, long long T, const int* k, int nk, const double* D,
                                        double* out) {
  long long ab = 0;
  for (int i = 0; i < nk; ++i) {
    double hits = 0.0, dcg = 0.0;
    for (long long t = 0; t < T; ++t) {
      const long long lo_r = counts[2 * t], hi_r = lo_r + counts[2 * t + 1];
      const double len = (double)counts[2 * t + 1];
      const int lo = lo_r < k[i] ? (int)lo_r : k[i], hi = hi_r < k[i] ? (int)hi_r : k[i];
      hits += (double)(hi - lo) / len;
      dcg += (D[hi] - D[lo]) / len;
      if (i == 0) ab += lo_r + hi_r + 1;
    }
    out[3 * i] = hits / (double)T;
    out[3 * i + 1] = dcg / D[T < k[i] ? (int)T : k[i]];
    out[3 * i + 2] = hits / (double)k[i];
  }
  return ab;
}

}  // namespace place
}  // namespace fm
