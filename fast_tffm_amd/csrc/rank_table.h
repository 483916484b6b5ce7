// The discount table of the ranking metrics (hip/rank_metrics.hip and its CPU twin): D[r] = sum_{j <= r} 1 / log2(j + 1),
// r in [0, kRankMaxCutoff], built by ONE sequential fp64 loop on the host so that both sides read the same bits.
// C_k(r), the discount mass of the ranks 1..min(r, k), is D[min(r, k)].
#pragma once
#include <cmath>

namespace fm {

constexpr int kRankMaxCutoff = 4096;  // the largest cutoff k of NDCG@k / recall@k / precision@k
constexpr int kRankMaxCutoffs = 4;    // cutoffs per call

inline void rank_dcg_table(double* d /*[kRankMaxCutoff + 1]*/) {
  d[0] = 0.0;
  for (int j = 1; j <= kRankMaxCutoff; ++j) d[j] = d[j - 1] + 1.0 / std::log2(static_cast<double>(j) + 1.0);
}

// 1 to 4 strictly ascending cutoffs in [1, kRankMaxCutoff]
inline bool rank_cutoffs_ok(const int* k, int nk) {
  if (!k || nk < 1 || nk > kRankMaxCutoffs) return false;
  for (int i = 0; i < nk; ++i)
    if (k[i] < 1 || k[i] > kRankMaxCutoff || (i && k[i] <= k[i - 1])) return false;
  return true;
}

}  // namespace fm
