// Exact weighted ROC AUC of (score, label, weight) triples (the trainer's validation AUC; the reference
// reports the validation loss only, run_tffm.py:64-75).
//
//   P = sum_{pos} w_i,  N = sum_{neg} w_j           (positive iff label > 0)
//   U2 = sum_{i pos} w_i (Nlt(s_i) + Nle(s_i)),     Nlt / Nle: weight of the negatives below / not above s_i
//   AUC = U2 / (2 P N)                              (a positive-negative tie counts one half)
//
// Scores are ordered as IEEE fp32 values by score_key.h's key (-0.0 == +0.0, denormals keep their order,
// +-inf are ordinary values); NaN scores are counted (the host reports NaN when there is one).  Two modes,
// both bitwise reproducible run to run (no float atomics, every sum in a fixed order): unweighted
// (weights == null) in uint64 -- exact --, weighted in fp64.
//
// Launch chain (no kernel waits for another workgroup; kernel boundaries order the steps):
//   key, sort, tile, base, cum: metric_common.hip's score sort and prefix chain with the channels
//          (negatives, positives): Nex[j] = cum[0][j] = weight of the negatives at sorted positions < j,
//          j in [0, n]; tot = [N, P];
//   rank:  a positive at sorted position j adds w (Nex[lb] + Nex[ub]), [lb, ub) = its run of equal keys:
//          (j, j + 1) when both neighbours differ, else a binary search in the sorted keys (a tie run may
//          span any number of tiles); per-tile partial sums;
//   final: one block sums the partials in tile order and writes the record [U2, P, N, nan count, sort
//          error word] (uint64 or fp64); a nonzero sort error also sets the sticky device error word.
// (Included by module.hip after metric_common.hip.)
#include "fm_common.h"

namespace fm {

template <typename T>
struct AucArgs : PrefixArgs<T> {
  T* part;  // [ntiles] U2 partial sums
  T* out;   // [5] U2, P, N, nan count, sort error word
};

template <typename T>
__global__ __launch_bounds__(kBlock) void auc_rank_kernel(AucArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  const T* nex = a.cum[0];
  uint32_t sv[kAucItems], k[kAucItems];
  load8(a.sv, j0, a.n, sv, 0u);
  load8(a.skeys, j0, a.n, k, 0u);
  const uint32_t kprev = (j0 > 0 && j0 <= a.n) ? a.skeys[j0 - 1] : 0u;
  const uint32_t knext = j0 + kAucItems < a.n ? a.skeys[j0 + kAucItems] : 0u;
  T u = 0;
  bool have = false;  // (lb, ub) of the previous position hold for this one: same key
  int lb = 0, ub = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    const float s = __uint_as_float(sv[q]);
    const bool tie_prev = j < a.n && j > 0 && (q ? k[q - 1] : kprev) == k[q];
    if (!(j < a.n && s > 0.f)) {
      have = have && tie_prev;
      continue;
    }
    if (!(have && tie_prev)) {
      const bool tie_next = j + 1 < a.n && (q + 1 < kAucItems ? k[q + 1] : knext) == k[q];
      lb = tie_prev ? auc_bound<false>(a.skeys, 0, j, k[q]) : j;
      ub = tie_next ? auc_bound<true>(a.skeys, j + 1, a.n, k[q]) : j + 1;
      have = true;
    }
    u += (T)s * (nex[lb] + nex[ub]);
  }
  T e, t;
  auc_block_scan<T, kWavesPerBlock>(u, e, t, sh);
  if (threadIdx.x == 0) a.part[blockIdx.x] = t;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void auc_final_kernel(AucArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  // thread t sums its contiguous share of the partials in tile order, then the block in thread order
  const int per = (a.ntiles + kBlock - 1) / kBlock;
  T u = 0;
  for (int i = threadIdx.x * per; i < min(a.ntiles, (threadIdx.x + 1) * per); ++i) u += a.part[i];
  T e, t;
  auc_block_scan<T, kWavesPerBlock>(u, e, t, sh);
  if (threadIdx.x == 0) {
    const int err = *a.sort_err;
    a.out[0] = t;
    a.out[1] = a.tot[1];
    a.out[2] = a.tot[0];
    a.out[3] = (T)*a.nan_count;
    a.out[4] = (T)err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
}

// Workspace: the prefix chain's pieces (one prefix; the fourth tile array holds the U2 partials), then the
// sort workspace.
struct AucLayout {
  PrefixLayout p;
  size_t sort, total;
};

static AucLayout auc_layout(int n) {
  WsCursor c;
  AucLayout l{};
  l.p = prefix_layout(c, n, AucChannels::kSecondPrefix);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

// Bytes of launch_auc's workspace for n scores; 0: n is out of range (n >= 2^30, the sort's bound).
size_t auc_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  if (n == 0) return 256;
  return auc_layout((int)n).total;
}

template <typename T>
static int launch_auc_t(const float* scores, const float* labels, const float* weights, int n, void* out, char* ws,
                        const AucLayout& l, hipStream_t st) {
  AucArgs<T> a{};
  const int se = launch_score_prefix<T, AucChannels>(scores, labels, weights, n, ws, l.p, ws + l.sort, st, a);
  if (se != 0) return se;
  a.part = reinterpret_cast<T*>(ws + l.p.tiles) + 3 * (size_t)l.p.ntiles;
  a.out = static_cast<T*>(out);
  hipLaunchKernelGGL(auc_rank_kernel<T>, dim3(l.p.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(auc_final_kernel<T>, dim3(1), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

// AUC statistics of n >= 1 scores into out[5] (uint64 when weights is null, else fp64), asynchronously on st.
// 0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30.
int launch_auc(const float* scores, const float* labels, const float* weights, int n, void* out, void* ws,
               size_t ws_bytes, hipStream_t st) {
  if (const int rc = metric_check_args(n, scores, labels, out, ws)) return rc;
  const AucLayout l = auc_layout(n);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  if (weights) return launch_auc_t<double>(scores, labels, weights, n, out, b, l, st);
  return launch_auc_t<uint64_t>(scores, labels, weights, n, out, b, l, st);
}

}  // namespace fm
