// DeLong statistics of one or two models' scores on the same examples (DeLong, DeLong & Clarke-Pearson 1988):
// what the variance of an AUC and the covariance of two AUCs are made of.  Unweighted, integers only.
//
//   positive i:  a_i = Nlt(s_i) + Nle(s_i)   negatives below + negatives not above, in [0, 2N]
//   negative j:  b_j = Pgt(s_j) + Pge(s_j)   positives above + positives not below, in [0, 2P]
//   U2 = sum_pos a_i = sum_neg b_j,  AUC = U2 / (2 P N)
//   M_pos(x, y) = sum_pos x_i y_i,  M_neg(x, y) = sum_neg x_j y_j over the placements of models x and y
// (ops/kernels.py DelongStats finishes the arithmetic in Python integers).  Scores are ordered as in auc.hip
// (score_key.h).  A placement is below 2^31 and a product t below 2^62; a second moment is kept as two uint64
// words, hi = sum (t >> 32) and lo = sum (t & 0xffffffff) -- both below 2^62 for n < 2^30, and, as integer sums,
// independent of the order of their terms.
//
// Launch chain (no kernel waits for another workgroup; kernel boundaries order the steps), per model:
//   key, sort, tile, base, cum: metric_common.hip's ascending score sort and prefix chain with the channels
//          (negatives, positives), both prefixes: cumN = cum[0], cumP = cum[1], P = cum[1][n];
//   place: per 2048 positions, 8 per thread: the run [lb, ub) of equal keys of every position (by its neighbours,
//          else binary searches: a run may span any number of tiles); a positive's placement cumN[lb] + cumN[ub],
//          a negative's (P - cumP[ub]) + (P - cumP[lb]), stored as uint32 in example order; per tile the sum of
//          the positives' placements; block 0 also keeps the model's P, N, NaN count and sort error word (the
//          second model's chain reuses the prefix pieces and the sort workspace in stream order);
// then once:
//   moments: over the examples in example order, per block the split sums of M_pos and M_neg of (a, a), (b, b)
//          and (a, b) (one model: (a, a) only);
//   final: one block sums the U2 and moment partials and writes the 20-word record; a nonzero sort error word of
//          either model also sets the sticky device error word.
// (Included by module.hip after metric_common.hip.)
#include "fm_common.h"

namespace fm {

constexpr int kDelongRecWords = 20;   // U2_a, U2_b, P, N, 6 x (hi, lo), nans_a, nans_b, has_b, sort error word
constexpr int kDelongMoments = 12;    // (hi, lo) of M_pos / M_neg of (a, a), (b, b), (a, b)
constexpr int kDelongMomBlocks = 1024;  // the most blocks of the moments kernel (a grid-stride loop over tiles)
constexpr int kDelongKeep = 4;        // per model: P, N, NaN count, sort error word

struct DelongPlaceArgs {
  PrefixArgs<uint64_t> p;
  uint32_t* pl;     // [n] placement of every example
  uint64_t* part;   // [ntiles] sum of the positives' placements in the tile
  uint64_t* keep;   // [kDelongKeep]
};

__global__ __launch_bounds__(kBlock) void delong_place_kernel(DelongPlaceArgs a) {
  __shared__ uint64_t sh[kWavesPerBlock];
  const int n = a.p.n;
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  const uint64_t* cn = a.p.cum[0];
  const uint64_t* cp = a.p.cum[1];
  const uint64_t P = cp[n];
  uint32_t sv[kAucItems], k[kAucItems];
  int ex[kAucItems];
  load8(a.p.sv, j0, n, sv, 0u);
  load8(a.p.skeys, j0, n, k, 0u);
  load8(a.p.sidx, j0, n, ex, -1);
  const uint32_t kprev = (j0 > 0 && j0 <= n) ? a.p.skeys[j0 - 1] : 0u;
  const uint32_t knext = j0 + kAucItems < n ? a.p.skeys[j0 + kAucItems] : 0u;
  uint64_t u = 0;
  bool have = false;  // (lb, ub) of the previous position hold for this one: same key
  int lb = 0, ub = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= n) break;
    const bool tie_prev = j > 0 && (q ? k[q - 1] : kprev) == k[q];
    if (!(have && tie_prev)) {
      const bool tie_next = j + 1 < n && (q + 1 < kAucItems ? k[q + 1] : knext) == k[q];
      lb = tie_prev ? auc_bound<false>(a.p.skeys, 0, j, k[q]) : j;
      ub = tie_next ? auc_bound<true>(a.p.skeys, j + 1, n, k[q]) : j + 1;
      have = true;
    }
    const float s = __uint_as_float(sv[q]);
    if ((unsigned)ex[q] >= (unsigned)n) continue;  // no example (only after a failed sort: its error word says so)
    uint64_t v;
    if (s > 0.f) {
      v = cn[lb] + cn[ub];
      u += v;
    } else {
      v = (P - cp[ub]) + (P - cp[lb]);
    }
    a.pl[ex[q]] = (uint32_t)v;
  }
  uint64_t e, t;
  auc_block_scan<uint64_t, kWavesPerBlock>(u, e, t, sh);
  if (threadIdx.x == 0) {
    a.part[blockIdx.x] = t;
    if (blockIdx.x == 0) {
      a.keep[0] = P;
      a.keep[1] = cn[n];
      a.keep[2] = (uint64_t)*a.p.nan_count;
      a.keep[3] = (uint64_t)(int64_t)*a.p.sort_err;
    }
  }
}

// The block's sums of every thread's v[0 .. NV) (in thread 0): integers, so any order gives the same words.
template <int NV>
__device__ inline void delong_block_sum(uint64_t (&v)[NV], uint64_t (*sh)[kWavesPerBlock] /*[NV]*/) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v[i] += __shfl_down(v[i], o, kWave);
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) sh[i][threadIdx.x >> 6] = v[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      uint64_t t = 0;
#pragma unroll
      for (int w = 0; w < kWavesPerBlock; ++w) t += sh[i][w];
      v[i] = t;
    }
  }
  __syncthreads();
}

struct DelongMomentArgs {
  int n, ntiles;
  const uint32_t* pl_a;  // [n]
  const uint32_t* pl_b;  // [n], or null: one model
  const float* labels;
  bool lab16;            // labels serve 16-byte loads (a caller's view need not)
  uint64_t* part;        // [gridDim.x][kDelongMoments]
};

// t = x * y into the split sum (hi, lo).
__device__ inline void delong_add(uint64_t& hi, uint64_t& lo, uint32_t x, uint32_t y) {
  const uint64_t t = (uint64_t)x * (uint64_t)y;
  hi += t >> 32;
  lo += t & 0xffffffffull;
}

template <bool kTwo>
__global__ __launch_bounds__(kBlock) void delong_moments_kernel(DelongMomentArgs a) {
  __shared__ uint64_t sh[kDelongMoments][kWavesPerBlock];
  uint64_t m[kDelongMoments];
#pragma unroll
  for (int i = 0; i < kDelongMoments; ++i) m[i] = 0;
  for (int tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    const int j0 = tile * kAucTile + threadIdx.x * kAucItems;
    uint32_t pa[kAucItems], pb[kAucItems], lab[kAucItems];
    load8(a.pl_a, j0, a.n, pa, 0u);
    if (kTwo) load8(a.pl_b, j0, a.n, pb, 0u);
    const uint32_t* lb = reinterpret_cast<const uint32_t*>(a.labels);
    if (a.lab16) {
      load8(lb, j0, a.n, lab, 0u);
    } else {
#pragma unroll
      for (int q = 0; q < kAucItems; ++q) lab[q] = j0 + q < a.n ? lb[j0 + q] : 0u;
    }
#pragma unroll
    for (int q = 0; q < kAucItems; ++q) {
      if (j0 + q >= a.n) break;
      const bool neg = !(__uint_as_float(lab[q]) > 0.f);  // (selects on the class, no divergent code)
      uint64_t h = 0, l = 0;
      delong_add(h, l, pa[q], pa[q]);
      m[0] += neg ? 0 : h; m[1] += neg ? 0 : l; m[2] += neg ? h : 0; m[3] += neg ? l : 0;
      if (kTwo) {
        h = l = 0;
        delong_add(h, l, pb[q], pb[q]);
        m[4] += neg ? 0 : h; m[5] += neg ? 0 : l; m[6] += neg ? h : 0; m[7] += neg ? l : 0;
        h = l = 0;
        delong_add(h, l, pa[q], pb[q]);
        m[8] += neg ? 0 : h; m[9] += neg ? 0 : l; m[10] += neg ? h : 0; m[11] += neg ? l : 0;
      }
    }
  }
  delong_block_sum<kDelongMoments>(m, sh);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < kDelongMoments; ++i) a.part[(size_t)blockIdx.x * kDelongMoments + i] = m[i];
  }
}

struct DelongFinalArgs {
  int ntiles, nmom;          // U2 partials per model; blocks of the moments kernel
  const uint64_t* part_u2[2];  // [ntiles] per model (1: null for one model; both null: moments only)
  const uint64_t* part_mom;  // [nmom][kDelongMoments]
  const uint64_t* keep[2];   // [kDelongKeep] per model
  uint64_t* out;             // [kDelongRecWords], or [kDelongMoments] for the moments alone
};

// kRecord: the whole record; else the 12 moment words alone (delong_moments).
template <bool kRecord>
__global__ __launch_bounds__(kBlock) void delong_final_kernel(DelongFinalArgs a) {
  __shared__ uint64_t sh[kDelongMoments + 2][kWavesPerBlock];
  uint64_t v[kDelongMoments + 2];
#pragma unroll
  for (int i = 0; i < kDelongMoments + 2; ++i) v[i] = 0;
  for (int i = threadIdx.x; i < a.nmom; i += kBlock) {
#pragma unroll
    for (int w = 0; w < kDelongMoments; ++w) v[w] += a.part_mom[(size_t)i * kDelongMoments + w];
  }
  if (kRecord) {
    for (int i = threadIdx.x; i < a.ntiles; i += kBlock) {
      v[kDelongMoments] += a.part_u2[0][i];
      if (a.part_u2[1]) v[kDelongMoments + 1] += a.part_u2[1][i];
    }
  }
  delong_block_sum<kDelongMoments + 2>(v, sh);
  if (threadIdx.x != 0) return;
  if (!kRecord) {
#pragma unroll
    for (int w = 0; w < kDelongMoments; ++w) a.out[w] = v[w];
    return;
  }
  const bool two = a.keep[1] != nullptr;
  const uint64_t err = a.keep[0][3] | (two ? a.keep[1][3] : 0);
  a.out[0] = v[kDelongMoments];
  a.out[1] = v[kDelongMoments + 1];
  a.out[2] = a.keep[0][0];
  a.out[3] = a.keep[0][1];
#pragma unroll
  for (int w = 0; w < kDelongMoments; ++w) a.out[4 + w] = v[w];
  a.out[16] = a.keep[0][2];
  a.out[17] = two ? a.keep[1][2] : 0;
  a.out[18] = two ? 1 : 0;
  a.out[19] = err;
  if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
}

static int delong_moment_blocks(int ntiles) { return ntiles < kDelongMomBlocks ? ntiles : kDelongMomBlocks; }

// Workspace: the prefix chain's pieces (both prefixes; reused by the second model), the placements and U2
// partials per model, the moment partials, what is kept per model, then the sort workspace.
struct DelongLayout {
  PrefixLayout p;
  size_t pl[2], part_u2[2], part_mom, keep, sort, total;
};

static DelongLayout delong_layout(int n, bool two) {
  WsCursor c;
  DelongLayout l{};
  l.p = prefix_layout(c, n, ThrChannels::kSecondPrefix);
  const size_t nt = (size_t)l.p.ntiles;
  for (int m = 0; m < (two ? 2 : 1); ++m) {
    l.pl[m] = c.take(4 * (size_t)n);
    l.part_u2[m] = c.take(8 * nt);
  }
  l.part_mom = c.take(8 * kDelongMoments * (size_t)delong_moment_blocks(l.p.ntiles));
  l.keep = c.take(8 * kDelongKeep * 2);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

// Bytes of launch_delong's workspace for n scores of one or two models; 0: n is out of range (n >= 2^30, the
// sort's bound).  (A workspace for two models serves one as well.)
size_t delong_workspace_bytes(long long n, bool two_models) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  if (n == 0) return 256;
  return delong_layout((int)n, two_models).total;
}

// Bytes of launch_delong_moments' workspace (the moment partials) for n examples; 0: n is out of range.
size_t delong_moments_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  const int ntiles = (int)((n + kAucTile - 1) / kAucTile);
  return rs_align(8 * kDelongMoments * (size_t)(ntiles < 1 ? 1 : delong_moment_blocks(ntiles)));
}

static void delong_launch_moments(const uint32_t* pl_a, const uint32_t* pl_b, const float* labels, int n,
                                  uint64_t* part, int nmom, hipStream_t st) {
  const DelongMomentArgs m{n, (n + kAucTile - 1) / kAucTile, pl_a, pl_b, labels,
                           (reinterpret_cast<uintptr_t>(labels) & 15) == 0, part};
  if (pl_b) hipLaunchKernelGGL(delong_moments_kernel<true>, dim3(nmom), dim3(kBlock), 0, st, m);
  else hipLaunchKernelGGL(delong_moments_kernel<false>, dim3(nmom), dim3(kBlock), 0, st, m);
}

// DeLong statistics of n >= 1 scores of one model (scores_b null) or two into out[kDelongRecWords] (uint64),
// asynchronously on st.  0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30.
int launch_delong(const float* scores_a, const float* scores_b, const float* labels, int n, void* out, void* ws,
                  size_t ws_bytes, hipStream_t st) {
  if (const int rc = metric_check_args(n, scores_a, labels, out, ws)) return rc;
  const bool two = scores_b != nullptr;
  const DelongLayout l = delong_layout(n, two);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  DelongFinalArgs f{};
  f.ntiles = l.p.ntiles;
  f.nmom = delong_moment_blocks(l.p.ntiles);
  uint32_t* pl[2] = {nullptr, nullptr};
  for (int m = 0; m < (two ? 2 : 1); ++m) {
    DelongPlaceArgs a{};
    const int se = launch_score_prefix<uint64_t, ThrChannels>(m ? scores_b : scores_a, labels, nullptr, n, b, l.p,
                                                              b + l.sort, st, a.p);
    if (se != 0) return se;
    a.pl = pl[m] = reinterpret_cast<uint32_t*>(b + l.pl[m]);
    a.part = reinterpret_cast<uint64_t*>(b + l.part_u2[m]);
    a.keep = reinterpret_cast<uint64_t*>(b + l.keep) + m * kDelongKeep;
    f.part_u2[m] = a.part;
    f.keep[m] = a.keep;
    hipLaunchKernelGGL(delong_place_kernel, dim3(l.p.ntiles), dim3(kBlock), 0, st, a);
  }
  uint64_t* part_mom = reinterpret_cast<uint64_t*>(b + l.part_mom);
  delong_launch_moments(pl[0], pl[1], labels, n, part_mom, f.nmom, st);
  f.part_mom = part_mom;
  f.out = static_cast<uint64_t*>(out);
  hipLaunchKernelGGL(delong_final_kernel<true>, dim3(1), dim3(kBlock), 0, st, f);
  return (int)hipGetLastError();
}

// The 12 moment words (hi, lo of M_pos / M_neg of (a, a), (b, b), (a, b); pl_b null: (a, a) only, the rest 0) of
// n >= 1 placements into out[kDelongMoments] (uint64), asynchronously on st.  Return codes as launch_delong.
int launch_delong_moments(const uint32_t* pl_a, const uint32_t* pl_b, const float* labels, int n, void* out, void* ws,
                          size_t ws_bytes, hipStream_t st) {
  if (const int rc = metric_check_args(n, pl_a, labels, out, ws)) return rc;
  if ((reinterpret_cast<uintptr_t>(pl_a) | reinterpret_cast<uintptr_t>(pl_b)) & 15) return -1;  // (16-byte loads)
  if (ws_bytes < delong_moments_workspace_bytes(n)) return -2;
  DelongFinalArgs f{};
  f.nmom = delong_moment_blocks((n + kAucTile - 1) / kAucTile);
  f.part_mom = static_cast<uint64_t*>(ws);
  f.out = static_cast<uint64_t*>(out);
  delong_launch_moments(pl_a, pl_b, labels, n, static_cast<uint64_t*>(ws), f.nmom, st);
  hipLaunchKernelGGL(delong_final_kernel<false>, dim3(1), dim3(kBlock), 0, st, f);
  return (int)hipGetLastError();
}

}  // namespace fm
