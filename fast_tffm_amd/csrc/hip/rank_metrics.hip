// Ranking metrics per group: NDCG@k, recall@k and precision@k of every group (a user, a query, a session) and
// their plain means over the ranked groups -- what the top of a recommendation list is judged by, next to
// gauc.hip's grouped AUC.
//
//   gain_i = y_i if y_i > 0 else 0; positive iff y_i > 0; rank 1 = the group's highest score (score_key.h order);
//   a run of equal scores of one group occupies the ranks a..b and every member gets the run's mean position
//   weight (the exact expectation under uniformly random tie-breaking, since every sum below is linear in the
//   position weights):  cbar = (C_k(b) - C_k(a - 1)) / (b - a + 1),  C_k(r) = sum_{j <= min(r, k)} c(j);
//   per group g and cutoff k:  DCG = sum gain_i cbar_i with c(j) = 1 / log2(j + 1)   (C_k(r) = D[min(r, k)], the
//                                                                         host-built table of ../rank_table.h)
//                              IDCG = the same sum with the gains as the scores
//                              hits = sum_{i positive} cbar_i with c(j) = [j <= k]
//                              NDCG = DCG / IDCG, recall = hits / P_g, precision = hits / k
//   ranked iff P_g > 0; every reported metric is the mean over the ranked groups.
//
// Launch chain (kernel boundaries order the steps; no host read, the workspace is the caller's: capturable):
//   gain:   the gain of every example;
//   then twice -- once on the scores (DCG, hits, P_g), once on the gains as scores (IDCG):
//     key, sort 1, gather, sort 2: as gauc.hip -> (group, score ascending) order;
//     tile:   score key and gain of every sorted position, every group's [first, end) range;
//     run:    a position with a positive gain finds its run [lb, ub) of equal (group, key) as gauc_rank_kernel
//             does (neighbours first, else binary searches clamped to the group's range) -> ranks a = end - ub + 1
//             .. b = end - lb; channel by channel (P_g, then DCG@k and hits@k per cutoff) the terms are summed
//             by a segmented scan in the tile: a group whose head lies in the tile gets its sum at its tail,
//             the one open at the tile's start leaves its partial sum;
//     carry:  one block per channel carries those partials over the tiles in tile order;
//   group:  one thread per group: n_g, and for a ranked group the three ratios per cutoff; block sums in a fixed
//           order;
//   final:  one block sums the blocks' partials in order and writes the record
//           [per cutoff: sum NDCG_g, sum recall_g, sum precision_g (fp64)] [ranked groups, examples in ranked
//            groups, NaN count, sort error word]; a nonzero sort error also sets the sticky device error word.
// Everything is fp64; every sum adds only non-negative terms of ONE group in a fixed order (a thread's positions in
// order, the segmented block scan, the tiles in tile order): bitwise the same run to run.  Only runs with a <= k add
// a nonzero term to a cutoff's DCG or hits.  (Included by module.hip after gauc.hip: the segmented scan, the group-id
// helpers and the gather kernel are defined there.)
#include <mutex>

#include "../rank_table.h"
#include "fm_common.h"

namespace fm {

constexpr int kRankMaxChannels = 1 + 2 * kRankMaxCutoffs;  // P_g, then (DCG@k, hits@k) per cutoff
constexpr int kRankMaxDevices = 64;

__device__ double g_rank_dcg[kRankMaxCutoff + 1];  // D (rank_table.h), uploaded once per device

enum RankKind : int { kRankPos = 0, kRankDcg = 1, kRankHits = 2 };

struct RankArgs {
  int n, ntiles, G, gblocks, nk, ncol, nch;
  int k[kRankMaxCutoffs];
  int kind[kRankMaxChannels];  // what channel c sums
  int ck[kRankMaxChannels];    // its cutoff
  int col[kRankMaxChannels];   // its column of per
  const float* gains;      // [n] gain of every example
  const uint32_t* keys;    // [n] score key of every example
  const int* sg;           // [n] group id of every (group, score)-sorted position
  const int* sidx;         // [n] example index of every sorted position
  uint32_t* fkeys;         // [n] score key of every sorted position
  uint32_t* gv;            // [n] float bits: gain of every sorted position
  int* grange;             // [G, 2] first position, last position + 1 (0, 0: empty)
  int* tflag;              // [ntiles] the tile holds a group head
  double* tu;              // [nch, ntiles] channel terms from the tile's last head (or its start) to its end
  double* fu;              // [nch, ntiles] the same from the tile's start to the tail of the group open there
  double* per;             // [G, ncol] n_g, P_g, then (DCG, IDCG, hits) per cutoff
  double* gpart;           // [gblocks, 3 nk + 2] per block of groups: the ratios' sums, ranked groups, their examples
  const unsigned* nan_count;
  int* errs;               // [4] the four sorts' error words
  const int* sort_err;     // the sort workspace's error word
  int err_slot;            // where the tile kernel saves it
  void* out;               // [3 nk + 4] the record
};

__global__ __launch_bounds__(kBlock) void rank_gain_kernel(int n, const float* labels, float* gains) {
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const float y = labels[e];
    gains[e] = y > 0.f ? y : 0.f;
  }
}

// the group ids of a thread's 8 positions, of the position before and of the one after (-1: none)
__device__ inline void rank_groups(const RankArgs& a, int j0, int (&g)[kAucItems], int& gprev, int& gnext) {
  load8(a.sg, j0, a.n, g, 0);
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) g[q] = gauc_gid(g[q], a.G);
  gprev = (j0 > 0 && j0 <= a.n) ? gauc_gid(a.sg[j0 - 1], a.G) : -1;
  gnext = j0 + kAucItems < a.n ? gauc_gid(a.sg[j0 + kAucItems], a.G) : -1;
}

__global__ __launch_bounds__(kBlock) void rank_tile_kernel(RankArgs a) {
  __shared__ int shany[kWavesPerBlock];
  if (blockIdx.x == 0 && threadIdx.x == 0) a.errs[a.err_slot] = *a.sort_err;
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  int ex[kAucItems], g[kAucItems], gprev, gnext;
  load8(a.sidx, j0, a.n, ex, -1);
  rank_groups(a, j0, g, gprev, gnext);
  bool hf = false;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    if (gauc_head(g, q, gprev)) {
      a.grange[2 * (size_t)g[q]] = j;
      hf = true;
    }
    if (gauc_tail(g, q, gnext, j, a.n)) a.grange[2 * (size_t)g[q] + 1] = j + 1;
    const bool ok = (unsigned)ex[q] < (unsigned)a.n;  // (not after a failed sort: its error word is reported)
    a.gv[j] = ok ? __float_as_uint(a.gains[ex[q]]) : 0u;
    a.fkeys[j] = ok ? a.keys[ex[q]] : 0u;
  }
  const bool any = __any(hf);
  if ((threadIdx.x & (kWave - 1)) == 0) shany[threadIdx.x >> 6] = any;
  __syncthreads();
  if (threadIdx.x == 0) {
    int f = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) f |= shany[w];
    a.tflag[blockIdx.x] = f;
  }
}

// The term of channel c for a position of gain > 0 whose run occupies the ranks a..b (1 <= a <= b).
__device__ inline double rank_term(int kind, int k, float gain, int ra, int rb) {
  if (kind == kRankPos) return 1.0;
  if (ra > k) return 0.0;
  const int lo = min(ra - 1, k), hi = min(rb, k);
  const double len = (double)(rb - ra + 1);
  if (kind == kRankHits) return (double)(hi - lo) / len;
  return (double)gain * ((g_rank_dcg[hi] - g_rank_dcg[lo]) / len);
}

__global__ __launch_bounds__(kBlock) void rank_run_kernel(RankArgs a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ double shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  uint32_t k[kAucItems], gb[kAucItems];
  float gn[kAucItems];
  int g[kAucItems], gprev, gnext;
  load8(a.fkeys, j0, a.n, k, 0u);
  load8(a.gv, j0, a.n, gb, 0u);
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) gn[q] = __uint_as_float(gb[q]);
  rank_groups(a, j0, g, gprev, gnext);
  const uint32_t kprev = (j0 > 0 && j0 <= a.n) ? a.fkeys[j0 - 1] : 0u;
  const uint32_t knext = j0 + kAucItems < a.n ? a.fkeys[j0 + kAucItems] : 0u;
  int ra[kAucItems], rb[kAucItems];  // the ranks of the position's run; ra == 0: the position adds nothing
  bool hf = false;
  bool have = false;  // (lb, ub) of the previous position hold for this one: same group and key
  int lb = 0, ub = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    ra[q] = 0;
    rb[q] = 0;
    if (j >= a.n) continue;
    const bool head = gauc_head(g, q, gprev);
    hf = hf || head;
    const bool tie_prev = !head && (q ? k[q - 1] : kprev) == k[q];
    if (!(gn[q] > 0.f)) {
      have = have && tie_prev;
      continue;
    }
    const int first = a.grange[2 * (size_t)g[q]], end = a.grange[2 * (size_t)g[q] + 1];
    if (!(have && tie_prev)) {
      const bool tail = gauc_tail(g, q, gnext, j, a.n);
      const bool tie_next = !tail && (q + 1 < kAucItems ? k[q + 1] : knext) == k[q];
      lb = j;
      ub = j + 1;
      if (tie_prev) lb = auc_bound<false>(a.fkeys, min(first, j), j, k[q]);
      if (tie_next) ub = auc_bound<true>(a.fkeys, j + 1, max(end, j + 1), k[q]);
      have = true;
    }
    // (lb <= j < ub <= end in a sorted set; the clamps keep a failed sort's ranks inside the table)
    ra[q] = max(end - ub + 1, 1);
    rb[q] = max(end - lb, ra[q]);
  }
#pragma unroll 1
  for (int c = 0; c < a.nch; ++c) {
    const int kind = a.kind[c], ck = a.ck[c], col = a.col[c];
    double u[kAucItems], usum = 0;
#pragma unroll
    for (int q = 0; q < kAucItems; ++q) {
      const int j = j0 + q;
      u[q] = 0;
      if (j >= a.n) continue;
      if (gauc_head(g, q, gprev)) usum = 0;
      if (ra[q]) u[q] = rank_term(kind, ck, gn[q], ra[q], rb[q]);
      usum += u[q];
    }
    bool ef, tf;
    double ev, tv;
    gauc_seg_scan<double, kWavesPerBlock>(hf, usum, ef, ev, tf, tv, shf, shv);
    if (threadIdx.x == 0) a.tu[(size_t)c * a.ntiles + blockIdx.x] = tv;
    double run = ev;
    bool seen = ef;  // a head of this tile lies before the position: its group's sum is whole
#pragma unroll
    for (int q = 0; q < kAucItems; ++q) {
      const int j = j0 + q;
      if (j >= a.n) continue;
      if (gauc_head(g, q, gprev)) {
        run = 0;
        seen = true;
      }
      run += u[q];
      if (gauc_tail(g, q, gnext, j, a.n)) {
        if (seen) a.per[(size_t)g[q] * a.ncol + col] = run;
        else a.fu[(size_t)c * a.ntiles + blockIdx.x] = run;
      }
    }
  }
}

// block c: channel c's partials over the tiles in tile order (gauc_ubase_kernel, one channel per block)
__global__ __launch_bounds__(kAucBaseThreads) void rank_carry_kernel(RankArgs a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ int shf[NW];
  __shared__ double shv[NW];
  const int c = blockIdx.x, col = a.col[c];
  const double* tu = a.tu + (size_t)c * a.ntiles;
  const double* fu = a.fu + (size_t)c * a.ntiles;
  double carry = 0;
  for (int b = 0; b < a.ntiles; b += kAucBaseThreads) {
    const int t = b + threadIdx.x;
    const bool ok = t < a.ntiles;
    bool ef, tf;
    double ev, tv;
    gauc_seg_scan<double, NW>(ok && a.tflag[t] != 0, ok ? tu[t] : 0.0, ef, ev, tf, tv, shf, shv);
    if (ok && t > 0) {
      // the group open at the tile's start, when it ends in this tile: what the tiles before it hold of it
      // (in tile order) plus this tile's share
      const int j0 = t * kAucTile;
      const int g = gauc_gid(a.sg[j0], a.G);
      if (g == gauc_gid(a.sg[j0 - 1], a.G) && a.grange[2 * (size_t)g + 1] <= min(a.n, j0 + kAucTile))
        a.per[(size_t)g * a.ncol + col] = (ef ? ev : carry + ev) + fu[t];
    }
    carry = tf ? tv : carry + tv;
  }
}

// The block's sums (in thread order) of a thread's 3 nk ratios and two counts into o[3 nk + 2] (64-bit words).
__device__ inline void rank_pack_sums(int nk, const double (&r)[3 * kRankMaxCutoffs], uint64_t ranked, uint64_t exs,
                                      double* o) {
  __shared__ double shd[kWavesPerBlock];
  __shared__ uint64_t shu[kWavesPerBlock];
  double ed, td;
  uint64_t eu, tr, te;
#pragma unroll
  for (int i = 0; i < 3 * kRankMaxCutoffs; ++i) {
    if (i < 3 * nk) {  // (uniform over the block)
      auc_block_scan<double, kWavesPerBlock>(r[i], ed, td, shd);
      if (threadIdx.x == 0) o[i] = td;
    }
  }
  auc_block_scan<uint64_t, kWavesPerBlock>(ranked, eu, tr, shu);
  auc_block_scan<uint64_t, kWavesPerBlock>(exs, eu, te, shu);
  if (threadIdx.x == 0) {
    reinterpret_cast<uint64_t*>(o)[3 * nk] = tr;
    reinterpret_cast<uint64_t*>(o)[3 * nk + 1] = te;
  }
}

__global__ __launch_bounds__(kBlock) void rank_group_kernel(RankArgs a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  double r[3 * kRankMaxCutoffs];
#pragma unroll
  for (int i = 0; i < 3 * kRankMaxCutoffs; ++i) r[i] = 0.0;
  uint64_t ranked = 0, exs = 0;
  if (g < a.G) {
    double* p = a.per + (size_t)g * a.ncol;
    const int ng = a.grange[2 * (size_t)g + 1] - a.grange[2 * (size_t)g];
    p[0] = (double)ng;
    const double pos = p[1];
    if (pos > 0) {
      ranked = 1;
      exs = (uint64_t)ng;
#pragma unroll
      for (int i = 0; i < kRankMaxCutoffs; ++i) {
        if (i < a.nk) {
          const double dcg = p[2 + 3 * i], idcg = p[3 + 3 * i], hits = p[4 + 3 * i];
          r[3 * i] = dcg / idcg;
          r[3 * i + 1] = hits / pos;
          r[3 * i + 2] = hits / (double)a.k[i];
        }
      }
    }
  }
  rank_pack_sums(a.nk, r, ranked, exs, a.gpart + (size_t)(3 * a.nk + 2) * blockIdx.x);
}

__global__ __launch_bounds__(kBlock) void rank_final_kernel(RankArgs a) {
  // thread t sums its contiguous share of the blocks' partials in block order, then the block in thread order
  const int per = (a.gblocks + kBlock - 1) / kBlock, w = 3 * a.nk + 2;
  double r[3 * kRankMaxCutoffs];
#pragma unroll
  for (int i = 0; i < 3 * kRankMaxCutoffs; ++i) r[i] = 0.0;
  uint64_t ranked = 0, exs = 0;
  for (long long b = (long long)threadIdx.x * per; b < min((long long)a.gblocks, (long long)(threadIdx.x + 1) * per);
       ++b) {
    const double* o = a.gpart + (size_t)w * b;
#pragma unroll
    for (int i = 0; i < 3 * kRankMaxCutoffs; ++i)
      if (i < 3 * a.nk) r[i] += o[i];
    ranked += reinterpret_cast<const uint64_t*>(o)[3 * a.nk];
    exs += reinterpret_cast<const uint64_t*>(o)[3 * a.nk + 1];
  }
  double* o = static_cast<double*>(a.out);
  rank_pack_sums(a.nk, r, ranked, exs, o);
  if (threadIdx.x == 0) {
    const int err = a.errs[0] | a.errs[1] | a.errs[2] | a.errs[3];
    reinterpret_cast<uint64_t*>(o)[w] = (uint64_t)*a.nan_count;
    reinterpret_cast<uint64_t*>(o)[w + 1] = (uint64_t)(unsigned)err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
}

// Workspace: [keys n][idx -> gv n][score-sorted keys -> final keys n][score-sorted idx n][group keys n]
// [sorted groups n][sorted idx n][gains n][tiles: 2 x 9 x 8 + 4 bytes each][grange 2 G][gpart 14 x 8 per block
// of groups][nan count, the ideal chain's, 4 sort errors][sort workspace]
struct RankLayout {
  size_t keys, bufa, bufb, si1, gk, sg, si2, gains, tiles, tflag, grange, gpart, misc, sort, total;
  int ntiles, gblocks;
};

static RankLayout rank_layout(int n, long long G) {
  WsCursor c;
  RankLayout l{};
  l.ntiles = (n + kAucTile - 1) / kAucTile;
  l.gblocks = (int)((G + kBlock - 1) / kBlock);
  l.keys = c.take(4 * (size_t)n);
  l.bufa = c.take(4 * (size_t)n);
  l.bufb = c.take(4 * (size_t)n);
  l.si1 = c.take(4 * (size_t)n);
  l.gk = c.take(4 * (size_t)n);
  l.sg = c.take(4 * (size_t)n);
  l.si2 = c.take(4 * (size_t)n);
  l.gains = c.take(4 * (size_t)n);
  l.tiles = c.take(8 * 2 * kRankMaxChannels * (size_t)l.ntiles);
  l.tflag = c.take(4 * (size_t)l.ntiles);
  l.grange = c.take(8 * (size_t)G);
  l.gpart = c.take(8 * (3 * kRankMaxCutoffs + 2) * (size_t)l.gblocks);
  l.misc = c.take(32);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

// Bytes of launch_rank_metrics's workspace for n scores in G groups; 0: out of range (as gauc_workspace_bytes).
size_t rank_metrics_workspace_bytes(long long n, long long G) {
  if (!gauc_sizes_ok(n, G)) return 0;
  return rank_layout((int)(n > 0 ? n : 1), G).total;
}

// D on the current device: uploaded by the first call there (a synchronous copy: not inside a stream capture).
static int rank_table_ready() {
  static std::mutex mu;
  static bool ready[kRankMaxDevices] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (dev < 0 || dev >= kRankMaxDevices) return -1;
  std::lock_guard<std::mutex> lock(mu);
  if (ready[dev]) return 0;
  static double d[kRankMaxCutoff + 1];
  rank_dcg_table(d);
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_rank_dcg), d, sizeof(d));
  if (e != hipSuccess) return (int)e;
  ready[dev] = true;
  return 0;
}

// Ranking statistics of n >= 1 scores with group ids in [0, G) at the nk cutoffs k (1 to 4, strictly ascending, in
// [1, 4096]): per-group records into per[G, 2 + 3 nk] (fp64) and the record into out[3 nk + 4] (64-bit words),
// asynchronously on st.  0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30;
// -6: G outside [1, 2^31); -7: bad cutoffs.
int launch_rank_metrics(const float* scores, const float* labels, const int* groups, int n, long long G,
                        const int* k, int nk, void* out, void* per, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!groups || !per || (reinterpret_cast<uintptr_t>(per) & 7)) return -1;
  if (const int rc = metric_check_args(n, scores, labels, out, ws)) return rc;
  if (G < 1 || G >= (1ll << 31)) return -6;
  if (!rank_cutoffs_ok(k, nk)) return -7;
  const RankLayout l = rank_layout(n, G);
  if (ws_bytes < l.total) return -2;
  if (const int rc = rank_table_ready()) return rc;
  char* b = static_cast<char*>(ws);
  uint32_t* keys = reinterpret_cast<uint32_t*>(b + l.keys);
  int* idx = reinterpret_cast<int*>(b + l.bufa);
  uint32_t* sk1 = reinterpret_cast<uint32_t*>(b + l.bufb);
  int* si1 = reinterpret_cast<int*>(b + l.si1);
  uint32_t* gk = reinterpret_cast<uint32_t*>(b + l.gk);
  uint32_t* sg = reinterpret_cast<uint32_t*>(b + l.sg);
  int* si2 = reinterpret_cast<int*>(b + l.si2);
  float* gains = reinterpret_cast<float*>(b + l.gains);
  double* tiles = reinterpret_cast<double*>(b + l.tiles);
  int* grange = reinterpret_cast<int*>(b + l.grange);
  unsigned* nan_count = reinterpret_cast<unsigned*>(b + l.misc);  // [1]: the ideal chain's (gains: always 0)
  int* errs = reinterpret_cast<int*>(b + l.misc) + 2;
  void* sort_ws = b + l.sort;
  const int ncol = 2 + 3 * nk;
  hipError_t e = hipMemsetAsync(grange, 0, 8 * (size_t)G, st);
  if (e == hipSuccess) e = hipMemsetAsync(per, 0, 8 * (size_t)ncol * (size_t)G, st);
  if (e != hipSuccess) return (int)e;
  const int grid = fill_grid(n, kBlock, 2048);
  hipLaunchKernelGGL(rank_gain_kernel, dim3(grid), dim3(kBlock), 0, st, n, labels, gains);
  RankArgs a{};
  a.n = n;
  a.ntiles = l.ntiles;
  a.G = (int)G;
  a.gblocks = l.gblocks;
  a.nk = nk;
  a.ncol = ncol;
  for (int i = 0; i < nk; ++i) a.k[i] = k[i];
  a.gains = gains;
  a.keys = keys;
  a.sg = reinterpret_cast<const int*>(sg);
  a.sidx = si2;
  a.fkeys = sk1;                          // the score-sorted keys are dead by then: the final order's keys
  a.gv = reinterpret_cast<uint32_t*>(idx);  // so is the identity index: the gains of the final order
  a.grange = grange;
  a.tflag = reinterpret_cast<int*>(b + l.tflag);
  a.tu = tiles;
  a.fu = tiles + (size_t)kRankMaxChannels * l.ntiles;
  a.per = static_cast<double*>(per);
  a.gpart = reinterpret_cast<double*>(b + l.gpart);
  a.nan_count = nan_count;
  a.errs = errs;
  a.out = out;
  for (int pass = 0; pass < 2; ++pass) {  // 0: the scores (P_g, DCG, hits); 1: the gains as scores (IDCG)
    ScoreSort s1;
    int se = launch_score_sort(pass ? gains : scores, n, keys, idx, sk1, si1, nan_count + pass, sort_ws, st, s1);
    if (se != 0) return se;
    hipLaunchKernelGGL(gauc_gather_kernel, dim3(grid), dim3(kBlock), 0, st, n, (int)G, groups, si1, gk, s1.sort_err,
                       errs + 2 * pass);
    se = launch_radix_sort(gk, si1, sg, si2, n, gauc_bits_for(G), sort_ws, radix_sort_ws_bytes(n), st);
    if (se != 0) return se;
    a.sort_err = s1.sort_err;
    a.err_slot = 2 * pass + 1;
    a.nch = 0;
    auto channel = [&a](int kind, int ck, int col) {
      a.kind[a.nch] = kind;
      a.ck[a.nch] = ck;
      a.col[a.nch++] = col;
    };
    if (!pass) channel(kRankPos, 0, 1);
    for (int i = 0; i < nk; ++i) {
      channel(kRankDcg, k[i], 2 + 3 * i + pass);
      if (!pass) channel(kRankHits, k[i], 4 + 3 * i);
    }
    hipLaunchKernelGGL(rank_tile_kernel, dim3(l.ntiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(rank_run_kernel, dim3(l.ntiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(rank_carry_kernel, dim3(a.nch), dim3(kAucBaseThreads), 0, st, a);
  }
  hipLaunchKernelGGL(rank_group_kernel, dim3(l.gblocks), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(rank_final_kernel, dim3(1), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace fm
