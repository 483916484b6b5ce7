// What the score-sorted metric chains (auc.hip, threshold_metrics.hip, isotonic.hip, gauc.hip) share: the tile
// constants and the ordered block scan, the score sort, the workspace cursor and the launchers' argument check,
// and the two-channel prefix kernels of the AUC, the threshold metrics and the isotonic fit.
//
// Score sort (launch_score_sort; scores ordered as score_key.h says, or from the highest down on request):
//   key:   key (complemented for the descending order) + example index per score, NaN count (integer atomic,
//          one per wave);
//   sort:  launch_radix_sort over all 32 key bits (radix_sort.hip: 4 passes of 8 bits, stable).
// Prefix chain (launch_score_prefix: the sort, then, per sum type T and channel policy):
//   tile:  per 2048-element tile of the sorted order the signed weight of every position (+w positive,
//          -w negative: the only gather through the sorted index) and the tile's totals of both channels;
//   base:  one block scans the tile totals in tile order -> every tile's exclusive prefix and the totals;
//   cum:   cum[c][j] = channel c's weight at the sorted positions < j, j in [0, n].
// Every sum has a fixed order and starts from zero: a thread's terms in position order, the block scan, the
// tiles in tile order; a channel that does not apply to a position adds an explicit zero (every term is >= 0).
// (Included by module.hip after dedup.hip: it defines load8 and includes the radix sort.  The names keep the
// prefix of the chain they were first written for.)
#include "../score_key.h"
#include "fm_common.h"

namespace fm {

constexpr int kAucItems = 8;                    // consecutive sorted positions per thread
constexpr int kAucTile = kBlock * kAucItems;    // 2048
constexpr int kAucBaseThreads = 1024;           // the single block of a tile-total scan

// Block-wide scan of one value per thread in a fixed order (wave scan by shuffles, then the waves' totals
// in wave order): excl = sum of the values of the threads before this one, total = the block's sum.
// (The exclusive value comes from a shifted inclusive scan, never from a subtraction: fp64.)
template <typename T, int NW>
__device__ inline void auc_block_scan(T v, T& excl, T& total, T* sh /*[NW]*/) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(inc, o, kWave);
    if (lane >= o) inc += up;
  }
  const T before = __shfl_up(inc, 1, kWave);
  if (lane == kWave - 1) sh[wv] = inc;
  __syncthreads();
  T b = 0, t = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w == wv) b = t;
    t += sh[w];
  }
  excl = lane ? b + before : b;
  total = t;
  __syncthreads();
}

// First position in [lo, hi) whose key is >= k (UPPER: > k); hi when there is none.
template <bool UPPER>
__device__ inline int auc_bound(const uint32_t* keys, int lo, int hi, uint32_t k) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    const uint32_t km = keys[mid];
    if (UPPER ? km <= k : km < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Signed weight of example ex: +w (label > 0) / -w; 0 when ex is no example (only after a failed sort: its
// error word is reported).
__device__ inline float signed_weight(const float* labels, const float* weights, int ex, int n) {
  if ((unsigned)ex >= (unsigned)n) return 0.f;
  const float w = weights ? weights[ex] : 1.f;
  return labels[ex] > 0.f ? w : -w;
}

// ---- score sort -----------------------------------------------------------------------------------------
// (kDesc: the complemented key, so that the ascending sort runs from the highest score down; ties stay in input
// order.)
template <bool kDesc = false>
__global__ __launch_bounds__(kBlock) void auc_key_kernel(int n, const uint32_t* score_bits, uint32_t* keys, int* idx,
                                                         unsigned* nan_count) {
  unsigned nn = 0;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const uint32_t b = score_bits[e];
    nn += score_is_nan(b);
    keys[e] = kDesc ? ~score_key(b) : score_key(b);
    idx[e] = e;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) nn += __shfl_down(nn, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && nn) atomicAdd(nan_count, nn);
}

struct ScoreSort {
  const uint32_t* skeys;      // [n] sorted keys
  const int* sidx;            // [n] example index of every sorted position (ties in input order)
  const unsigned* nan_count;  // NaN scores
  const int* sort_err;        // the sort's error word (in its workspace)
};

// Keys n >= 1 scores into keys / idx (the identity index), counts the NaNs and sorts into skeys / sidx,
// asynchronously on st; sort_ws holds radix_sort_ws_bytes(n).  0, a hip error code or launch_radix_sort's.
// descending: the keys are complemented (the highest score first).
static int launch_score_sort(const float* scores, int n, uint32_t* keys, int* idx, uint32_t* skeys, int* sidx,
                             unsigned* nan_count, void* sort_ws, hipStream_t st, ScoreSort& s,
                             bool descending = false) {
  const hipError_t e = hipMemsetAsync(nan_count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  const dim3 grid(fill_grid(n, kBlock, 2048));
  const uint32_t* bits = reinterpret_cast<const uint32_t*>(scores);
  if (descending) hipLaunchKernelGGL(auc_key_kernel<true>, grid, dim3(kBlock), 0, st, n, bits, keys, idx, nan_count);
  else hipLaunchKernelGGL(auc_key_kernel<false>, grid, dim3(kBlock), 0, st, n, bits, keys, idx, nan_count);
  s = ScoreSort{skeys, sidx, nan_count, radix_sort_error(sort_ws, n)};
  return launch_radix_sort(keys, idx, skeys, sidx, n, 32, sort_ws, radix_sort_ws_bytes(n), st);
}

// ---- workspace layout and argument check ----------------------------------------------------------------
// Hands out consecutive 256-byte-aligned pieces of a workspace; off is the size so far.
struct WsCursor {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += rs_align(bytes);
    return o;
  }
};

// The launchers' common check: -1 bad arguments (the workspace serves 16-byte loads), -5 n >= 2^30.
static int metric_check_args(int n, const void* scores, const void* labels, const void* out, const void* ws) {
  if (n < 1 || !scores || !labels || !out || !ws) return -1;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return -1;
  if ((unsigned)n > kOsCnt) return -5;
  return 0;
}

// ---- two-channel prefix chain ---------------------------------------------------------------------------
// A channel policy names the two non-negative terms a position's signed weight s adds -- the first channel takes
// the negatives' weight, or with kAll everybody's; the second the positives' -- and whether the second channel
// gets per-tile bases and a per-position prefix (its tile totals and its total are always kept).
template <bool kAll, bool kSecond>
struct Channels {
  static constexpr bool kSecondPrefix = kSecond;
  template <typename T>
  static __device__ T first(float s) { return s > 0.f ? (kAll ? (T)s : (T)0) : (T)(-s); }
  template <typename T>
  static __device__ T second(float s) { return s > 0.f ? (T)s : (T)0; }
};
using AucChannels = Channels<false, false>;  // (negatives, positives), the negatives' prefix only
using IsoChannels = Channels<true, true>;    // (all, positives), both prefixes
using ThrChannels = Channels<false, true>;   // (negatives, positives), both prefixes

template <typename T>
struct PrefixArgs {
  int n, ntiles;
  const float* labels;
  const float* weights;    // null: all ones
  const uint32_t* skeys;   // [n] sorted keys
  const int* sidx;         // [n] example index of every sorted position
  uint32_t* sv;            // [n] float bits: the signed weight of every sorted position
  T* cum[2];               // [n + 1] channel c's weight before every position (1: null without kSecondPrefix)
  T* tile_tot[2];          // [ntiles] channel c's weight in the tile
  T* tile_base[2];         // [ntiles] channel c's weight before the tile (1: null without kSecondPrefix)
  T* tot;                  // [2] channel c's total
  const unsigned* nan_count;
  const int* sort_err;
};

template <typename T, typename C>
__global__ __launch_bounds__(kBlock) void prefix_tile_kernel(PrefixArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  int ex[kAucItems];
  load8(a.sidx, j0, a.n, ex, -1);
  T c0 = 0, c1 = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    if (j0 + q >= a.n) continue;
    const float s = signed_weight(a.labels, a.weights, ex[q], a.n);
    a.sv[j0 + q] = __float_as_uint(s);
    c0 += C::template first<T>(s);
    c1 += C::template second<T>(s);
  }
  T e, t;
  auc_block_scan<T, kWavesPerBlock>(c0, e, t, sh);
  if (threadIdx.x == 0) a.tile_tot[0][blockIdx.x] = t;
  auc_block_scan<T, kWavesPerBlock>(c1, e, t, sh);
  if (threadIdx.x == 0) a.tile_tot[1][blockIdx.x] = t;
}

template <typename T, typename C>
__global__ __launch_bounds__(kAucBaseThreads) void prefix_base_kernel(PrefixArgs<T> a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ T sh[NW];
  T carry0 = 0, carry1 = 0;
  for (int c = 0; c < a.ntiles; c += kAucBaseThreads) {
    const int t = c + threadIdx.x;
    const bool ok = t < a.ntiles;
    T e, t0, t1;
    auc_block_scan<T, NW>(ok ? a.tile_tot[0][t] : (T)0, e, t0, sh);
    if (ok) a.tile_base[0][t] = carry0 + e;
    carry0 += t0;
    auc_block_scan<T, NW>(ok ? a.tile_tot[1][t] : (T)0, e, t1, sh);
    if (C::kSecondPrefix && ok) a.tile_base[1][t] = carry1 + e;
    carry1 += t1;
  }
  if (threadIdx.x == 0) {
    a.tot[0] = carry0;
    a.tot[1] = carry1;
  }
}

template <typename T, typename C>
__global__ __launch_bounds__(kBlock) void prefix_cum_kernel(PrefixArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  uint32_t sv[kAucItems];
  load8(a.sv, j0, a.n, sv, 0u);
  T m0[kAucItems], m1[kAucItems], c0 = 0, c1 = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const float s = __uint_as_float(sv[q]);
    const bool in = j0 + q < a.n;
    m0[q] = in ? C::template first<T>(s) : (T)0;
    c0 += m0[q];
    if constexpr (C::kSecondPrefix) {
      m1[q] = in ? C::template second<T>(s) : (T)0;
      c1 += m1[q];
    }
  }
  T e0, e1 = 0, t;
  auc_block_scan<T, kWavesPerBlock>(c0, e0, t, sh);
  if constexpr (C::kSecondPrefix) auc_block_scan<T, kWavesPerBlock>(c1, e1, t, sh);
  T r0 = a.tile_base[0][blockIdx.x] + e0, r1 = 0;
  if constexpr (C::kSecondPrefix) r1 = a.tile_base[1][blockIdx.x] + e1;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    a.cum[0][j] = r0;
    r0 += m0[q];
    if (j == a.n - 1) a.cum[0][a.n] = r0;
    if constexpr (C::kSecondPrefix) {
      a.cum[1][j] = r1;
      r1 += m1[q];
      if (j == a.n - 1) a.cum[1][a.n] = r1;
    }
  }
}

// Workspace pieces of the prefix chain, in this order: [keys n][idx n][sorted keys n][sorted idx n][sv n]
// [cum: n + 1 per kept prefix][tile_tot 0, tile_tot 1, tile_base 0, and tile_base 1 or the caller's own:
// ntiles each][tot 2 + nan count]
struct PrefixLayout {
  size_t keys, idx, skeys, sidx, sv, cum[2], tiles, misc;
  int ntiles;
};

static PrefixLayout prefix_layout(WsCursor& c, int n, bool second_prefix) {
  PrefixLayout l{};
  l.ntiles = (n + kAucTile - 1) / kAucTile;
  l.keys = c.take(4 * (size_t)n);
  l.idx = c.take(4 * (size_t)n);
  l.skeys = c.take(4 * (size_t)n);
  l.sidx = c.take(4 * (size_t)n);
  l.sv = c.take(4 * (size_t)n);
  l.cum[0] = c.take(8 * ((size_t)n + 1));
  if (second_prefix) l.cum[1] = c.take(8 * ((size_t)n + 1));
  l.tiles = c.take(8 * 4 * (size_t)l.ntiles);
  l.misc = c.take(32);
  return l;
}

// The score sort and the prefix chain of channel policy C over the pieces l of ws; a = the kernels' arguments.
// 0, or what launch_score_sort returned (nothing more is launched then).  descending: from the highest score down.
template <typename T, typename C>
static int launch_score_prefix(const float* scores, const float* labels, const float* weights, int n, char* ws,
                               const PrefixLayout& l, void* sort_ws, hipStream_t st, PrefixArgs<T>& a,
                               bool descending = false) {
  const size_t nt = (size_t)l.ntiles;
  T* tiles = reinterpret_cast<T*>(ws + l.tiles);
  T* misc = reinterpret_cast<T*>(ws + l.misc);
  ScoreSort s;
  const int se = launch_score_sort(scores, n, reinterpret_cast<uint32_t*>(ws + l.keys),
                                   reinterpret_cast<int*>(ws + l.idx), reinterpret_cast<uint32_t*>(ws + l.skeys),
                                   reinterpret_cast<int*>(ws + l.sidx), reinterpret_cast<unsigned*>(misc + 2), sort_ws,
                                   st, s, descending);
  if (se != 0) return se;
  constexpr bool k2 = C::kSecondPrefix;
  a = PrefixArgs<T>{n, l.ntiles, labels, weights, s.skeys, s.sidx, reinterpret_cast<uint32_t*>(ws + l.sv),
                    {reinterpret_cast<T*>(ws + l.cum[0]), k2 ? reinterpret_cast<T*>(ws + l.cum[1]) : nullptr},
                    {tiles, tiles + nt}, {tiles + 2 * nt, k2 ? tiles + 3 * nt : nullptr}, misc, s.nan_count,
                    s.sort_err};
  hipLaunchKernelGGL((prefix_tile_kernel<T, C>), dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL((prefix_base_kernel<T, C>), dim3(1), dim3(kAucBaseThreads), 0, st, a);
  hipLaunchKernelGGL((prefix_cum_kernel<T, C>), dim3(l.ntiles), dim3(kBlock), 0, st, a);
  return 0;
}

}  // namespace fm
