// Exact weighted ROC AUC of (score, label, weight) triples (the trainer's validation AUC; the reference
// reports the validation loss only, run_tffm.py:64-75).
//
//   P = sum_{pos} w_i,  N = sum_{neg} w_j           (positive iff label > 0)
//   U2 = sum_{i pos} w_i (Nlt(s_i) + Nle(s_i)),     Nlt / Nle: weight of the negatives below / not above s_i
//   AUC = U2 / (2 P N)                              (a positive-negative tie counts one half)
//
// Scores are ordered as IEEE fp32 values by the usual order-preserving key (negatives: all bits
// flipped; the others: sign bit set); -0.0 is folded onto +0.0 by its bit pattern (arithmetic may flush
// denormals, which keep their order here), +-inf are ordinary values, NaN scores are counted (the host
// reports NaN when there is one).  Two modes, both bitwise reproducible run to run (no float atomics, every
// sum in a fixed order): unweighted (weights == null) in uint64 -- exact --, weighted in fp64.
//
// Launch chain (no kernel waits for another workgroup; kernel boundaries order the steps):
//   key:   key + example index per score, NaN count (integer atomic, one per wave);
//   sort:  launch_radix_sort over all 32 key bits (radix_sort.hip: 4 passes of 8 bits);
//   tile:  per 2048-element tile of the sorted order the signed weight of every position (+w positive,
//          -w negative: the only gather through the sorted index) and the tile's negative / positive totals;
//   base:  one block scans the tile totals in tile order -> every tile's exclusive negative prefix, P and N;
//   nex:   Nex[j] = weight of the negatives at sorted positions < j, j in [0, n];
//   rank:  a positive at sorted position j adds w (Nex[lb] + Nex[ub]), [lb, ub) = its run of equal keys:
//          (j, j + 1) when both neighbours differ, else a binary search in the sorted keys (a tie run may
//          span any number of tiles); per-tile partial sums;
//   final: one block sums the partials in tile order and writes the record [U2, P, N, nan count, sort
//          error word] (uint64 or fp64); a nonzero sort error also sets the sticky device error word.
// (Included by module.hip after dedup.hip: load8 and the radix sort come from there.)
#include "fm_common.h"

namespace fm {

constexpr int kAucItems = 8;                    // consecutive sorted positions per thread
constexpr int kAucTile = kBlock * kAucItems;    // 2048
constexpr int kAucBaseThreads = 1024;           // the single block of the tile-total scan

__device__ inline uint32_t auc_key(uint32_t bits) {
  if (bits == 0x80000000u) bits = 0u;  // -0.0 == +0.0
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__global__ __launch_bounds__(kBlock) void auc_key_kernel(int n, const uint32_t* score_bits, uint32_t* keys, int* idx,
                                                         unsigned* nan_count) {
  unsigned nn = 0;
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const uint32_t b = score_bits[e];
    nn += (b & 0x7fffffffu) > 0x7f800000u;
    keys[e] = auc_key(b);
    idx[e] = e;
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) nn += __shfl_down(nn, o, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && nn) atomicAdd(nan_count, nn);
}

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

template <typename T>
struct AucArgs {
  int n, ntiles;
  const float* labels;
  const float* weights;    // null: all ones
  const uint32_t* skeys;   // [n] sorted keys
  const int* sidx;         // [n] example index of every sorted position
  uint32_t* sv;            // [n] float bits: +w (positive) / -w (negative) of every sorted position
  T* nex;                  // [n + 1]
  T* tile_neg;             // [ntiles]
  T* tile_pos;             // [ntiles]
  T* tile_base;            // [ntiles] negatives before the tile
  T* part;                 // [ntiles] U2 partial sums
  T* tot;                  // [2] P, N
  const unsigned* nan_count;
  const int* sort_err;
  T* out;                  // [5] U2, P, N, nan count, sort error word
};

template <typename T>
__global__ __launch_bounds__(kBlock) void auc_tile_kernel(AucArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  int ex[kAucItems];
  load8(a.sidx, j0, a.n, ex, -1);
  T neg = 0, pos = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    if (j0 + q >= a.n) continue;
    float s = 0.f;
    if ((unsigned)ex[q] < (unsigned)a.n) {  // (always, unless the sort failed: its error word is reported)
      const float w = a.weights ? a.weights[ex[q]] : 1.f;
      s = a.labels[ex[q]] > 0.f ? w : -w;
    }
    a.sv[j0 + q] = __float_as_uint(s);
    if (s > 0.f) pos += (T)s;
    else neg += (T)(-s);
  }
  T e, t;
  auc_block_scan<T, kWavesPerBlock>(neg, e, t, sh);
  if (threadIdx.x == 0) a.tile_neg[blockIdx.x] = t;
  auc_block_scan<T, kWavesPerBlock>(pos, e, t, sh);
  if (threadIdx.x == 0) a.tile_pos[blockIdx.x] = t;
}

template <typename T>
__global__ __launch_bounds__(kAucBaseThreads) void auc_base_kernel(AucArgs<T> a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ T sh[NW];
  T carry = 0, psum = 0;
  for (int c = 0; c < a.ntiles; c += kAucBaseThreads) {
    const int t = c + threadIdx.x;
    const bool ok = t < a.ntiles;
    T e, tn, tp;
    auc_block_scan<T, NW>(ok ? a.tile_neg[t] : (T)0, e, tn, sh);
    if (ok) a.tile_base[t] = carry + e;
    carry += tn;
    auc_block_scan<T, NW>(ok ? a.tile_pos[t] : (T)0, e, tp, sh);
    psum += tp;
  }
  if (threadIdx.x == 0) {
    a.tot[0] = psum;
    a.tot[1] = carry;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void auc_nex_kernel(AucArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  uint32_t sv[kAucItems];
  load8(a.sv, j0, a.n, sv, 0u);
  T m[kAucItems], neg = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const float s = __uint_as_float(sv[q]);
    m[q] = (j0 + q < a.n && !(s > 0.f)) ? (T)(-s) : (T)0;
    neg += m[q];
  }
  T e, t;
  auc_block_scan<T, kWavesPerBlock>(neg, e, t, sh);
  T run = a.tile_base[blockIdx.x] + e;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    a.nex[j] = run;
    run += m[q];
    if (j == a.n - 1) a.nex[a.n] = run;
  }
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

template <typename T>
__global__ __launch_bounds__(kBlock) void auc_rank_kernel(AucArgs<T> a) {
  __shared__ T sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
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
    u += (T)s * (a.nex[lb] + a.nex[ub]);
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
    a.out[1] = a.tot[0];
    a.out[2] = a.tot[1];
    a.out[3] = (T)*a.nan_count;
    a.out[4] = (T)err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
}

// Workspace: [keys n][idx n][sorted keys n][sorted idx n][sv n][nex n + 1][tile_neg, tile_pos, tile_base,
// part: ntiles each][tot 2 + nan count][sort workspace]
struct AucLayout {
  size_t keys, idx, skeys, sidx, sv, nex, tiles, misc, sort, total;
  int ntiles;
};

static AucLayout auc_layout(int n) {
  AucLayout l{};
  l.ntiles = (n + kAucTile - 1) / kAucTile;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off += rs_align(bytes);
    return o;
  };
  l.keys = take(4 * (size_t)n);
  l.idx = take(4 * (size_t)n);
  l.skeys = take(4 * (size_t)n);
  l.sidx = take(4 * (size_t)n);
  l.sv = take(4 * (size_t)n);
  l.nex = take(8 * ((size_t)n + 1));
  l.tiles = take(8 * 4 * (size_t)l.ntiles);
  l.misc = take(32);
  l.sort = take(radix_sort_ws_bytes(n));
  l.total = off;
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
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + l.keys);
  int* idx = reinterpret_cast<int*>(ws + l.idx);
  uint32_t* skeys = reinterpret_cast<uint32_t*>(ws + l.skeys);
  int* sidx = reinterpret_cast<int*>(ws + l.sidx);
  T* tiles = reinterpret_cast<T*>(ws + l.tiles);
  T* misc = reinterpret_cast<T*>(ws + l.misc);
  unsigned* nan_count = reinterpret_cast<unsigned*>(misc + 2);
  void* sort_ws = ws + l.sort;
  hipError_t e = hipMemsetAsync(nan_count, 0, sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(auc_key_kernel, dim3(fill_grid(n, kBlock, 2048)), dim3(kBlock), 0, st, n,
                     reinterpret_cast<const uint32_t*>(scores), keys, idx, nan_count);
  const int se = launch_radix_sort(keys, idx, skeys, sidx, n, 32, sort_ws, radix_sort_ws_bytes(n), st);
  if (se != 0) return se;
  AucArgs<T> a{n, l.ntiles, labels, weights, skeys, sidx, reinterpret_cast<uint32_t*>(ws + l.sv),
               reinterpret_cast<T*>(ws + l.nex), tiles, tiles + l.ntiles, tiles + 2 * (size_t)l.ntiles,
               tiles + 3 * (size_t)l.ntiles, misc, nan_count, radix_sort_error(sort_ws, n), static_cast<T*>(out)};
  hipLaunchKernelGGL(auc_tile_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(auc_base_kernel<T>, dim3(1), dim3(kAucBaseThreads), 0, st, a);
  hipLaunchKernelGGL(auc_nex_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(auc_rank_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(auc_final_kernel<T>, dim3(1), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

// AUC statistics of n >= 1 scores into out[5] (uint64 when weights is null, else fp64), asynchronously on st.
// 0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30.
int launch_auc(const float* scores, const float* labels, const float* weights, int n, void* out, void* ws,
               size_t ws_bytes, hipStream_t st) {
  if (n < 1 || !scores || !labels || !out || !ws) return -1;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(out) & 7)) return -1;  // (16-byte loads)
  if ((unsigned)n > kOsCnt) return -5;
  const AucLayout l = auc_layout(n);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  if (weights) return launch_auc_t<double>(scores, labels, weights, n, out, b, l, st);
  return launch_auc_t<uint64_t>(scores, labels, weights, n, out, b, l, st);
}

}  // namespace fm
