// Exact isotonic regression of (score, label, weight) triples: the best non-decreasing map from score to
// P(positive), for recalibrating a trained model on held-out data (ops/kernels.py isotonic_fit; the reference has
// no calibration).
//
// With the examples sorted by score (score_key.h's order: IEEE fp32 values, -0.0 == +0.0, NaN scores counted), cW[j]
// / cY[j] the weight / positive weight of the sorted positions < j, and position j a candidate iff j == 0, j == n or
// the keys at j - 1 and j differ (tied scores share one value), the fit is the slope of the lower convex hull of
// the candidate points (cW[j], cY[j]) with the minimal vertex set (iso_hull.h: collinear points are no vertices).
// Consecutive vertices H[b], H[b + 1] are block b: sorted positions [H[b], H[b + 1]), value Y_b / W_b in fp64.
// Two modes: unweighted in uint64 (exact), weighted (w > 0) in fp64 in a fixed order; both bitwise reproducible run
// to run.
//
// Launch chain (no kernel waits for another workgroup; kernel boundaries order the steps; no host read):
//   key, sort, tile, base, cum: metric_common.hip's score sort and prefix chain with the channels (all,
//            positives): cW = cum[0], cY = cum[1], each [0 .. n]; tot = [W, Y];
//   leaf:    one workgroup per tile of 2048 points of [0, n]: the tile's points staged in LDS, the serial stack per
//            thread over its 8 points, 8 bridge merges in LDS, the vertex positions to hullA[tile start ...] and
//            their count (a hull never has more vertices than points: every node's list fits in the node's own
//            range, no scan places it);
//   merge:   ceil(log2(tiles)) launches (a count fixed by n), one workgroup per pair of sibling nodes, ping-pong
//            between hullA and hullB: the bridge (a, b) by a nested binary search (iso_hull.h), then
//            L[0 .. a] ++ R[b ..) copied by the whole workgroup; a node without a sibling is copied;
//   extract: block arrays lo, hi (fp32 scores of the block's first / last position), W, Y, v = Y / W and the
//            record [blocks, total weight, positive weight, nan count, sort error word];
//   fitted:  (optional) v of its block for every example, in input order.
// (Included by module.hip after metric_common.hip.)
#include "../iso_hull.h"
#include "fm_common.h"

namespace fm {

template <typename T>
struct IsoArgs : PrefixArgs<T> {
  int npt, ntl;            // npt = n + 1 points, ntl = their tiles
  float* blo;              // block arrays, [n] each
  float* bhi;
  T* bW;
  T* bY;
  double* bv;
  double* fitted;          // [n] or null
  T* out;                  // [5] blocks, W, Y, nan count, sort error word
};

// Points of tile t: [t * kAucTile, min((t + 1) * kAucTile, npt)), staged in LDS.  Every thread builds the hull of
// its 8 consecutive points with the serial stack; 8 levels then merge sibling hulls by their bridges (one thread
// per pair searches, the whole workgroup copies), ping-pong between two LDS lists: the merge kernel's scheme with
// tile-local positions.  A node's list starts at its first point, its count stands at its number in the level.
template <typename T>
__global__ __launch_bounds__(kBlock) void iso_leaf_kernel(IsoArgs<T> a, int* hull, int* cnt) {
  __shared__ T w[kAucTile], y[kAucTile];
  __shared__ int list[2][kAucTile];
  __shared__ int count[2][kBlock];
  __shared__ int keep_l[kBlock / 2], keep_r[kBlock / 2], from_r[kBlock / 2];
  __shared__ uint8_t cand[kAucTile];
  const int base = blockIdx.x * kAucTile, tid = threadIdx.x;
  const int c = min(kAucTile, a.npt - base);
  for (int k = tid; k < c; k += kBlock) {
    const int j = base + k;
    w[k] = a.cum[0][j];
    y[k] = a.cum[1][j];
    cand[k] = j == 0 || j == a.n || a.skeys[j - 1] != a.skeys[j];
  }
  __syncthreads();
  {
    const int k0 = tid * kAucItems;
    const int top = iso::leaf_hull<T>(w + k0, y + k0, cand + k0, min(kAucItems, c - k0), list[0] + k0);
    for (int k = 0; k < top; ++k) list[0][k0 + k] += k0;
    count[0][tid] = top;
  }
  __syncthreads();
  const iso::Diagram<T> d{w, y, c - 1};
  int cur = 0;
  for (int span = kAucItems; span < kAucTile; span <<= 1, cur ^= 1) {  // span: points of a node of this level
    const int pairs = kAucTile / (2 * span);
    if (tid < pairs) {
      const int* L = list[cur] + 2 * tid * span;
      const int* R = L + span;
      const int nL = min(max(count[cur][2 * tid], 0), span), nR = min(max(count[cur][2 * tid + 1], 0), span);
      int a_ = nL - 1, b_ = 0;
      if (nL > 0 && nR > 0) {
        iso::bridge<T>(d, L, nL, R, nR, a_, b_);
        a_ = min(max(a_, 0), nL - 1);
        b_ = min(max(b_, 0), nR - 1);
      }
      keep_l[tid] = a_ + 1;
      from_r[tid] = b_;
      keep_r[tid] = nR - b_;
      count[cur ^ 1][tid] = a_ + 1 + nR - b_;
    }
    __syncthreads();
    for (int k = tid; k < kAucTile; k += kBlock) {
      const int p = k / (2 * span), i = k - p * 2 * span;  // slot i of pair p's merged list (<= 2 span entries)
      if (i < keep_l[p]) list[cur ^ 1][k] = list[cur][k];
      else if (i < keep_l[p] + keep_r[p])
        list[cur ^ 1][k] = list[cur][p * 2 * span + span + from_r[p] + i - keep_l[p]];
    }
    __syncthreads();
  }
  const int top = min(max(count[cur][0], 0), c);
  for (int k = tid; k < top; k += kBlock) hull[base + k] = base + list[cur][k];
  if (tid == 0) cnt[blockIdx.x] = top;
}

// Level l: workgroup k merges the nodes whose first tiles are (2k) << l and (2k + 1) << l into the node at
// (2k) << l of the other buffer.  A node's list starts at its first point and its count stands at its first tile.
template <typename T>
__global__ __launch_bounds__(kBlock) void iso_merge_kernel(IsoArgs<T> a, int level, const int* src, const int* scnt,
                                                           int* dst, int* dcnt) {
  const long long tl = (2ll * blockIdx.x) << level, tr = (2ll * blockIdx.x + 1) << level;
  if (tl >= a.ntl) return;
  const long long span = (long long)kAucTile << level;
  const int pl = (int)(tl * kAucTile);  // (< npt <= 2^30)
  const int capL = (int)min(span, (long long)a.npt - pl);
  const int nL = min(max(scnt[tl], 0), capL);
  const int* L = src + pl;
  int* D = dst + pl;
  int nR = 0, a_ = nL - 1, b_ = 0;
  const int* R = L;
  if (tr < a.ntl) {
    const int pr = (int)(tr * kAucTile);
    nR = min(max(scnt[tr], 0), (int)min(span, (long long)a.npt - pr));
    R = src + pr;
    if (nL > 0 && nR > 0) {  // (every thread the same search: the loads broadcast)
      const iso::Diagram<T> d{a.cum[0], a.cum[1], a.n};
      iso::bridge<T>(d, L, nL, R, nR, a_, b_);
      a_ = min(max(a_, 0), nL - 1);
      b_ = min(max(b_, 0), nR - 1);
    }
  }
  const int keepL = a_ + 1, keepR = nR - b_;  // keepL + keepR <= nL + nR <= the two nodes' points
  for (int i = threadIdx.x; i < keepL; i += kBlock) D[i] = L[i];
  for (int i = threadIdx.x; i < keepR; i += kBlock) D[keepL + i] = R[b_ + i];
  if (threadIdx.x == 0) dcnt[tl] = keepL + keepR;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void iso_extract_kernel(IsoArgs<T> a, const int* H, const int* hcnt) {
  const int c = min(max(hcnt[0], 0), a.npt);
  const int m = c > 1 ? c - 1 : 0;
  for (int b = blockIdx.x * kBlock + threadIdx.x; b < m; b += gridDim.x * kBlock) {
    const int p = min(max(H[b], 0), a.n - 1), q = min(max(H[b + 1], 1), a.n);
    a.blo[b] = __uint_as_float(score_key_bits(a.skeys[p]));
    a.bhi[b] = __uint_as_float(score_key_bits(a.skeys[q - 1]));
    const T W = a.cum[0][q] - a.cum[0][p], Y = a.cum[1][q] - a.cum[1][p];
    a.bW[b] = W;
    a.bY[b] = Y;
    a.bv[b] = (double)Y / (double)W;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int err = *a.sort_err;
    a.out[0] = (T)m;
    a.out[1] = a.tot[0];
    a.out[2] = a.tot[1];
    a.out[3] = (T)*a.nan_count;
    a.out[4] = (T)err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void iso_fitted_kernel(IsoArgs<T> a, const int* H, const int* hcnt) {
  const int c = min(max(hcnt[0], 0), a.npt);
  if (c < 2) return;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < a.n; j += gridDim.x * kBlock) {
    const int b = min(iso::block_of(H, c, j), c - 2);
    const int ex = a.sidx[j];
    if ((unsigned)ex < (unsigned)a.n) a.fitted[ex] = a.bv[b];
  }
}

// Workspace: the prefix chain's pieces (two prefixes: cW, cY), then [hullA, hullB: ntl * 2048 each][cntA, cntB:
// ntl each][block W, Y, v: n each][sort workspace].  The chain's keys / idx pieces are dead after the sort: the
// block scores lo / hi reuse them.
struct IsoLayout {
  PrefixLayout p;
  size_t hull_a, hull_b, cnt_a, cnt_b, bw, by, bv, sort, total;
  int ntl;
};

static IsoLayout iso_layout(int n) {
  WsCursor c;
  IsoLayout l{};
  l.ntl = n / kAucTile + 1;  // ceil((n + 1) / tile)
  l.p = prefix_layout(c, n, IsoChannels::kSecondPrefix);
  l.hull_a = c.take(4 * (size_t)l.ntl * kAucTile);
  l.hull_b = c.take(4 * (size_t)l.ntl * kAucTile);
  l.cnt_a = c.take(4 * (size_t)l.ntl);
  l.cnt_b = c.take(4 * (size_t)l.ntl);
  l.bw = c.take(8 * (size_t)n);
  l.by = c.take(8 * (size_t)n);
  l.bv = c.take(8 * (size_t)n);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

// Bytes of launch_isotonic's workspace for n scores; 0: n is out of range (n >= 2^30, the sort's bound).
size_t isotonic_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  if (n == 0) return 256;
  return iso_layout((int)n).total;
}

// Byte offsets of the block arrays lo, hi (fp32), W, Y (uint64 / fp64), v (fp64) in the workspace, n >= 1.
void isotonic_block_offsets(int n, size_t off[5]) {
  const IsoLayout l = iso_layout(n);
  off[0] = l.p.keys, off[1] = l.p.idx, off[2] = l.bw, off[3] = l.by, off[4] = l.bv;
}

template <typename T>
static int launch_isotonic_t(const float* scores, const float* labels, const float* weights, int n, double* fitted,
                             void* out, char* ws, const IsoLayout& l, hipStream_t st) {
  IsoArgs<T> a{};
  const int se = launch_score_prefix<T, IsoChannels>(scores, labels, weights, n, ws, l.p, ws + l.sort, st, a);
  if (se != 0) return se;
  a.npt = n + 1, a.ntl = l.ntl;
  a.blo = reinterpret_cast<float*>(ws + l.p.keys), a.bhi = reinterpret_cast<float*>(ws + l.p.idx);
  a.bW = reinterpret_cast<T*>(ws + l.bw), a.bY = reinterpret_cast<T*>(ws + l.by);
  a.bv = reinterpret_cast<double*>(ws + l.bv);
  a.fitted = fitted, a.out = static_cast<T*>(out);
  int* hull[2] = {reinterpret_cast<int*>(ws + l.hull_a), reinterpret_cast<int*>(ws + l.hull_b)};
  int* cnt[2] = {reinterpret_cast<int*>(ws + l.cnt_a), reinterpret_cast<int*>(ws + l.cnt_b)};
  hipLaunchKernelGGL(iso_leaf_kernel<T>, dim3(l.ntl), dim3(kBlock), 0, st, a, hull[0], cnt[0]);
  int cur = 0;
  for (int level = 0; (1ll << level) < l.ntl; ++level, cur ^= 1) {
    const int nodes = (int)((l.ntl + (1ll << level) - 1) >> level);  // nodes of this level
    hipLaunchKernelGGL(iso_merge_kernel<T>, dim3((nodes + 1) / 2), dim3(kBlock), 0, st, a, level, hull[cur], cnt[cur],
                       hull[cur ^ 1], cnt[cur ^ 1]);
  }
  hipLaunchKernelGGL(iso_extract_kernel<T>, dim3(fill_grid(n, kBlock, 2048)), dim3(kBlock), 0, st, a, hull[cur],
                     cnt[cur]);
  if (fitted)
    hipLaunchKernelGGL(iso_fitted_kernel<T>, dim3(fill_grid(n, kBlock, 2048)), dim3(kBlock), 0, st, a, hull[cur],
                       cnt[cur]);
  return (int)hipGetLastError();
}

// Isotonic fit of n >= 1 scores (weights null or all > 0): the record into out[5] (uint64 when weights is null,
// else fp64), the block arrays into the workspace (isotonic_block_offsets), fitted[n] (fp64, input order) when it
// is not null; asynchronously on st.  0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >=
// 2^30.
int launch_isotonic(const float* scores, const float* labels, const float* weights, int n, double* fitted, void* out,
                    void* ws, size_t ws_bytes, hipStream_t st) {
  if (const int rc = metric_check_args(n, scores, labels, out, ws)) return rc;
  const IsoLayout l = iso_layout(n);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  if (weights) return launch_isotonic_t<double>(scores, labels, weights, n, fitted, out, b, l, st);
  return launch_isotonic_t<uint64_t>(scores, labels, weights, n, fitted, out, b, l, st);
}

__global__ __launch_bounds__(kBlock) void calib_apply_kernel(int n, const float* scores, const float* x,
                                                             const float* y, int m2, float* out) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock)
    out[i] = iso::calib_value(scores[i], x, y, m2, [](float t, float d, float v) { return fmaf(t, d, v); });
}

// out[i] = the calibrated probability of scores[i] from the thresholds x[m2] and values y[m2] (m2 even, >= 2).
int launch_calib_apply(const float* scores, int n, const float* x, const float* y, int m2, float* out,
                       hipStream_t st) {
  if (n < 0 || m2 < 2 || (m2 & 1) || !x || !y || (n > 0 && (!scores || !out))) return -1;
  if (n == 0) return 0;
  hipLaunchKernelGGL(calib_apply_kernel, dim3(fill_grid(n, kBlock, 4096)), dim3(kBlock), 0, st, n, scores, x, y, m2,
                     out);
  return (int)hipGetLastError();
}

}  // namespace fm
