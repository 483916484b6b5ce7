// Listwise ranking loss: the softmax cross-entropy of every group (a user, a query, a session) of one batch.
//
//   s_i score, a_i = w_i max(y_i, 0) gain (rank_metrics.hip's, times the example weight); per group g over its
//   examples in the batch:   m = max s_i,  Z = sum exp(s_i - m),  A = sum a_i,  T = sum a_i s_i
//   L_g = A (m + log Z) - T  (= -sum a_i log softmax_g(s)_i),   dL/ds_i = A exp(s_i - m) / Z - a_i
//   a group with A == 0 adds exactly 0 to the loss and to every gradient; so does an excluded example (id < 0, or
//   >= the all-ones key of the sort's key_bits) -- whatever its score.  A group of one gives 0 by the arithmetic.
//
// Two halves, each a launch chain on the caller's stream into the caller's workspace (no host read, no float
// atomic: capturable):
//   plan (the batch alone -- it runs where the batch's dedup runs, beside the step before):
//     key:    sort key (the id; the all-ones key for an excluded example) + example index;
//     sort:   launch_radix_sort over key_bits (stable: a group's examples stay in batch order);
//     range:  every sorted position's group range [first, end) -- a thread's eight positions from their
//             neighbours, a range that leaves the thread by one binary search each way; end == 0 marks an excluded
//             position.  The sort's error word is saved, and set in the sticky device error word when nonzero.
//   softmax (the plan, scores, labels, weights, grad_scale):
//     max:    per tile of 1024 sorted positions: the (score, gain) of every position (the only gathers through
//             the sorted index) and a segmented max scan -- a group that begins in the tile and ends there gets m
//             at once, the one open at the tile's start leaves its partial;
//     carry:  one block carries those partials over the tiles in tile order (one group over any number of tiles);
//     sum, carry: the same for Z (terms exp(s - m), kept per position), A and T;
//     grad:   p = z / Z, dpred[example] = fp32(grad_scale (A p - a)); the head of every group adds L_g to its
//             tile's loss partial (thread order, then the block scan);
//     final:  one block sums the tile partials in tile order -> fp32 loss.
// Everything is fp64 (exp and log too), every reduction has a fixed shape, dpred and the loss are rounded once:
// bitwise the same run to run.  Thousands of one- and two-example groups sit several to a wave; one group may own
// the whole batch.  (Included by module.hip after gauc.hip: auc_block_scan, auc_bound, load8, WsCursor and the
// radix sort are defined before it.)
#include "fm_common.h"

namespace fm {

constexpr int kGlItems = 4;                   // consecutive sorted positions per thread
constexpr int kGlTile = kBlock * kGlItems;    // 1024
constexpr int kGlChannels = 3;                // Z, A, T

struct GlMax {
  static __device__ double id() { return -__builtin_huge_val(); }
  static __device__ double op(double a, double b) { return fmax(a, b); }
};
struct GlAdd {
  static __device__ double id() { return 0.0; }
  static __device__ double op(double a, double b) { return a + b; }
};

// gauc_seg_scan with the operation O in place of the sum (the earlier operand first): (ef, ev) the open segment's
// reduction over the threads before this one and whether one of them had a flag, (tf, tv) the same over the block.
template <typename O, int NW>
__device__ inline void gl_seg_scan(bool f, double v, bool& ef, double& ev, bool& tf, double& tv, int* shf /*[NW]*/,
                                   double* shv /*[NW]*/) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  int fi = f ? 1 : 0;
  double inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const double up = __shfl_up(inc, o, kWave);
    const int uf = __shfl_up(fi, o, kWave);
    if (lane >= o) {
      if (!fi) inc = O::op(up, inc);
      fi |= uf;
    }
  }
  double bv = __shfl_up(inc, 1, kWave);
  int bf = __shfl_up(fi, 1, kWave);
  if (lane == 0) {
    bv = O::id();
    bf = 0;
  }
  if (lane == kWave - 1) {
    shf[wv] = fi;
    shv[wv] = inc;
  }
  __syncthreads();
  int pf = 0, cf = 0;
  double pv = O::id(), cv = O::id();
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w == wv) {
      pf = cf;
      pv = cv;
    }
    cv = shf[w] ? shv[w] : O::op(cv, shv[w]);
    cf |= shf[w];
  }
  ef = (pf | bf) != 0;
  ev = bf ? bv : O::op(pv, bv);
  tf = cf != 0;
  tv = cv;
  __syncthreads();
}

// ---- group key of a training example ------------------------------------------------------------------------
// keys[i] = the table row of example i's pos-th feature; -1 (excluded) when it has fewer, or the row is no row.
__global__ __launch_bounds__(kBlock) void gl_feature_key_kernel(int B, const int* offsets, const int* rows, int pos,
                                                                int num_rows, int* keys) {
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < B; i += gridDim.x * kBlock) {
    const int o0 = offsets[i], o1 = offsets[i + 1];
    int k = -1;
    if (o0 >= 0 && o1 - o0 > pos) {
      const int r = rows[o0 + pos];
      if ((unsigned)r < (unsigned)num_rows) k = r;
    }
    keys[i] = k;
  }
}

int launch_group_keys(int B, const int* offsets, const int* rows, int pos, int num_rows, int* keys, hipStream_t st) {
  if (B < 0 || pos < 0 || num_rows < 1 || !keys) return -1;
  if (B == 0) return 0;
  if (!offsets || !rows) return -1;
  hipLaunchKernelGGL(gl_feature_key_kernel, dim3(fill_grid(B, kBlock, 2048)), dim3(kBlock), 0, st, B, offsets, rows,
                     pos, num_rows, keys);
  return (int)hipGetLastError();
}

// ---- workspace --------------------------------------------------------------------------------------------
// One workspace serves both halves: [sorted idx n][first n][end n][error word] stay from the plan to the softmax;
// [keys n][idx n][sorted keys n][sort workspace] are the plan's own; the rest is the softmax's.
struct GlLayout {
  size_t sidx, first, end, misc, keys, idx, skeys, sort;        // plan
  size_t ss, sa, sz, gm, gred, tflag, tv, fv, lpart, total;     // softmax
  int ntiles;
};

static GlLayout gl_layout(int n) {
  WsCursor c;
  GlLayout l{};
  const size_t N = (size_t)n;
  l.ntiles = (n + kGlTile - 1) / kGlTile;
  const size_t nt = (size_t)l.ntiles;
  l.sidx = c.take(4 * N);
  l.first = c.take(4 * N);
  l.end = c.take(4 * N);
  l.misc = c.take(32);
  l.keys = c.take(4 * N);
  l.idx = c.take(4 * N);
  l.skeys = c.take(4 * N);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.ss = c.take(4 * N);
  l.sa = c.take(8 * N);
  l.sz = c.take(8 * N);
  l.gm = c.take(8 * N);
  l.gred = c.take(8 * kGlChannels * N);
  l.tflag = c.take(4 * nt);
  l.tv = c.take(8 * kGlChannels * nt);
  l.fv = c.take(8 * kGlChannels * nt);
  l.lpart = c.take(8 * nt);
  l.total = c.off;
  return l;
}

// Bytes of the workspace for up to n examples; 0: n outside [0, 2^30).
size_t group_loss_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  return gl_layout((int)(n > 0 ? n : 1)).total;
}

// Byte offsets of the plan's results in a workspace for n examples: sorted idx, first, end, error word.
void group_plan_offsets(int n, size_t (&off)[4]) {
  const GlLayout l = gl_layout(n > 0 ? n : 1);
  off[0] = l.sidx;
  off[1] = l.first;
  off[2] = l.end;
  off[3] = l.misc;
}

// ---- plan ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gl_key_kernel(int n, const int* ids, uint32_t excl, uint32_t* keys, int* idx) {
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const int g = ids[e];
    keys[e] = (g < 0 || (uint32_t)g >= excl) ? excl : (uint32_t)g;
    idx[e] = e;
  }
}

// One thread per eight sorted positions: their group ranges.  first is in [0, j], end in [j + 1, n] (0: excluded)
// whatever the keys hold (a failed sort: its error word is reported).
__global__ __launch_bounds__(kBlock) void gl_range_kernel(int n, const uint32_t* skeys, uint32_t excl, int* first,
                                                          int* end, const int* sort_err, int* err_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int err = *sort_err;
    *err_out = err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
  const int j0 = (blockIdx.x * kBlock + threadIdx.x) * 8;
  if (j0 >= n) return;
  uint32_t k[8];
  load8(skeys, j0, n, k, 0u);
  const int cnt = min(8, n - j0);
  int fi[8], en[8];
  fi[0] = j0;
  if (j0 > 0 && skeys[j0 - 1] == k[0]) fi[0] = auc_bound<false>(skeys, 0, j0, k[0]);
#pragma unroll
  for (int q = 1; q < 8; ++q) fi[q] = (q < cnt && k[q] == k[q - 1]) ? fi[q - 1] : j0 + q;
  const int jl = j0 + cnt - 1;
  int e = jl + 1;
  if (jl + 1 < n && skeys[jl + 1] == k[cnt - 1]) e = auc_bound<true>(skeys, jl + 1, n, k[cnt - 1]);
#pragma unroll
  for (int q = 7; q >= 0; --q) {
    if (q >= cnt) continue;
    if (q < cnt - 1 && k[q] != k[q < 7 ? q + 1 : 7]) e = j0 + q + 1;
    en[q] = e;
  }
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    if (q >= cnt) continue;
    const bool ex = k[q] >= excl;
    first[j0 + q] = ex ? j0 + q : fi[q];
    end[j0 + q] = ex ? 0 : en[q];
  }
}

// Plan of n >= 1 group ids (int32; < 0 or >= 2^key_bits - 1: excluded) into ws, asynchronously on st.  0 or a hip
// error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30; -8: key_bits outside [1, 31].
int launch_group_plan(const int* ids, int n, int key_bits, void* ws, size_t ws_bytes, hipStream_t st) {
  if (n < 1 || !ids || !ws || (reinterpret_cast<uintptr_t>(ws) & 15)) return -1;
  if ((unsigned)n > kOsCnt) return -5;
  if (key_bits < 1 || key_bits > 31) return -8;
  const GlLayout l = gl_layout(n);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  uint32_t* keys = reinterpret_cast<uint32_t*>(b + l.keys);
  int* idx = reinterpret_cast<int*>(b + l.idx);
  uint32_t* skeys = reinterpret_cast<uint32_t*>(b + l.skeys);
  int* sidx = reinterpret_cast<int*>(b + l.sidx);
  void* sort_ws = b + l.sort;
  const uint32_t excl = (1u << key_bits) - 1u;
  hipLaunchKernelGGL(gl_key_kernel, dim3(fill_grid(n, kBlock, 2048)), dim3(kBlock), 0, st, n, ids, excl, keys, idx);
  const int se = launch_radix_sort(keys, idx, skeys, sidx, n, key_bits, sort_ws, radix_sort_ws_bytes(n), st);
  if (se != 0) return se;
  const int rblocks = (n + 8 * kBlock - 1) / (8 * kBlock);
  hipLaunchKernelGGL(gl_range_kernel, dim3(rblocks), dim3(kBlock), 0, st, n, skeys, excl,
                     reinterpret_cast<int*>(b + l.first), reinterpret_cast<int*>(b + l.end),
                     radix_sort_error(sort_ws, n), reinterpret_cast<int*>(b + l.misc));
  return (int)hipGetLastError();
}

// ---- softmax ------------------------------------------------------------------------------------------------
struct GlArgs {
  int n, ntiles;
  double grad_scale;
  const float* scores;
  const float* labels;
  const float* weights;   // null: all ones
  const int* sidx;        // [n] example index of every sorted position
  const int* first;       // [n] the position's group range (end == 0: excluded)
  const int* end;
  float* ss;              // [n] score of every sorted position
  double* sa;             // [n] gain
  double* sz;             // [n] exp(s - m)
  double* gm;             // [n] at a group's first position: m
  double* gred;           // [3, n] at a group's first position: Z, A, T
  int* tflag;             // [ntiles] the tile holds a group head
  double* tv;             // [3, ntiles] reduction from the tile's last head (or its start) to its end
  double* fv;             // [3, ntiles] the same from the tile's start to the tail of the group open there
  double* lpart;          // [ntiles] loss of the groups that begin in the tile
  float* dpred;           // [n] example order
  float* loss;            // [1]
};

// the ranges of a thread's positions: head / tail / excluded flags
struct GlPos {
  int fi[kGlItems];
  bool in[kGlItems], head[kGlItems], tail[kGlItems], excl[kGlItems];
  bool any_head;
};

__device__ inline void gl_positions(const GlArgs& a, int j0, GlPos& p) {
  p.any_head = false;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    p.in[q] = j < a.n;
    const int f = p.in[q] ? a.first[j] : 0, e = p.in[q] ? a.end[j] : 0;
    p.fi[q] = min(max(f, 0), j);  // (a plan always has first in [0, j]: the clamp keeps any workspace's writes inside)
    p.excl[q] = p.in[q] && e == 0;
    p.head[q] = p.in[q] && (e == 0 || f == j);
    p.tail[q] = p.in[q] && (e == 0 || e == j + 1);
    p.any_head = p.any_head || p.head[q];
  }
}

// The segmented reduction O of the tile's values v (the identity at excluded positions): a group that begins and
// ends in the tile gets its result at g[first]; the group open at the tile's start leaves fv[tile] at its tail; the
// tile leaves tv[tile].  tflag: written when non-null.
template <typename O>
__device__ inline void gl_tile_reduce(const GlPos& p, const double (&v)[kGlItems], double* g, double* tv, double* fv,
                                      int* tflag, int* shf, double* shv) {
  double acc = O::id();
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    if (!p.in[q]) continue;
    if (p.head[q]) acc = O::id();
    acc = O::op(acc, v[q]);
  }
  bool ef, tf;
  double ev, tot;
  gl_seg_scan<O, kWavesPerBlock>(p.any_head, acc, ef, ev, tf, tot, shf, shv);
  if (threadIdx.x == 0) {
    tv[blockIdx.x] = tot;
    if (tflag) tflag[blockIdx.x] = tf;
  }
  double run = ev;
  bool seen = ef;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    if (!p.in[q]) continue;
    if (p.head[q]) {
      run = O::id();
      seen = true;
    }
    run = O::op(run, v[q]);
    if (p.tail[q] && !p.excl[q]) {
      if (seen) g[p.fi[q]] = run;
      else fv[blockIdx.x] = run;
    }
  }
}

// One block: the tiles' partials in tile order; completes every group that ends in a later tile than it began.
template <typename O>
__device__ inline void gl_carry(const GlArgs& a, double* g, const double* tv, const double* fv) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ int shf[NW];
  __shared__ double shv[NW];
  double carry = O::id();
  for (int b = 0; b < a.ntiles; b += kAucBaseThreads) {
    const int t = b + threadIdx.x;
    const bool ok = t < a.ntiles;
    bool ef, tf;
    double ev, tot;
    gl_seg_scan<O, NW>(ok && a.tflag[t] != 0, ok ? tv[t] : O::id(), ef, ev, tf, tot, shf, shv);
    if (ok && t > 0) {
      const int j0 = t * kGlTile;
      const int f = a.first[j0], e = a.end[j0];
      if (e != 0 && f >= 0 && f < j0 && e <= min(a.n, j0 + kGlTile)) g[f] = O::op(ef ? ev : O::op(carry, ev), fv[t]);
    }
    carry = tf ? tot : O::op(carry, tot);
  }
}

__global__ __launch_bounds__(kBlock) void gl_max_kernel(GlArgs a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ double shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  GlPos p;
  gl_positions(a, j0, p);
  double s[kGlItems];
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    s[q] = GlMax::id();
    if (!p.in[q]) continue;
    const int j = j0 + q;
    const int ex = a.sidx[j];
    float sc = 0.f;
    double gain = 0.0;
    if (!p.excl[q] && (unsigned)ex < (unsigned)a.n) {  // (not after a failed sort: its error word is reported)
      sc = a.scores[ex];
      const float y = a.labels[ex];
      gain = (a.weights ? (double)a.weights[ex] : 1.0) * (y > 0.f ? (double)y : 0.0);
      s[q] = (double)sc;
    }
    a.ss[j] = sc;
    a.sa[j] = gain;
  }
  gl_tile_reduce<GlMax>(p, s, a.gm, a.tv, a.fv, a.tflag, shf, shv);
}

__global__ __launch_bounds__(kAucBaseThreads) void gl_max_carry_kernel(GlArgs a) { gl_carry<GlMax>(a, a.gm, a.tv, a.fv); }

__global__ __launch_bounds__(kBlock) void gl_sum_kernel(GlArgs a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ double shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  GlPos p;
  gl_positions(a, j0, p);
  double z[kGlItems], g[kGlItems], t[kGlItems];
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    z[q] = g[q] = t[q] = 0.0;
    if (!p.in[q] || p.excl[q]) continue;
    const int j = j0 + q;
    const double s = (double)a.ss[j];
    z[q] = exp(s - a.gm[p.fi[q]]);
    g[q] = a.sa[j];
    t[q] = g[q] * s;
    a.sz[j] = z[q];
  }
  const size_t N = (size_t)a.n, nt = (size_t)a.ntiles;
  gl_tile_reduce<GlAdd>(p, z, a.gred, a.tv, a.fv, nullptr, shf, shv);
  gl_tile_reduce<GlAdd>(p, g, a.gred + N, a.tv + nt, a.fv + nt, nullptr, shf, shv);
  gl_tile_reduce<GlAdd>(p, t, a.gred + 2 * N, a.tv + 2 * nt, a.fv + 2 * nt, nullptr, shf, shv);
}

// block c: channel c (Z, A, T)
__global__ __launch_bounds__(kAucBaseThreads) void gl_sum_carry_kernel(GlArgs a) {
  const size_t c = blockIdx.x;
  gl_carry<GlAdd>(a, a.gred + c * (size_t)a.n, a.tv + c * (size_t)a.ntiles, a.fv + c * (size_t)a.ntiles);
}

__global__ __launch_bounds__(kBlock) void gl_grad_kernel(GlArgs a) {
  __shared__ double sh[kWavesPerBlock];
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  const size_t N = (size_t)a.n;
  double lsum = 0.0;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    const int ex = a.sidx[j];
    if ((unsigned)ex >= (unsigned)a.n) continue;
    const int f = min(max(a.first[j], 0), j), e = a.end[j];
    double d = 0.0;
    if (e != 0) {
      const double Z = a.gred[f], A = a.gred[N + f];
      if (A != 0.0) {
        d = A * (a.sz[j] / Z) - a.sa[j];
        if (f == j) lsum += A * (a.gm[f] + log(Z)) - a.gred[2 * N + f];
      }
    }
    a.dpred[ex] = (float)(a.grad_scale * d);
  }
  double ex_, tot;
  auc_block_scan<double, kWavesPerBlock>(lsum, ex_, tot, sh);
  if (threadIdx.x == 0) a.lpart[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kAucBaseThreads) void gl_final_kernel(GlArgs a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ double sh[NW];
  // thread t sums its contiguous share of the tiles' partials in tile order, then the block in thread order
  const int per = (a.ntiles + kAucBaseThreads - 1) / kAucBaseThreads;
  double r = 0.0;
  for (long long t = (long long)threadIdx.x * per; t < min((long long)a.ntiles, (long long)(threadIdx.x + 1) * per); ++t)
    r += a.lpart[t];
  double ex_, tot;
  auc_block_scan<double, NW>(r, ex_, tot, sh);
  if (threadIdx.x == 0) *a.loss = (float)tot;
}

// The loss of the n >= 1 examples planned into plan_ws: dpred[n] (example order) and loss[1], asynchronously on st;
// ws (the plan's own workspace, or another one of the same size) holds the intermediates.  0 or a hip error code;
// -1: bad arguments; -2: a workspace is too small.
int launch_group_softmax(const void* plan_ws, size_t plan_bytes, int n, const float* scores, const float* labels,
                         const float* weights, double grad_scale, float* dpred, float* loss, void* ws, size_t ws_bytes,
                         hipStream_t st) {
  if (n < 1 || (unsigned)n > kOsCnt || !plan_ws || !scores || !labels || !dpred || !loss || !ws) return -1;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(plan_ws) & 15)) return -1;
  const GlLayout l = gl_layout(n);
  if (ws_bytes < l.total || plan_bytes < l.total) return -2;
  const char* pb = static_cast<const char*>(plan_ws);
  char* b = static_cast<char*>(ws);
  GlArgs a{};
  a.n = n;
  a.ntiles = l.ntiles;
  a.grad_scale = grad_scale;
  a.scores = scores;
  a.labels = labels;
  a.weights = weights;
  a.sidx = reinterpret_cast<const int*>(pb + l.sidx);
  a.first = reinterpret_cast<const int*>(pb + l.first);
  a.end = reinterpret_cast<const int*>(pb + l.end);
  a.ss = reinterpret_cast<float*>(b + l.ss);
  a.sa = reinterpret_cast<double*>(b + l.sa);
  a.sz = reinterpret_cast<double*>(b + l.sz);
  a.gm = reinterpret_cast<double*>(b + l.gm);
  a.gred = reinterpret_cast<double*>(b + l.gred);
  a.tflag = reinterpret_cast<int*>(b + l.tflag);
  a.tv = reinterpret_cast<double*>(b + l.tv);
  a.fv = reinterpret_cast<double*>(b + l.fv);
  a.lpart = reinterpret_cast<double*>(b + l.lpart);
  a.dpred = dpred;
  a.loss = loss;
  const dim3 tiles(l.ntiles), blk(kBlock), one(kAucBaseThreads);
  hipLaunchKernelGGL(gl_max_kernel, tiles, blk, 0, st, a);
  if (l.ntiles > 1) hipLaunchKernelGGL(gl_max_carry_kernel, dim3(1), one, 0, st, a);  // (one tile: nothing is open)
  hipLaunchKernelGGL(gl_sum_kernel, tiles, blk, 0, st, a);
  if (l.ntiles > 1) hipLaunchKernelGGL(gl_sum_carry_kernel, dim3(kGlChannels), one, 0, st, a);
  hipLaunchKernelGGL(gl_grad_kernel, tiles, blk, 0, st, a);
  hipLaunchKernelGGL(gl_final_kernel, dim3(1), one, 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace fm
