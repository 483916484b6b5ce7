// Grouped AUC (GAUC): the exact weighted ROC AUC of every group (a user, a query, a session) and their
// weight-averaged mean -- the offline metric of a ranking model, next to auc.hip's global AUC.
//
//   per group g:  P_g / N_g = weight of its positives / negatives (positive iff label > 0)
//                 U2_g = sum_{i pos in g} w_i (Nlt_g(s_i) + Nle_g(s_i))   (negatives OF THE SAME GROUP below /
//                                                                          not above s_i)
//   valid iff P_g > 0 and N_g > 0;  AUC_g = U2_g / (2 P_g N_g),  W_g = P_g + N_g
//   GAUC = sum_valid W_g AUC_g / sum_valid W_g
//
// Scores are keyed, ordered and NaN-counted by metric_common.hip's score sort.  Two modes: unweighted in uint64
// (the per-group records are exact integers), weighted in fp64; every sum has a fixed order and adds only
// non-negative terms of ONE group (no group sum is a difference of two global prefixes), so the results are
// bitwise the same run to run and a small group next to a huge one keeps its full precision.
//
// Launch chain (kernel boundaries order the steps; no host sync, the workspace is the caller's: capturable):
//   key, sort 1: launch_score_sort: key + example index per score, NaN count, stable sort by the 32 key bits;
//   gather:  group id of every score-sorted position (the first sort's error word is saved here: the second
//            sort reuses its workspace);
//   sort 2:  the same stable sort over bits_for(G) bits of the group id -> (group, score) order;
//   tile:    per 2048-position tile: signed weight and score key of every position (the gathers through the
//            sorted index), every group's [first, last + 1) range at its head / tail, and the tile's
//            segmented totals of the negatives' and positives' weight (a "segment" restarts at a group head);
//   base:    one block scans the tile totals with the segmented operator -> what every tile inherits;
//   nex:     ex[j] = weight of the negatives of j's group at positions < j; P_g and N_g at every group's tail;
//   rank:    a positive at j adds w (ex[lb] + ex[ub - 1] + neg[ub - 1]), [lb, ub) = its run of equal (group,
//            key): neighbours first, else binary searches clamped to the group's range (a run may span any
//            number of tiles, equal scores of adjacent groups never join); the contributions are summed by a
//            segmented scan in the tile: a group whose head lies in the tile gets its U2 at its tail, the one
//            open at the tile's start leaves its partial sum;
//   ubase:   one block carries those partials over the tiles in tile order (a group spanning hundreds of
//            tiles) and completes the U2 of every group that ends in a later tile than it began;
//   group:   one thread per group: validity and W_g AUC_g, block sums in a fixed order;
//   final:   one block sums the blocks' partials in order and writes the record
//            [sum_valid W_g AUC_g (fp64), sum_valid W_g, valid groups, examples in valid groups, NaN count,
//             sort error word]; a nonzero sort error also sets the sticky device error word.
// Groups of a few examples sit several to a wave (eight positions per lane, the segmented scan keeps them
// apart); the same scan carries one group over any number of tiles.  Empty groups keep the zeros of the
// chain's memset.  (Included by module.hip after metric_common.hip: the tile constants, auc_block_scan, auc_bound,
// signed_weight, the workspace cursor and the argument check are defined there.)
#include "fm_common.h"

namespace fm {

// Block-wide segmented scan of one (head flag, value) per thread, in thread order: a thread whose flag is set
// starts a new segment with its value.  (ef, ev): the open segment's sum over the threads before this one and
// whether one of them had a flag (ev counts from the last such thread); (tf, tv): the same over the whole
// block.  Exclusive values come from shifted inclusive ones, never from a subtraction.
template <typename T, int NW>
__device__ inline void gauc_seg_scan(bool f, T v, bool& ef, T& ev, bool& tf, T& tv, int* shf /*[NW]*/,
                                     T* shv /*[NW]*/) {
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  int fi = f ? 1 : 0;
  T inc = v;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const T up = __shfl_up(inc, o, kWave);
    const int uf = __shfl_up(fi, o, kWave);
    if (lane >= o) {
      if (!fi) inc += up;
      fi |= uf;
    }
  }
  T bv = __shfl_up(inc, 1, kWave);
  int bf = __shfl_up(fi, 1, kWave);
  if (lane == 0) {
    bv = 0;
    bf = 0;
  }
  if (lane == kWave - 1) {
    shf[wv] = fi;
    shv[wv] = inc;
  }
  __syncthreads();
  int pf = 0, cf = 0;
  T pv = 0, cv = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    if (w == wv) {
      pf = cf;
      pv = cv;
    }
    if (shf[w]) cv = shv[w];
    else cv += shv[w];
    cf |= shf[w];
  }
  ef = (pf | bf) != 0;
  ev = bf ? bv : pv + bv;
  tf = cf != 0;
  tv = cv;
  __syncthreads();
}

template <typename T>
struct GaucArgs {
  int n, ntiles, G, gblocks;
  const float* labels;
  const float* weights;    // null: all ones
  const uint32_t* keys;    // [n] score key of every example
  const int* sg;           // [n] group id of every (group, score)-sorted position
  const int* sidx;         // [n] example index of every sorted position
  uint32_t* fkeys;         // [n] score key of every sorted position
  uint32_t* sv;            // [n] float bits: +w (positive) / -w (negative) of every sorted position
  T* ex;                   // [n] negatives' weight of the position's group before it
  int* grange;             // [G, 2] first position, last position + 1 (0, 0: empty)
  int* tflag;              // [ntiles] the tile holds a group head
  T* tn;                   // [ntiles] negatives' weight from the tile's last head (or its start) to its end
  T* tp;                   // [ntiles] the same of the positives
  T* cn;                   // [ntiles] negatives' weight the tile inherits: its first group's, before the tile
  T* cp;                   // [ntiles]
  T* tu;                   // [ntiles] U2 terms from the tile's last head (or its start) to its end
  T* fu;                   // [ntiles] U2 terms from the tile's start to the tail of the group open there
  T* rec;                  // [G, 3] U2_g, P_g, N_g
  unsigned char* gpart;    // [gblocks, 32] per block of groups: sum W AUC (fp64), sum W (T), valid, examples
  const unsigned* nan_count;
  const int* sort_err1;    // the score sort's error word (saved by the gather kernel)
  const int* sort_err2;    // the group sort's
  void* out;               // [6] the record
};

// group id of sorted position j (clamped: a failed sort may leave anything there; its error word is reported)
__device__ inline int gauc_gid(int v, int G) { return (unsigned)v < (unsigned)G ? v : G - 1; }

// the group ids of a thread's 8 positions, of the position before and of the one after (-1: none)
template <typename T>
__device__ inline void gauc_groups(const GaucArgs<T>& a, int j0, int (&g)[kAucItems], int& gprev, int& gnext) {
  load8(a.sg, j0, a.n, g, 0);
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) g[q] = gauc_gid(g[q], a.G);
  gprev = (j0 > 0 && j0 <= a.n) ? gauc_gid(a.sg[j0 - 1], a.G) : -1;
  gnext = j0 + kAucItems < a.n ? gauc_gid(a.sg[j0 + kAucItems], a.G) : -1;
}

// position j = j0 + q (< n) is the first / the last of its group (gprev == -1 at j == 0)
__device__ inline bool gauc_head(const int (&g)[kAucItems], int q, int gprev) {
  return g[q] != (q ? g[q - 1] : gprev);
}
__device__ inline bool gauc_tail(const int (&g)[kAucItems], int q, int gnext, int j, int n) {
  return j == n - 1 || g[q] != (q + 1 < kAucItems ? g[q + 1] : gnext);
}

__global__ __launch_bounds__(kBlock) void gauc_gather_kernel(int n, int G, const int* groups, const int* sidx,
                                                             uint32_t* gk, const int* sort_err, int* err_out) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *err_out = *sort_err;
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const int e = sidx[j];
    gk[j] = (unsigned)e < (unsigned)n ? (uint32_t)gauc_gid(groups[e], G) : 0u;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauc_tile_kernel(GaucArgs<T> a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ T shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  int ex[kAucItems], g[kAucItems], gprev, gnext;
  load8(a.sidx, j0, a.n, ex, -1);
  gauc_groups(a, j0, g, gprev, gnext);
  T neg = 0, pos = 0;
  bool hf = false;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    if (gauc_head(g, q, gprev)) {
      a.grange[2 * (size_t)g[q]] = j;
      neg = 0;
      pos = 0;
      hf = true;
    }
    if (gauc_tail(g, q, gnext, j, a.n)) a.grange[2 * (size_t)g[q] + 1] = j + 1;
    const float s = signed_weight(a.labels, a.weights, ex[q], a.n);
    a.sv[j] = __float_as_uint(s);
    a.fkeys[j] = (unsigned)ex[q] < (unsigned)a.n ? a.keys[ex[q]] : 0u;  // (as signed_weight: a failed sort)
    if (s > 0.f) pos += (T)s;
    else neg += (T)(-s);
  }
  bool ef, tf;
  T ev, tv;
  gauc_seg_scan<T, kWavesPerBlock>(hf, neg, ef, ev, tf, tv, shf, shv);
  if (threadIdx.x == 0) {
    a.tflag[blockIdx.x] = tf;
    a.tn[blockIdx.x] = tv;
  }
  gauc_seg_scan<T, kWavesPerBlock>(hf, pos, ef, ev, tf, tv, shf, shv);
  if (threadIdx.x == 0) a.tp[blockIdx.x] = tv;
}

template <typename T>
__global__ __launch_bounds__(kAucBaseThreads) void gauc_base_kernel(GaucArgs<T> a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ int shf[NW];
  __shared__ T shv[NW];
  T carry_n = 0, carry_p = 0;
  for (int c = 0; c < a.ntiles; c += kAucBaseThreads) {
    const int t = c + threadIdx.x;
    const bool ok = t < a.ntiles;
    const bool f = ok && a.tflag[t] != 0;
    bool ef, tf;
    T ev, tv;
    gauc_seg_scan<T, NW>(f, ok ? a.tn[t] : (T)0, ef, ev, tf, tv, shf, shv);
    if (ok) a.cn[t] = ef ? ev : carry_n + ev;
    carry_n = tf ? tv : carry_n + tv;
    gauc_seg_scan<T, NW>(f, ok ? a.tp[t] : (T)0, ef, ev, tf, tv, shf, shv);
    if (ok) a.cp[t] = ef ? ev : carry_p + ev;
    carry_p = tf ? tv : carry_p + tv;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauc_nex_kernel(GaucArgs<T> a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ T shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  uint32_t sv[kAucItems];
  int g[kAucItems], gprev, gnext;
  load8(a.sv, j0, a.n, sv, 0u);
  gauc_groups(a, j0, g, gprev, gnext);
  T m[kAucItems], p[kAucItems], neg = 0, pos = 0;
  bool hf = false;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    const float s = __uint_as_float(sv[q]);
    m[q] = (j < a.n && !(s > 0.f)) ? (T)(-s) : (T)0;
    p[q] = (j < a.n && s > 0.f) ? (T)s : (T)0;
    if (j < a.n && gauc_head(g, q, gprev)) {
      neg = 0;
      pos = 0;
      hf = true;
    }
    neg += m[q];
    pos += p[q];
  }
  bool efn, efp, tf;
  T evn, evp, tv;
  gauc_seg_scan<T, kWavesPerBlock>(hf, neg, efn, evn, tf, tv, shf, shv);
  gauc_seg_scan<T, kWavesPerBlock>(hf, pos, efp, evp, tf, tv, shf, shv);
  T run_n = efn ? evn : a.cn[blockIdx.x] + evn;
  T run_p = efp ? evp : a.cp[blockIdx.x] + evp;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) continue;
    if (gauc_head(g, q, gprev)) {
      run_n = 0;
      run_p = 0;
    }
    a.ex[j] = run_n;
    run_n += m[q];
    run_p += p[q];
    if (gauc_tail(g, q, gnext, j, a.n)) {
      a.rec[3 * (size_t)g[q] + 1] = run_p;
      a.rec[3 * (size_t)g[q] + 2] = run_n;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauc_rank_kernel(GaucArgs<T> a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ T shv[kWavesPerBlock];
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  uint32_t sv[kAucItems], k[kAucItems];
  int g[kAucItems], gprev, gnext;
  load8(a.sv, j0, a.n, sv, 0u);
  load8(a.fkeys, j0, a.n, k, 0u);
  gauc_groups(a, j0, g, gprev, gnext);
  const uint32_t kprev = (j0 > 0 && j0 <= a.n) ? a.fkeys[j0 - 1] : 0u;
  const uint32_t knext = j0 + kAucItems < a.n ? a.fkeys[j0 + kAucItems] : 0u;
  T u[kAucItems], usum = 0;
  bool hf = false;
  bool have = false;  // (lb, ub) of the previous position hold for this one: same group and key
  int lb = 0, ub = 0;
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    u[q] = 0;
    if (j >= a.n) continue;
    const bool head = gauc_head(g, q, gprev);
    if (head) {
      usum = 0;
      hf = true;
    }
    const float s = __uint_as_float(sv[q]);
    const bool tie_prev = !head && (q ? k[q - 1] : kprev) == k[q];
    if (!(s > 0.f)) {
      have = have && tie_prev;
      continue;
    }
    if (!(have && tie_prev)) {
      const bool tail = gauc_tail(g, q, gnext, j, a.n);
      const bool tie_next = !tail && (q + 1 < kAucItems ? k[q + 1] : knext) == k[q];
      lb = j;
      ub = j + 1;
      if (tie_prev) lb = auc_bound<false>(a.fkeys, min(a.grange[2 * (size_t)g[q]], j), j, k[q]);
      if (tie_next) ub = auc_bound<true>(a.fkeys, j + 1, max(a.grange[2 * (size_t)g[q] + 1], j + 1), k[q]);
      have = true;
    }
    // (lb <= j < ub <= n: every index below is a position of the set)
    const float sl = __uint_as_float(a.sv[ub - 1]);
    const T last = sl > 0.f ? (T)0 : (T)(-sl);
    u[q] = (T)s * (a.ex[lb] + (a.ex[ub - 1] + last));
    usum += u[q];
  }
  bool ef, tf;
  T ev, tv;
  gauc_seg_scan<T, kWavesPerBlock>(hf, usum, ef, ev, tf, tv, shf, shv);
  if (threadIdx.x == 0) a.tu[blockIdx.x] = tv;
  T run = ev;
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
      if (seen) a.rec[3 * (size_t)g[q]] = run;
      else a.fu[blockIdx.x] = run;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kAucBaseThreads) void gauc_ubase_kernel(GaucArgs<T> a) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ int shf[NW];
  __shared__ T shv[NW];
  T carry = 0;
  for (int c = 0; c < a.ntiles; c += kAucBaseThreads) {
    const int t = c + threadIdx.x;
    const bool ok = t < a.ntiles;
    bool ef, tf;
    T ev, tv;
    gauc_seg_scan<T, NW>(ok && a.tflag[t] != 0, ok ? a.tu[t] : (T)0, ef, ev, tf, tv, shf, shv);
    if (ok && t > 0) {
      // the group open at the tile's start, when it ends in this tile: what the tiles before it hold of it
      // (in tile order) plus this tile's share
      const int j0 = t * kAucTile;
      const int g = gauc_gid(a.sg[j0], a.G);
      if (g == gauc_gid(a.sg[j0 - 1], a.G) && a.grange[2 * (size_t)g + 1] <= min(a.n, j0 + kAucTile))
        a.rec[3 * (size_t)g] = (ef ? ev : carry + ev) + a.fu[t];
    }
    carry = tf ? tv : carry + tv;
  }
}

// The block's sums (in thread order) of a thread's four quantities, packed by thread 0 into the 32-byte record o:
// [sum W AUC (fp64), sum W (T), valid groups, examples in valid groups].
template <typename T>
__device__ inline void gauc_pack_sums(double wa, T w, uint64_t valid, uint64_t exs, unsigned char* o) {
  __shared__ double shd[kWavesPerBlock];
  __shared__ T sht[kWavesPerBlock];
  __shared__ uint64_t shu[kWavesPerBlock];
  double ed, td;
  T et, tt;
  uint64_t eu, tv, te;
  auc_block_scan<double, kWavesPerBlock>(wa, ed, td, shd);
  auc_block_scan<T, kWavesPerBlock>(w, et, tt, sht);
  auc_block_scan<uint64_t, kWavesPerBlock>(valid, eu, tv, shu);
  auc_block_scan<uint64_t, kWavesPerBlock>(exs, eu, te, shu);
  if (threadIdx.x == 0) {
    *reinterpret_cast<double*>(o) = td;
    *reinterpret_cast<T*>(o + 8) = tt;
    *reinterpret_cast<uint64_t*>(o + 16) = tv;
    *reinterpret_cast<uint64_t*>(o + 24) = te;
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauc_group_kernel(GaucArgs<T> a) {
  const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
  double wa = 0.0;
  T w = 0;
  uint64_t valid = 0, exs = 0;
  if (g < a.G) {
    const T u2 = a.rec[3 * (size_t)g], p = a.rec[3 * (size_t)g + 1], ng = a.rec[3 * (size_t)g + 2];
    if (p > 0 && ng > 0) {
      w = p + ng;
      wa = (double)w * ((double)u2 / (2.0 * (double)p * (double)ng));
      valid = 1;
      exs = (uint64_t)(a.grange[2 * (size_t)g + 1] - a.grange[2 * (size_t)g]);
    }
  }
  gauc_pack_sums<T>(wa, w, valid, exs, a.gpart + 32 * (size_t)blockIdx.x);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gauc_final_kernel(GaucArgs<T> a) {
  // thread t sums its contiguous share of the blocks' partials in block order, then the block in thread order
  const int per = (a.gblocks + kBlock - 1) / kBlock;
  double wa = 0.0;
  T w = 0;
  uint64_t valid = 0, exs = 0;
  for (long long i = (long long)threadIdx.x * per; i < min((long long)a.gblocks, (long long)(threadIdx.x + 1) * per);
       ++i) {
    const unsigned char* o = a.gpart + 32 * (size_t)i;
    wa += *reinterpret_cast<const double*>(o);
    w += *reinterpret_cast<const T*>(o + 8);
    valid += *reinterpret_cast<const uint64_t*>(o + 16);
    exs += *reinterpret_cast<const uint64_t*>(o + 24);
  }
  unsigned char* o = static_cast<unsigned char*>(a.out);
  gauc_pack_sums<T>(wa, w, valid, exs, o);
  if (threadIdx.x == 0) {
    const int err = *a.sort_err1 | *a.sort_err2;
    *reinterpret_cast<uint64_t*>(o + 32) = (uint64_t)*a.nan_count;
    *reinterpret_cast<uint64_t*>(o + 40) = (uint64_t)(unsigned)err;
    if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
  }
}

// Workspace: [keys n][idx -> sv n][score-sorted keys -> final keys n][score-sorted idx n][group keys n]
// [sorted groups n][sorted idx n][ex n][tiles: 6 x 8 + 4 bytes each][grange 2 G][gpart 32 per block of
// groups][nan count, first sort error][sort workspace]
struct GaucLayout {
  size_t keys, bufa, bufb, si1, gk, sg, si2, ex, tiles, tflag, grange, gpart, misc, sort, total;
  int ntiles, gblocks;
};

static GaucLayout gauc_layout(int n, long long G) {
  WsCursor c;
  GaucLayout l{};
  l.ntiles = (n + kAucTile - 1) / kAucTile;
  l.gblocks = (int)((G + kBlock - 1) / kBlock);
  l.keys = c.take(4 * (size_t)n);
  l.bufa = c.take(4 * (size_t)n);
  l.bufb = c.take(4 * (size_t)n);
  l.si1 = c.take(4 * (size_t)n);
  l.gk = c.take(4 * (size_t)n);
  l.sg = c.take(4 * (size_t)n);
  l.si2 = c.take(4 * (size_t)n);
  l.ex = c.take(8 * (size_t)n);
  l.tiles = c.take(8 * 6 * (size_t)l.ntiles);
  l.tflag = c.take(4 * (size_t)l.ntiles);
  l.grange = c.take(8 * (size_t)G);
  l.gpart = c.take(32 * (size_t)l.gblocks);
  l.misc = c.take(32);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

static bool gauc_sizes_ok(long long n, long long G) {
  return n >= 0 && n <= (long long)kOsCnt && G >= 1 && G < (1ll << 31);
}

// Bytes of launch_gauc's workspace for n scores in G groups; 0: out of range (n >= 2^30, G outside [1, 2^31)).
size_t gauc_workspace_bytes(long long n, long long G) {
  if (!gauc_sizes_ok(n, G)) return 0;
  return gauc_layout((int)(n > 0 ? n : 1), G).total;
}

static int gauc_bits_for(long long G) {  // bits that hold every id in [0, G)
  int b = 1;
  while ((1ll << b) < G) ++b;
  return b;
}

template <typename T>
static int launch_gauc_t(const float* scores, const float* labels, const float* weights, const int* groups, int n,
                         int G, void* out, void* rec, char* ws, const GaucLayout& l, hipStream_t st) {
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + l.keys);
  int* idx = reinterpret_cast<int*>(ws + l.bufa);
  uint32_t* sk1 = reinterpret_cast<uint32_t*>(ws + l.bufb);
  int* si1 = reinterpret_cast<int*>(ws + l.si1);
  uint32_t* gk = reinterpret_cast<uint32_t*>(ws + l.gk);
  uint32_t* sg = reinterpret_cast<uint32_t*>(ws + l.sg);
  int* si2 = reinterpret_cast<int*>(ws + l.si2);
  T* tiles = reinterpret_cast<T*>(ws + l.tiles);
  int* grange = reinterpret_cast<int*>(ws + l.grange);
  unsigned* nan_count = reinterpret_cast<unsigned*>(ws + l.misc);
  int* err1 = reinterpret_cast<int*>(ws + l.misc) + 1;  // (written by the gather kernel)
  void* sort_ws = ws + l.sort;
  hipError_t e = hipMemsetAsync(grange, 0, 8 * (size_t)G, st);
  if (e == hipSuccess) e = hipMemsetAsync(rec, 0, 24 * (size_t)G, st);
  if (e != hipSuccess) return (int)e;
  ScoreSort s1;
  int se = launch_score_sort(scores, n, keys, idx, sk1, si1, nan_count, sort_ws, st, s1);
  if (se != 0) return se;
  hipLaunchKernelGGL(gauc_gather_kernel, dim3(fill_grid(n, kBlock, 2048)), dim3(kBlock), 0, st, n, G, groups, si1, gk,
                     s1.sort_err, err1);
  se = launch_radix_sort(gk, si1, sg, si2, n, gauc_bits_for(G), sort_ws, radix_sort_ws_bytes(n), st);
  if (se != 0) return se;
  const size_t nt = (size_t)l.ntiles;
  GaucArgs<T> a{n, l.ntiles, G, l.gblocks, labels, weights, keys, reinterpret_cast<const int*>(sg), si2,
                sk1 /* the score-sorted keys are dead: the final order's keys */,
                reinterpret_cast<uint32_t*>(idx) /* so is the identity index: the signed weights */,
                reinterpret_cast<T*>(ws + l.ex), grange, reinterpret_cast<int*>(ws + l.tflag), tiles, tiles + nt,
                tiles + 2 * nt, tiles + 3 * nt, tiles + 4 * nt, tiles + 5 * nt, static_cast<T*>(rec),
                reinterpret_cast<unsigned char*>(ws + l.gpart), nan_count, err1, s1.sort_err, out};
  hipLaunchKernelGGL(gauc_tile_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(gauc_base_kernel<T>, dim3(1), dim3(kAucBaseThreads), 0, st, a);
  hipLaunchKernelGGL(gauc_nex_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(gauc_rank_kernel<T>, dim3(l.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(gauc_ubase_kernel<T>, dim3(1), dim3(kAucBaseThreads), 0, st, a);
  hipLaunchKernelGGL(gauc_group_kernel<T>, dim3(l.gblocks), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(gauc_final_kernel<T>, dim3(1), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

// GAUC statistics of n >= 1 scores with group ids in [0, G): the per-group records into rec[G, 3] and the
// record into out[6] (64-bit words; the weight sums uint64 when weights is null, else fp64), asynchronously on
// st.  0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30; -6: G outside [1, 2^31).
int launch_gauc(const float* scores, const float* labels, const float* weights, const int* groups, int n,
                long long G, void* out, void* rec, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!groups || !rec || (reinterpret_cast<uintptr_t>(rec) & 7)) return -1;
  if (const int rc = metric_check_args(n, scores, labels, out, ws)) return rc;
  if (G < 1 || G >= (1ll << 31)) return -6;
  const GaucLayout l = gauc_layout(n, G);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  if (weights) return launch_gauc_t<double>(scores, labels, weights, groups, n, (int)G, out, rec, b, l, st);
  return launch_gauc_t<uint64_t>(scores, labels, weights, groups, n, (int)G, out, rec, b, l, st);
}

}  // namespace fm
