// Threshold metrics of (score, label, weight) triples: average precision, KS, best F1 and the operating points
// of up to 4 precision and 4 recall targets (threshold_rule.h has the rules, ops/kernels.py the definitions).
//
// Every distinct score t is a candidate threshold "positive iff score >= t":
//   TP(t) / FP(t) = weight of the positives / negatives with score >= t,  PP = TP + FP  (a candidate: PP > 0)
//   AP = (1 / P) sum_{i positive, w_i > 0} w_i TP(s_i) / PP(s_i)
//   KS = max_t |TP / P - FP / N|,  best F1 = max_t 2 TP / (PP + P)        (equal maxima: the highest score)
//   precision target: the greatest TP among TP >= target PP;  recall target: the highest t with TP >= target P
// Scores are ordered as in auc.hip (score_key.h) but from the highest down: the sort runs on the complemented
// key, so TP and FP of a run of equal scores are the inclusive prefixes at the run's end -- sums of
// non-negative terms, never a difference of prefixes.  Two modes as in auc.hip: uint64 (exact) without weights,
// fp64 with; the AP numerator is an fp64 sum in both.  No float atomics, every sum in a fixed order, every
// selection independent of the order of its comparisons: bitwise the same run to run.
//
// Launch chain (no kernel waits for another workgroup; kernel boundaries order the steps):
//   key, sort, tile, base, cum: metric_common.hip's descending score sort and prefix chain with the channels
//          (negatives, positives), both prefixes: FP = cum[0][e + 1], TP = cum[1][e + 1] at a run's end e;
//          P = cum[1][n], N = cum[0][n] (so that the last run has TP == P bit for bit);
//   tile:  per 2048 positions, 8 per thread: every run end is tried for KS, F1 and each target; every positive
//          adds its AP term (its run's end by the neighbour, or by a binary search when tied: a run may span
//          any number of tiles); per tile the AP sum, the best candidate of KS, F1 and each precision target,
//          the first passing position of each recall target;
//   final: one block reduces the partials in tile order and writes the record (threshold_rule.h); a nonzero
//          sort error also sets the sticky device error word.
// (Included by module.hip after auc.hip.)
#include "../threshold_rule.h"
#include "fm_common.h"

namespace fm {

template <typename T>
struct ThrArgs : PrefixArgs<T> {
  thr::Targets tg;
  double* part_ap;         // [ntiles] AP partial sums
  thr::Cand<T>* part_sel;  // [ntiles][kSel] best candidates: KS, F1, the precision targets
  int* part_rc;            // [ntiles][kMaxTargets] first position that passes each recall target
  T* out;                  // [thr::kRecWords]
};

// The best of the block's candidates (in every thread); better(a, b) is a strict order with no ties.
template <typename T, typename B>
__device__ inline thr::Cand<T> thr_block_best(thr::Cand<T> c, B better, thr::Cand<T>* sh /*[kWavesPerBlock]*/) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const thr::Cand<T> d{__shfl_down(c.tp, o, kWave), __shfl_down(c.fp, o, kWave), __shfl_down(c.pos, o, kWave)};
    if (better(d, c)) c = d;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = c;
  __syncthreads();
  thr::Cand<T> r = sh[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w)
    if (better(sh[w], r)) r = sh[w];
  __syncthreads();
  return r;
}

__device__ inline int thr_block_min(int v, int* sh /*[kWavesPerBlock]*/) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = min(v, __shfl_down(v, o, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  int r = sh[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) r = min(r, sh[w]);
  __syncthreads();
  return r;
}

// What a thread, a tile and the whole input keep: the AP sum and the selections so far.
template <typename T>
struct ThrBest {
  double ap = 0;
  thr::Cand<T> sel[thr::kSel];
  int rc[thr::kMaxTargets];
  __device__ ThrBest() {
#pragma unroll
    for (int s = 0; s < thr::kSel; ++s) sel[s] = thr::no_cand<T>();
#pragma unroll
    for (int i = 0; i < thr::kMaxTargets; ++i) rc[i] = thr::kNoPos;
  }
};

// b = the better of b and c, selection by selection.
template <typename T>
__device__ inline void thr_merge_sel(ThrBest<T>& b, const thr::Cand<T>* c, const int* rc, const thr::Targets& tg,
                                     T P, T N) {
  if (thr::ks_better(c[0], b.sel[0], P, N)) b.sel[0] = c[0];
  if (thr::f1_better(c[1], b.sel[1], P)) b.sel[1] = c[1];
#pragma unroll
  for (int i = 0; i < thr::kMaxTargets; ++i) {
    if (i < tg.np && thr::tp_better(c[2 + i], b.sel[2 + i])) b.sel[2 + i] = c[2 + i];
    if (i < tg.nr) b.rc[i] = min(b.rc[i], rc[i]);
  }
}

// The block's reduction of every thread's b (in every thread); ap: the block's sum in thread order.
template <typename T>
__device__ inline void thr_block_reduce(ThrBest<T>& b, const thr::Targets& tg, T P, T N) {
  __shared__ thr::Cand<T> shc[kWavesPerBlock];
  __shared__ double shd[kWavesPerBlock];
  __shared__ int shi[kWavesPerBlock];
  double e, t;
  auc_block_scan<double, kWavesPerBlock>(b.ap, e, t, shd);
  b.ap = t;
  b.sel[0] = thr_block_best(b.sel[0], [=](const thr::Cand<T>& x, const thr::Cand<T>& y) {
    return thr::ks_better(x, y, P, N);
  }, shc);
  b.sel[1] = thr_block_best(b.sel[1], [=](const thr::Cand<T>& x, const thr::Cand<T>& y) {
    return thr::f1_better(x, y, P);
  }, shc);
#pragma unroll
  for (int i = 0; i < thr::kMaxTargets; ++i) {
    if (i < tg.np)
      b.sel[2 + i] = thr_block_best(b.sel[2 + i], [](const thr::Cand<T>& x, const thr::Cand<T>& y) {
        return thr::tp_better(x, y);
      }, shc);
    if (i < tg.nr) b.rc[i] = thr_block_min(b.rc[i], shi);
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void thr_tile_kernel(ThrArgs<T> a) {
  const int j0 = blockIdx.x * kAucTile + threadIdx.x * kAucItems;
  const T* fpc = a.cum[0];
  const T* tpc = a.cum[1];
  const T P = tpc[a.n], N = fpc[a.n];
  const double dP = (double)P;
  uint32_t sv[kAucItems], k[kAucItems];
  load8(a.sv, j0, a.n, sv, 0u);
  load8(a.skeys, j0, a.n, k, 0u);
  const uint32_t knext = j0 + kAucItems < a.n ? a.skeys[j0 + kAucItems] : 0u;
  ThrBest<T> b;
  bool have = false;  // (etp, efp) of the previous position hold for this one: same key
  T etp = 0, efp = 0;  // TP and FP at the end of the current positive's run
#pragma unroll
  for (int q = 0; q < kAucItems; ++q) {
    const int j = j0 + q;
    if (j >= a.n) break;
    const bool run_end = j + 1 >= a.n || (q + 1 < kAucItems ? k[q + 1] : knext) != k[q];
    const bool tie_prev = q > 0 && k[q - 1] == k[q];
    have = have && tie_prev;
    if (run_end) {
      etp = tpc[j + 1];
      efp = fpc[j + 1];
      have = true;
      const T pp = etp + efp;
      if (pp > (T)0) {
        const thr::Cand<T> c{etp, efp, j};
        const double dtp = (double)etp, dpp = (double)pp;
        thr::Cand<T> cand[thr::kSel];
        int rc[thr::kMaxTargets];
        cand[0] = cand[1] = c;
#pragma unroll
        for (int i = 0; i < thr::kMaxTargets; ++i) {
          cand[2 + i] = (i < a.tg.np && thr::precision_ok(dtp, dpp, a.tg.pt[i])) ? c : thr::no_cand<T>();
          rc[i] = (i < a.tg.nr && thr::recall_ok(dtp, dP, a.tg.rt[i])) ? j : thr::kNoPos;
        }
        thr_merge_sel(b, cand, rc, a.tg, P, N);
      }
    }
    const float s = __uint_as_float(sv[q]);
    if (!(s > 0.f)) continue;
    if (!have) {
      const int ub = auc_bound<true>(a.skeys, j + 1, a.n, k[q]);
      etp = tpc[ub];
      efp = fpc[ub];
      have = true;
    }
    b.ap = thr::ap_add(b.ap, (double)s, (double)etp, (double)(etp + efp));
  }
  thr_block_reduce(b, a.tg, P, N);
  if (threadIdx.x == 0) {
    a.part_ap[blockIdx.x] = b.ap;
#pragma unroll
    for (int s = 0; s < thr::kSel; ++s) a.part_sel[(size_t)blockIdx.x * thr::kSel + s] = b.sel[s];
#pragma unroll
    for (int i = 0; i < thr::kMaxTargets; ++i) a.part_rc[(size_t)blockIdx.x * thr::kMaxTargets + i] = b.rc[i];
  }
}

// A 64-bit record word of type T holding the bits of an fp64 value.
template <typename T>
__device__ inline T thr_f64_word(double v) {
  if constexpr (std::is_same<T, double>::value) return v;
  else return (T)__double_as_longlong(v);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void thr_final_kernel(ThrArgs<T> a) {
  const T* fpc = a.cum[0];
  const T* tpc = a.cum[1];
  const T P = tpc[a.n], N = fpc[a.n];
  // thread t reduces its contiguous share of the partials in tile order, then the block in thread order
  const int per = (a.ntiles + kBlock - 1) / kBlock;
  ThrBest<T> b;
  for (int i = threadIdx.x * per; i < min(a.ntiles, (threadIdx.x + 1) * per); ++i) {
    b.ap += a.part_ap[i];
    thr_merge_sel(b, a.part_sel + (size_t)i * thr::kSel, a.part_rc + (size_t)i * thr::kMaxTargets, a.tg, P, N);
  }
  thr_block_reduce(b, a.tg, P, N);
  if (threadIdx.x != 0) return;
  const int err = *a.sort_err;
  a.out[0] = thr_f64_word<T>(b.ap);
  a.out[1] = P;
  a.out[2] = N;
  // point s of the record: the candidate at position pos (kNoPos: no such threshold, all zero)
  const auto put = [&](int s, int pos) {
    const bool ok = pos >= 0 && pos < a.n;
    T* o = a.out + thr::kPoint0 + 3 * s;
    o[0] = ok ? tpc[pos + 1] : (T)0;
    o[1] = ok ? fpc[pos + 1] : (T)0;
    o[2] = ok ? (T)score_key_bits(~a.skeys[pos]) : (T)0;
  };
#pragma unroll
  for (int s = 0; s < thr::kSel; ++s) put(s, b.sel[s].pos);
#pragma unroll
  for (int i = 0; i < thr::kMaxTargets; ++i) put(thr::kSel + i, b.rc[i]);
  a.out[thr::kRecWords - 2] = (T)*a.nan_count;
  a.out[thr::kRecWords - 1] = (T)err;
  if (err) atomicOr(&g_fm_dev_error, kDevErrSort);
}

// Workspace: the prefix chain's pieces (both prefixes), the tile partials, then the sort workspace.
struct ThrLayout {
  PrefixLayout p;
  size_t part_ap, part_sel, part_rc, sort, total;
};
static_assert(sizeof(thr::Cand<uint64_t>) == sizeof(thr::Cand<double>), "one layout for both modes");

static ThrLayout thr_layout(int n) {
  WsCursor c;
  ThrLayout l{};
  l.p = prefix_layout(c, n, ThrChannels::kSecondPrefix);
  const size_t nt = (size_t)l.p.ntiles;
  l.part_ap = c.take(8 * nt);
  l.part_sel = c.take(sizeof(thr::Cand<double>) * thr::kSel * nt);
  l.part_rc = c.take(4 * thr::kMaxTargets * nt);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.total = c.off;
  return l;
}

// Bytes of launch_threshold's workspace for n scores; 0: n is out of range (n >= 2^30, the sort's bound).
size_t threshold_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  if (n == 0) return 256;
  return thr_layout((int)n).total;
}

template <typename T>
static int launch_threshold_t(const float* scores, const float* labels, const float* weights, int n,
                              const thr::Targets& tg, void* out, char* ws, const ThrLayout& l, hipStream_t st) {
  ThrArgs<T> a{};
  const int se =
      launch_score_prefix<T, ThrChannels>(scores, labels, weights, n, ws, l.p, ws + l.sort, st, a, /*descending=*/true);
  if (se != 0) return se;
  a.tg = tg;
  a.part_ap = reinterpret_cast<double*>(ws + l.part_ap);
  a.part_sel = reinterpret_cast<thr::Cand<T>*>(ws + l.part_sel);
  a.part_rc = reinterpret_cast<int*>(ws + l.part_rc);
  a.out = static_cast<T*>(out);
  hipLaunchKernelGGL(thr_tile_kernel<T>, dim3(l.p.ntiles), dim3(kBlock), 0, st, a);
  hipLaunchKernelGGL(thr_final_kernel<T>, dim3(1), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

// Threshold metrics of n >= 1 scores into out[thr::kRecWords] (uint64 when weights is null, else fp64; word 0
// holds fp64 bits in both), asynchronously on st; pt[np] / rt[nr]: the precision / recall targets.
// 0 or a hip error code; -1: bad arguments; -2: workspace too small; -5: n >= 2^30; -6: more than 4 targets of
// a kind, or one outside (0, 1].
int launch_threshold(const float* scores, const float* labels, const float* weights, int n, const double* pt,
                     int np, const double* rt, int nr, void* out, void* ws, size_t ws_bytes, hipStream_t st) {
  if (const int rc = metric_check_args(n, scores, labels, out, ws)) return rc;
  if (np < 0 || np > thr::kMaxTargets || nr < 0 || nr > thr::kMaxTargets || (np && !pt) || (nr && !rt)) return -6;
  thr::Targets tg{};
  tg.np = np;
  tg.nr = nr;
  for (int i = 0; i < np; ++i) {
    if (!(pt[i] > 0.0 && pt[i] <= 1.0)) return -6;
    tg.pt[i] = pt[i];
  }
  for (int i = 0; i < nr; ++i) {
    if (!(rt[i] > 0.0 && rt[i] <= 1.0)) return -6;
    tg.rt[i] = rt[i];
  }
  const ThrLayout l = thr_layout(n);
  if (ws_bytes < l.total) return -2;
  char* b = static_cast<char*>(ws);
  if (weights) return launch_threshold_t<double>(scores, labels, weights, n, tg, out, b, l, st);
  return launch_threshold_t<uint64_t>(scores, labels, weights, n, tg, out, b, l, st);
}

}  // namespace fm

