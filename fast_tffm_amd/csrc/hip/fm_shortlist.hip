// Recommend and place among every query's own shortlist of candidates (re-ranking what a retrieval stage handed
// over; the sampled-negative leave-one-out protocol.  The reference only scores examples).
//
// A shortlist per query is a CSR pair (SeenArgs, fm_rank_common.h): off int32 [nq + 1], idx int32 [nnz], a query's
// indices strictly ascending in [0, nc).  L_q is query q's set; the score s(q, c) is fm_topk.hip's, bit for bit.
//   top-k: row q holds the k greatest keys over c in L_q (-1 / -inf where |L_q| < k);
//   place: the competitors are L_q and the target t: greater = #{c in L_q, c != t : s(q, c) > s_t},
//          equal = 1 + #{c in L_q, c != t : s(q, c) == s_t}; a query with target -1 stays all zeros.
// The lists are checked by the caller (ops/kernels.py).  A malformed list gives unspecified results but no read out
// of bounds: a query's window is clamped to [0, nnz] and an index outside [0, nc) is skipped.
//
// shortlist_kernel<J, COUNT>: one wave (a 64-thread workgroup) per (query, part) pair; a query's list is cut into
// `parts` runs of whole 64-entry steps (../topk_order.h: shortlist_plan, shortlist_run), so most parts of a short
// list are empty -- and still write their k zero keys / zero counts: the passes behind read every slot and the
// workspace is never cleared.  The wave keeps the query's A operands in registers for the whole walk, in
// load_operands' layout (lane (r, h): columns 16 g + 4 h .. + 3) -- the same query in all 16 rows of the tile.  A
// step takes 64 list entries: one coalesced load of 64 indices (lane l: entry l), then four 16-candidate tiles;
// for tile t lane (r, h) fetches the index of entry 16 t + r from its lane and loads 16 bytes per column group of
// that candidate's row straight from C -- four lanes cover 64 contiguous bytes of a row, 16 rows per instruction
// -- and v_mfma_f32_16x16x4_f32 runs over the groups as in fm_topk.hip, so the fmaf chain is the same by
// construction.  Every row of an accumulator holds the same 16 scores; lane (r, h) keeps tile h's, which is the
// score of entry 16 h + r = its own lane's entry: after four tiles each lane holds exactly one (score, candidate)
// pair, next to the index and cb[c] it loaded itself.  Profiles of Kp <= 64 run two steps ahead: the indices of
// step i + 2 and the row gathers of step i + 1 are issued before step i is multiplied and ranked, so the gathers
// -- the walk's bound -- are in flight under it; wider profiles gather in place (in two halves above Kp = 128, to
// stay in registers) and lean on the other waves of the SIMD.
// Select epilogue (COUNT = false): select_append_row, topk_merge_kernel's selection on one row -- a lane whose key
// beats the current k-th key is found by ballot and appended to an LDS buffer of 2 kcap keys (kcap = max(64, pow2 >=
// k)), cut to k when it passes kcap -- and the k keys go to ws[(q parts + part) k ..], fm_topk's workspace
// layout: topk_merge_kernel with a.parts = this plan's parts finishes the job unchanged.
// Count epilogue (COUNT = true): after place_target_kernel; a lane compares its score with s_t, skipping c == t,
// the wave's two int32 sums are added across lanes in a fixed pattern and lane 0 writes the (query, part) partial,
// part 0 of a ranked query with the target's own equal = 1.  place_sum_kernel and the metric pass of fm_place.hip
// run unchanged on this call's parts; the count pass over the catalogue is not launched.
// A single huge list among many short ones walks on one wave per part: correct, but slow.
//
// (Included by module.hip after fm_topk.hip and fm_place.hip, whose merge, target, sum and metric passes it
// launches.)  No atomics, no host read, no allocation; graph-capturable and
// bitwise repeatable.
#include "fm_rank_common.h"

namespace fm {

struct ShortlistArgs : ProfileArgs {
  int k;
  SeenArgs sl;                          // the lists
  int parts;                            // topk::shortlist_plan
  unsigned long long* ws;               // select: [nq][parts][k] keys
  const int* target;                    // count: [nq]
  const float* st;                      // count: [nq] s_t (place_target_kernel)
  const int* flag;                      // count: [nq] 1: ranked
  int* part;                            // count: [nq][parts][2]
};

template <int J, bool COUNT>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ __launch_bounds__(kWave) void shortlist_kernel(ShortlistArgs a, int kcap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
  constexpr int kTiles = topk::kShortStep / topk::kTile;   // 4 candidate tiles per step
  constexpr bool kPrefetch = J <= 4;                       // two steps ahead (16 J VGPRs per step in flight)
  constexpr int TB = J <= 8 ? kTiles : 2;                  // tiles gathered at a time without prefetch

  const int lane = threadIdx.x;
  const int r = lane & 15, h = lane >> 4;
  const long long b = blockIdx.x;
  const long long q = b / a.parts;
  const int part = (int)(b - q * a.parts);

  // this part's run [pb, pe) of the query's window
  int b0, e0;
  csr_window(a.sl.off, a.sl.nnz, q, b0, e0);
  const long long run = topk::shortlist_run((long long)e0 - b0, a.parts);
  const long long pb = b0 + part * run;
  const long long pe = pb + run < e0 ? pb + run : e0;

  bool ranked = true;
  int tq = -1;
  float stq = 0.f;
  if constexpr (COUNT) {
    ranked = a.flag[q] != 0;
    tq = a.target[q];
    stq = a.st[q];
  }
  if (pb >= pe || !ranked) {   // (wave-uniform) nothing to walk: the slot is written all the same
    if constexpr (COUNT) {
      if (lane == 0) {
        int* o = a.part + b * 2;
        o[0] = 0;
        o[1] = ranked && part == 0 ? 1 : 0;
      }
    } else {
      for (int t = lane; t < a.k; t += kWave) a.ws[b * a.k + t] = 0ull;
    }
    return;
  }

  // A operands: the query's row (load_operands), the same in all 16 rows
  f32x4 qa[J];
  load_operands<J>(a.Q + q * a.q_stride + 4 * h, h, a.Kp, qa);
  const float qbq = a.qb[q];

  // this lane's candidate of the step at p0: entry p0 + lane, -1 past the run's end or outside [0, nc)
  const auto load_idx = [&](long long p0) {
    const long long p = p0 + lane;
    int c = -1;
    if (p < pe) {
      c = a.sl.idx[p];
      if (c < 0 || c >= a.nc) c = -1;
    }
    return c;
  };
  // B operands of the tiles T0 .. T0 + NT - 1 of a step whose lanes hold the candidates cl: lane (r, h) loads the
  // row of entry 16 t + r, columns as on the query side (no candidate: no load, zeros)
  const auto gather = [&](int cl, int T0, auto& v) {
    constexpr int NT = sizeof(v) / sizeof(v[0]);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int ct = __builtin_amdgcn_ds_bpermute((topk::kTile * (T0 + t) + r) << 2, cl);
      load_operands<J>(a.C + (long long)(ct < 0 ? 0 : ct) * a.c_stride + 4 * h, h, a.Kp, v[t], ct >= 0);
    }
  };
  // acc[T0 + t] += the tiles' products, the accumulators independent of each other
  const auto multiply = [&](f32x4 (&acc)[kTiles], int T0, const auto& v) {
    constexpr int NT = sizeof(v) / sizeof(v[0]);
#pragma unroll
    for (int g = 0; g < J; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[T0 + t] = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], v[t][g][e], acc[T0 + t], 0, 0, 0);
  };

  unsigned long long* buf = reinterpret_cast<unsigned long long*>(topk_smem);  // [cap] (select)
  const int cap = 2 * kcap;  // kcap >= 64: a step appends up to 64 keys
  unsigned long long* thr_s = buf + cap;
  int* cnt_s = reinterpret_cast<int*>(thr_s + 1);
  unsigned long long thr = 0ull;
  int gt = 0, eq = 0;
  if constexpr (!COUNT) {
    if (lane == 0) {
      *thr_s = 0ull;
      *cnt_s = 0;
    }
    __syncthreads();
  }

  int c1 = -1, c2 = -1;               // the candidates of the next step and of the one after it
  f32x4 nv[kPrefetch ? kTiles : 1][J];
  float ncb = 0.f;
  if constexpr (kPrefetch) {
    c1 = load_idx(pb);
    c2 = load_idx(pb + topk::kShortStep);
    gather(c1, 0, nv);
    ncb = c1 >= 0 ? a.cb[c1] : 0.f;
  }

  for (long long p0 = pb; p0 < pe; p0 += topk::kShortStep) {
    f32x4 acc[kTiles];
#pragma unroll
    for (int t = 0; t < kTiles; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    int c;
    float cbv;
    if constexpr (kPrefetch) {
      f32x4 v[kTiles][J];
#pragma unroll
      for (int t = 0; t < kTiles; ++t)
#pragma unroll
        for (int g = 0; g < J; ++g) v[t][g] = nv[t][g];
      c = c1;
      cbv = ncb;
      c1 = c2;
      c2 = load_idx(p0 + 2 * topk::kShortStep);
      if (p0 + topk::kShortStep < pe) {
        gather(c1, 0, nv);
        ncb = c1 >= 0 ? a.cb[c1] : 0.f;
      }
      multiply(acc, 0, v);
    } else {
      c = load_idx(p0);
      cbv = c >= 0 ? a.cb[c] : 0.f;
#pragma unroll
      for (int T0 = 0; T0 < kTiles; T0 += TB) {
        f32x4 v[TB][J];
        gather(c, T0, v);
        multiply(acc, T0, v);
      }
    }
    // tile h's score in this lane's column r: entry 16 h + r, this lane's own
    const float dot = h == 0 ? acc[0][0] : h == 1 ? acc[1][0] : h == 2 ? acc[2][0] : acc[3][0];
    const float s = score_of(qbq, cbv, dot);
    if constexpr (COUNT) {
      const bool on = c >= 0 && c != tq;
      gt += (int)(on && s > stq);
      eq += (int)(on && s == stq);
    } else {
      const unsigned long long key = c >= 0 ? topk::make_key(__float_as_uint(s), (uint32_t)c) : 0ull;
      thr = select_append_row(buf, cnt_s, thr_s, key, thr, kcap, a.k, lane);
    }
  }

  if constexpr (COUNT) {
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
      gt += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, gt);
      eq += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, eq);
    }
    if (lane == 0) {
      int* o = a.part + b * 2;
      o[0] = gt;
      o[1] = eq + (part == 0 ? 1 : 0);
    }
  } else {
    // the part's best k keys, best first, 0 where it had fewer
    topk_compact_rows(buf, cap, a.k, 1, cnt_s, thr_s, lane);
    for (int t = lane; t < a.k; t += kWave) a.ws[b * a.k + t] = buf[t];
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
inline long long shortlist_select_bytes(long long nq, int parts, int k) {
  return nq * parts * k * (long long)sizeof(unsigned long long);
}
// Workspace bytes that serve both a top-k call of k results and a place call of any cutoffs on lists of nnz entries.
inline long long shortlist_workspace_bytes(long long nq, long long nnz, long long nc, int k) {
  const int parts = topk::shortlist_plan(nq, nnz, nc);
  const long long s = shortlist_select_bytes(nq, parts, k), c = place_layout_bytes(nq, parts, kRankMaxCutoffs);
  return s > c ? s : c;
}

template <bool COUNT>
inline int launch_shortlist_walk(const ShortlistArgs& a, hipStream_t stream) {
  const long long blocks = a.nq * a.parts;
  if (blocks >= (1ll << 31)) return -1;
  const int kc = COUNT ? 0 : topk_kcap(a.k, kWave);
  const size_t lds = COUNT ? 0 : topk_lds_bytes(1, kc);
  if (dispatch_groups(a.Kp, [&](auto j) {
        hipLaunchKernelGGL((shortlist_kernel<decltype(j)::value, COUNT>), dim3((unsigned)blocks), dim3(kWave), lds,
                           stream, a, kc);
      }))
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// idx / score [nq, k]: the k best of every query's list `sl`.  -1: bad arguments; -2: workspace too small.
inline int launch_topk_shortlist(TopkArgs a, SeenArgs sl, size_t ws_bytes, hipStream_t stream) {
  long long qtiles = 0, blocks = 0;
  if (topk_prepare(a, qtiles, blocks) || !seen_args_ok(sl)) return -1;
  if (a.nq == 0) return 0;
  a.parts = topk::shortlist_plan(a.nq, sl.nnz, a.nc);
  if ((long long)ws_bytes < shortlist_select_bytes(a.nq, a.parts, a.k)) return -2;
  ShortlistArgs s{};
  static_cast<ProfileArgs&>(s) = a;
  s.k = a.k; s.sl = sl; s.parts = a.parts; s.ws = a.ws;
  if (const int rc = launch_shortlist_walk<false>(s, stream)) return rc;
  return launch_topk_merge(a, stream);
}

// counts [nq, 2] and the record of nq >= 1 queries, each against its list `sl` and its target.  Codes as launch_place.
inline int launch_place_shortlist(PlaceArgs a, SeenArgs sl, const int* k, int nk, void* rec, void* ws, size_t ws_bytes,
                                  hipStream_t st) {
  if (!place_args_ok(a, ws) || !seen_args_ok(sl)) return -1;
  if (!rank_cutoffs_ok(k, nk)) return -7;
  a.parts = topk::shortlist_plan(a.nq, sl.nnz, a.nc);
  if ((long long)ws_bytes < place_layout_bytes(a.nq, a.parts, nk)) return -2;
  place_carve(a, ws, nk);
  const unsigned qgrid = (unsigned)((a.nq + kPlaceThreads - 1) / kPlaceThreads);
  hipLaunchKernelGGL(place_target_kernel, dim3(qgrid), dim3(kPlaceThreads), 0, st, a);
  ShortlistArgs s{};
  static_cast<ProfileArgs&>(s) = a;
  s.sl = sl; s.parts = a.parts; s.target = a.target; s.st = a.st; s.flag = a.flag; s.part = a.part;
  if (const int rc = launch_shortlist_walk<true>(s, st)) return rc;
  launch_place_sum(a.part, a.counts, a.nq, a.parts, st);
  if (hipGetLastError() != hipSuccess) return -3;
  const long long mbytes = place_metrics_workspace_bytes(a.nq, nk);
  return launch_place_metrics(a.counts, a.nq, k, nk, rec, mbytes ? ws : nullptr, (size_t)mbytes, st);
}

}  // namespace fm
