// Recommend and place with every query's already-seen candidates left out (the standard leave-one-out protocol
// ranks the held-out item among the items the user has not interacted with; the reference only scores examples).
//
// A seen list per query is a CSR pair (SeenArgs, fm_topk.hip): off int32 [nq + 1], idx int32 [nnz], a query's
// indices strictly ascending in [0, nc).  E_q is query q's set; the score s(q, c) is fm_topk.hip's, bit for bit.
//   top-k: row q holds the k greatest keys over c not in E_q (-1 / -inf where fewer than k remain);
//   place: greater / equal count the c not in E_q \ {t} -- the query's own target always competes.
// The lists are checked by the caller (ops/kernels.py).  A malformed list gives unspecified membership but no read
// out of bounds: a query's window is clamped to [0, nnz], a binary search never leaves its window, and the place
// pass skips an index outside [0, nc).
//
// 1. topk_slab_kernel<J, true>: fm_topk.hip's slab kernel instantiated with SEEN.  At its start every lane finds, for
//    each of its 4 result rows, the part [slo, shi) of the row's list that lies inside the workgroup's slab (two
//    lower-bound searches, kept in registers).  The hot path stays one compare per score: membership -- a binary
//    search of idx[slo, shi) -- is tested only for a key that already beats its row's threshold, and only when the
//    row has a seen candidate in the slab.  A hit clears the lane's win flag before the ballot, so a seen candidate
//    never enters the LDS buffer and never raises a threshold; append, compaction and topk_merge_kernel are as
//    they were.  Cost: the window search per workgroup, then (#keys that beat the threshold + #seen candidates of
//    the slab that beat it) x log2(window).  Degenerate case: a list that covers most of the catalogue keeps the
//    thresholds at 0, so every candidate pays a search -- correct, but slow.
// 2. place_seen_kernel: a correction after place_sum_kernel; the matrix-core count pass is untouched.  Counts over
//    all candidates minus counts over the seen ones is exact, both being integers over the same exact fp32 scores.
//    A group of 16 lanes takes one query (four queries to a wave) and strides over its list; a lane computes
//    s(q, e) with place_target_kernel's fmaf chain in pi's order from 16-byte row fragments -- the chain the matrix
//    instruction is -- compares it with s_t from the workspace, and skips e == target[q]; unranked queries are
//    skipped whole.  The group's (greater, equal) are added across its lanes in a fixed pattern and its first lane
//    subtracts them from counts[q]: one writer per query, no atomics, no host read.  A long list is walked by its
//    16 lanes.  Compiled, like the other fp32 score kernels of fm_place.hip, without the packed fp32 instructions.
//
// (Included by module.hip after fm_place.hip -- PlaceArgs, FM_PLACE_FN.)  Graph-capturable and bitwise repeatable.
#include "fm_common.h"

namespace fm {

inline bool seen_args_ok(const SeenArgs& sn) { return sn.off && sn.nnz >= 0 && (sn.idx || sn.nnz == 0); }

// launch_topk with the lists `sn`: the same plan, workspace and merge pass.
inline int launch_topk_seen(TopkArgs a, SeenArgs sn, hipStream_t stream) {
  long long qtiles = 0, blocks = 0;
  if (topk_prepare(a, qtiles, blocks) || !seen_args_ok(sn)) return -1;
  if (a.nq == 0) return 0;
  const int kc1 = topk_kcap(a.k, 32);
  const size_t lds1 = topk_lds_bytes(topk::kTile, kc1);
#define FM_SEEN_CASE(JJ)                                                                                     \
  case JJ:                                                                                                   \
    hipLaunchKernelGGL((topk_slab_kernel<JJ, true>), dim3((unsigned)blocks), dim3(kWave), lds1, stream, a, qtiles, \
                       kc1, so);                                                                             \
    break;
  SeenOpt<true> so;
  static_cast<SeenArgs&>(so) = sn;
  switch (topk::groups(a.Kp)) {
    FM_SEEN_CASE(1) FM_SEEN_CASE(2) FM_SEEN_CASE(3) FM_SEEN_CASE(4) FM_SEEN_CASE(5) FM_SEEN_CASE(6)
    FM_SEEN_CASE(7) FM_SEEN_CASE(8) FM_SEEN_CASE(9) FM_SEEN_CASE(10) FM_SEEN_CASE(11) FM_SEEN_CASE(12)
    FM_SEEN_CASE(13) FM_SEEN_CASE(14) FM_SEEN_CASE(15) FM_SEEN_CASE(16)
    default: return -1;
  }
#undef FM_SEEN_CASE
  return launch_topk_merge(a, stream);
}

constexpr int kSeenLanes = 16;  // lanes per query of place_seen_kernel

__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void place_seen_kernel(PlaceArgs a, SeenArgs sn) {
  const int tid = threadIdx.x;
  const int sub = tid & (kSeenLanes - 1);
  const long long q = ((long long)blockIdx.x * kPlaceThreads + tid) / kSeenLanes;
  const bool ranked = q < a.nq && a.flag[q] != 0;   // (uniform over the 16 lanes)
  int gt = 0, eq = 0;
  if (ranked) {
    const int o0 = sn.off[q], o1 = sn.off[q + 1];
    const int b0 = o0 < 0 ? 0 : o0 > sn.nnz ? sn.nnz : o0;
    const int e0 = o1 < b0 ? b0 : o1 > sn.nnz ? sn.nnz : o1;
    const int t = a.target[q];
    const float stq = a.st[q], qbq = a.qb[q];
    const float* qr = a.Q + q * a.q_stride;
    const int G = (a.Kp + topk::kGroup - 1) / topk::kGroup;
    for (int p = b0 + sub; p < e0; p += kSeenLanes) {
      const int c = sn.idx[p];
      if (c < 0 || c >= a.nc || c == t) continue;
      const float* cr = a.C + (long long)c * a.c_stride;
      float dot = 0.f;
      for (int g = 0; g < G; ++g) {
        // the group's 4 fragments of both rows (zeros past Kp: fmaf(0, 0, dot) == dot, ../topk_order.h)
        f32x4 qf[4], cf[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          qf[h] = cf[h] = f32x4{0.f, 0.f, 0.f, 0.f};
          if (topk::kGroup * g + 4 * h < a.Kp) {
            qf[h] = *reinterpret_cast<const f32x4*>(qr + topk::kGroup * g + 4 * h);
            cf[h] = *reinterpret_cast<const f32x4*>(cr + topk::kGroup * g + 4 * h);
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int h = 0; h < 4; ++h) dot = __builtin_fmaf(qf[h][e], cf[h][e], dot);
      }
      const float s = ((qbq + a.cb[c]) + dot) + 0.f;
      gt += (int)(s > stq);
      eq += (int)(s == stq);
    }
  }
  const int lane = tid & (kWave - 1);
#pragma unroll
  for (int m = 1; m < kSeenLanes; m <<= 1) {
    gt += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, gt);
    eq += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, eq);
  }
  if (ranked && sub == 0 && (gt | eq)) {
    a.counts[2 * q] -= gt;
    a.counts[2 * q + 1] -= eq;
  }
}

// After place_sum_kernel on the same stream: counts[q] -= the (greater, equal) of q's seen candidates.
inline int launch_place_seen(const PlaceArgs& a, const SeenArgs& sn, hipStream_t st) {
  if (!seen_args_ok(sn)) return -1;
  const long long threads = a.nq * kSeenLanes;
  hipLaunchKernelGGL(place_seen_kernel, dim3((unsigned)((threads + kPlaceThreads - 1) / kPlaceThreads)),
                     dim3(kPlaceThreads), 0, st, a, sn);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fm
