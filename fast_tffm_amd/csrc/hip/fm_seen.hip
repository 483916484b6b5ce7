// Recommend and place with every query's already-seen candidates left out (the standard leave-one-out protocol
// ranks the held-out item among the items the user has not interacted with; the reference only scores examples).
//
// A seen list per query is a CSR pair (SeenArgs, fm_rank_common.h): off int32 [nq + 1], idx int32 [nnz], a query's
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
//    s(q, e) with score_chain (fm_rank_common.h), as place_target_kernel does -- the chain the matrix
//    instruction is -- compares it with s_t from the workspace, and skips e == target[q]; unranked queries are
//    skipped whole.  The group's (greater, equal) are added across its lanes in a fixed pattern and its first lane
//    subtracts them from counts[q]: one writer per query, no atomics, no host read.  A long list is walked by its
//    16 lanes.  Compiled, like the other fp32 score kernels of fm_place.hip, without the packed fp32 instructions.
//
// (Included by module.hip after fm_topk.hip and fm_place.hip, whose kernels and arguments these passes extend.)
// Graph-capturable and bitwise repeatable.
#include "fm_rank_common.h"

namespace fm {

// launch_topk with the lists `sn`: the same plan, workspace and merge pass.
inline int launch_topk_seen(const TopkArgs& a, SeenArgs sn, hipStream_t stream) {
  if (!seen_args_ok(sn)) return -1;
  SeenOpt<true> so;
  static_cast<SeenArgs&>(so) = sn;
  return launch_topk_slabs<true>(a, so, stream);
}

constexpr int kSeenLanes = 16;  // lanes per query of place_seen_kernel

__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void place_seen_kernel(PlaceArgs a, SeenArgs sn) {
  const int tid = threadIdx.x;
  const int sub = tid & (kSeenLanes - 1);
  const long long q = ((long long)blockIdx.x * kPlaceThreads + tid) / kSeenLanes;
  const bool ranked = q < a.nq && a.flag[q] != 0;   // (uniform over the 16 lanes)
  int gt = 0, eq = 0;
  if (ranked) {
    int b0, e0;
    csr_window(sn.off, sn.nnz, q, b0, e0);
    const int t = a.target[q];
    const float stq = a.st[q], qbq = a.qb[q];
    const float* qr = a.Q + q * a.q_stride;
    for (int p = b0 + sub; p < e0; p += kSeenLanes) {
      const int c = sn.idx[p];
      if (c < 0 || c >= a.nc || c == t) continue;
      const float s = score_of(qbq, a.cb[c], score_chain(qr, a.C + (long long)c * a.c_stride, a.Kp));
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
