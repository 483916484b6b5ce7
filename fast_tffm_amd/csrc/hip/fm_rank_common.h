// What the ranking kernels share (fm_topk, fm_seen, fm_place, fm_shortlist, fm_place_multi, fm_diversify): the
// profile arguments and their check, the dispatch on the profile width, the operand load, the scalar score chain,
// the CSR window, list membership and the single-row selection.
//
//   s(q, c) = ((qb[q] + cb[c]) + dot(q, c)) + 0.f,   dot = fmaf chain over the columns in the order pi(Kp)
//
// (../topk_order.h).  Every path of every kernel computes s bit for bit the same -- the matrix instruction
// v_mfma_f32_16x16x4_f32 is that chain, the scalar kernels run it with score_chain, the CPU twin with
// topk::for_each_col -- and it does so because the pieces below are defined once.
//
// The place kernels are compiled without the packed fp32 instructions, and a function compiled for other target
// features than its caller's is called, not inlined.  So every __device__ function here that such a kernel uses
// carries FM_PLACE_FN itself and spells pi's column out (topk::col has the default features); a function with fewer
// features still inlines into the default-feature kernels, so one definition serves both.
#pragma once
#include <type_traits>
#include "fm_common.h"
#include "../place_order.h"

namespace fm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#if defined(__HIP_DEVICE_COMPILE__)
#define FM_PLACE_FN __attribute__((target("no-packed-fp32-ops")))
#else
#define FM_PLACE_FN
#endif
// (The HIP header's wrappers have the default features too: the place kernels use the compiler's builtins directly.)
#define FM_PLACE_BARRIER()                              \
  do {                                                  \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); \
    __builtin_amdgcn_s_barrier();                       \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); \
  } while (0)

constexpr int kPlaceThreads = place::kWaves * kWave;

// ---- arguments ------------------------------------------------------------------------------------------------
struct ProfileArgs {
  long long nq, nc;
  int Kp;
  const float* Q; long long q_stride;   // [nq, Kp], row stride in elements (16-byte aligned rows)
  const float* C; long long c_stride;   // [nc, Kp]
  const float* qb;                      // [nq]
  const float* cb;                      // [nc]
};

inline bool profile_sizes_ok(long long nq, long long nc, int Kp) {
  return Kp >= 4 && Kp <= topk::kMaxKp && Kp % 4 == 0 && nq >= 0 && nq < (1ll << 31) && nc >= 0 && nc < (1ll << 31);
}
inline bool profile_args_ok(const ProfileArgs& p) { return profile_sizes_ok(p.nq, p.nc, p.Kp); }
// ... of a call that needs a query and a candidate, and so all four arrays
inline bool profile_rows_ok(const ProfileArgs& p) {
  return profile_args_ok(p) && p.nq >= 1 && p.nc >= 1 && p.Q && p.C && p.qb && p.cb;
}

// f(std::integral_constant<int, J>) for the J = topk::groups(Kp) column groups of 16 of a profile width: Kp in
// (16 (J - 1), 16 J].  -1: no such width.
template <typename F>
inline int dispatch_groups(int Kp, F&& f) {
#define FM_GROUPS_CASE(JJ) \
  case JJ:                 \
    f(std::integral_constant<int, JJ>{}); \
    return 0;
  switch (topk::groups(Kp)) {
    FM_GROUPS_CASE(1) FM_GROUPS_CASE(2) FM_GROUPS_CASE(3) FM_GROUPS_CASE(4) FM_GROUPS_CASE(5) FM_GROUPS_CASE(6)
    FM_GROUPS_CASE(7) FM_GROUPS_CASE(8) FM_GROUPS_CASE(9) FM_GROUPS_CASE(10) FM_GROUPS_CASE(11) FM_GROUPS_CASE(12)
    FM_GROUPS_CASE(13) FM_GROUPS_CASE(14) FM_GROUPS_CASE(15) FM_GROUPS_CASE(16)
    default: return -1;
  }
#undef FM_GROUPS_CASE
}

// ---- operands ---------------------------------------------------------------------------------------------------
// Lane (r, h) of a wave holds columns 16 g + 4 h .. + 3 of row r, one 16-byte load per column group g, zeros for a
// group cut short by Kp (fmaf(0, 0, dot) == dot, ../topk_order.h); element e of group g is the lane's operand of
// matrix instruction 4 g + e.  The same load serves the A and the B side, so both see the same pi.
// `row_at_4h`: the row's column 4 h.
// `there`: false for a row that is absent -- zeros, and no load.
FM_PLACE_FN __device__ inline f32x4 load_fragment(const float* row_at_4h, int g, int h, int Kp, bool there = true) {
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (there && topk::kGroup * g + 4 * h < Kp) v = *reinterpret_cast<const f32x4*>(row_at_4h + topk::kGroup * g);
  return v;
}
template <int J>
FM_PLACE_FN __device__ inline void load_operands(const float* row_at_4h, int h, int Kp, f32x4 (&v)[J],
                                                 bool there = true) {
#pragma unroll
  for (int g = 0; g < J; ++g) v[g] = load_fragment(row_at_4h, g, h, Kp, there);
}

// ---- the score on a scalar path -------------------------------------------------------------------------------
// dot(q, c) from +0 in pi's order -- g, then e, then h: the chain the matrix instruction is -- from the 16-byte
// fragments a lane of the matrix path loads (rows are 16-byte aligned and their stride a multiple of 4).  Nothing
// else is exact against the matrix path.
FM_PLACE_FN __device__ inline float score_chain(const float* qr, const float* cr, int Kp) {
  float dot = 0.f;
  const int G = (Kp + topk::kGroup - 1) / topk::kGroup;
  for (int g = 0; g < G; ++g) {
    f32x4 qf[4], cf[4];
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      qf[h] = load_fragment(qr + 4 * h, g, h, Kp);
      cf[h] = load_fragment(cr + 4 * h, g, h, Kp);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int h = 0; h < 4; ++h) dot = __builtin_fmaf(qf[h][e], cf[h][e], dot);
  }
  return dot;
}
// s from the base scores and dot (the matrix path's accumulator element or score_chain's result)
FM_PLACE_FN __device__ inline float score_of(float qb, float cb, float dot) { return ((qb + cb) + dot) + 0.f; }

// ---- per-query lists (CSR) ------------------------------------------------------------------------------------
// Lists of candidates per query (seen candidates, shortlists, targets): a query's indices strictly ascending in
// [0, nc).
struct SeenArgs {
  const int* off;   // [nq + 1]
  const int* idx;   // [nnz]
  int nnz;
};
inline bool seen_args_ok(const SeenArgs& sn) { return sn.off && sn.nnz >= 0 && (sn.idx || sn.nnz == 0); }

// Query q's window [b0, e0) of the entries, clamped into [0, nnz]: a malformed list cannot lead a read out of bounds.
FM_PLACE_FN __device__ inline void csr_window(const int* off, long long nnz, long long q, int& b0, int& e0) {
  const int o0 = off[q], o1 = off[q + 1];
  b0 = o0 < 0 ? 0 : o0 > nnz ? (int)nnz : o0;
  e0 = o1 < b0 ? b0 : o1 > nnz ? (int)nnz : o1;
}
// The first position p of [lo, hi) with idx[p] >= v (hi if none).  Reads stay inside [lo, hi) whatever the order.
FM_PLACE_FN __device__ inline int seen_lower_bound(const int* idx, int lo, int hi, int v) {
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (idx[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}
FM_PLACE_FN __device__ inline bool seen_contains(const int* idx, int lo, int hi, int v) {
  const int p = seen_lower_bound(idx, lo, hi, v);
  return p < hi && idx[p] == v;
}

// ---- selection: the k greatest keys of a row, in LDS ------------------------------------------------------------
// A row's buffer holds 2 kcap keys (kcap a power of two >= k and >= the most keys one step can append); next to
// the buffers lie one threshold (the row's current k-th key, 0 until k keys are known) and one count per row.
inline int topk_kcap(int k, int floor_) { return next_pow2(k < floor_ ? floor_ : k); }
inline size_t topk_lds_bytes(int rows, int kcap) {
  return (size_t)rows * (2 * kcap) * sizeof(unsigned long long) + rows * (sizeof(unsigned long long) + sizeof(int));
}

// Sort each of `rows` consecutive buffers of cap keys descending, all in the same passes (cap a power of two
// >= 2); every lane of the single-wave workgroup calls.
__device__ inline void topk_sort_rows(unsigned long long* buf, int cap, int rows, int lane) {
  const int half = cap >> 1;          // compare-exchanges per row and pass
  const int hs = __ffs(half) - 1;     // log2(half)
  for (int size = 2; size <= cap; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = lane; t < rows * half; t += kWave) {
        const int tt = t & (half - 1);
        const int i = 2 * tt - (tt & (stride - 1));
        unsigned long long* rb = buf + (t >> hs) * cap;
        const bool desc = (i & size) == 0;
        const unsigned long long x = rb[i], y = rb[i + stride];
        if ((x < y) == desc) {
          rb[i] = y;
          rb[i + stride] = x;
        }
      }
      __syncthreads();
    }
  }
}

// Sort `rows` buffers (cnt[row] entries each, the rest zeroed first) and cut every one that holds k or more
// keys to its best k: its count becomes k and its threshold the k-th key.  Wave-uniform call.
__device__ inline void topk_compact_rows(unsigned long long* buf, int cap, int k, int rows, int* cnt,
                                         unsigned long long* thr, int lane) {
  const int cs = __ffs(cap) - 1;
  __syncthreads();
  for (int t = lane; t < rows * cap; t += kWave)
    if ((t & (cap - 1)) >= cnt[t >> cs]) buf[t] = 0ull;
  __syncthreads();
  topk_sort_rows(buf, cap, rows, lane);
  if (lane < rows && cnt[lane] >= k) {
    cnt[lane] = k;
    thr[lane] = buf[lane * cap + k - 1];
  }
  __syncthreads();
}

// One step of the selection on a single row, a key per lane (0: none, it never wins) against the threshold `thr`:
// the lanes whose key beats it are found by ballot and appended to the row's buffer, which is cut to its best k
// when it passes kcap entries (kcap >= 64: a step appends up to 64 keys).  Returns the row's threshold after the
// step; a step without a winner touches no LDS.  Wave-uniform call.
__device__ inline unsigned long long select_append_row(unsigned long long* buf, int* cnt_s, unsigned long long* thr_s,
                                                       unsigned long long key, unsigned long long thr, int kcap, int k,
                                                       int lane) {
  const bool win = key > thr;
  const unsigned long long m = __ballot(win);
  if (m == 0ull) return thr;
  if (win) buf[*cnt_s + __popcll(m & ((1ull << lane) - 1ull))] = key;
  __syncthreads();
  if (lane == 0) *cnt_s += __popcll(m);
  __syncthreads();
  if (*cnt_s > kcap) topk_compact_rows(buf, 2 * kcap, k, 1, cnt_s, thr_s, lane);
  return *thr_s;
}

}  // namespace fm
