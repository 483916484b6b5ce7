// Top-k ranking of a candidate set per query from FM profiles (the reference only scores examples).
//
//   s(q, c) = ((qb[q] + cb[c]) + dot(q, c)) + 0.f,   dot = fmaf chain over the columns in the order pi(Kp)
//
// (../topk_order.h: pi, the 64-bit selection key and the slab plan, shared with the CPU twin), and row q of
// the output holds the k candidates of greatest s, equal s by ascending candidate: the k greatest keys.
// Exact fp32 and bitwise reproducible: gfx950's fp32-input v_mfma_f32_16x16x4_f32 is a k-ordered fmaf
// chain with one rounding per product, there are no atomics, and keys are unique, so neither the slab cut
// nor any order of arrival can change a result.  The [nq, nc] score matrix never reaches memory.
//
// Phase 1, topk_slab_kernel: one wave (a 64-thread workgroup) per (16-query tile, slab).  The wave keeps
// the tile's A operands in registers for the whole pass (4 VGPRs per 16 columns) and walks its slab two
// 16-candidate tiles at a time: two independent accumulators cover the instruction's dependent latency,
// and profiles of Kp <= 64 fetch the next two tiles meanwhile.  Each lane loads 16 bytes of a candidate
// row per column group -- the same load on the query side, so both operands see the same pi -- and then
// holds 4 queries x 1 candidate of each tile.  Selection: per query row the current k-th key is the
// threshold (0 until k keys are known); lanes whose key beats it are found by ballot and appended to the
// row's LDS buffer of 2 kcap keys (kcap = max(32, pow2 >= k)); when a buffer passes kcap entries, all the
// tile's buffers are sorted (bitonic, in LDS, the rows in the same passes) and cut to their best k, which
// raises every threshold.  After warm-up a tile rarely has a winner and costs one compare per score.  The
// wave ends by writing every row's best k keys (0 = none) to the workspace [nq][parts][k].
// Phase 2, topk_merge_kernel: one wave per query streams its parts x k keys through the same threshold /
// buffer selection and decodes the k best into idx / score (-1 / -inf where nc < k).
// No host synchronisation, no allocation: the workspace comes from the caller (graph-capturable).
// topk_slab_kernel<J, true> (fm_seen.hip) is the same pass with each query's already-seen candidates left out; the
// plain instantiation takes no list and has no instruction for it.
// The operand load, the score and the LDS selection are fm_rank_common.h's, shared with the other
// ranking kernels.
#include "fm_rank_common.h"

namespace fm {

struct TopkArgs : ProfileArgs {
  int k;
  long long slab; int parts;            // topk::plan
  unsigned long long* ws;               // [nq][parts][k] keys
  int* idx;                             // [nq, k]
  float* score;                         // [nq, k]
};

// The lists as a kernel argument: nothing at all for the plain instantiation.
template <bool SEEN> struct SeenOpt {};
template <> struct SeenOpt<true> : SeenArgs {};

// SEEN (launched by fm_seen.hip) leaves out every row's listed candidates; the plain instantiation has no code for it.
template <int J, bool SEEN = false>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ __launch_bounds__(kWave) void topk_slab_kernel(TopkArgs a, long long qtiles, int kcap, SeenOpt<SEEN> sn) {
  extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
  const int cap = 2 * kcap;
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(topk_smem);       // [16][cap]
  unsigned long long* thr_s = buf + topk::kTile * cap;                                // [16]
  int* cnt_s = reinterpret_cast<int*>(thr_s + topk::kTile);                           // [16]

  const int lane = threadIdx.x;
  const int r = lane & 15, h = lane >> 4;
  const long long b = blockIdx.x;
  const long long qt = b % qtiles;             // consecutive workgroups share a slab (cache reuse)
  const int part = (int)(b / qtiles);
  const long long q0 = qt * topk::kTile;
  const int vrows = a.nq - q0 < topk::kTile ? (int)(a.nq - q0) : topk::kTile;  // rows of real queries
  const long long c_begin = (long long)part * a.slab;
  const long long c_end = c_begin + a.slab < a.nc ? c_begin + a.slab : a.nc;

  if (lane < topk::kTile) {
    thr_s[lane] = 0ull;
    cnt_s[lane] = 0;
  }
  __syncthreads();

  // A operands: query row q0 + r (load_operands)
  f32x4 qa[J];
  {
    const long long qr = q0 + r < a.nq ? q0 + r : a.nq - 1;
    load_operands<J>(a.Q + qr * a.q_stride + 4 * h, h, a.Kp, qa);
  }
  // this lane's 4 result rows: queries q0 + 4 h + i
  float qbv[4];
  bool qok[4];
  unsigned long long thr[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long q = q0 + 4 * h + i;
    qok[i] = q < a.nq;
    qbv[i] = qok[i] ? a.qb[q] : 0.f;
    thr[i] = 0ull;
  }
  // SEEN: the part [slo, shi) of each of this lane's rows' lists that lies inside the slab
  int slo[4] = {0, 0, 0, 0}, shi[4] = {0, 0, 0, 0};
  if constexpr (SEEN) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!qok[i]) continue;
      int b0, e0;
      csr_window(sn.off, sn.nnz, q0 + 4 * h + i, b0, e0);
      slo[i] = seen_lower_bound(sn.idx, b0, e0, (int)c_begin);
      shi[i] = seen_lower_bound(sn.idx, slo[i], e0, (int)c_end);
    }
  }

  // B operands of the two candidate tiles at c0: rows c0 + r and c0 + 16 + r (clamped into the slab: loads
  // stay in bounds, the clamped lanes' scores are dropped), columns as on the query side
  const auto load_pair = [&](long long c0, f32x4 (&va)[J], f32x4 (&vb)[J], float& cba, float& cbb) {
    const long long ca = c0 + r, cbi = c0 + topk::kTile + r;
    const long long la = ca < c_end ? ca : c_end - 1, lb = cbi < c_end ? cbi : c_end - 1;
    load_operands<J>(a.C + la * a.c_stride + 4 * h, h, a.Kp, va);
    load_operands<J>(a.C + lb * a.c_stride + 4 * h, h, a.Kp, vb);
    cba = a.cb[la];
    cbb = a.cb[lb];
  };
  // Narrow profiles (Kp <= 64) have the registers to fetch the next pair of tiles while this one is
  // multiplied and ranked; wider ones load in place and lean on the other waves of the SIMD.
  constexpr bool kPrefetch = J <= 4;
  f32x4 va[J], vb[J], na[J], nb[J];
  float cba = 0.f, cbb = 0.f, ncba = 0.f, ncbb = 0.f;
  if (kPrefetch && c_begin < c_end) load_pair(c_begin, na, nb, ncba, ncbb);

  for (long long c0 = c_begin; c0 < c_end; c0 += 2 * topk::kTile) {
    const long long ca = c0 + r, cbi = c0 + topk::kTile + r;
    const bool oka = ca < c_end, okb = cbi < c_end;
    if constexpr (kPrefetch) {
#pragma unroll
      for (int g = 0; g < J; ++g) {
        va[g] = na[g];
        vb[g] = nb[g];
      }
      cba = ncba;
      cbb = ncbb;
      if (c0 + 2 * topk::kTile < c_end) load_pair(c0 + 2 * topk::kTile, na, nb, ncba, ncbb);
    } else {
      load_pair(c0, va, vb, cba, cbb);
    }
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < J; ++g) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], va[g][e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], vb[g][e], acc1, 0, 0, 0);
      }
    }
    // keys of this lane's 4 x 2 scores; the rare winners go to the rows' buffers
#pragma unroll
    for (int tile = 0; tile < 2; ++tile) {
      const f32x4 acc = tile ? acc1 : acc0;
      const float cbv = tile ? cbb : cba;
      const bool cok = tile ? okb : oka;
      const uint32_t c32 = (uint32_t)(tile ? cbi : ca);
      unsigned long long key[4];
      bool win[4];
      bool any = false;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float s = score_of(qbv[i], cbv, acc[i]);
        key[i] = topk::make_key(__float_as_uint(s), c32);
        win[i] = cok && qok[i] && key[i] > thr[i];
        any = any || win[i];
      }
      bool some = __any(any);
      if constexpr (SEEN) {
        // Off the hot path: only a tile with a would-be winner looks at the lists.  A winner that its row has seen
        // is cleared before the ballots, so it never reaches the buffer or a threshold.
        if (some) {
          any = false;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (win[i] && slo[i] < shi[i] && seen_contains(sn.idx, slo[i], shi[i], (int)c32)) win[i] = false;
            any = any || win[i];
          }
          some = __any(any);
        }
      }
      if (some) {
        // every lane's 4 rows are different (4 h + i): all counts are read, then the keys and counts written
        int pos[4], newc[4];
        bool full = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const unsigned grp = (unsigned)(__ballot(win[i]) >> (16 * h)) & 0xffffu;
          const int n0 = cnt_s[4 * h + i];
          pos[i] = n0 + __popc(grp & ((1u << r) - 1u));
          newc[i] = n0 + __popc(grp);
          full = full || newc[i] > kcap;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          if (win[i]) buf[(4 * h + i) * cap + pos[i]] = key[i];
          if (r == 0) cnt_s[4 * h + i] = newc[i];
        }
        __syncthreads();
        // (count <= kcap before a tile, a tile adds <= 16 per row, kcap >= 32: the buffer cannot overflow.)
        // One full row has all the tile's rows sorted and cut in the same passes, which refreshes every threshold.
        if (__any(full)) {
          topk_compact_rows(buf, cap, a.k, vrows, cnt_s, thr_s, lane);
#pragma unroll
          for (int i = 0; i < 4; ++i) thr[i] = thr_s[4 * h + i];
        }
      }
    }
  }

  // every row's best k keys, best first, 0 where the slab had fewer
  topk_compact_rows(buf, cap, a.k, vrows, cnt_s, thr_s, lane);
  for (int row = 0; row < vrows; ++row) {
    unsigned long long* out = a.ws + ((q0 + row) * a.parts + part) * a.k;
    for (int t = lane; t < a.k; t += kWave) out[t] = buf[row * cap + t];
  }
}

__global__ __launch_bounds__(kWave) void topk_merge_kernel(TopkArgs a, int kcap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
  const int cap = 2 * kcap;  // kcap >= 64: a step appends up to 64 keys
  unsigned long long* buf = reinterpret_cast<unsigned long long*>(topk_smem);  // [cap]
  unsigned long long* thr_s = buf + cap;
  int* cnt_s = reinterpret_cast<int*>(thr_s + 1);
  const int lane = threadIdx.x;
  const long long q = blockIdx.x;
  if (lane == 0) {
    *thr_s = 0ull;
    *cnt_s = 0;
  }
  __syncthreads();
  const long long n = (long long)a.parts * a.k;
  const unsigned long long* in = a.ws + q * n;
  unsigned long long thr = 0ull;
  for (long long t0 = 0; t0 < n; t0 += kWave) {
    const long long t = t0 + lane;
    thr = select_append_row(buf, cnt_s, thr_s, t < n ? in[t] : 0ull, thr, kcap, a.k, lane);
  }
  topk_compact_rows(buf, cap, a.k, 1, cnt_s, thr_s, lane);
  for (int t = lane; t < a.k; t += kWave) {
    const unsigned long long key = buf[t];
    a.idx[q * a.k + t] = topk::key_index(key);
    a.score[q * a.k + t] = __uint_as_float(topk::key_score_bits(key));
  }
}

// Workspace bytes of a call (topk::plan's parts lists of k keys per query).
inline long long topk_workspace_bytes(long long nq, long long nc, int k) {
  const topk::Plan p = topk::plan(nq, nc, k);
  return nq * p.parts * k * (long long)sizeof(unsigned long long);
}

// Checks a call's sizes and fills in its plan and phase 1's grid (shared with fm_seen.hip).  -1: bad arguments.
inline int topk_prepare(TopkArgs& a, long long& qtiles, long long& blocks) {
  if (a.k < 1 || a.k > topk::kMaxK || !profile_args_ok(a)) return -1;
  const topk::Plan p = topk::plan(a.nq, a.nc, a.k);
  a.slab = p.slab;
  a.parts = p.parts;
  qtiles = (a.nq + topk::kTile - 1) / topk::kTile;
  blocks = qtiles * a.parts;
  return blocks >= (1ll << 31) ? -1 : 0;
}

inline int launch_topk_merge(const TopkArgs& a, hipStream_t stream) {
  const int kc2 = topk_kcap(a.k, kWave);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)a.nq), dim3(kWave), topk_lds_bytes(1, kc2), stream, a, kc2);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

// Both phases of a call; `sn`: the lists to leave out (fm_seen.hip) or nothing.
template <bool SEEN>
inline int launch_topk_slabs(TopkArgs a, SeenOpt<SEEN> sn, hipStream_t stream) {
  long long qtiles = 0, blocks = 0;
  if (topk_prepare(a, qtiles, blocks)) return -1;
  if (a.nq == 0) return 0;
  const int kc1 = topk_kcap(a.k, 32);
  const size_t lds1 = topk_lds_bytes(topk::kTile, kc1);
  if (dispatch_groups(a.Kp, [&](auto j) {
        hipLaunchKernelGGL((topk_slab_kernel<decltype(j)::value, SEEN>), dim3((unsigned)blocks), dim3(kWave), lds1,
                           stream, a, qtiles, kc1, sn);
      }))
    return -1;
  return launch_topk_merge(a, stream);
}

inline int launch_topk(const TopkArgs& a, hipStream_t stream) {
  return launch_topk_slabs<false>(a, SeenOpt<false>{}, stream);
}

}  // namespace fm
