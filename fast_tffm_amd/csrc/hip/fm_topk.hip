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
#include "fm_common.h"
#include "../topk_order.h"

namespace fm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

struct TopkArgs {
  long long nq, nc;
  int Kp, k;
  const float* Q; long long q_stride;   // [nq, Kp], row stride in elements (16-byte aligned rows)
  const float* C; long long c_stride;   // [nc, Kp]
  const float* qb;                      // [nq]
  const float* cb;                      // [nc]
  long long slab; int parts;            // topk::plan
  unsigned long long* ws;               // [nq][parts][k] keys
  int* idx;                             // [nq, k]
  float* score;                         // [nq, k]
};

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

template <int J>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ __launch_bounds__(kWave) void topk_slab_kernel(TopkArgs a, long long qtiles, int kcap) {
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

  // A operands: query row q0 + r, columns 16 g + 4 h .. + 3 (zeros past Kp)
  f32x4 qa[J];
  {
    const long long qr = q0 + r < a.nq ? q0 + r : a.nq - 1;
    const float* qp = a.Q + qr * a.q_stride + 4 * h;
#pragma unroll
    for (int g = 0; g < J; ++g) {
      qa[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (topk::col(g, 0, h) < a.Kp) qa[g] = *reinterpret_cast<const f32x4*>(qp + topk::kGroup * g);
    }
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

  // B operands of the two candidate tiles at c0: rows c0 + r and c0 + 16 + r (clamped into the slab: loads
  // stay in bounds, the clamped lanes' scores are dropped), columns as on the query side
  const auto load_pair = [&](long long c0, f32x4 (&va)[J], f32x4 (&vb)[J], float& cba, float& cbb) {
    const long long ca = c0 + r, cbi = c0 + topk::kTile + r;
    const long long la = ca < c_end ? ca : c_end - 1, lb = cbi < c_end ? cbi : c_end - 1;
    const float* pa = a.C + la * a.c_stride + 4 * h;
    const float* pb = a.C + lb * a.c_stride + 4 * h;
#pragma unroll
    for (int g = 0; g < J; ++g) {
      va[g] = vb[g] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (topk::col(g, 0, h) < a.Kp) {
        va[g] = *reinterpret_cast<const f32x4*>(pa + topk::kGroup * g);
        vb[g] = *reinterpret_cast<const f32x4*>(pb + topk::kGroup * g);
      }
    }
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
        const float s = ((qbv[i] + cbv) + acc[i]) + 0.f;
        key[i] = topk::make_key(__float_as_uint(s), c32);
        win[i] = cok && qok[i] && key[i] > thr[i];
        any = any || win[i];
      }
      if (__any(any)) {
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
    const unsigned long long key = t < n ? in[t] : 0ull;
    const bool win = key > thr;  // (an empty place is 0 and never wins)
    const unsigned long long m = __ballot(win);
    if (m == 0ull) continue;
    if (win) buf[*cnt_s + __popcll(m & ((1ull << lane) - 1ull))] = key;
    __syncthreads();
    if (lane == 0) *cnt_s += __popcll(m);
    __syncthreads();
    if (*cnt_s > kcap) topk_compact_rows(buf, cap, a.k, 1, cnt_s, thr_s, lane);
    thr = *thr_s;
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

inline int launch_topk(TopkArgs a, hipStream_t stream) {
  if (a.k < 1 || a.k > topk::kMaxK || a.Kp < 4 || a.Kp > topk::kMaxKp || a.Kp % 4 || a.nq < 0 || a.nc < 0 ||
      a.nc >= (1ll << 31))
    return -1;
  if (a.nq == 0) return 0;
  const topk::Plan p = topk::plan(a.nq, a.nc, a.k);
  a.slab = p.slab;
  a.parts = p.parts;
  const long long qtiles = (a.nq + topk::kTile - 1) / topk::kTile;
  const long long blocks = qtiles * a.parts;
  if (blocks >= (1ll << 31) || a.nq >= (1ll << 31)) return -1;
  const int kc1 = topk_kcap(a.k, 32);
  const size_t lds1 = topk_lds_bytes(topk::kTile, kc1);
#define FM_TOPK_CASE(JJ)                                                                                       \
  case JJ:                                                                                                     \
    hipLaunchKernelGGL((topk_slab_kernel<JJ>), dim3((unsigned)blocks), dim3(kWave), lds1, stream, a, qtiles, kc1); \
    break;
  switch (topk::groups(a.Kp)) {
    FM_TOPK_CASE(1) FM_TOPK_CASE(2) FM_TOPK_CASE(3) FM_TOPK_CASE(4) FM_TOPK_CASE(5) FM_TOPK_CASE(6)
    FM_TOPK_CASE(7) FM_TOPK_CASE(8) FM_TOPK_CASE(9) FM_TOPK_CASE(10) FM_TOPK_CASE(11) FM_TOPK_CASE(12)
    FM_TOPK_CASE(13) FM_TOPK_CASE(14) FM_TOPK_CASE(15) FM_TOPK_CASE(16)
    default: return -1;
  }
#undef FM_TOPK_CASE
  const int kc2 = topk_kcap(a.k, kWave);
  hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)a.nq), dim3(kWave), topk_lds_bytes(1, kc2), stream, a, kc2);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace fm
