// The strongest feature pairs of every example's FM score, on gfx950 (the reference has no equivalent).
//
// Example i has occurrences 0 .. n-1 with (row r_j, value x_j).  For every j < l
//
//   p_jl = (x_j * x_l) * dot_jl,   dot_jl = fmaf chain over the columns of v_{r_j}, v_{r_l} in the order pi(Kp)
//
// (../topk_order.h: pi; ../pairs_key.h: the selection key and the limits, shared with the CPU twin), the
// score is bias + sum_j x_j w_j + sum_{j<l} p_jl, and the example's output row holds its `top` pairs of
// greatest |p|, equal |p| by ascending (j, l): the `top` greatest keys.  Exact fp32 and bitwise
// reproducible, as fm_topk.hip is: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain, keys are unique and
// there are no atomics, so no order of arrival can change a result.
//
// Design: one wave (a 64-thread workgroup, so the in-LDS sort's barriers are the wave's own) per example,
// workgroups striding over the batch.  The example's Gram matrix V V^T is walked by its upper-triangle 16 x
// 16 tiles: T = ceil(n / 16) row tiles, T (T + 1) / 2 tile pairs.  Lane (r, h) loads the 16 bytes (bf16: 8,
// widened exactly) at columns 16 g + 4 h .. + 3 of row r of a tile straight from the table; element e of
// that load is its operand of matrix instruction 4 g + e -- fm_topk's layout, hence its pi.  Row tile I's
// operands stay in registers (Kp / 4 VGPRs) while J runs over I .. T-1; tile J's rows are gathered again,
// from L2, which the same example has just filled.  Slots past n read the example's last row and are masked.
// The accumulator is 256 candidates, 4 per lane (rows 4 h + i of tile I against row r of tile J); each is
// scaled by x_j x_l (tile I's values fetched once per I by shuffle, tile J's value is the lane's own) and
// keyed.  Selection, one threshold per example: the lanes whose key beats the current top-th key (0 until
// `top` keys are known) are found by ballot and appended to the wave's LDS buffer of kPairBuf keys; when the
// buffer could not take another whole tile it is sorted (fm_topk's bitonic passes) and cut back to `top`, and
// the threshold moves.  After the first cut a tile rarely has more than a few winners.  One more sort at the
// end, and the keys decode to (j, l, p): the sign of p travels in the key.  The [n, n] matrix never reaches
// memory; no host read, no cross-wave wait, every loop bounded by n <= pairs::kMaxN.
//
// (Included after fm_topk.hip, which brings in fm_rank_common.h: f32x4 and topk_sort_rows are that header's.)
#include "fm_common.h"
#include "../pairs_key.h"

namespace fm {

struct PairsArgs {
  int B;
  const int* offsets;   // [B+1] CSR offsets into rows/vals
  const int* rows;      // [nnz] plain row index into v (table rows or wire rows)
  const float* vals;    // [nnz] feature values, nullptr => all 1
  const void* v;        // factor rows (fp32 or bf16), v_stride elements apart
  long long v_stride;
  int Kp, top;
  int* first;           // [B, top] occurrence position j within the example (-1: none)
  int* second;          // [B, top] occurrence position l > j
  float* value;         // [B, top] signed p_jl (0: none)
  int* count;           // [B] pairs returned; -1: the example has more than pairs::kMaxN occurrences
};

constexpr int kPairTile = topk::kTile * topk::kTile;  // candidates of one accumulator
constexpr int kPairBuf = 2 * kPairTile;               // keys of the wave's buffer: a power of two >= top + 256
static_assert(pairs::kMaxTop <= kPairTile, "a cut leaves room for a whole tile");

// One lane's operands of a tile row: columns 16 g + 4 h .. + 3 of every group g, zeros past Kp.
template <int G, typename TV>
__device__ inline void pairs_load_row(const char* row_h, int Kp, int h, f32x4 (&o)[G]) {
#pragma unroll
  for (int g = 0; g < G; ++g) {
    o[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (topk::col(g, 0, h) < Kp) {
      float f[4];
      Frag<TV>::load(reinterpret_cast<const TV*>(row_h) + topk::kGroup * g, f);
      o[g] = f32x4{f[0], f[1], f[2], f[3]};
    }
  }
}

template <int G, typename TV>  // column groups of 16: Kp in (16 (G - 1), 16 G]
__global__ __launch_bounds__(kWave) void fm_pairs_kernel(PairsArgs a) {
  __shared__ unsigned long long buf[kPairBuf];
  const int lane = threadIdx.x;
  const int r = lane & 15, h = lane >> 4;
  const char* vbytes = reinterpret_cast<const char*>(a.v) + 4 * h * (int)sizeof(TV);
  const uint32_t vsb = (uint32_t)(a.v_stride * (long long)sizeof(TV));  // (< 2^32: host-checked)
  const unsigned long long below = (1ull << lane) - 1ull;

  for (int ex = blockIdx.x; ex < a.B; ex += gridDim.x) {
    const int s = a.offsets[ex];
    const int n = a.offsets[ex + 1] - s;
    int cnt = 0;                    // keys in buf (wave-uniform)
    unsigned long long thr = 0ull;  // the top-th key once `top` keys are known
    // Sort the cnt keys, best first, and keep the best `top` (wave-uniform call).
    const auto compact = [&]() {
      int sz = 2;
      while (sz < cnt) sz <<= 1;
      __syncthreads();
      for (int t = cnt + lane; t < sz; t += kWave) buf[t] = 0ull;
      __syncthreads();
      topk_sort_rows(buf, sz, 1, lane);
      if (cnt >= a.top) {
        cnt = a.top;
        thr = buf[a.top - 1];
      }
      __syncthreads();
    };

    if (n >= 2 && n <= pairs::kMaxN) {
      const int T = (n + topk::kTile - 1) / topk::kTile;
      // row and value of occurrence 16 t + r (past n: the last occurrence, masked by its position below)
      const auto load_occ = [&](int t, float& x) -> const char* {
        const int o = s + min(t * topk::kTile + r, n - 1);
        x = a.vals ? a.vals[o] : 1.f;
        return vbytes + (uint64_t)(uint32_t)a.rows[o] * vsb;
      };
      for (int I = 0; I < T; ++I) {
        f32x4 qa[G];
        float xa;
        pairs_load_row<G, TV>(load_occ(I, xa), a.Kp, h, qa);
        float xi[4];  // values of this lane's 4 result rows: occurrences 16 I + 4 h + i
#pragma unroll
        for (int i = 0; i < 4; ++i) xi[i] = __shfl(xa, 4 * h + i, kWave);
        for (int J = I; J < T; ++J) {
          f32x4 vb[G];
          float xb = xa;
          if (J == I) {
#pragma unroll
            for (int g = 0; g < G; ++g) vb[g] = qa[g];
          } else {
            pairs_load_row<G, TV>(load_occ(J, xb), a.Kp, h, vb);
          }
          f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int g = 0; g < G; ++g) {
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], vb[g][e], acc, 0, 0, 0);
          }
          // this lane's candidates (16 I + 4 h + i, 16 J + r); the winners' places follow the ballots
          const int l = J * topk::kTile + r;
          unsigned long long key[4];
          bool win[4];
          int pos[4], add = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int j = I * topk::kTile + 4 * h + i;
            const float p = __fmul_rn(__fmul_rn(xi[i], xb), acc[i]);  // (two roundings, no contraction)
            key[i] = pairs::make_key(__float_as_uint(p), j, l);
            win[i] = j < l && l < n && key[i] > thr;
            const unsigned long long m = __ballot(win[i]);
            pos[i] = cnt + add + __popcll(m & below);
            add += __popcll(m);
          }
          if (add) {
            // (cnt <= kPairTile before a tile and a tile adds <= kPairTile keys: the buffer cannot overflow)
#pragma unroll
            for (int i = 0; i < 4; ++i)
              if (win[i]) buf[pos[i]] = key[i];
            cnt += add;
            if (cnt > kPairTile) compact();
          }
        }
      }
      compact();
    }

    const long long out = (long long)ex * a.top;
    for (int t = lane; t < a.top; t += kWave) {
      const unsigned long long key = t < cnt ? buf[t] : 0ull;
      a.first[out + t] = pairs::key_first(key);
      a.second[out + t] = pairs::key_second(key);
      a.value[out + t] = __uint_as_float(pairs::key_value_bits(key));
    }
    if (lane == 0) a.count[ex] = n > pairs::kMaxN ? -1 : cnt;
    __syncthreads();  // (the next example writes buf)
  }
}

// The launch's wave cap is the explain launcher's (16384 waves); longer batches stride.
inline int launch_pairs(const PairsArgs& a, int dtype, hipStream_t st) {
  if (a.top < 1 || a.top > pairs::kMaxTop || a.Kp < 4 || a.Kp > topk::kMaxKp || a.Kp % 4 ||
      (dtype != kF32 && dtype != kBF16))
    return -1;
  if (a.B <= 0) return 0;
  const int grid = fill_grid(a.B, 1, 4096 * kWavesPerBlock);
#define FM_PAIRS_CASE(GG)                                                                              \
  case GG:                                                                                             \
    if (dtype == kBF16)                                                                                \
      hipLaunchKernelGGL((fm_pairs_kernel<GG, __hip_bfloat16>), dim3(grid), dim3(kWave), 0, st, a);    \
    else                                                                                               \
      hipLaunchKernelGGL((fm_pairs_kernel<GG, float>), dim3(grid), dim3(kWave), 0, st, a);             \
    break;
  switch (topk::groups(a.Kp)) {
    FM_PAIRS_CASE(1) FM_PAIRS_CASE(2) FM_PAIRS_CASE(3) FM_PAIRS_CASE(4) FM_PAIRS_CASE(5) FM_PAIRS_CASE(6)
    FM_PAIRS_CASE(7) FM_PAIRS_CASE(8) FM_PAIRS_CASE(9) FM_PAIRS_CASE(10) FM_PAIRS_CASE(11) FM_PAIRS_CASE(12)
    FM_PAIRS_CASE(13) FM_PAIRS_CASE(14) FM_PAIRS_CASE(15) FM_PAIRS_CASE(16)
    default: return -1;
  }
#undef FM_PAIRS_CASE
  return (int)hipGetLastError();
}

}  // namespace fm
