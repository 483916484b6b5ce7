// Diversified recommendations: greedy maximal-marginal-relevance (MMR) re-ranking of every context's pool, the
// rows fm_topk wrote (the reference only scores examples).
//
// A pool is M <= 128 positions of one context: pool_idx [nq, M] candidates (-1: no candidate; a value outside
// [0, nc) counts as -1) and pool_score [nq, M].  For positions j, l holding candidates a, b
//   dot_jl = the fmaf chain of C[a] and C[b] over the columns in the order of ../topk_order.h, from +0
//   sim_jl = (dot_jl * inv[a]) * inv[b]                               (two roundings; inv: the caller's scale)
// and n picks are made, t = 0 .. n-1, P the positions picked so far in pick order:
//   pen_j = 0 (t = 0), else max_{s in P} sim_js                       (fmaxf in pick order)
//   m_j   = fmaf(-mu, pen_j, lam * pool_score[j]) + 0                 (mu = 1 - lam from the host; -0 becomes +0)
//   pick the unpicked position holding a candidate of greatest m, equal m by lower position
// by the 64-bit key of topk_order.h: m's order-preserving image above the inverted position.  A pick writes the
// candidate, its pool score and m; a context that runs out of candidates ends in -1 / -inf / -inf.
// dot_jl and dot_lj are one chain (a product commutes), but sim_jl and sim_lj round in different orders: the two
// triangles of the matrix are scaled separately, each as the definition has it.
//
// diversify_kernel<J>: one wave (a 64-thread workgroup) per context, T = ceil(M / 16) tiles of 16 positions.
// Gather: lane l keeps the candidate, score and inv of positions l and l + 64.  For tile t lane (r, h) fetches the
// candidate of position 16 t + r from its lane and loads 16 bytes per column group of that row straight from C,
// load_operands' layout (fm_rank_common.h) -- which serves as the A and as the B operand of v_mfma_f32_16x16x4_f32 alike.
// Gram: row tile I's operands stay in registers while J runs over I .. T-1 (the diagonal tile multiplies I's
// operands with themselves: no load); widths up to Kp = 128 gather tile J + 1 under tile J's products.  An
// accumulator of lane (r, h) holds dot of positions 16 I + 4 h + i and 16 J + r; scaled, it goes to the fp32
// [16 T, 16 T] matrix in dynamic LDS as G[row s][column j] = sim_js, the tile itself and (off the diagonal) its
// transpose, one 16-byte store per lane.  1 KB at M <= 16, 64 KB at M = 128: small pools keep their occupancy.
// Greedy: a step computes m for the lane's two positions, reduces the keys over the wave by DPP and gfx950's
// permlane swaps (VALU only), reads the winner's candidate and score from its lane, and reads row s of G -- lane l
// columns l and l + 64, contiguous, so without bank conflicts -- into pen.  Lane t (mod 64) keeps step t's three
// outputs; they are stored coalesced at the end.
// Not tried: padding G's rows against the 4-way bank conflict of the tile stores; n matrix-vector passes in place
// of the Gram for pools much larger than n; several contexts per workgroup.
//
// No atomics, no host read, no workspace; graph-capturable and bitwise repeatable.
#include "fm_rank_common.h"

namespace fm {

struct DiversifyArgs {
  long long nq, nc;
  int Kp, M, n;
  const float* C; long long c_stride;   // [nc, Kp], row stride in elements (16-byte aligned rows)
  const float* inv;                     // [nc]
  const int* pool_idx;                  // [nq, M]
  const float* pool_score;              // [nq, M]
  float lam, neg_mu;                    // lam and -(1 - lam)
  int* idx;                             // [nq, n]
  float* score;                         // [nq, n]
  float* mmr;                           // [nq, n]
};

// The greatest key of the wave in every lane (all 64 lanes active).  Steps 1, 2: quad_perm; 4: row_half_mirror and
// 8: row_mirror (a max may pair any lanes of the other half); 16 and 32: permlane swaps, as xor_add does.
template <int CTRL>
__device__ inline unsigned long long diversify_dpp_max(unsigned long long k) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)k, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(k >> 32), CTRL, 0xf, 0xf, false);
  const unsigned long long o = ((unsigned long long)hi << 32) | lo;
  return o > k ? o : k;
}
__device__ inline unsigned long long diversify_wave_max(unsigned long long k) {
  k = diversify_dpp_max<0xB1>(k);
  k = diversify_dpp_max<0x4E>(k);
  k = diversify_dpp_max<0x141>(k);
  k = diversify_dpp_max<0x140>(k);
  {
    const auto lo = __builtin_amdgcn_permlane16_swap((uint32_t)k, (uint32_t)k, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((uint32_t)(k >> 32), (uint32_t)(k >> 32), false, false);
    const unsigned long long x = ((unsigned long long)hi[0] << 32) | lo[0], y = ((unsigned long long)hi[1] << 32) | lo[1];
    k = x > y ? x : y;
  }
  {
    const auto lo = __builtin_amdgcn_permlane32_swap((uint32_t)k, (uint32_t)k, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((uint32_t)(k >> 32), (uint32_t)(k >> 32), false, false);
    const unsigned long long x = ((unsigned long long)hi[0] << 32) | lo[0], y = ((unsigned long long)hi[1] << 32) | lo[1];
    k = x > y ? x : y;
  }
  return k;
}

template <int J>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ __launch_bounds__(kWave) void diversify_kernel(DiversifyArgs a) {
  extern __shared__ __attribute__((aligned(16))) float diversify_gram[];  // [16 T][16 T]
  constexpr bool kPrefetch = J <= 8;  // tile J + 1 in flight under tile J (2 x 4 J more VGPRs)

  const int lane = threadIdx.x;
  const int r = lane & 15, h = lane >> 4;
  const long long q = blockIdx.x;
  const int T = (a.M + topk::kTile - 1) / topk::kTile, MP = topk::kTile * T;
  float* G = diversify_gram;

  // positions lane and lane + 64: the candidate (-1: none), its pool score and its scale
  int c[2];
  float sc[2], iv[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int pos = lane + kWave * p;
    c[p] = -1;
    sc[p] = -INFINITY;
    iv[p] = 0.f;
    if (pos < a.M) {
      const int v = a.pool_idx[q * a.M + pos];
      if (v >= 0 && v < a.nc) {
        c[p] = v;
        sc[p] = a.pool_score[q * a.M + pos];
        iv[p] = a.inv[v];
      }
    }
  }
  // the value lane (pos mod 64) holds for position pos of tile t (t < 4: the lane's first position)
  const auto cand_of = [&](int t, int w) {
    return __builtin_amdgcn_ds_bpermute((topk::kTile * (t & 3) + w) << 2, t < 4 ? c[0] : c[1]);
  };
  const auto inv_of = [&](int t, int w) {
    return __int_as_float(
        __builtin_amdgcn_ds_bpermute((topk::kTile * (t & 3) + w) << 2, __float_as_int(t < 4 ? iv[0] : iv[1])));
  };
  // operands of tile t: lane (r, h) loads columns 16 g + 4 h .. + 3 of position 16 t + r's row (none: zeros)
  const auto gather = [&](int t, f32x4 (&v)[J]) {
    const int ct = cand_of(t, r);
    load_operands<J>(a.C + (long long)(ct < 0 ? 0 : ct) * a.c_stride + 4 * h, h, a.Kp, v, ct >= 0);
  };

  for (int I = 0; I < T; ++I) {
    f32x4 A[J];
    gather(I, A);
    float ivI[4];  // of the accumulator's rows 16 I + 4 h + i
#pragma unroll
    for (int i = 0; i < 4; ++i) ivI[i] = inv_of(I, 4 * h + i);
    // tile (I, Jt) from the operands B of tile Jt: G[16 I + 4 h + i][16 Jt + r] and, off the diagonal, its transpose
    const auto tile = [&](int Jt, const f32x4 (&B)[J]) {
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int g = 0; g < J; ++g)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[g][e], B[g][e], acc, 0, 0, 0);
      const float ivJ = inv_of(Jt, r);
      float* d = G + (topk::kTile * I + 4 * h) * MP + topk::kTile * Jt + r;
#pragma unroll
      for (int i = 0; i < 4; ++i) d[i * MP] = (acc[i] * ivJ) * ivI[i];  // row s = 16 I + 4 h + i, column j = 16 Jt + r
      if (Jt != I) {
        f32x4 tr;
#pragma unroll
        for (int i = 0; i < 4; ++i) tr[i] = (acc[i] * ivI[i]) * ivJ;    // row s = 16 Jt + r, column j = 16 I + 4 h + i
        *reinterpret_cast<f32x4*>(G + (topk::kTile * Jt + r) * MP + topk::kTile * I + 4 * h) = tr;
      }
    };
    tile(I, A);
    if constexpr (kPrefetch) {
      f32x4 nb[J];
      if (I + 1 < T) gather(I + 1, nb);
      for (int Jt = I + 1; Jt < T; ++Jt) {
        f32x4 b[J];
#pragma unroll
        for (int g = 0; g < J; ++g) b[g] = nb[g];
        if (Jt + 1 < T) gather(Jt + 1, nb);
        tile(Jt, b);
      }
    } else {
      for (int Jt = I + 1; Jt < T; ++Jt) {
        f32x4 b[J];
        gather(Jt, b);
        tile(Jt, b);
      }
    }
  }
  __syncthreads();

  const float rel[2] = {a.lam * sc[0], a.lam * sc[1]};
  float pen[2] = {0.f, 0.f};
  bool open[2] = {c[0] >= 0, c[1] >= 0};
  int oi[2] = {-1, -1};                        // step lane (+ 64)'s outputs
  float os[2] = {-INFINITY, -INFINITY}, om[2] = {-INFINITY, -INFINITY};
  for (int t = 0; t < a.n; ++t) {
    unsigned long long key = 0ull;  // (no candidate left in this lane: 0, below every key)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float m = __builtin_fmaf(a.neg_mu, pen[p], rel[p]) + 0.f;
      const unsigned long long k = topk::make_key(__float_as_uint(m), (uint32_t)(lane + kWave * p));
      if (open[p] && k > key) key = k;
    }
    key = diversify_wave_max(key);
    const uint32_t klo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)key);
    const uint32_t khi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(key >> 32));
    if (klo == 0u && khi == 0u) break;  // (wave-uniform) the pool is used up
    const int s = (int)(0xFFFFFFFFu - klo);  // in [0, M): only this wave's own keys are reduced
    const int sl = s & (kWave - 1);
    const bool up = s >= kWave;
    const int ci = up ? __builtin_amdgcn_readlane(c[1], sl) : __builtin_amdgcn_readlane(c[0], sl);
    const int si = up ? __builtin_amdgcn_readlane(__float_as_int(sc[1]), sl)
                      : __builtin_amdgcn_readlane(__float_as_int(sc[0]), sl);
    const float mi = __uint_as_float(topk::unorder_u32(khi));
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      if (lane + kWave * p == t) {
        oi[p] = ci;
        os[p] = __int_as_float(si);
        om[p] = mi;
      }
      if (lane + kWave * p == s) open[p] = false;
    }
    const float* row = G + s * MP;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int pos = lane + kWave * p;
      if (pos < MP) {
        const float sim = row[pos];
        pen[p] = t == 0 ? sim : fmaxf(pen[p], sim);
      }
    }
  }
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int t = lane + kWave * p;
    if (t < a.n) {
      a.idx[q * a.n + t] = oi[p];
      a.score[q * a.n + t] = os[p];
      a.mmr[q * a.n + t] = om[p];
    }
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
inline size_t diversify_lds_bytes(int M) {
  const size_t mp = (size_t)topk::kTile * ((M + topk::kTile - 1) / topk::kTile);
  return mp * mp * sizeof(float);
}

// idx / score / mmr [nq, n]: n greedy picks from every context's pool.  -1: bad arguments; -3: launch error.
inline int launch_diversify(const DiversifyArgs& a, hipStream_t stream) {
  if (!profile_sizes_ok(a.nq, a.nc, a.Kp) || a.M < 1 || a.M > topk::kMaxK || a.n < 1 || a.n > a.M ||
      !(a.lam >= 0.f && a.lam <= 1.f) || a.c_stride < a.Kp || a.c_stride % 4)
    return -1;
  if (a.nq == 0) return 0;
  if ((a.nc > 0 && (!a.C || !a.inv)) || !a.pool_idx || !a.pool_score || !a.idx || !a.score || !a.mmr ||
      (reinterpret_cast<uintptr_t>(a.C) & 15))
    return -1;
  const size_t lds = diversify_lds_bytes(a.M);
  if (dispatch_groups(a.Kp, [&](auto j) {
        hipLaunchKernelGGL((diversify_kernel<decltype(j)::value>), dim3((unsigned)a.nq), dim3(kWave), lds, stream, a);
      }))
    return -1;
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace fm
