// Exact per-occurrence attributions of the FM score, and their per-feature sums, on gfx950.
//
// An FM score is a linear term plus pairwise terms; splitting every pair's term equally between its
// two occurrences gives each occurrence's exact Shapley value against the empty example:
//
//   c_j = x_j w_j + 1/2 sum_f x_j v_jf (S_f - x_j v_jf),   S_f = sum_j x_j v_jf
//
// and sum_j c_j = pred - bias (repeated ids count as separate occurrences, as in the scorer).  The
// reference has no equivalent.
//
// Design: the forward's shape (fm_fwd.hip) -- one wave64 per example, the example's (row, value) pairs
// loaded lane-parallel and broadcast with ds_bpermute, rows fetched 16 B per lane, G = 64/LPR rows per
// wave instruction.  Pass 1 accumulates S exactly as the forward accumulates s1.  Pass 2 hands each lane
// group one occurrence per round, dots the row's fragment with S and sums over the group; the results
// are collected (one ds_bpermute per row group) so that lane l holds occurrence base + l, and 64
// contributions leave in one coalesced store.
//
// Pass-2 rows are gathered again rather than kept in registers: pass 1 has just read them, so they
// come from L2, and keeping an example's rows live across the S reduction would cost UNR * 4 VGPRs
// more per lane for the one-round case only (examples longer than a round need the re-gather anyway).
// No atomics and no LDS: results are bitwise repeatable.
#include "fm_common.h"

namespace fm {

struct ExplainArgs {
  int B;
  const int* offsets;   // [B+1] CSR offsets into rows/vals
  const int* rows;      // [nnz] plain row index into the v/w sources (table rows or wire rows)
  const float* vals;    // [nnz] feature values, nullptr => all 1
  const void* v;        // factor rows (TV), v_stride elements apart
  long long v_stride;
  const float* w;       // linear weights, w_stride elements apart (fp8: [w, scale, |v|^2, .] tails)
  long long w_stride;
  int Kp;
  const float* bias;    // [1] or nullptr
  float* contrib;       // [nnz]
  float* pred;          // [B] sum of the example's contributions + bias
};

// Row groups in flight per lane in either pass: the forward's generic choice, capped at 8 (pass 2
// holds S and the collected results next to the fragments).
template <int G>
struct ExplainUnroll {
  static constexpr int v = FwdUnroll<G>::v > 8 ? 8 : FwdUnroll<G>::v;
};

template <int LPR, typename TV>
__global__ __launch_bounds__(kBlock) void fm_explain_kernel(ExplainArgs a) {
  using F = Frag<TV>;
  constexpr int EPL = F::N;
  constexpr int G = kWave / LPR;
  constexpr int UNR = ExplainUnroll<G>::v;
  constexpr bool kRaw = F::kScaled;   // fp8: raw fragments converted with the row scale
  constexpr bool kNorm = F::kScaled;  // fp8: the self term from the stored row norm (as the forward)
  const int lane = threadIdx.x & (kWave - 1);
  const int g = lane / LPR, t = lane % LPR;
  const int nv = a.Kp / EPL;
  const bool tact = t < nv;
  const int tE = tact ? t : nv - 1;  // clamped: loads never leave the row
  const float tmask = tact ? 1.f : 0.f;
  const uint32_t coff = (uint32_t)(tE * EPL * (int)sizeof(TV));
  const char* vbytes = reinterpret_cast<const char*>(a.v) + coff;
  const uint32_t vsb = (uint32_t)(a.v_stride * (long long)sizeof(TV));  // (< 2^32: host-checked)
  const int wave = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int nwaves = gridDim.x * kWavesPerBlock;
  const int src_b = ((lane % G) * LPR) << 2;  // collect: a lane of the group that holds occurrence (lane % G)
  const float bias = a.bias ? a.bias[0] : 0.f;

  for (int i = wave; i < a.B; i += nwaves) {
    const int s = a.offsets[i], e = a.offsets[i + 1];
    // the 64 occurrences of one piece, one per lane: row, x, w (fp8: scale and stored |v|^2)
    int my_row = 0;
    float my_x = 0.f, my_w = 0.f, my_s = 1.f, my_n2 = 0.f;
    int have = -1;  // base of the piece these hold
    auto load_piece = [&](int base, int m) {
      my_row = 0;
      my_x = 0.f; my_w = 0.f; my_s = 1.f; my_n2 = 0.f;
      if (lane < m) {
        my_row = a.rows[base + lane];
        my_x = a.vals ? a.vals[base + lane] : 1.f;
        const float* wp = a.w + (long long)my_row * a.w_stride;
        if constexpr (kNorm) {  // [w, scale, |v|^2, .]: one 16-byte load (alignment host-checked)
          const float4 wr = *reinterpret_cast<const float4*>(wp);
          my_w = wr.x;
          my_s = wr.y;
          my_n2 = wr.z;
        } else {
          my_w = *wp;
        }
      }
      have = base;
    };
    // Issue the UNR row loads of round q (slots past the example read row 0 / wrap around the wave and
    // are masked afterwards, as in the forward); fx: the occurrence's x, 0 past the example.
    auto load_round = [&](int q, int m, float (&fr)[UNR][EPL], float (&fx)[UNR]) {
      int fraw[kRaw ? UNR : 1];
      float fs[kRaw ? UNR : 1];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const int f = q + u * G + g;
        const int fb = (f & (kWave - 1)) << 2;
        const float x = __int_as_float(__builtin_amdgcn_ds_bpermute(fb, __float_as_int(my_x)));
        fx[u] = f < m ? x : 0.f;
        const int row = __builtin_amdgcn_ds_bpermute(fb, my_row);
        const char* rp = vbytes + (uint64_t)(uint32_t)row * vsb;
        if constexpr (kRaw) {
          fraw[u] = *reinterpret_cast<const int*>(rp);
          fs[u] = __int_as_float(__builtin_amdgcn_ds_bpermute(fb, __float_as_int(my_s)));
        } else {
          F::load(reinterpret_cast<const TV*>(rp), fr[u]);
        }
      }
      if constexpr (kRaw) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) F::cvt_scaled(fraw[u], fs[u], fr[u]);
      }
    };

    // ---- pass 1: S = sum_j x_j v_j, every lane group holding its share, then summed across groups
    float S[EPL];
#pragma unroll
    for (int k = 0; k < EPL; ++k) S[k] = 0.f;
    for (int base = s; base < e; base += kWave) {
      const int m = min(kWave, e - base);
      load_piece(base, m);
      for (int q = 0; q < m; q += G * UNR) {
        float fr[UNR][EPL], fx[UNR];
        load_round(q, m, fr, fx);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const float xm = fx[u] * tmask;
#pragma unroll
          for (int k = 0; k < EPL; ++k) S[k] += xm * fr[u][k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < EPL; ++k) S[k] = across_groups_sum<LPR>(S[k]);

    // ---- pass 2: one occurrence per lane group and round
    float total = 0.f;
    for (int base = s; base < e; base += kWave) {
      const int m = min(kWave, e - base);
      if (have != base) load_piece(base, m);  // (an example of one piece keeps pass 1's registers)
      float out = 0.f;  // pairwise part of occurrence base + lane
      for (int q = 0; q < m; q += G * UNR) {
        float fr[UNR][EPL], fx[UNR];
        load_round(q, m, fr, fx);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          float d = 0.f;
          if constexpr (kNorm) {
            // <v_j, S> on the dequantised row; the self term comes from the stored norm below
#pragma unroll
            for (int k = 0; k < EPL; ++k) d += fr[u][k] * S[k];
            d *= fx[u] * tmask;
          } else {
            const float xm = fx[u] * tmask;
#pragma unroll
            for (int k = 0; k < EPL; ++k) {
              const float xv = xm * fr[u][k];
              d += xv * (S[k] - xv);
            }
          }
          d = group_sum<LPR>(d);
          // lane l takes occurrence l's value from its group, when this row group is the one that held it
          const float c = G == kWave ? d : __int_as_float(__builtin_amdgcn_ds_bpermute(src_b, __float_as_int(d)));
          const int rel = lane - q - u * G;
          if (rel >= 0 && rel < G) out = c;
        }
      }
      if constexpr (kNorm) out -= my_x * my_x * my_n2;
      const float c = lane < m ? my_x * my_w + 0.5f * out : 0.f;
      if (lane < m) a.contrib[base + lane] = c;
      total += c;
    }
    total = group_sum<kWave>(total);
    if (lane == 0) a.pred[i] = total + bias;
  }
}

// The launch's wave cap is the forward's (16384 waves); longer batches stride.
int launch_explain(const ExplainArgs& a, int dtype, hipStream_t st) {
  if (a.B <= 0) return 0;
  const int lpr = lanes_per_row(a.Kp, dtype);
  if (dtype == kFP8 && (((uintptr_t)a.w & 15) != 0 || a.w_stride % 4 != 0)) return -7;
  const int grid = fill_grid(a.B, kWavesPerBlock, 4096);
  FM_DISPATCH(dtype, lpr, fm_explain_kernel, grid, st, a);
  return (int)hipGetLastError();
}

// ---- per-feature importance -------------------------------------------------------------------------
// count, sum |c| and sum c of every segment of a dedup of the batch's ids (perm: occurrence index in
// sorted order, seg_start: [U + 1]).  fp64, fixed order: lane-strided partial sums over the segment in
// sorted order, then a butterfly.  Segments of up to kImpShort occurrences are packed 8 to a wave (8
// lanes each); a wave then takes its longer segments one at a time with all 64 lanes, 4 loads in
// flight per lane (a Criteo-shaped batch has segments of 1 and of > 100k occurrences).
constexpr int kImpSub = 8;                     // lanes of a packed segment
constexpr int kImpPack = kWave / kImpSub;      // segments per wave
constexpr int kImpShort = 64;                  // longest packed segment

struct ImportanceArgs {
  int U;
  const float* contrib;  // [n]
  const int* perm;       // [n]
  const int* seg_start;  // [U + 1]
  int* count;            // [U]
  double* sum_abs;       // [U]
  double* sum;           // [U]
};

__global__ __launch_bounds__(kBlock) void fm_importance_kernel(ImportanceArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane / kImpSub, sl = lane % kImpSub;
  const int nwaves = gridDim.x * kWavesPerBlock;
  const int ngroups = (a.U + kImpPack - 1) / kImpPack;
  for (int grp = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); grp < ngroups; grp += nwaves) {
    const int u = grp * kImpPack + sub;
    int s = 0, e = 0;
    if (u < a.U) {
      s = a.seg_start[u];
      e = a.seg_start[u + 1];
    }
    const int n = e - s;
    double sa = 0.0, sm = 0.0;
    if (n <= kImpShort) {
      for (int j = s + sl; j < e; j += kImpSub) {
        const double c = (double)a.contrib[a.perm[j]];
        sa += fabs(c);
        sm += c;
      }
    }
#pragma unroll
    for (int o = kImpSub / 2; o > 0; o >>= 1) {  // (all lanes: shuffles stay outside the guards)
      sa += __shfl_xor(sa, o, kWave);
      sm += __shfl_xor(sm, o, kWave);
    }
    if (u < a.U && n <= kImpShort && sl == 0) {
      a.count[u] = n;
      a.sum_abs[u] = sa;
      a.sum[u] = sm;
    }
    // the wave's long segments, one at a time (wave-uniform loop over the ballot)
    unsigned long long big = __ballot(sl == 0 && n > kImpShort);
    while (big) {
      const int src = __ffsll((long long)big) - 1;
      big &= big - 1;
      const int bs = __shfl(s, src, kWave), be = __shfl(e, src, kWave);
      double ba = 0.0, bm = 0.0;
      int j = bs + lane;
      for (; j + 3 * kWave < be; j += 4 * kWave) {  // 4 gathers in flight, added in order
        const float c0 = a.contrib[a.perm[j]], c1 = a.contrib[a.perm[j + kWave]];
        const float c2 = a.contrib[a.perm[j + 2 * kWave]], c3 = a.contrib[a.perm[j + 3 * kWave]];
        ba += fabs((double)c0); bm += (double)c0;
        ba += fabs((double)c1); bm += (double)c1;
        ba += fabs((double)c2); bm += (double)c2;
        ba += fabs((double)c3); bm += (double)c3;
      }
      for (; j < be; j += kWave) {
        const double c = (double)a.contrib[a.perm[j]];
        ba += fabs(c);
        bm += c;
      }
#pragma unroll
      for (int o = kWave / 2; o > 0; o >>= 1) {
        ba += __shfl_xor(ba, o, kWave);
        bm += __shfl_xor(bm, o, kWave);
      }
      if (lane == 0) {
        const int bu = grp * kImpPack + src / kImpSub;
        a.count[bu] = be - bs;
        a.sum_abs[bu] = ba;
        a.sum[bu] = bm;
      }
    }
  }
}

int launch_importance(const ImportanceArgs& a, hipStream_t st) {
  if (a.U <= 0) return 0;
  const int grid = fill_grid((a.U + kImpPack - 1) / kImpPack, kWavesPerBlock, 4096);
  hipLaunchKernelGGL(fm_importance_kernel, dim3(grid), dim3(kBlock), 0, st, a);
  return (int)hipGetLastError();
}

}  // namespace fm
