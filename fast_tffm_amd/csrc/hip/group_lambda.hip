// LambdaRank loss: the logistic loss of every pair of different gains of every group of one batch, each pair
// weighted by the NDCG@K it would move if the two swapped their places in the group's current order by score.
//
//   s_i score, G_i = max(y_i, 0) gain (rank_metrics.hip's; example weights are no input); per group g over its n_g
//   examples in the batch:  r_i in 1..n_g the place of i by score descending (score_key.h's order, equal scores in
//   example order -- no tie-run mean: tied scores of different gains keep a gradient),
//   c(r) = 1 / log2(r + 1) for r <= K (every r when K = 0), else 0;  IDCG = sum_r G_(r) c(r), gains descending;
//   for every pair G_i > G_j:  delta_ij = (G_i - G_j) |c(r_i) - c(r_j)| / IDCG   (a constant: no gradient through r)
//   L_g = sum delta_ij softplus(s_j - s_i),   dL/ds_i -= delta_ij sigma(s_j - s_i),   dL/ds_j += the same
//   softplus(d) = max(d, 0) + log1p(t), sigma(d) = 1 / (1 + t) or t / (1 + t), t = exp(-|d|)   (group_walk.hip's)
//   A group with IDCG == 0, a group of one and an excluded example add exactly 0 and get exactly 0, whatever their
//   scores hold: no arithmetic touches them.  A pair counts only when one of its two places is <= K.
//
// The plan half is group_loss.hip's (group_plan), read only; this is a third score half, a launch chain on the
// caller's stream into a workspace of its own (no host read, no float atomic, no cross-workgroup wait beyond the
// radix sort's own: capturable):
//   inverse: gpos[example] = first[j] of its sorted position j, n for an excluded example;
//   order (on the gains, then on the scores): complemented score keys + example index, the stable radix sort
//           over 32 bits, then over bits_for(n + 1) bits of gpos[example].  Both sorts are stable and the second
//           key is the group's first position, so group g lands again on [first, end) of the plan -- its first /
//           end arrays index the new order unchanged -- now from the highest value down, equal values in example
//           order; excluded examples land on the plan's excluded tail.  Place = j - first + 1: no tie-run search;
//   ideal:  per tile of 1024 positions of the gain order the term G c(place), reduced per group by the listwise
//           loss's segmented tile reduction and carry: IDCG at the group's first position;
//   head:   per tile of the score order: score, gain (fp32) and discount (fp64) per position (the only gathers of
//           the pair stage) and the tile's column span: the union over its rows of what each needs -- a row of
//           place <= K its whole group, a row of place > K only the group's head [first, min(first + K, end));
//   pair:   group_walk.hip's pair stage, grid (row tile) x (column slab): a slab stages its chunks (score, gain,
//           discount) through LDS; a thread keeps its 4 rows' (s, G, c, column range) in registers and walks, per
//           staged chunk, only its row's own range, columns ascending, skipping columns of equal gain.  Per pair
//           delta' = |dG| |dc|; the sigma term goes to the row's "up" sum when the row has the larger gain (with
//           the softplus term to a third sum), else to its "down" sum.  One fp64 partial set per (slab,
//           position).  With K = 10 a tile wholly in a big group's tail has a one-chunk span and one live slab, the
//           tile that holds the head fans out over all slabs: about sum_g 2 n_g min(K, n_g) pairs (K = 0: n_g^2);
//   grad:   every position adds its slab partials in slab order, takes down - up once and divides by IDCG once;
//           dpred[example] = fp32(grad_scale ...); the rows' softplus sums / IDCG go to the tile's loss partial
//           (thread order, block scan);
//   final:  gl_final_kernel: the tile partials in tile order -> fp32 loss.
// Everything is fp64 (exp, log1p, log2 and the divisions too); every sum adds non-negative terms in an order fixed
// by n, K and the group structure; dpred and the loss are rounded once: bitwise the same run to run.  Every pair
// is evaluated from both of its rows.  (Included by module.hip after group_pair.hip: GlArgs, gl_bind, GlPos /
// gl_positions, gl_tile_reduce, the carry and final kernels, gauc_bits_for, score_key, the radix sort and WsCursor,
// and group_walk.hip's geometry, GwSpan and logistic pair term come before.)
#include "fm_common.h"

namespace fm {

constexpr int kGmMaxCutoff = 4096;   // K = 0 (no truncation) or 1..kGmMaxCutoff

struct GmLayout {
  size_t gpos, keys, idx, sk1, si1, gk, sg, oscore, ogain, sort;                  // order
  size_t ss, sgain, sc, gred, pup, pdn, psp, tflag, tv, fv, lpart, tlo, thi, total;
  int ntiles;
};

static GmLayout gm_layout(int n) {
  WsCursor c;
  GmLayout l{};
  const size_t N = (size_t)n;
  l.ntiles = (n + kGlTile - 1) / kGlTile;
  const size_t nt = (size_t)l.ntiles;
  l.gpos = c.take(4 * N);
  l.keys = c.take(4 * N);
  l.idx = c.take(4 * N);
  l.sk1 = c.take(4 * N);
  l.si1 = c.take(4 * N);
  l.gk = c.take(4 * N);
  l.sg = c.take(4 * N);
  l.oscore = c.take(4 * N);
  l.ogain = c.take(4 * N);
  l.sort = c.take(radix_sort_ws_bytes(n));
  l.ss = c.take(4 * N);
  l.sgain = c.take(4 * N);
  l.sc = c.take(8 * N);
  l.gred = c.take(8 * N);
  l.pup = c.take(8 * (size_t)kGwSlabs * N);
  l.pdn = c.take(8 * (size_t)kGwSlabs * N);
  l.psp = c.take(8 * (size_t)kGwSlabs * N);
  l.tflag = c.take(4 * nt);
  l.tv = c.take(8 * nt);
  l.fv = c.take(8 * nt);
  l.lpart = c.take(8 * nt);
  l.tlo = c.take(4 * nt);
  l.thi = c.take(4 * nt);
  l.total = c.off;
  return l;
}

// Bytes of the LambdaRank loss's workspace for up to n examples; 0: n outside [0, 2^30).
size_t group_lambda_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  return gm_layout((int)(n > 0 ? n : 1)).total;
}

struct GmArgs {
  GlArgs g;             // n, ntiles, grad_scale, inputs, the plan, ss, gred [n] (IDCG), tflag, tv, fv, lpart, outputs
  int cutoff;           // K (0: none)
  const int* order;     // [n] example index of every position of the (group, value descending) order in use
  const int* sort_err;  // the error word of the sort that made it
  float* sgain;         // [n] gain of every position of the score order
  double* sc;           // [n] its discount
  double* pup;          // [kGwSlabs, n] sigma sums over the columns of smaller gain
  double* pdn;          // [kGwSlabs, n] ... of larger gain
  double* psp;          // [kGwSlabs, n] softplus sums over the columns of smaller gain
  int* tlo;             // [ntiles] the tile's column span
  int* thi;
};

__device__ inline double gm_discount(int place, int K) {
  return (K == 0 || place <= K) ? 1.0 / log2((double)place + 1.0) : 0.0;
}

// The group range [fi, e) of position j (gl_positions' clamps) and whether its rows take part: not excluded, two
// examples or more, IDCG > 0.
__device__ inline bool gm_row_group(const GlArgs& g, int j, int& fi, int& e) {
  const int en = g.end[j];
  fi = min(max(g.first[j], 0), j);
  e = min(max(en, j + 1), g.n);
  return en != 0 && e - fi >= 2 && g.gred[fi] > 0.0;
}

// The columns a row of the given place needs: its whole group, or the group's head when it lies below the cutoff.
__device__ inline int gm_row_end(int fi, int e, int place, int K) {
  return (K == 0 || place <= K) ? e : min(fi + K, e);
}

__device__ inline void gm_report_sort(const int* sort_err) {
  if (blockIdx.x == 0 && threadIdx.x == 0 && *sort_err) atomicOr(&g_fm_dev_error, kDevErrSort);
}

// ---- inverse, order -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gm_inverse_kernel(int n, const int* sidx, const int* first, const int* end,
                                                            uint32_t* gpos) {
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const int ex = sidx[j];
    if ((unsigned)ex >= (unsigned)n) continue;  // (only after a failed plan sort: its error word is reported)
    gpos[ex] = end[j] == 0 ? (uint32_t)n : (uint32_t)min(max(first[j], 0), j);
  }
}

// The complemented score key (the ascending sort runs from the highest value down; ties stay in example order) of
// every score, or with kGain of every gain max(y, 0), and the identity index.
template <bool kGain>
__global__ __launch_bounds__(kBlock) void gm_key_kernel(int n, const float* v, uint32_t* keys, int* idx) {
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < n; e += gridDim.x * kBlock) {
    const float x = v[e];
    const uint32_t b = kGain ? (x > 0.f ? __float_as_uint(x) : 0u) : __float_as_uint(x);
    keys[e] = ~score_key(b);
    idx[e] = e;
  }
}

__global__ __launch_bounds__(kBlock) void gm_group_key_kernel(int n, const int* si1, const uint32_t* gpos,
                                                              uint32_t* gk, const int* sort_err) {
  gm_report_sort(sort_err);
  for (int j = blockIdx.x * kBlock + threadIdx.x; j < n; j += gridDim.x * kBlock) {
    const int ex = si1[j];
    gk[j] = (unsigned)ex < (unsigned)n ? min(gpos[ex], (uint32_t)n) : (uint32_t)n;
  }
}

// ---- ideal ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gm_ideal_kernel(GmArgs a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ double shv[kWavesPerBlock];
  const GlArgs& g = a.g;
  gm_report_sort(a.sort_err);
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  GlPos p;
  gl_positions(g, j0, p);
  double v[kGlItems];
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    v[q] = 0.0;
    if (!p.in[q] || p.excl[q]) continue;
    const int j = j0 + q;
    const int ex = a.order[j];
    if ((unsigned)ex >= (unsigned)g.n) continue;  // (not after a failed sort: its error word is reported)
    const float y = g.labels[ex];
    if (y > 0.f) v[q] = (double)y * gm_discount(j - p.fi[q] + 1, a.cutoff);
  }
  gl_tile_reduce<GlAdd>(p, v, g.gred, g.tv, g.fv, g.tflag, shf, shv);
}

// ---- head -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gm_head_kernel(GmArgs a) {
  __shared__ GwSpan span;
  const GlArgs& g = a.g;
  gw_span_open(span, g.n);
  gm_report_sort(a.sort_err);
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  int lo = g.n, hi = 0;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    if (j >= g.n) continue;
    float sc = 0.f, gain = 0.f;
    double c = 0.0;
    int fi, e;
    const int ex = a.order[j];
    if (gm_row_group(g, j, fi, e) && (unsigned)ex < (unsigned)g.n) {
      sc = g.scores[ex];
      const float y = g.labels[ex];
      gain = y > 0.f ? y : 0.f;
      const int place = j - fi + 1;
      c = gm_discount(place, a.cutoff);
      lo = min(lo, fi);
      hi = max(hi, gm_row_end(fi, e, place, a.cutoff));
    }
    g.ss[j] = sc;
    a.sgain[j] = gain;
    a.sc[j] = c;
  }
  gw_span_add(span, lo, hi);
  __syncthreads();
  gw_span_close(span, a.tlo, a.thi);
}

// ---- pair -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gm_pair_kernel(GmArgs a) {
  __shared__ float shs[kGwChunk];
  __shared__ float shg[kGwChunk];
  __shared__ double shc[kGwChunk];
  const GlArgs& g = a.g;
  const int n = g.n;
  const int lo = max(a.tlo[blockIdx.x], 0), hi = min(a.thi[blockIdx.x], n);
  int cb, ce;
  if (!gw_slab(lo, hi, blockIdx.y, cb, ce)) return;
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  int f[kGlItems], e[kGlItems];
  double rs[kGlItems], rg[kGlItems], rc[kGlItems], up[kGlItems], dn[kGlItems], sp[kGlItems];
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    f[q] = e[q] = 0;
    rs[q] = rg[q] = rc[q] = up[q] = dn[q] = sp[q] = 0.0;
    if (j >= n) continue;
    int fi, en;
    if (!gm_row_group(g, j, fi, en)) continue;
    f[q] = max(fi, lo);
    e[q] = min(gm_row_end(fi, en, j - fi + 1, a.cutoff), hi);
    rs[q] = (double)g.ss[j];
    rg[q] = (double)a.sgain[j];
    rc[q] = a.sc[j];
  }
  for (int c = cb; c < ce; ++c) {
    const int clo = c * kGwChunk;
    if (threadIdx.x < kGwChunk) {
      const int col = clo + (int)threadIdx.x;
      const bool ok = col < n;
      shs[threadIdx.x] = ok ? g.ss[col] : 0.f;
      shg[threadIdx.x] = ok ? a.sgain[col] : 0.f;
      shc[threadIdx.x] = ok ? a.sc[col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGlItems; ++q) {
      const int c0 = max(f[q], clo) - clo, c1 = min(e[q], clo + kGwChunk) - clo;
      for (int k = c0; k < c1; ++k) {
        const double gk = (double)shg[k];
        if (gk == rg[q]) continue;
        const bool larger = rg[q] > gk;
        const double dl = fabs(rg[q] - gk) * fabs(rc[q] - shc[k]);
        const double sk = (double)shs[k];
        const double d = larger ? sk - rs[q] : rs[q] - sk;  // s of the smaller gain - s of the larger
        const double t = exp(-fabs(d));
        const double sg = dl * gw_sigma(d, t);
        if (larger) {
          up[q] += sg;
          sp[q] += dl * gw_softplus(d, t);
        } else {
          dn[q] += sg;
        }
      }
    }
    __syncthreads();
  }
  const size_t base = (size_t)blockIdx.y * (size_t)n;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    if (j >= n) continue;
    a.pup[base + j] = up[q];
    a.pdn[base + j] = dn[q];
    a.psp[base + j] = sp[q];
  }
}

// ---- grad -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void gm_grad_kernel(GmArgs a) {
  __shared__ double sh[kWavesPerBlock];
  const GlArgs& g = a.g;
  const int n = g.n;
  const int lo = max(a.tlo[blockIdx.x], 0), hi = min(a.thi[blockIdx.x], n);
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  double lsum = 0.0;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    if (j >= n) continue;
    const int ex = a.order[j];
    if ((unsigned)ex >= (unsigned)n) continue;
    double d = 0.0;
    int fi, en;
    if (gm_row_group(g, j, fi, en)) {
      double up = 0.0, dn = 0.0, sp = 0.0;
      for (int s = 0; s < kGwSlabs; ++s) {
        int cb, ce;
        if (!gw_slab(lo, hi, s, cb, ce)) continue;
        up += a.pup[(size_t)s * n + j];
        dn += a.pdn[(size_t)s * n + j];
        sp += a.psp[(size_t)s * n + j];
      }
      const double idcg = g.gred[fi];
      d = (dn - up) / idcg;
      lsum += sp / idcg;
    }
    g.dpred[ex] = (float)(g.grad_scale * d);
  }
  double ex_, tot;
  auc_block_scan<double, kWavesPerBlock>(lsum, ex_, tot, sh);
  if (threadIdx.x == 0) g.lpart[blockIdx.x] = tot;
}

// The LambdaRank loss at cutoff K of the n >= 1 examples planned into plan_ws (read only): dpred[n] (example order)
// and loss[1], asynchronously on st; ws (group_lambda_workspace_bytes) holds the intermediates.  0, a hip error
// code or launch_radix_sort's; -1: bad arguments; -2: a workspace is too small; -9: K outside [0, 4096].
int launch_group_lambda(const void* plan_ws, size_t plan_bytes, int n, const float* scores, const float* labels,
                        int cutoff, double grad_scale, float* dpred, float* loss, void* ws, size_t ws_bytes,
                        hipStream_t st) {
  if (!gl_args_ok(plan_ws, n, scores, labels, dpred, loss, ws)) return -1;
  if (cutoff < 0 || cutoff > kGmMaxCutoff) return -9;
  const GmLayout l = gm_layout(n);
  if (ws_bytes < l.total || plan_bytes < gl_layout(n).total) return -2;
  char* b = static_cast<char*>(ws);
  GmArgs a{};
  GlArgs& g = a.g;
  gl_bind(g, l, ws, plan_ws, n, scores, labels, nullptr, grad_scale, dpred, loss);
  a.cutoff = cutoff;
  a.sgain = reinterpret_cast<float*>(b + l.sgain);
  a.sc = reinterpret_cast<double*>(b + l.sc);
  a.pup = reinterpret_cast<double*>(b + l.pup);
  a.pdn = reinterpret_cast<double*>(b + l.pdn);
  a.psp = reinterpret_cast<double*>(b + l.psp);
  a.tlo = reinterpret_cast<int*>(b + l.tlo);
  a.thi = reinterpret_cast<int*>(b + l.thi);
  uint32_t* gpos = reinterpret_cast<uint32_t*>(b + l.gpos);
  uint32_t* keys = reinterpret_cast<uint32_t*>(b + l.keys);
  int* idx = reinterpret_cast<int*>(b + l.idx);
  uint32_t* sk1 = reinterpret_cast<uint32_t*>(b + l.sk1);
  int* si1 = reinterpret_cast<int*>(b + l.si1);
  uint32_t* gk = reinterpret_cast<uint32_t*>(b + l.gk);
  uint32_t* sg = reinterpret_cast<uint32_t*>(b + l.sg);
  void* sort_ws = b + l.sort;
  const size_t sort_bytes = radix_sort_ws_bytes(n);
  a.sort_err = radix_sort_error(sort_ws, n);
  const dim3 tiles(l.ntiles), blk(kBlock), one(kAucBaseThreads), flat(fill_grid(n, kBlock, 2048));
  hipLaunchKernelGGL(gm_inverse_kernel, flat, blk, 0, st, n, g.sidx, g.first, g.end, gpos);
  for (int pass = 0; pass < 2; ++pass) {  // the gains (the ideal order), then the scores
    int* order = reinterpret_cast<int*>(b + (pass ? l.oscore : l.ogain));
    if (pass) hipLaunchKernelGGL(gm_key_kernel<false>, flat, blk, 0, st, n, scores, keys, idx);
    else hipLaunchKernelGGL(gm_key_kernel<true>, flat, blk, 0, st, n, labels, keys, idx);
    int se = launch_radix_sort(keys, idx, sk1, si1, n, 32, sort_ws, sort_bytes, st);
    if (se != 0) return se;
    hipLaunchKernelGGL(gm_group_key_kernel, flat, blk, 0, st, n, si1, gpos, gk, a.sort_err);
    se = launch_radix_sort(gk, si1, sg, order, n, gauc_bits_for((long long)n + 1), sort_ws, sort_bytes, st);
    if (se != 0) return se;
    a.order = order;
    if (pass == 0) {
      hipLaunchKernelGGL(gm_ideal_kernel, tiles, blk, 0, st, a);
      if (l.ntiles > 1) hipLaunchKernelGGL(gl_sum_carry_kernel, dim3(1), one, 0, st, g);  // (one tile: nothing is open)
    }
  }
  hipLaunchKernelGGL(gm_head_kernel, tiles, blk, 0, st, a);
  hipLaunchKernelGGL(gm_pair_kernel, dim3(l.ntiles, kGwSlabs), blk, 0, st, a);
  hipLaunchKernelGGL(gm_grad_kernel, tiles, blk, 0, st, a);
  hipLaunchKernelGGL(gl_final_kernel, dim3(1), one, 0, st, g);
  return (int)hipGetLastError();
}

}  // namespace fm
