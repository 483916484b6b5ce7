// Pairwise ranking loss: the logistic loss of every (positive, negative) pair of every group of one batch -- the
// smooth surrogate of what GAUC counts (RankNet; BPR over a group's in-batch negatives).
//
//   s_i score; example i is positive iff y_i > 0; p_i = w_i for a positive (else 0), q_i = w_i for a non-positive
//   (else 0); per group g over its examples in the batch:   P = sum p_i,  N = sum q_j,  c = (P + N) / (P N)
//   L_g = c sum_{i: p_i > 0} sum_{j: q_j > 0} p_i q_j softplus(s_j - s_i)
//   dL/ds_i = -c p_i sum_j q_j sigma(s_j - s_i)   (positive i)      dL/ds_j = +c q_j sum_i p_i sigma(s_j - s_i)
//   softplus(d) = max(d, 0) + log1p(t), sigma(d) = 1 / (1 + t) or t / (1 + t), t = exp(-|d|)
//   a group is valid iff P > 0 and N > 0 (GAUC's rule).  An invalid group, a group of one, an excluded example and
//   an example of weight 0 add exactly 0 and get exactly 0, whatever their scores hold: a pair is evaluated only
//   when p_i > 0 and q_j > 0, and no arithmetic touches the rest.
//
// The plan half is group_loss.hip's (group_plan), read only; this is a second score half, a launch chain on the
// caller's stream into a workspace of its own (no host read, no float atomic, no cross-workgroup wait: capturable):
//   class:  per tile of 1024 sorted positions: the score and one signed class weight (+p, -q or 0) of every
//           position (the only gathers through the sorted index), P and N per group by the segmented tile
//           reduction, and the tile's column span [lo, hi): the union of the ranges of the groups that touch it;
//   carry:  gl_sum_carry_kernel, two channels: the groups that cross tiles;
//   pair:   grid (row tile) x (column slab).  The span is cut into kGpChunk-aligned column chunks, the chunks
//           into kGpSlabs slabs of equally many; a slab stages its chunks (score, signed weight) through LDS and
//           every thread walks, per row it owns, the part of the chunk inside the row's group range, columns
//           ascending, and evaluates the columns of the opposite class.  One fp64 partial per (slab, position):
//           the sigma sum, for a positive row the softplus sum too.  A workgroup whose slab is empty returns;
//   grad:   every position adds its slab partials in slab order; dpred[example] = fp32(grad_scale (-+) c |w| sum);
//           a positive row adds c p_i (its softplus sum) to the tile's loss partial (thread order, block scan);
//   final:  gl_final_kernel: the tile partials in tile order -> fp32 loss.
// Thousands of two-example groups sit several to a wave (a row's walk is as long as its group); one group over the
// whole batch is 128 row tiles x 16 slabs (of 64 chunks each) at B = 131072.  d = (double)s_j - (double)s_i; exp,
// log1p, the division and every sum are fp64; every sum adds non-negative terms in an order fixed by n and the group structure; dpred
// and the loss are rounded once: bitwise the same run to run.  Every pair is evaluated from both of its rows.
// (Included by module.hip after group_loss.hip: GlArgs, GlPos / gl_positions, gl_tile_reduce, the carry and final
// kernels, auc_block_scan and WsCursor are defined before it.)
#include "fm_common.h"

namespace fm {

constexpr int kGpChunk = 128;      // columns staged per step (a row tile's own 1024 columns: 8 or 9 slabs of one)
static_assert(kGpChunk <= kBlock, "one thread stages one column");
constexpr int kGpSlabs = 16;       // column slabs of a row tile's span

struct GpLayout {
  size_t ss, cw, gred, psig, psp, tflag, tv, fv, lpart, tlo, thi, total;
  int ntiles;
};

static GpLayout gp_layout(int n) {
  WsCursor c;
  GpLayout l{};
  const size_t N = (size_t)n;
  l.ntiles = (n + kGlTile - 1) / kGlTile;
  const size_t nt = (size_t)l.ntiles;
  l.ss = c.take(4 * N);
  l.cw = c.take(8 * N);
  l.gred = c.take(8 * 2 * N);
  l.psig = c.take(8 * (size_t)kGpSlabs * N);
  l.psp = c.take(8 * (size_t)kGpSlabs * N);
  l.tflag = c.take(4 * nt);
  l.tv = c.take(8 * 2 * nt);
  l.fv = c.take(8 * 2 * nt);
  l.lpart = c.take(8 * nt);
  l.tlo = c.take(4 * nt);
  l.thi = c.take(4 * nt);
  l.total = c.off;
  return l;
}

// Bytes of the pairwise loss's workspace for up to n examples; 0: n outside [0, 2^30).
size_t group_pair_workspace_bytes(long long n) {
  if (n < 0 || n > (long long)kOsCnt) return 0;
  return gp_layout((int)(n > 0 ? n : 1)).total;
}

struct GpArgs {
  GlArgs g;        // n, ntiles, grad_scale, inputs, the plan, ss, gred [2, n] (P, N), tflag, tv, fv, lpart, outputs
  double* cw;      // [n] signed class weight of every sorted position: +p, -q, 0
  double* psig;    // [kGpSlabs, n] sigma sums
  double* psp;     // [kGpSlabs, n] softplus sums (positive rows)
  int* tlo;        // [ntiles] the tile's column span
  int* thi;
};

// The chunks [cb, ce) of slab s of the span [lo, hi); false: none.
__device__ inline bool gp_slab(int lo, int hi, int s, int& cb, int& ce) {
  if (hi <= lo) return false;
  const int c0 = lo / kGpChunk, c1 = (hi + kGpChunk - 1) / kGpChunk;
  const int per = (c1 - c0 + kGpSlabs - 1) / kGpSlabs;
  cb = c0 + s * per;
  ce = min(c1, cb + per);
  return cb < ce;
}

__global__ __launch_bounds__(kBlock) void gp_class_kernel(GpArgs a) {
  __shared__ int shf[kWavesPerBlock];
  __shared__ double shv[kWavesPerBlock];
  __shared__ int slo, shi;
  const GlArgs& g = a.g;
  if (threadIdx.x == 0) {
    slo = g.n;
    shi = 0;
  }
  __syncthreads();
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  GlPos p;
  gl_positions(g, j0, p);
  double vp[kGlItems], vn[kGlItems];
  int lo = g.n, hi = 0;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    vp[q] = vn[q] = 0.0;
    if (!p.in[q]) continue;
    const int j = j0 + q;
    const int ex = g.sidx[j];
    float sc = 0.f;
    double cw = 0.0;
    if (!p.excl[q] && (unsigned)ex < (unsigned)g.n) {  // (not after a failed sort: its error word is reported)
      const double w = g.weights ? (double)g.weights[ex] : 1.0;
      if (w > 0.0) {
        sc = g.scores[ex];
        if (g.labels[ex] > 0.f) vp[q] = w;
        else vn[q] = w;
        cw = vp[q] - vn[q];
      }
    }
    if (!p.excl[q]) {
      lo = min(lo, p.fi[q]);
      hi = max(hi, min(max(g.end[j], j + 1), g.n));
    }
    g.ss[j] = sc;
    a.cw[j] = cw;
  }
  if (lo < hi) {
    atomicMin(&slo, lo);
    atomicMax(&shi, hi);
  }
  const size_t N = (size_t)g.n, nt = (size_t)g.ntiles;
  gl_tile_reduce<GlAdd>(p, vp, g.gred, g.tv, g.fv, g.tflag, shf, shv);
  gl_tile_reduce<GlAdd>(p, vn, g.gred + N, g.tv + nt, g.fv + nt, nullptr, shf, shv);
  if (threadIdx.x == 0) {  // (the reductions' barriers lie between the atomics and this read)
    a.tlo[blockIdx.x] = min(slo, shi);
    a.thi[blockIdx.x] = shi;
  }
}

__global__ __launch_bounds__(kBlock) void gp_pair_kernel(GpArgs a) {
  __shared__ float shs[kGpChunk];
  __shared__ double shw[kGpChunk];
  const GlArgs& g = a.g;
  const int n = g.n;
  const int lo = max(a.tlo[blockIdx.x], 0), hi = min(a.thi[blockIdx.x], n);
  int cb, ce;
  if (!gp_slab(lo, hi, blockIdx.y, cb, ce)) return;
  const int j0 = blockIdx.x * kGlTile + threadIdx.x * kGlItems;
  int f[kGlItems], e[kGlItems];
  double rs[kGlItems], rw[kGlItems], sig[kGlItems], sp[kGlItems];
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    f[q] = e[q] = 0;
    rs[q] = rw[q] = sig[q] = sp[q] = 0.0;
    if (j >= n) continue;
    const int en = g.end[j];
    const double w = a.cw[j];
    if (en == 0 || w == 0.0) continue;
    const int fi = min(max(g.first[j], 0), j);  // (gl_positions' clamp)
    if (!(g.gred[fi] > 0.0 && g.gred[(size_t)n + fi] > 0.0)) continue;  // an invalid group: no opposite class
    f[q] = max(fi, lo);
    e[q] = min(min(max(en, j + 1), n), hi);
    rs[q] = (double)g.ss[j];
    rw[q] = w;
  }
  for (int c = cb; c < ce; ++c) {
    const int clo = c * kGpChunk;
    if (threadIdx.x < kGpChunk) {
      const int col = clo + (int)threadIdx.x;
      const bool ok = col < n;
      shs[threadIdx.x] = ok ? g.ss[col] : 0.f;
      shw[threadIdx.x] = ok ? a.cw[col] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kGlItems; ++q) {
      const int c0 = max(f[q], clo) - clo, c1 = min(e[q], clo + kGpChunk) - clo;
      const bool pos = rw[q] > 0.0;
      for (int k = c0; k < c1; ++k) {
        const double w = shw[k];
        if (pos ? !(w < 0.0) : !(w > 0.0)) continue;
        const double sc = (double)shs[k];
        const double d = pos ? sc - rs[q] : rs[q] - sc;  // s_neg - s_pos
        const double t = exp(-fabs(d));
        const double aw = fabs(w);
        sig[q] += aw * ((d >= 0.0 ? 1.0 : t) / (1.0 + t));
        if (pos) sp[q] += aw * (fmax(d, 0.0) + log1p(t));
      }
    }
    __syncthreads();
  }
  const size_t base = (size_t)blockIdx.y * (size_t)n;
#pragma unroll
  for (int q = 0; q < kGlItems; ++q) {
    const int j = j0 + q;
    if (j >= n) continue;
    a.psig[base + j] = sig[q];
    a.psp[base + j] = sp[q];
  }
}

__global__ __launch_bounds__(kBlock) void gp_grad_kernel(GpArgs a) {
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
    const int ex = g.sidx[j];
    if ((unsigned)ex >= (unsigned)n) continue;
    const double w = a.cw[j];
    double d = 0.0;
    if (g.end[j] != 0 && w != 0.0) {
      const int fi = min(max(g.first[j], 0), j);
      const double P = g.gred[fi], N = g.gred[(size_t)n + fi];
      if (P > 0.0 && N > 0.0) {
        double sig = 0.0, sp = 0.0;
        for (int s = 0; s < kGpSlabs; ++s) {
          int cb, ce;
          if (!gp_slab(lo, hi, s, cb, ce)) continue;
          sig += a.psig[(size_t)s * n + j];
          if (w > 0.0) sp += a.psp[(size_t)s * n + j];
        }
        const double c = (P + N) / (P * N);
        d = -(c * w) * sig;  // w is signed: -c p sum for a positive, +c q sum for a negative
        if (w > 0.0) lsum += (c * w) * sp;
      }
    }
    g.dpred[ex] = (float)(g.grad_scale * d);
  }
  double ex_, tot;
  auc_block_scan<double, kWavesPerBlock>(lsum, ex_, tot, sh);
  if (threadIdx.x == 0) g.lpart[blockIdx.x] = tot;
}

// The pairwise loss of the n >= 1 examples planned into plan_ws (read only): dpred[n] (example order) and loss[1],
// asynchronously on st; ws (group_pair_workspace_bytes) holds the intermediates.  0 or a hip error code; -1: bad
// arguments; -2: a workspace is too small.
int launch_group_pairwise(const void* plan_ws, size_t plan_bytes, int n, const float* scores, const float* labels,
                          const float* weights, double grad_scale, float* dpred, float* loss, void* ws, size_t ws_bytes,
                          hipStream_t st) {
  if (n < 1 || (unsigned)n > kOsCnt || !plan_ws || !scores || !labels || !dpred || !loss || !ws) return -1;
  if ((reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(plan_ws) & 15)) return -1;
  const GlLayout pl = gl_layout(n);
  const GpLayout l = gp_layout(n);
  if (ws_bytes < l.total || plan_bytes < pl.total) return -2;
  const char* pb = static_cast<const char*>(plan_ws);
  char* b = static_cast<char*>(ws);
  GpArgs a{};
  GlArgs& g = a.g;
  g.n = n;
  g.ntiles = l.ntiles;
  g.grad_scale = grad_scale;
  g.scores = scores;
  g.labels = labels;
  g.weights = weights;
  g.sidx = reinterpret_cast<const int*>(pb + pl.sidx);
  g.first = reinterpret_cast<const int*>(pb + pl.first);
  g.end = reinterpret_cast<const int*>(pb + pl.end);
  g.ss = reinterpret_cast<float*>(b + l.ss);
  g.gred = reinterpret_cast<double*>(b + l.gred);
  g.tflag = reinterpret_cast<int*>(b + l.tflag);
  g.tv = reinterpret_cast<double*>(b + l.tv);
  g.fv = reinterpret_cast<double*>(b + l.fv);
  g.lpart = reinterpret_cast<double*>(b + l.lpart);
  g.dpred = dpred;
  g.loss = loss;
  a.cw = reinterpret_cast<double*>(b + l.cw);
  a.psig = reinterpret_cast<double*>(b + l.psig);
  a.psp = reinterpret_cast<double*>(b + l.psp);
  a.tlo = reinterpret_cast<int*>(b + l.tlo);
  a.thi = reinterpret_cast<int*>(b + l.thi);
  const dim3 tiles(l.ntiles), blk(kBlock), one(kAucBaseThreads);
  hipLaunchKernelGGL(gp_class_kernel, tiles, blk, 0, st, a);
  if (l.ntiles > 1) hipLaunchKernelGGL(gl_sum_carry_kernel, dim3(2), one, 0, st, g);  // (one tile: nothing is open)
  hipLaunchKernelGGL(gp_pair_kernel, dim3(l.ntiles, kGpSlabs), blk, 0, st, a);
  hipLaunchKernelGGL(gp_grad_kernel, tiles, blk, 0, st, a);
  hipLaunchKernelGGL(gl_final_kernel, dim3(1), one, 0, st, g);
  return (int)hipGetLastError();
}

}  // namespace fm
