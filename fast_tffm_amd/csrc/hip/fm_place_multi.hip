// The places of several held-out candidates per context among all candidates, on one pass over the score matrix
// (recall@k / NDCG@k / precision@k of a hold-out split; the reference only scores examples).
//
// The targets are a CSR pair: off int32 [nq + 1], idx int32 [nnz], a context's targets strictly ascending in
// [0, nc).  For every entry (q, t), with fm_topk.hip's score s(q, c) bit for bit,
//   greater = #{c in Comp_q : s(q, c) > s(q, t)},  equal = #{c in Comp_q : s(q, c) == s(q, t)}   (>= 1: t itself)
// over all candidates, or with seen lists over the candidates outside E_q \ T_q.  Every score is computed once and
// placed among all of its context's target scores; fm_place on the contexts repeated once per target computes the
// same counts with |T_q| times the matrix work.  Integer counts of exact fp32 scores, LDS integer adds only: no
// float or global atomics, no cross-workgroup wait, no host read, bitwise repeatable, independent of the slab plan.
//
// 1. Rows.  A context's list is cut into segments of at most S = place::kSegment entries; a row of the count pass
//    is one (context, segment).  multi_rows_tile / _base / _fill_kernel scan ceil(T_q / S) over the contexts
//    (metric_common.hip's block scan per tile of 256, then the tile totals) and write the row table (context, first
//    entry, length); the grid of every later pass is sized from nq + nnz / S, the most rows there can be, and the
//    surplus rows have length 0.
// 2. multi_segment_kernel: 32 lanes per row.  A lane runs score_chain (fm_rank_common.h) for its entry -- nothing
//    else is exact against the matrix instruction -- leaves s(q, t) and the entry's context, and the segment is
//    sorted descending in LDS by rank counting (equal scores in entry order), carrying the entry's position.
// 3. multi_count_kernel: place_count_kernel's skeleton -- one workgroup of 4 waves per (64-row block, slab), a
//    wave's 16 rows' A operands in registers, candidate chunks staged once per workgroup through two LDS buffers in
//    operand order, two tiles per step on v_mfma_f32_16x16x4_f32 -- with a new epilogue.  The workgroup holds its 64
//    rows' sorted thresholds (64 x (S + 1) floats) and one integer histogram per row (64 x (2 S + 1) ints) in LDS; a
//    lane keeps each of its 4 rows' smallest threshold in a register (NaN for an absent row).  A score below it
//    costs one compare.  A score s >= it is placed: lo = #{thr > s} by a branch-free binary search that the lane's
//    8 scores of a step walk together, hi = #{thr >= s} from lo (one more read unless s ties a threshold), and one
//    LDS integer add to bucket lo + hi.  For an entry whose tie run among the sorted thresholds is [L, H): a score
//    equal to it lands in bucket L + H, a greater one in a bucket <= 2 L, a smaller one in a bucket >= 2 H, so
//    equal = hist[L + H] and greater = sum_{f < L + H} hist[f].  At the slab's end four threads per row turn the
//    histogram into its prefix sums and (greater, equal) of every entry goes to part[entry][slab].
// 4. place_sum_kernel (fm_place.hip) adds an entry's parts into counts[nnz, 2], in entry order.
// 5. multi_seen_kernel: place_seen_kernel's method per entry -- 16 lanes stride over the context's seen list, skip
//    the members of T_q (a binary search of the ascending targets), score the rest with score_chain, and the
//    group's first lane subtracts the sums from counts[entry].
// 6. multi_metric_kernel: a thread per context walks its entries (place::multi_terms: fp64 in ascending target
//    order); 1024 contexts per workgroup in context order, place_final_kernel (fm_place.hip) the tiles in tile
//    order, as place_metric_kernel does.  A context with thousands of targets is walked by one thread: correct, but
//    slow.
//
// A malformed list gives unspecified counts but no access out of bounds: windows are clamped to [0, nnz], targets
// into [0, nc), and no row index past the table is written.
// (Included by module.hip after fm_place.hip, whose sum and metric passes it launches.  The score kernels are compiled
// without the packed fp32 instructions.)
#include "fm_rank_common.h"

namespace fm {

constexpr int kMultiScanTile = kBlock;    // contexts per tile of the row scan
constexpr int kMultiSegRows = kBlock / place::kSegment;   // rows per workgroup of multi_segment_kernel
static_assert(place::kSegment == 32, "multi_segment_kernel: one entry per lane of half a wave");

struct MultiArgs : ProfileArgs {
  long long nnz;
  const int* off;       // [nq + 1]
  const int* idx;       // [nnz]
  long long rows_max;   // place::multi_rows_max(nq, nnz)
  long long slab; int parts;   // place::plan(rows_max, nc)
  // workspace
  float* est;           // [nnz] s(q, t) per entry
  int* entq;            // [nnz] the entry's context
  int* rowstart;        // [nq] rows before the context within its scan tile
  int* tiletot;         // [scan tiles + 1] rows before the tile; the last word: the rows there are
  int* rowq;            // [rows_max]
  int* rowbeg;          // [rows_max]
  int* rowlen;          // [rows_max] (0: surplus)
  float* thr;           // [rows_max][S] a row's scores, descending, -inf past its length
  int* ent;             // [rows_max][S] the entry (less rowbeg) at each sorted position
  int* part;            // [nnz][parts][2]
  int* counts;          // [nnz, 2]
};

struct MultiMetricArgs : MetricArgs {   // counts [nnz, 2]; the record: place::multi_rec_words
  long long nnz;
  const int* off;      // [n + 1]
};

__global__ __launch_bounds__(kBlock) void multi_rows_tile_kernel(MultiArgs a) {
  __shared__ int sh[kWavesPerBlock];
  const long long q = (long long)blockIdx.x * kMultiScanTile + threadIdx.x;
  int n = 0;
  if (q < a.nq) {
    int b0, e0;
    csr_window(a.off, a.nnz, q, b0, e0);
    n = (int)place::segments(e0 - b0);
  }
  int excl, total;
  auc_block_scan<int, kWavesPerBlock>(n, excl, total, sh);
  if (q < a.nq) a.rowstart[q] = excl;
  if (threadIdx.x == 0) a.tiletot[blockIdx.x] = total;
}

__global__ __launch_bounds__(kAucBaseThreads) void multi_rows_base_kernel(MultiArgs a, long long ntiles) {
  constexpr int NW = kAucBaseThreads / kWave;
  __shared__ int sh[NW];
  long long carry = 0;
  for (long long base = 0; base < ntiles; base += kAucBaseThreads) {
    const long long t = base + threadIdx.x;
    int excl, total;
    auc_block_scan<int, NW>(t < ntiles ? a.tiletot[t] : 0, excl, total, sh);
    if (t < ntiles) a.tiletot[t] = (int)(carry + excl);
    carry += total;
  }
  if (threadIdx.x == 0) a.tiletot[ntiles] = (int)(carry < a.rows_max ? carry : a.rows_max);
}

__global__ __launch_bounds__(kBlock) void multi_rows_fill_kernel(MultiArgs a, long long ntiles) {
  const long long i = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (i < a.nq) {
    int b0, e0;
    csr_window(a.off, a.nnz, i, b0, e0);
    const long long base = (long long)a.tiletot[i / kMultiScanTile] + a.rowstart[i];
    for (long long seg = 0; b0 + seg * place::kSegment < e0; ++seg) {
      const long long r = base + seg;
      if (r >= a.rows_max) break;   // (only a malformed list gets here)
      const int left = e0 - b0 - (int)seg * place::kSegment;
      a.rowq[r] = (int)i;
      a.rowbeg[r] = b0 + (int)seg * place::kSegment;
      a.rowlen[r] = left < place::kSegment ? left : place::kSegment;
    }
  }
  if (i < a.rows_max && i >= a.tiletot[ntiles]) a.rowq[i] = a.rowbeg[i] = a.rowlen[i] = 0;
}

__global__ FM_PLACE_FN __launch_bounds__(kBlock) void multi_segment_kernel(MultiArgs a) {
  constexpr int S = place::kSegment;
  __shared__ uint32_t skey[kMultiSegRows][S];
  const int tid = threadIdx.x;
  const int rl = tid / S, j = tid % S;
  const long long row = (long long)blockIdx.x * kMultiSegRows + rl;
  const int len = row < a.rows_max ? a.rowlen[row] : 0;
  float s = -__builtin_inff();
  if (j < len) {
    const long long q = a.rowq[row];
    const long long e = (long long)a.rowbeg[row] + j;
    int t = a.idx[e];
    t = t < 0 ? 0 : t >= a.nc ? (int)(a.nc - 1) : t;
    s = score_of(a.qb[q], a.cb[t], score_chain(a.Q + q * a.q_stride, a.C + (long long)t * a.c_stride, a.Kp));
    a.est[e] = s;
    a.entq[e] = (int)q;
  }
  // the order-preserving image of the score (a total order: the ranks are a permutation of 0 .. len - 1)
  const uint32_t key = topk::order_u32(__builtin_bit_cast(uint32_t, s));
  skey[rl][j] = key;
  FM_PLACE_BARRIER();
  if (row >= a.rows_max) return;
  int rank = j;   // (past the length: -inf stays where it is)
  if (j < len) {
    rank = 0;
    for (int i = 0; i < len; ++i) {
      const uint32_t ki = skey[rl][i];
      rank += (int)(ki > key || (ki == key && i < j));
    }
  }
  a.thr[row * S + rank] = s;
  a.ent[row * S + rank] = j < len ? j : 0;
}

template <int J>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void multi_count_kernel(MultiArgs a, long long rblocks) {
  constexpr int NT = place_chunk_tiles(J);
  constexpr int CH = NT * topk::kTile;
  constexpr int ITEMS = NT * J;
  constexpr int SI = (ITEMS + place::kWaves - 1) / place::kWaves;
  constexpr int S = place::kSegment;
  constexpr int TS = S + 1;        // a row's thresholds and one -inf (odd: rows start in different banks)
  constexpr int HB = 2 * S + 1;    // a row's buckets lo + hi in [0, 2 S]
  constexpr int RB = place::kQueryBlock;
  static_assert(CH <= kPlaceThreads && CH <= place::kSlabUnit && place::kSlabUnit % CH == 0, "chunk length");
  __shared__ f32x4 sB[2][ITEMS * kWave];
  __shared__ float sCb[2][CH];
  __shared__ float sThr[RB * TS];
  __shared__ int sH[RB * HB];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid >> 6;
  const int r = lane & 15, h = lane >> 4;
  const long long b = blockIdx.x;
  const long long rblk = b % rblocks;          // consecutive workgroups share a slab (cache reuse)
  const int part = (int)(b / rblocks);
  const long long nrows = a.tiletot[(a.nq + kMultiScanTile - 1) / kMultiScanTile];
  if (rblk * RB >= nrows) return;              // a surplus block (workgroup-uniform, before any barrier)
  const long long r0 = (rblk * place::kWaves + w) * topk::kTile;
  const bool active = r0 < nrows;              // (wave-uniform)
  const long long c_begin = (long long)part * a.slab;
  const long long c_end = c_begin + a.slab < a.nc ? c_begin + a.slab : a.nc;   // > c_begin: part < parts

  for (int i = tid; i < RB * TS; i += kPlaceThreads) {
    const int rl = i / TS, j = i - rl * TS;
    const long long R = rblk * RB + rl;
    sThr[i] = (R < nrows && j < S) ? a.thr[R * S + j] : -__builtin_inff();
  }
  for (int i = tid; i < RB * HB; i += kPlaceThreads) sH[i] = 0;

  // A operands: the context of row r0 + r (load_operands; an idle wave's stay zero, as in place_count_kernel)
  f32x4 qa[J];
#pragma unroll
  for (int g = 0; g < J; ++g) qa[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    const long long qr = r0 + r < nrows ? a.rowq[r0 + r] : a.rowq[nrows - 1];
    load_operands<J>(a.Q + qr * a.q_stride + 4 * h, h, a.Kp, qa);
  }
  // this lane's 4 result rows r0 + 4 h + i: the context's base score and the row's smallest threshold
  float qbv[4], mn[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long R = r0 + 4 * h + i;
    const bool ok = R < nrows;
    qbv[i] = ok ? a.qb[a.rowq[R]] : 0.f;
    mn[i] = ok ? a.thr[R * S + a.rowlen[R] - 1] : __builtin_nanf("");
  }
  const float* th0 = sThr + (topk::kTile * w + 4 * h) * TS;   // row i of this lane: th0 + i TS
  int* hb0 = sH + (topk::kTile * w + 4 * h) * HB;

  f32x4 stg[SI];
  float stcb = 0.f;
  const auto load_chunk = [&](long long c0) FM_PLACE_FN {
#pragma unroll
    for (int s = 0; s < SI; ++s) {
      const int it = w + place::kWaves * s;
      stg[s] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (it < ITEMS) {
        const int T = it / J, g = it - T * J;
        const long long c = c0 + T * topk::kTile + r;
        const long long lc = c < c_end ? c : c_end - 1;
        stg[s] = load_fragment(a.C + lc * a.c_stride + 4 * h, g, h, a.Kp);
      }
    }
    if (tid < CH) {
      const long long c = c0 + tid;
      stcb = a.cb[c < c_end ? c : c_end - 1];
    }
  };
  const auto store_chunk = [&](int buf) FM_PLACE_FN {
#pragma unroll
    for (int s = 0; s < SI; ++s) {
      const int it = w + place::kWaves * s;
      if (it < ITEMS) sB[buf][it * kWave + lane] = stg[s];
    }
    if (tid < CH) sCb[buf][tid] = stcb;
  };

  load_chunk(c_begin);
  store_chunk(0);
  FM_PLACE_BARRIER();   // (also: the thresholds and the zeroed histograms)
  int buf = 0;
  for (long long c0 = c_begin; c0 < c_end; c0 += CH, buf ^= 1) {
    const bool more = c0 + CH < c_end;   // (workgroup-uniform)
    if (more) load_chunk(c0 + CH);
    if (active) {
#pragma unroll
      for (int T = 0; T < NT; T += 2) {
        const long long ct = c0 + T * topk::kTile;
        if (ct >= c_end) break;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        const f32x4* pa = &sB[buf][(T * J) * kWave + lane];
        const f32x4* pb = pa + J * kWave;
#pragma unroll
        for (int g = 0; g < J; ++g) {
          const f32x4 va = pa[g * kWave], vb = pb[g * kWave];
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], va[e], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(qa[g][e], vb[e], acc1, 0, 0, 0);
          }
        }
        const float cba = sCb[buf][T * topk::kTile + r], cbb = sCb[buf][(T + 1) * topk::kTile + r];
        const bool oka = ct + r < c_end, okb = ct + topk::kTile + r < c_end;
        float sc[8];
        bool tk[8], any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          sc[2 * i] = ((qbv[i] + cba) + acc0[i]) + 0.f;
          sc[2 * i + 1] = ((qbv[i] + cbb) + acc1[i]) + 0.f;
          tk[2 * i] = oka && sc[2 * i] >= mn[i];
          tk[2 * i + 1] = okb && sc[2 * i + 1] >= mn[i];
          any = any || tk[2 * i] || tk[2 * i + 1];
        }
        if (any) {
          // lo = #{thr > s} of all 8 scores together (a score that is not taken walks along: every read stays
          // inside its row's S + 1 words)
          int lo[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) lo[u] = 0;
#pragma unroll
          for (int step = S / 2; step >= 1; step >>= 1)
#pragma unroll
            for (int u = 0; u < 8; ++u) lo[u] += th0[(u >> 1) * TS + lo[u] + step - 1] > sc[u] ? step : 0;
#pragma unroll
          for (int u = 0; u < 8; ++u) lo[u] += th0[(u >> 1) * TS + lo[u]] > sc[u] ? 1 : 0;
          float at[8];
#pragma unroll
          for (int u = 0; u < 8; ++u) at[u] = th0[(u >> 1) * TS + lo[u]];   // (lo == S: the -inf behind the row)
#pragma unroll
          for (int u = 0; u < 8; ++u)
            if (tk[u]) {
              int hi = lo[u];
              if (at[u] == sc[u]) {   // the score ties a threshold: the run's end
                ++hi;
                while (hi < S && th0[(u >> 1) * TS + hi] == sc[u]) ++hi;
              }
              __hip_atomic_fetch_add(hb0 + (u >> 1) * HB + lo[u] + hi, 1, __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
      }
    }
    if (more) store_chunk(buf ^ 1);   // last read before the barrier that ended the previous chunk
    FM_PLACE_BARRIER();
  }

  // every row's histogram into its inclusive prefix sums: four threads per row, a quarter of the buckets each
  {
    constexpr int QB = (HB + 3) / 4;
    int* hrow = sH + (tid >> 2) * HB;
    const int sub = tid & 3;
    const int f0 = sub * QB, f1 = f0 + QB < HB ? f0 + QB : HB;
    int sum = 0;
    for (int f = f0; f < f1; ++f) sum += hrow[f];
    int run = 0;
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int o = __builtin_amdgcn_ds_bpermute(((lane & ~3) + m) << 2, sum);
      run += m < sub ? o : 0;
    }
    for (int f = f0; f < f1; ++f) {
      run += hrow[f];
      hrow[f] = run;
    }
  }
  FM_PLACE_BARRIER();
  for (int i = tid; i < RB * S; i += kPlaceThreads) {
    const int rl = i / S, j = i - rl * S;
    const long long R = rblk * RB + rl;
    if (R >= nrows) continue;
    const int len = a.rowlen[R];
    if (j >= len) continue;
    const float* th = sThr + rl * TS;
    const float v = th[j];
    int L = j, H = j + 1;   // the tie run [L, H) of position j
    while (L > 0 && th[L - 1] == v) --L;
    while (H < len && th[H] == v) ++H;
    const int below = sH[rl * HB + L + H - 1], upto = sH[rl * HB + L + H];   // (L + H >= 1)
    const long long e = (long long)a.rowbeg[R] + a.ent[R * S + j];
    int* o = a.part + (e * a.parts + part) * 2;
    o[0] = below;
    o[1] = upto - below;
  }
}

constexpr int kMultiSeenLanes = 16;  // lanes per entry of multi_seen_kernel

__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void multi_seen_kernel(MultiArgs a, SeenArgs sn) {
  const int tid = threadIdx.x;
  const int sub = tid & (kMultiSeenLanes - 1);
  const long long e = ((long long)blockIdx.x * kPlaceThreads + tid) / kMultiSeenLanes;
  int gt = 0, eq = 0;
  if (e < a.nnz) {
    const int qe = a.entq[e];
    const long long q = qe < 0 ? 0 : qe >= a.nq ? a.nq - 1 : qe;   // (in range unless the lists are malformed)
    int b0, e0, t0, t1;
    csr_window(sn.off, sn.nnz, q, b0, e0);
    csr_window(a.off, a.nnz, q, t0, t1);
    const float ste = a.est[e], qbq = a.qb[q];
    const float* qr = a.Q + q * a.q_stride;
    for (int p = b0 + sub; p < e0; p += kMultiSeenLanes) {
      const int c = sn.idx[p];
      if (c < 0 || c >= a.nc) continue;
      if (seen_contains(a.idx, t0, t1, c)) continue;   // one of the context's targets: they always compete
      const float s = score_of(qbq, a.cb[c], score_chain(qr, a.C + (long long)c * a.c_stride, a.Kp));
      gt += (int)(s > ste);
      eq += (int)(s == ste);
    }
  }
  const int lane = tid & (kWave - 1);
#pragma unroll
  for (int m = 1; m < kMultiSeenLanes; m <<= 1) {
    gt += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, gt);
    eq += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, eq);
  }
  if (e < a.nnz && sub == 0 && (gt | eq)) {
    a.counts[2 * e] -= gt;
    a.counts[2 * e + 1] -= eq;
  }
}

// The record words of one tile of 1024 contexts: thread c < 3 nk owns fp64 channel c, threads 32 .. 34 the three
// integer words; each adds its channel's terms in context order (place_metric_kernel's reduce).
__global__ __launch_bounds__(kPlaceThreads) void multi_metric_kernel(MultiMetricArgs m) {
  __shared__ double sd[kPlaceThreads][3 * kRankMaxCutoffs];
  __shared__ long long si[kPlaceThreads][3];
  const int tid = threadIdx.x;
  const long long tile = blockIdx.x;
  const int nch = 3 * m.nk;
  double acc = 0.0;
  long long iacc = 0;
  for (int round = 0; round < place::kMetricTile / kPlaceThreads; ++round) {
    const long long q = tile * place::kMetricTile + round * kPlaceThreads + tid;
    double term[3 * kRankMaxCutoffs] = {};
    long long ranked = 0, entries = 0, ab = 0;
    if (q < m.n) {
      int b0, e0;
      csr_window(m.off, m.nnz, q, b0, e0);
      if (e0 > b0) {
        ranked = 1;
        entries = e0 - b0;
        ab = place::multi_terms(m.counts + 2 * (long long)b0, entries, m.k, m.nk, g_rank_dcg, term);
      }
    }
    for (int c = 0; c < nch; ++c) sd[tid][c] = term[c];
    si[tid][0] = ranked;
    si[tid][1] = entries;
    si[tid][2] = ab;
    __syncthreads();
    if (tid < nch) {
      for (int j = 0; j < kPlaceThreads; ++j) acc += sd[j][tid];
    } else if (tid >= 32 && tid < 35) {
      for (int j = 0; j < kPlaceThreads; ++j) iacc += si[j][tid - 32];
    }
    __syncthreads();
  }
  unsigned long long* out = m.ntiles == 1 ? m.rec : m.tiles + tile * place::multi_rec_words(m.nk);
  if (tid < nch) out[3 + tid] = (unsigned long long)__double_as_longlong(acc);
  if (tid >= 32 && tid < 35) out[tid - 32] = (unsigned long long)iacc;
}

// ---- host side ------------------------------------------------------------------------------------------------
inline long long multi_scan_tiles(long long nq) { return (nq + kMultiScanTile - 1) / kMultiScanTile; }

// Bytes of place_multi_metrics' scratch (the tiles' partial records; none for up to 1024 contexts).
inline long long place_multi_metrics_workspace_bytes(long long n, int nk) {
  return metric_workspace_bytes(n, place::multi_rec_words(nk));
}

// Workspace bytes of a launch_place_multi call:
// [tiles][est][entq][rowstart][tiletot][rowq][rowbeg][rowlen][thr][ent][part].
inline long long place_multi_workspace_bytes(long long nq, long long nc, long long nnz, int nk) {
  const long long rows = place::multi_rows_max(nq, nnz);
  const place::Plan p = place::plan(rows, nc);
  return place_multi_metrics_workspace_bytes(nq, nk) + 2 * place_pad8(nnz * 4) + place_pad8(nq * 4) +
         place_pad8((multi_scan_tiles(nq) + 1) * 4) + 3 * place_pad8(rows * 4) +
         2 * place_pad8(rows * place::kSegment * 4) + nnz * p.parts * 8;
}

// The record of n >= 1 contexts from the (greater, equal) pairs of their entries (off [n + 1] over counts [nnz, 2]),
// asynchronously on st.  Codes as launch_metric_pass.
inline int launch_place_multi_metrics(const int* counts, const int* off, long long n, long long nnz, const int* k,
                                      int nk, void* rec, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!off || nnz < 0 || nnz >= (1ll << 31) || (!counts && nnz)) return -1;
  MultiMetricArgs m{};
  m.nnz = nnz; m.off = off;
  return launch_metric_pass<3>(multi_metric_kernel, m, counts, n, k, nk, rec, ws, ws_bytes, st);
}

// counts[nnz, 2] and the record of nq >= 1 contexts with nnz >= 0 targets together against nc >= 1 candidates;
// `sn`: the lists of candidates that do not compete (null: none).  Codes as launch_metric_pass.
inline int launch_place_multi(MultiArgs a, const int* k, int nk, void* rec, void* ws, size_t ws_bytes,
                              hipStream_t st, const SeenArgs* sn = nullptr) {
  a.rows_max = place::multi_rows_max(a.nq, a.nnz);
  if (!profile_rows_ok(a) || a.nnz < 0 || a.rows_max >= (1ll << 31) || !a.off || (a.nnz && (!a.idx || !a.counts)) ||
      !ws || (reinterpret_cast<uintptr_t>(ws) & 7))
    return -1;
  if (!rank_cutoffs_ok(k, nk)) return -7;
  if ((long long)ws_bytes < place_multi_workspace_bytes(a.nq, a.nc, a.nnz, nk)) return -2;
  if (sn && !seen_args_ok(*sn)) return -1;
  const place::Plan p = place::plan(a.rows_max, a.nc);
  a.slab = p.slab;
  a.parts = p.parts;
  const long long rblocks = (a.rows_max + place::kQueryBlock - 1) / place::kQueryBlock;
  const long long blocks = rblocks * a.parts;
  if (blocks >= (1ll << 31)) return -1;
  const long long stiles = multi_scan_tiles(a.nq);
  const long long mbytes = place_multi_metrics_workspace_bytes(a.nq, nk);
  char* cur = static_cast<char*>(ws) + mbytes;
  const auto take = [&cur](long long bytes) {
    char* at = cur;
    cur += place_pad8(bytes);
    return at;
  };
  a.est = reinterpret_cast<float*>(take(a.nnz * 4));
  a.entq = reinterpret_cast<int*>(take(a.nnz * 4));
  a.rowstart = reinterpret_cast<int*>(take(a.nq * 4));
  a.tiletot = reinterpret_cast<int*>(take((stiles + 1) * 4));
  a.rowq = reinterpret_cast<int*>(take(a.rows_max * 4));
  a.rowbeg = reinterpret_cast<int*>(take(a.rows_max * 4));
  a.rowlen = reinterpret_cast<int*>(take(a.rows_max * 4));
  a.thr = reinterpret_cast<float*>(take(a.rows_max * place::kSegment * 4));
  a.ent = reinterpret_cast<int*>(take(a.rows_max * place::kSegment * 4));
  a.part = reinterpret_cast<int*>(cur);
  if (a.nnz) {
    const auto grid = [](long long threads) { return dim3((unsigned)((threads + kBlock - 1) / kBlock)); };
    hipLaunchKernelGGL(multi_rows_tile_kernel, dim3((unsigned)stiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(multi_rows_base_kernel, dim3(1), dim3(kAucBaseThreads), 0, st, a, stiles);
    hipLaunchKernelGGL(multi_rows_fill_kernel, grid(a.nq > a.rows_max ? a.nq : a.rows_max), dim3(kBlock), 0, st, a,
                       stiles);
    hipLaunchKernelGGL(multi_segment_kernel, grid(a.rows_max * place::kSegment), dim3(kBlock), 0, st, a);
    if (dispatch_groups(a.Kp, [&](auto j) {
          hipLaunchKernelGGL((multi_count_kernel<decltype(j)::value>), dim3((unsigned)blocks), dim3(kPlaceThreads), 0,
                             st, a, rblocks);
        }))
      return -1;
    launch_place_sum(a.part, a.counts, a.nnz, a.parts, st);
    if (sn)
      hipLaunchKernelGGL(multi_seen_kernel, grid(a.nnz * kMultiSeenLanes), dim3(kPlaceThreads), 0, st, a, *sn);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  return launch_place_multi_metrics(a.counts, a.off, a.nq, a.nnz, k, nk, rec, mbytes ? ws : nullptr, (size_t)mbytes,
                                    st);
}

}  // namespace fm
