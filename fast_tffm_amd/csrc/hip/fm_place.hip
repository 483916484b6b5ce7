// The place of a held-out candidate among all candidates, per query, from FM profiles (leave-one-out HR@k /
// NDCG@k / MRR; the reference only scores examples).
//
//   s(q, c) = ((qb[q] + cb[c]) + dot(q, c)) + 0.f      fm_topk.hip's score, bit for bit (fm_rank_common.h)
//   s_t = s(q, target[q]);  greater[q] = #{c : s(q, c) > s_t},  equal[q] = #{c : s(q, c) == s_t}  (>= 1: the target)
//
// and target[q] outside [0, nc) makes q unranked: all zeros.  The target holds the places greater + 1 .. greater +
// equal; the metrics are their exact expectation under uniform tie-breaking (../place_order.h).  Integer counts of
// exact fp32 scores: no atomics, no host read, bitwise repeatable, and independent of the slab plan.  The
// [nq, nc] score matrix never reaches memory.
//
// 1. place_target_kernel: a thread per query runs score_chain, the plain fmaf chain in pi's order -- the chain
//    v_mfma_f32_16x16x4_f32 is -- and leaves s_t and a ranked flag in the workspace.
// 2. place_count_kernel: the hot path, one workgroup of 4 waves per (64-query block, slab).  Wave w keeps the A
//    operands of query tile 4 block + w in registers (load_operands' layout: lane (r, h) holds columns
//    16 g + 4 h .. + 3 of row r).  The candidates go through LDS once per workgroup instead of once per wave: a chunk
//    of NT 16-candidate tiles is staged as NT J items of 64 x 16 bytes, item (T, g) being exactly what the 64 lanes of a
//    wave feed to the matrix instructions 4 g .. 4 g + 3 of tile T, in lane order -- the waves split the items,
//    each a coalesced-per-row 16-byte global load and a contiguous, conflict-free 1 KB LDS write, and every wave
//    then reads its B operands back with contiguous 16-byte LDS reads.  Two buffers: the next chunk's global
//    loads are issued before this chunk's products and land in LDS after them, one barrier per chunk.  A step
//    multiplies two tiles into two independent accumulators; a lane then compares its 4 x 2 scores with its rows'
//    s_t (NaN for a row that is absent or unranked: it never counts) into int32 counters -- no ballot, no LDS, no
//    barrier.  At the slab's end the 16 lanes of an h are added across lanes and lane r == 0 writes (greater,
//    equal) to part[q][slab].  A wave whose tile lies past nq stages and keeps the barriers, and multiplies nothing.
// 3. place_sum_kernel adds a query's parts into counts[nq, 2]; place_metric_kernel sums the metric terms of 1024
//    contexts per workgroup in fp64 in context order, place_final_kernel the tiles in tile order, into the record.
//    fm_shortlist.hip and fm_place_multi.hip run these passes on their own parts and terms.
//
// (Included by module.hip after rank_metrics.hip -- the discount table and its upload.  Every score kernel here is
// compiled without the packed fp32 instructions.)
#include "fm_rank_common.h"

namespace fm {

__device__ double g_rank_harm[kRankMaxCutoff + 1];  // H (rank_table.h), uploaded once per device

struct PlaceArgs : ProfileArgs {
  const int* target;                    // [nq]
  long long slab; int parts;            // place::plan
  float* st;                            // [nq] s_t (workspace)
  int* flag;                            // [nq] 1: ranked (workspace)
  int* part;                            // [nq][parts][2] (workspace)
  int* counts;                          // [nq, 2]
};

// A reduce pass over n contexts: NI integer words, then 3 nk fp64 words (place::rec_words, place::multi_rec_words).
struct MetricArgs {
  long long n;
  const int* counts;   // [n, 2], or [nnz, 2] under MultiMetricArgs
  int nk, k[kRankMaxCutoffs];
  long long ntiles;
  unsigned long long* tiles;  // [ntiles][NI + 3 nk] (unused when ntiles == 1)
  unsigned long long* rec;    // [NI + 3 nk]
};

__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void place_target_kernel(PlaceArgs a) {
  const long long q = (long long)blockIdx.x * kPlaceThreads + threadIdx.x;
  if (q >= a.nq) return;
  const int t = a.target[q];
  const bool ranked = t >= 0 && t < a.nc;
  float s = 0.f;
  if (ranked)
    s = score_of(a.qb[q], a.cb[t], score_chain(a.Q + q * a.q_stride, a.C + (long long)t * a.c_stride, a.Kp));
  a.st[q] = s;
  a.flag[q] = ranked ? 1 : 0;
}

// 16-candidate tiles per staged chunk: two buffers of NT J KB, 32 KB together up to Kp = 128 and 64 KB above
constexpr int place_chunk_tiles(int J) { return J <= 2 ? 8 : J <= 4 ? 4 : 2; }

template <int J>  // column groups of 16: Kp in (16 (J - 1), 16 J]
__global__ FM_PLACE_FN __launch_bounds__(kPlaceThreads) void place_count_kernel(PlaceArgs a, long long qblocks) {
  constexpr int NT = place_chunk_tiles(J);       // tiles per chunk (even: a step takes two)
  constexpr int CH = NT * topk::kTile;           // candidates per chunk
  constexpr int ITEMS = NT * J;                  // 1 KB staging items per chunk
  constexpr int SI = (ITEMS + place::kWaves - 1) / place::kWaves;  // items per wave
  static_assert(CH <= kPlaceThreads && CH <= place::kSlabUnit && place::kSlabUnit % CH == 0, "chunk length");
  __shared__ f32x4 sB[2][ITEMS * kWave];
  __shared__ float sCb[2][CH];

  const int tid = threadIdx.x;
  const int lane = tid & (kWave - 1), w = tid >> 6;
  const int r = lane & 15, h = lane >> 4;
  const long long b = blockIdx.x;
  const long long qblk = b % qblocks;          // consecutive workgroups share a slab (cache reuse)
  const int part = (int)(b / qblocks);
  const long long q0 = (qblk * place::kWaves + w) * topk::kTile;
  const bool active = q0 < a.nq;               // (wave-uniform)
  const long long c_begin = (long long)part * a.slab;
  const long long c_end = c_begin + a.slab < a.nc ? c_begin + a.slab : a.nc;   // > c_begin: part < parts

  // A operands: query row q0 + r (load_operands; an idle wave's stay zero -- a wave-uniform branch, not a per-lane
  // condition on every load)
  f32x4 qa[J];
#pragma unroll
  for (int g = 0; g < J; ++g) qa[g] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (active) {
    const long long qr = q0 + r < a.nq ? q0 + r : a.nq - 1;
    load_operands<J>(a.Q + qr * a.q_stride + 4 * h, h, a.Kp, qa);
  }
  // this lane's 4 result rows: queries q0 + 4 h + i
  float qbv[4], stv[4];
  int gt[4], eq[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long q = q0 + 4 * h + i;
    const bool ok = q < a.nq && a.flag[q] != 0;
    qbv[i] = ok ? a.qb[q] : 0.f;
    stv[i] = ok ? a.st[q] : __builtin_nanf("");
    gt[i] = eq[i] = 0;
  }

  // Staging: item it = T J + g is the B operand of tile T, group g for all 64 lanes (rows past the slab's end are
  // clamped into it: loads stay in bounds, their scores are dropped).  Wave w takes the items w, w + 4, ...
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
  FM_PLACE_BARRIER();
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
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float s0 = ((qbv[i] + cba) + acc0[i]) + 0.f;
          const float s1 = ((qbv[i] + cbb) + acc1[i]) + 0.f;
          gt[i] += (int)(oka && s0 > stv[i]) + (int)(okb && s1 > stv[i]);
          eq[i] += (int)(oka && s0 == stv[i]) + (int)(okb && s1 == stv[i]);
        }
      }
    }
    if (more) store_chunk(buf ^ 1);   // last read before the barrier that ended the previous chunk
    FM_PLACE_BARRIER();
  }

  if (active) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int m = 1; m < topk::kTile; m <<= 1) {
        gt[i] += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, gt[i]);
        eq[i] += __builtin_amdgcn_ds_bpermute((lane ^ m) << 2, eq[i]);
      }
      const long long q = q0 + 4 * h + i;
      if (r == 0 && q < a.nq) {
        int* o = a.part + (q * a.parts + part) * 2;
        o[0] = gt[i];
        o[1] = eq[i];
      }
    }
  }
}

// counts[i] = the sum of row i's parts, of n rows (queries, or entries of fm_place_multi.hip); L lanes (a power of
// two <= 64) per row
__global__ __launch_bounds__(kPlaceThreads) void place_sum_kernel(const int* part, int* counts, long long n, int parts,
                                                                  int L) {
  const long long t = (long long)blockIdx.x * kPlaceThreads + threadIdx.x;
  const long long q = t / L;
  const int sub = (int)(t - q * L);
  int gt = 0, eq = 0;
  if (q < n) {
    const int* p = part + q * parts * 2;
    for (int j = sub; j < parts; j += L) {
      gt += p[2 * j];
      eq += p[2 * j + 1];
    }
  }
  for (int m = 1; m < L; m <<= 1) {
    gt += __shfl_xor(gt, m);
    eq += __shfl_xor(eq, m);
  }
  if (sub == 0 && q < n) {
    counts[2 * q] = gt;
    counts[2 * q + 1] = eq;
  }
}

// The record words of one tile of 1024 contexts: thread c < 3 nk owns fp64 channel c, threads 32 / 33 the two
// integer words; each adds its channel's terms in context order.  (multi_metric_kernel of fm_place_multi.hip is the
// same reduce with other terms and three integer words; written as one function over a terms callback, both kept
// their term arrays in scratch memory, so they stay apart.)
__global__ __launch_bounds__(kPlaceThreads) void place_metric_kernel(MetricArgs m) {
  __shared__ double sd[kPlaceThreads][3 * kRankMaxCutoffs];
  __shared__ long long si[kPlaceThreads][2];
  const int tid = threadIdx.x;
  const long long tile = blockIdx.x;
  const int nch = 3 * m.nk;
  double acc = 0.0;
  long long iacc = 0;
  for (int round = 0; round < place::kMetricTile / kPlaceThreads; ++round) {
    const long long q = tile * place::kMetricTile + round * kPlaceThreads + tid;
    double term[3 * kRankMaxCutoffs] = {};
    long long ranked = 0, ab = 0;
    if (q < m.n) {
      const int gt = m.counts[2 * q], eq = m.counts[2 * q + 1];
      if (gt >= 0 && eq > 0) {
        ranked = 1;
        ab = place::terms(gt, eq, m.k, m.nk, g_rank_dcg, g_rank_harm, term);
      }
    }
    for (int c = 0; c < nch; ++c) sd[tid][c] = term[c];
    si[tid][0] = ranked;
    si[tid][1] = ab;
    __syncthreads();
    if (tid < nch) {
      for (int j = 0; j < kPlaceThreads; ++j) acc += sd[j][tid];
    } else if (tid == 32 || tid == 33) {
      for (int j = 0; j < kPlaceThreads; ++j) iacc += si[j][tid - 32];
    }
    __syncthreads();
  }
  unsigned long long* out = m.ntiles == 1 ? m.rec : m.tiles + tile * place::rec_words(m.nk);
  if (tid < nch) out[2 + tid] = (unsigned long long)__double_as_longlong(acc);
  if (tid == 32 || tid == 33) out[tid - 32] = (unsigned long long)iacc;
}

// The tiles' partial records added in tile order: ni integer words, then the fp64 words.
__global__ __launch_bounds__(kWave) void place_final_kernel(MetricArgs m, int ni) {
  const int tid = threadIdx.x;
  const int words = ni + 3 * m.nk;
  if (tid >= words) return;
  if (tid < ni) {
    long long s = 0;
    for (long long t = 0; t < m.ntiles; ++t) s += (long long)m.tiles[t * words + tid];
    m.rec[tid] = (unsigned long long)s;
  } else {
    double s = 0.0;
    for (long long t = 0; t < m.ntiles; ++t) s += __longlong_as_double((long long)m.tiles[t * words + tid]);
    m.rec[tid] = (unsigned long long)__double_as_longlong(s);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------
inline long long place_tiles(long long n) { return (n + place::kMetricTile - 1) / place::kMetricTile; }
inline long long place_pad8(long long b) { return (b + 7) / 8 * 8; }

// Bytes of a reduce pass's scratch (the tiles' partial records of `words` words; none for up to 1024 contexts).
inline long long metric_workspace_bytes(long long n, int words) {
  const long long t = place_tiles(n);
  return t > 1 ? t * words * 8 : 0;
}
inline long long place_metrics_workspace_bytes(long long n, int nk) {
  return metric_workspace_bytes(n, place::rec_words(nk));
}

// The layout [tiles][s_t][flag][parts] of a call with `parts` partial counts per query: its bytes, and its arrays
// into `a` (ws 8-byte aligned).
inline long long place_layout_bytes(long long nq, int parts, int nk) {
  return place_metrics_workspace_bytes(nq, nk) + place_pad8(nq * 4) * 2 + nq * parts * 8;
}
inline void place_carve(PlaceArgs& a, void* ws, int nk) {
  char* base = static_cast<char*>(ws) + place_metrics_workspace_bytes(a.nq, nk);
  a.st = reinterpret_cast<float*>(base);
  a.flag = reinterpret_cast<int*>(base + place_pad8(a.nq * 4));
  a.part = reinterpret_cast<int*>(base + 2 * place_pad8(a.nq * 4));
}

// Workspace bytes of a launch_place call.
inline long long place_workspace_bytes(long long nq, long long nc, int nk) {
  return place_layout_bytes(nq, place::plan(nq, nc).parts, nk);
}

// D and H on the current device: uploaded by the first call there (a synchronous copy: not inside a capture).
static int place_tables_ready() {
  if (const int rc = rank_table_ready()) return rc;
  static std::mutex mu;
  static bool ready[kRankMaxDevices] = {};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return (int)e;
  if (dev < 0 || dev >= kRankMaxDevices) return -1;
  std::lock_guard<std::mutex> lock(mu);
  if (ready[dev]) return 0;
  static double hsum[kRankMaxCutoff + 1];
  rank_harmonic_table(hsum);
  e = hipMemcpyToSymbol(HIP_SYMBOL(g_rank_harm), hsum, sizeof(hsum));
  if (e != hipSuccess) return (int)e;
  ready[dev] = true;
  return 0;
}

// A reduce pass on st: `m` holds what the tile kernel reads beyond the common fields, which are filled in here.
// 0 or a hip error code; -1: bad arguments; -2: workspace too small; -7: bad cutoffs.
template <int NI, typename M>
inline int launch_metric_pass(void (*tile_kernel)(M), M m, const int* counts, long long n, const int* k, int nk,
                              void* rec, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!rec || n < 1 || n >= (1ll << 31) || (reinterpret_cast<uintptr_t>(rec) & 7) ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return -1;
  if (!rank_cutoffs_ok(k, nk)) return -7;
  if ((long long)ws_bytes < metric_workspace_bytes(n, NI + 3 * nk) || (!ws && place_tiles(n) > 1)) return -2;
  if (const int rc = place_tables_ready()) return rc;
  m.n = n; m.counts = counts; m.nk = nk;
  for (int i = 0; i < nk; ++i) m.k[i] = k[i];
  m.ntiles = place_tiles(n);
  m.tiles = static_cast<unsigned long long*>(ws);
  m.rec = static_cast<unsigned long long*>(rec);
  hipLaunchKernelGGL(tile_kernel, dim3((unsigned)m.ntiles), dim3(kPlaceThreads), 0, st, m);
  if (m.ntiles > 1)
    hipLaunchKernelGGL(place_final_kernel, dim3(1), dim3(kWave), 0, st, static_cast<const MetricArgs&>(m), NI);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// The record of n >= 1 (greater, equal) rows (equal <= 0: unranked) at the nk cutoffs k, asynchronously on st.
inline int launch_place_metrics(const int* counts, long long n, const int* k, int nk, void* rec, void* ws,
                                size_t ws_bytes, hipStream_t st) {
  if (!counts) return -1;
  return launch_metric_pass<2>(place_metric_kernel, MetricArgs{}, counts, n, k, nk, rec, ws, ws_bytes, st);
}

// counts[i] = the sum of row i's `parts` partial counts, of n rows.
inline void launch_place_sum(const int* part, int* counts, long long n, int parts, hipStream_t st) {
  int L = 1;
  while (L < kWave && L < parts) L <<= 1;
  hipLaunchKernelGGL(place_sum_kernel, dim3((unsigned)((n * L + kPlaceThreads - 1) / kPlaceThreads)),
                     dim3(kPlaceThreads), 0, st, part, counts, n, parts, L);
}

// What launch_place and fm_shortlist.hip's launch_place_shortlist ask of their common arguments.
inline bool place_args_ok(const PlaceArgs& a, const void* ws) {
  return profile_rows_ok(a) && a.target && a.counts && ws && !(reinterpret_cast<uintptr_t>(ws) & 7);
}

// fm_seen.hip: takes every query's seen candidates (its target apart) out of counts again.
inline int launch_place_seen(const PlaceArgs& a, const SeenArgs& sn, hipStream_t st);

// counts[nq, 2] and the record of nq >= 1 queries against nc >= 1 candidates; `sn`: the lists of candidates that do
// not compete (null: none, and nothing more is launched).  Codes as launch_metric_pass.
inline int launch_place(PlaceArgs a, const int* k, int nk, void* rec, void* ws, size_t ws_bytes, hipStream_t st,
                        const SeenArgs* sn = nullptr) {
  if (!place_args_ok(a, ws)) return -1;
  if (!rank_cutoffs_ok(k, nk)) return -7;
  if ((long long)ws_bytes < place_workspace_bytes(a.nq, a.nc, nk)) return -2;
  const place::Plan p = place::plan(a.nq, a.nc);
  a.slab = p.slab;
  a.parts = p.parts;
  const long long qblocks = (a.nq + place::kQueryBlock - 1) / place::kQueryBlock;
  const long long blocks = qblocks * a.parts;
  if (blocks >= (1ll << 31)) return -1;
  place_carve(a, ws, nk);
  const unsigned qgrid = (unsigned)((a.nq + kPlaceThreads - 1) / kPlaceThreads);
  hipLaunchKernelGGL(place_target_kernel, dim3(qgrid), dim3(kPlaceThreads), 0, st, a);
  if (dispatch_groups(a.Kp, [&](auto j) {
        hipLaunchKernelGGL((place_count_kernel<decltype(j)::value>), dim3((unsigned)blocks), dim3(kPlaceThreads), 0, st,
                           a, qblocks);
      }))
    return -1;
  launch_place_sum(a.part, a.counts, a.nq, a.parts, st);
  if (hipGetLastError() != hipSuccess) return -3;
  if (sn)
    if (const int rc = launch_place_seen(a, *sn, st)) return rc;
  const long long mbytes = place_metrics_workspace_bytes(a.nq, nk);
  return launch_place_metrics(a.counts, a.nq, k, nk, rec, mbytes ? ws : nullptr, (size_t)mbytes, st);
}

}  // namespace fm
