// What the pair losses (group_pair.hip, group_lambda.hip) share of their column walk: every row of a group meets the
// columns of its group that its loss pairs it with, and the meetings are summed per row.
//   span:   a row tile's column span [lo, hi) is the union of what its rows need (GwSpan: block min / max in LDS);
//   pair:   grid (row tile) x (column slab).  The span is cut into kGwChunk-aligned column chunks, the chunks into
//           kGwSlabs slabs of equally many (gw_slab); a slab stages its chunks through LDS and every thread walks
//           its rows' own column ranges, adding gw_sigma / gw_softplus terms: one fp64 partial set per (slab,
//           position).  Each loss writes this kernel out itself (gp_pair_kernel, gm_pair_kernel): as one template
//           over what a column and a row carry, the LambdaRank kernel's sums went to 80-112 bytes of scratch a lane;
//   grad:   every position adds its slab partials in slab order over the non-empty slabs (gw_slab again), finishes
//           them into dpred[example] = fp32(grad_scale d) and a term of the tile's loss partial.  Written out per
//           loss too: as one template the second partial's load waited for the first one's in every slab (+7 us on
//           groups of 8 at B = 131072).
// Every sum is fp64 over non-negative terms in an order fixed by n and the group structure.  (Included by module.hip
// after group_loss.hip, whose kBlock-sized tiles the geometry cuts.)
#include "fm_common.h"

namespace fm {

constexpr int kGwChunk = 128;      // columns staged per step (a row tile's own 1024 columns: 8 or 9 slabs of one)
static_assert(kGwChunk <= kBlock, "one thread stages one column");
constexpr int kGwSlabs = 16;       // column slabs of a row tile's span

// The chunks [cb, ce) of slab s of the span [lo, hi); false: none.
__device__ inline bool gw_slab(int lo, int hi, int s, int& cb, int& ce) {
  if (hi <= lo) return false;
  const int c0 = lo / kGwChunk, c1 = (hi + kGwChunk - 1) / kGwChunk;
  const int per = (c1 - c0 + kGwSlabs - 1) / kGwSlabs;
  cb = c0 + s * per;
  ce = min(c1, cb + per);
  return cb < ce;
}

// A row tile's column span, one in LDS per workgroup: open (a barrier ends it), every thread adds the union [lo, hi)
// of its rows' ranges, close writes tlo / thi of the tile.  close has no barrier of its own: the caller puts one
// between the last add and it -- __syncthreads, or a block reduction that has some.
struct GwSpan {
  int lo, hi;
};

__device__ inline void gw_span_open(GwSpan& s, int n) {
  if (threadIdx.x == 0) {
    s.lo = n;
    s.hi = 0;
  }
  __syncthreads();
}

__device__ inline void gw_span_add(GwSpan& s, int lo, int hi) {
  if (lo < hi) {
    atomicMin(&s.lo, lo);
    atomicMax(&s.hi, hi);
  }
}

__device__ inline void gw_span_close(const GwSpan& s, int* tlo, int* thi) {
  if (threadIdx.x == 0) {
    tlo[blockIdx.x] = min(s.lo, s.hi);
    thi[blockIdx.x] = s.hi;
  }
}

// The logistic pair term of d = s_lower - s_upper with t = exp(-|d|): sigma(d) and softplus(d).
__device__ inline double gw_sigma(double d, double t) { return (d >= 0.0 ? 1.0 : t) / (1.0 + t); }
__device__ inline double gw_softplus(double d, double t) { return fmax(d, 0.0) + log1p(t); }

}  // namespace fm
