// Sparse checkpoints: the rows of a table shard that differ from their initial state.
//
// Table init is counter-based (init.hip: a row's initial value is a function of (seed, global id,
// column) only) and the optimizer slots start from one constant each, so "this row was never
// written" can be decided from the row alone: it still holds, bit for bit, what init_rows and
// torch.full put there.  A checkpoint then stores only the other rows (utils/checkpoint.py) and
// restore regenerates the rest.  No dirty tracking in the training step.
//
// changed_rows: the ascending local rows r < rows for which, over columns 0 .. K-1 (pads ignored),
//   v[r]  differs from init_rows' bits (fp8: the stored bytes, and the row scale; the norm word is
//         derived data and not looked at), or
//   w[r]  differs from init_uniform(seed, gid, 0, range), or
//   a slot (s0v, s0w, s1v, s1w) differs from its initial bit pattern (given by the caller).
//
// Launch chain (kernel boundaries order the steps; no atomics, no kernel waits for a workgroup):
//   flags: one pass over the table, every byte read once.  A wave takes 64 consecutive rows at a
//          time: w / s0w / s1w (and the fp8 scale) with one row per lane, then the factor and state
//          rows with one LPR-lane group per row (fm_common.h), G = 64 / LPR rows per instruction; a
//          ballot folds each group's lanes into the row's bit.  Out: a bitmap (one 64-bit word per
//          64 rows) and the count of set bits per tile of kCkTile rows.
//   scan:  one block turns the tile counts into exclusive 64-bit offsets, in tile order; the last
//          entry is the total (the one value the host reads, to size the output).
//   emit:  one block per tile writes the set bits' row numbers at the tile's offset, in row order.
// (Included by module.hip after metric_common.hip and init.hip: auc_block_scan and the init functions.)
#include "fm_common.h"

namespace fm {

constexpr int kCkWords = 4;                               // bitmap words per wave and tile
constexpr int kCkTile = kWavesPerBlock * kCkWords * 64;   // 1024 rows per tile
constexpr int kCkScanItems = 8;                           // tile counts per thread and round of the scan

struct ChangedArgs {
  const void* v; long long v_stride;      // elements of the table dtype
  const float* w; long long w_stride;     // fp8: [w, scale, norm, pad] rows
  const void* s0v; const void* s1v; long long s_stride;   // s1v / s1w: null when the optimizer has no slot 1
  const float* s0w; const float* s1w;
  long long rows;                         // rows scanned: the local rows whose global id is a real one
  int K, Kp;
  long long gid_mul, gid_add;
  unsigned long long seed; float range;
  uint32_t sv_bits[2], sw_bits[2];        // initial bit patterns of s0v / s1v (fp32, or bf16 in the low half), s0w / s1w
  unsigned long long* bitmap;             // [ceil(rows / 64)]
  unsigned int* tile_cnt;                 // [ntiles]
  long long ntiles;
};

// Does this lane's part of row `r` (columns 4 t .. 4 t + 3, those below K) differ from its init?
// `scale_bits`: fp8, the row's stored scale word.  Every lane of the row's group calls (fp8 reduces
// the row's largest |value| over the group, as store_row does).
template <int LPR, typename TV>
__device__ inline bool ck_row_differs(const ChangedArgs& a, long long r, int t, bool tact, uint32_t scale_bits) {
  const long long gid = r * a.gid_mul + a.gid_add;
  const int c0 = 4 * t;
  float val[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) val[k] = init_uniform(a.seed, gid, c0 + k + 1, a.range);
  bool d = false;
  if constexpr (std::is_same<TV, fp8e4m3>::value) {
    float m = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) m = fmaxf(m, tact && c0 + k < a.K ? fabsf(val[k]) : 0.f);
    m = group_max<LPR>(m);  // (max of non-negative values: the same in any order as init_rows_fp8_kernel's loop)
    const float s = fp8_row_scale(m);
    if (tact) {
      float q[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = c0 + k < a.K ? fminf(fmaxf(val[k] / s, -kFp8Max), kFp8Max) : 0.f;
      int u = __builtin_amdgcn_cvt_pk_fp8_f32(q[0], q[1], 0, false);
      u = __builtin_amdgcn_cvt_pk_fp8_f32(q[2], q[3], u, true);
      const int have = *reinterpret_cast<const int*>(reinterpret_cast<const uint8_t*>(a.v) + r * a.v_stride + c0);
      const int live = a.K - c0 >= 4 ? 4 : a.K - c0;  // bytes of this lane below K
      const uint32_t mask = live >= 4 ? 0xffffffffu : live > 0 ? (1u << (8 * live)) - 1u : 0u;
      d = (((uint32_t)have ^ (uint32_t)u) & mask) != 0u;
      if (t == 0) d = d || scale_bits != __float_as_uint(s);
    }
  } else if constexpr (std::is_same<TV, __hip_bfloat16>::value) {
    if (tact) {
      const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(a.v) + r * a.v_stride + c0);
      const uint32_t have[4] = {h.x & 0xffffu, h.x >> 16, h.y & 0xffffu, h.y >> 16};
#pragma unroll
      for (int k = 0; k < 4; ++k) d = d || (c0 + k < a.K && have[k] != (f32_to_bf16_bits(val[k]) & 0xffffu));
    }
  } else {
    if (tact) {
      const uint4 h = *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(a.v) + r * a.v_stride + c0);
      const uint32_t have[4] = {h.x, h.y, h.z, h.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) d = d || (c0 + k < a.K && have[k] != __float_as_uint(val[k]));
    }
  }
  if (!tact) return false;
  // optimizer slots: bf16 next to fp8 tables (StateBf16), else fp32
#pragma unroll
  for (int slot = 0; slot < 2; ++slot) {
    const void* sp = slot ? a.s1v : a.s0v;
    if (!sp) continue;
    uint32_t have[4];
    if constexpr (StateBf16<TV>::v) {
      const uint2 h = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint16_t*>(sp) + r * a.s_stride + c0);
      have[0] = h.x & 0xffffu; have[1] = h.x >> 16; have[2] = h.y & 0xffffu; have[3] = h.y >> 16;
    } else {
      const uint4 h = *reinterpret_cast<const uint4*>(reinterpret_cast<const float*>(sp) + r * a.s_stride + c0);
      have[0] = h.x; have[1] = h.y; have[2] = h.z; have[3] = h.w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) d = d || (c0 + k < a.K && have[k] != a.sv_bits[slot]);
  }
  return d;
}

template <int LPR, typename TV>
__global__ __launch_bounds__(kBlock) void changed_flags_kernel(ChangedArgs a) {
  constexpr int G = kWave / LPR;
  constexpr unsigned long long kGroupMask = LPR == 64 ? ~0ull : ((1ull << (LPR % 64)) - 1ull);
  __shared__ unsigned int wave_cnt[kWavesPerBlock];
  const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
  const int t = lane % LPR, g = lane / LPR;
  const bool tact = t < a.Kp / 4;
  for (long long tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
    unsigned int cnt = 0;
    for (int j = 0; j < kCkWords; ++j) {
      const long long word = (tile * kWavesPerBlock + wv) * kCkWords + j;
      const long long row0 = word * 64;
      if (row0 >= a.rows) break;  // (wave-uniform)
      // one row per lane: w, the fp32 slots, the fp8 scale
      const long long rl = row0 + lane;
      bool dw = false;
      uint32_t scale_bits = 0;
      if (rl < a.rows) {
        const long long gid = rl * a.gid_mul + a.gid_add;
        dw = __float_as_uint(a.w[rl * a.w_stride]) != __float_as_uint(init_uniform(a.seed, gid, 0, a.range));
        if (a.s0w) dw = dw || __float_as_uint(a.s0w[rl]) != a.sw_bits[0];
        if (a.s1w) dw = dw || __float_as_uint(a.s1w[rl]) != a.sw_bits[1];
        if constexpr (Frag<TV>::kScaled) scale_bits = __float_as_uint(a.w[rl * a.w_stride + 1]);
      }
      unsigned long long bits = __ballot(dw);
      // one LPR-lane group per row
#pragma unroll 4
      for (int i = 0; i < kWave / G; ++i) {
        const int sub = i * G + g;  // row of this group within the word
        const long long r = row0 + sub;
        const uint32_t sb = (uint32_t)__shfl((int)scale_bits, sub, kWave);
        // (rows past the end compare row rows - 1 again and are masked: fp8's group reduction needs every lane)
        const bool live = r < a.rows;
        const bool d = ck_row_differs<LPR, TV>(a, live ? r : a.rows - 1, t, tact, sb) && live;
        const unsigned long long lanes = __ballot(d);
        const bool mine = lane < G && ((lanes >> (lane * LPR % 64)) & kGroupMask) != 0ull;
        bits |= __ballot(mine) << (i * G);
      }
      if (lane == 0) a.bitmap[word] = bits;
      cnt += (unsigned int)__popcll(bits);
    }
    if (lane == 0) wave_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned int tot = 0;
#pragma unroll
      for (int k = 0; k < kWavesPerBlock; ++k) tot += wave_cnt[k];
      a.tile_cnt[tile] = tot;
    }
    __syncthreads();
  }
}

// tile_off[i] = sum of tile_cnt[0 .. i-1], i in [0, ntiles]; one block, tiles in order.
__global__ __launch_bounds__(kBlock) void changed_scan_kernel(const unsigned int* tile_cnt, long long ntiles,
                                                              unsigned long long* tile_off) {
  __shared__ unsigned long long sh[kWavesPerBlock];
  unsigned long long carry = 0;
  for (long long base = 0; base < ntiles; base += (long long)kBlock * kCkScanItems) {
    const long long i0 = base + (long long)threadIdx.x * kCkScanItems;
    unsigned int c[kCkScanItems];
    unsigned long long mine = 0;
#pragma unroll
    for (int q = 0; q < kCkScanItems; ++q) {
      c[q] = i0 + q < ntiles ? tile_cnt[i0 + q] : 0u;
      mine += c[q];
    }
    unsigned long long excl, total;
    auc_block_scan<unsigned long long, kWavesPerBlock>(mine, excl, total, sh);
    unsigned long long o = carry + excl;
#pragma unroll
    for (int q = 0; q < kCkScanItems; ++q) {
      if (i0 + q < ntiles) tile_off[i0 + q] = o;
      o += c[q];
    }
    carry += total;
  }
  if (threadIdx.x == 0) tile_off[ntiles] = carry;
}

// Thread j of a tile's block owns 4 consecutive rows (a nibble of the bitmap).
__global__ __launch_bounds__(kBlock) void changed_emit_kernel(const unsigned long long* bitmap, long long rows,
                                                              long long ntiles, const unsigned long long* tile_off,
                                                              long long* out) {
  __shared__ unsigned int sh[kWavesPerBlock];
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long long row0 = tile * kCkTile + 4 * (long long)threadIdx.x;
    unsigned int nib = 0;
    if (row0 < rows) nib = (unsigned int)(bitmap[row0 >> 6] >> (row0 & 63)) & 15u;
    unsigned int excl, total;
    auc_block_scan<unsigned int, kWavesPerBlock>((unsigned int)__popc(nib), excl, total, sh);
    unsigned long long o = tile_off[tile] + excl;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      if (nib & (1u << b)) out[o++] = row0 + b;
  }
}

size_t changed_workspace_bytes(long long rows) {
  if (rows < 0) rows = 0;
  const size_t words = ((size_t)rows + 63) / 64, ntiles = ((size_t)rows + kCkTile - 1) / kCkTile;
  // [tile_off[ntiles + 1] | bitmap[words] | tile_cnt[ntiles]]
  return 8 * (ntiles + 1) + 8 * words + 4 * ntiles + 16;
}

// Byte offset of the total (a 64-bit count) in the workspace.
size_t changed_total_offset(long long rows) {
  if (rows < 0) rows = 0;
  return 8 * (((size_t)rows + kCkTile - 1) / kCkTile);
}

static void ck_carve(void* ws, long long rows, unsigned long long*& tile_off, unsigned long long*& bitmap,
                     unsigned int*& tile_cnt) {
  const size_t words = ((size_t)rows + 63) / 64, ntiles = ((size_t)rows + kCkTile - 1) / kCkTile;
  tile_off = reinterpret_cast<unsigned long long*>(ws);
  bitmap = tile_off + ntiles + 1;
  tile_cnt = reinterpret_cast<unsigned int*>(bitmap + words);
}

static int ck_grid(long long ntiles) { return (int)(ntiles < 65536 ? ntiles : 65536); }

// flags + scan.  a.rows: the rows to scan (<= 2^31); ws: changed_workspace_bytes(a.rows), 8-byte aligned.
int launch_changed_scan(ChangedArgs a, int dtype, void* ws, size_t ws_bytes, hipStream_t st) {
  if (a.rows < 0 || a.rows > (1ll << 31) || a.K < 1 || a.K > a.Kp || a.Kp % 4 != 0) return -1;
  if (ws_bytes < changed_workspace_bytes(a.rows) || (reinterpret_cast<uintptr_t>(ws) & 7)) return -2;
  if (dtype == kFP8 && a.w_stride <= kFp8Norm) return -1;
  unsigned long long* tile_off;
  ck_carve(ws, a.rows, tile_off, a.bitmap, a.tile_cnt);
  a.ntiles = (a.rows + kCkTile - 1) / kCkTile;
  if (a.ntiles > 0) {
    const int lpr = lanes_per_row(a.Kp, dtype), grid = ck_grid(a.ntiles);
    FM_DISPATCH(dtype, lpr, changed_flags_kernel, grid, st, a);
    if (hipGetLastError() != hipSuccess) return -3;
  }
  hipLaunchKernelGGL(changed_scan_kernel, dim3(1), dim3(kBlock), 0, st, a.tile_cnt, a.ntiles, tile_off);
  return (int)hipGetLastError();
}

// emit: out[total] (the count launch_changed_scan left at changed_total_offset), ascending.
int launch_changed_emit(long long rows, void* ws, long long* out, hipStream_t st) {
  if (rows <= 0) return 0;
  unsigned long long *tile_off, *bitmap;
  unsigned int* tile_cnt;
  ck_carve(ws, rows, tile_off, bitmap, tile_cnt);
  const long long ntiles = (rows + kCkTile - 1) / kCkTile;
  hipLaunchKernelGGL(changed_emit_kernel, dim3(ck_grid(ntiles)), dim3(kBlock), 0, st, bitmap, rows, ntiles, tile_off,
                     out);
  return (int)hipGetLastError();
}

}  // namespace fm
