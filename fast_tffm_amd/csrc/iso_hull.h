// Lower convex hull of the cumulative (weight, positive weight) diagram of an isotonic fit: the predicate,
// the serial stack, and the bridge between two neighbouring hulls -- one definition for the host (cpu/kernels.cpp)
// and for the gfx950 kernels (hip/isotonic.hip).
//
// The diagram has the points (cW[j], cY[j]), j in [0, n]: the weight / positive weight of the sorted positions
// below j.  T is uint64 (unweighted: every product is below 2^60 because n < 2^30, so the predicate is exact) or
// double (weighted).  A hull is an ascending list of positions; every position read from a list is clamped into
// [0, n] before it indexes the diagram, and every loop is a counted loop or a bounded binary search.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FM_ISO_HD __host__ __device__ inline
#else
#define FM_ISO_HD inline
#endif

namespace fm {
namespace iso {

template <typename T>
struct Diagram {
  const T* cW;  // [n + 1]
  const T* cY;  // [n + 1]
  int n;
  FM_ISO_HD int at(int p) const { return p < 0 ? 0 : (p > n ? n : p); }
};

// b lies strictly below the segment a - c (a < b < c: every difference is >= 0).
template <typename T>
FM_ISO_HD bool below(T wa, T ya, T wb, T yb, T wc, T yc) {
  return (yb - ya) * (wc - wb) < (yc - yb) * (wb - wa);
}

template <typename T>
FM_ISO_HD bool below(const Diagram<T>& d, int a, int b, int c) {
  a = d.at(a), b = d.at(b), c = d.at(c);
  return below<T>(d.cW[a], d.cY[a], d.cW[b], d.cY[b], d.cW[c], d.cY[c]);
}

// Serial stack over cnt consecutive points whose coordinates are w[k], y[k] and whose candidate flags are
// cand[k]: st[0 .. return) = the k of the hull's vertices, ascending (collinear points are no vertices).
template <typename T>
FM_ISO_HD int leaf_hull(const T* w, const T* y, const uint8_t* cand, int cnt, int* st) {
  int top = 0;
  for (int c = 0; c < cnt; ++c) {
    if (!cand[c]) continue;
    while (top >= 2 && !below<T>(w[st[top - 2]], y[st[top - 2]], w[st[top - 1]], y[st[top - 1]], w[c], y[c])) --top;
    st[top++] = c;
  }
  return top;
}

// Tangent from position p (left of R) to the hull R[0 .. nR), nR >= 1: the first j with below(p, R[j], R[j + 1]),
// else nR - 1 (false ... false true ... true in j: a binary search).
template <typename T>
FM_ISO_HD int tangent(const Diagram<T>& d, int p, const int* R, int nR) {
  int lo = 0, hi = nR - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (below(d, p, R[mid], R[mid + 1])) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// Bridge of the hulls L[0 .. nL) and R[0 .. nR) (nL, nR >= 1, every position of L before every one of R): the
// merged hull is L[0 .. a] ++ R[b ..).  keep(i) = i == 0 or below(L[i - 1], L[i], R[tangent(L[i])]) holds for a
// prefix of L; a is its last index, b the tangent from L[a].
template <typename T>
FM_ISO_HD void bridge(const Diagram<T>& d, const int* L, int nL, const int* R, int nR, int& a, int& b) {
  int lo = 0, hi = nL - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if (below(d, L[mid - 1], L[mid], R[tangent(d, L[mid], R, nR)])) lo = mid;
    else hi = mid - 1;
  }
  a = lo;
  b = tangent(d, L[lo], R, nR);
}

// The block b of the ascending vertex list H[0 .. nH) that holds sorted position j: H[b] <= j < H[b + 1].
FM_ISO_HD int block_of(const int* H, int nH, int j) {
  int lo = 0, hi = nH - 1;  // first index with H[index] > j, minus one
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (H[mid] > j) hi = mid;
    else lo = mid + 1;
  }
  return lo > 0 ? lo - 1 : 0;
}

// Calibrated probability of score s from the thresholds x[2m] (lo_0, hi_0, lo_1, hi_1, ...: ascending) and values
// y[2m] (v_0, v_0, v_1, v_1, ...), m >= 1; fma is fmaf.
template <typename F>
FM_ISO_HD float calib_value(float s, const float* x, const float* y, int m2, F fma) {
  if (s != s) return s;
  const int m = m2 >> 1;
  if (s <= x[1]) return y[1];
  if (s >= x[m2 - 2]) return y[m2 - 2];
  // the last block b with lo_b <= s (block 0 qualifies: s > hi_0 >= lo_0; block m - 1 does not)
  int lo = 0, hi = m - 1;
  while (lo < hi) {
    const int mid = lo + ((hi - lo + 1) >> 1);
    if (x[2 * mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  const int b = lo < m - 1 ? lo : m - 2;  // (m >= 2 here)
  const float hb = x[2 * b + 1], ln = x[2 * b + 2], vb = y[2 * b], vn = y[2 * b + 2];
  if (s <= hb) return vb;
  const bool inf_hi = ln > 3.4028234663852886e38f, inf_lo = hb < -3.4028234663852886e38f;
  const float t = inf_hi ? (inf_lo ? 0.5f : 0.f) : (inf_lo ? 1.f : (s - hb) / (ln - hb));
  float p = fma(t, vn - vb, vb);
  p = p < vb ? vb : p;
  return p > vn ? vn : p;
}

}  // namespace iso
}  // namespace fm
