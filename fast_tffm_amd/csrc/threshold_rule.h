// The rules of the threshold metrics (average precision, KS, best F1, operating points), shared by the gfx950
// chain (hip/threshold_metrics.hip) and its CPU twin (cpu/kernels.cpp): the record, the comparison keys of the
// selections with their tie rules, the two target tests and the average precision's term.
//
// Positions count from the highest score down, so "the highest score among equals" is the smallest position;
// with that rule inside every comparison a selection does not depend on the order in which candidates are met.
// A candidate threshold is a run of equal scores with TP + FP > 0, given by (TP, FP, position of the run's
// last example).  T is uint64 (unweighted: every comparison exact) or double (weighted).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define FM_THR_HD __host__ __device__ inline
#else
#define FM_THR_HD inline
#endif

namespace fm {
namespace thr {

constexpr int kMaxTargets = 4;             // precision targets, and recall targets, per call
constexpr int kSel = 2 + kMaxTargets;      // arg-max selections: KS, best F1, the precision targets
constexpr int kNoPos = 0x7fffffff;         // no candidate (loses every comparison against one)

// The record, 64-bit words (T, but word 0): [AP numerator (fp64 bits), P, N, kSel + kMaxTargets points of
// (TP, FP, fp32 bits of the threshold) -- KS, best F1, the precision targets, the recall targets; a point
// without a threshold is all zero (a candidate has TP + FP > 0) --, NaN scores, sort error word].
constexpr int kPoint0 = 3;
constexpr int kPoints = kSel + kMaxTargets;
constexpr int kRecWords = kPoint0 + 3 * kPoints + 2;

struct Targets {
  int np, nr;               // how many of each
  double pt[kMaxTargets];   // precision targets in (0, 1]
  double rt[kMaxTargets];   // recall targets in (0, 1]
};

template <typename T>
struct Cand {
  T tp, fp;
  int pos;
};

template <typename T>
FM_THR_HD Cand<T> no_cand() {
  return Cand<T>{(T)0, (T)0, kNoPos};
}

// KS: |TP / P - FP / N|, in integers as |TP N - FP P| (< 2^60 for n < 2^30).
FM_THR_HD uint64_t ks_key(uint64_t tp, uint64_t fp, uint64_t P, uint64_t N) {
  const uint64_t a = tp * N, b = fp * P;
  return a > b ? a - b : b - a;
}
FM_THR_HD double ks_key(double tp, double fp, double P, double N) {
  const double d = tp / P - fp / N;
  return d < 0 ? -d : d;
}

template <typename T>
FM_THR_HD bool ks_better(const Cand<T>& a, const Cand<T>& b, T P, T N) {
  const auto ka = ks_key(a.tp, a.fp, P, N), kb = ks_key(b.tp, b.fp, P, N);
  return ka > kb || (ka == kb && a.pos < b.pos);
}

// F1 = 2 TP / (PP + P): integers compare the fractions by cross-multiplication (< 2^62 for n < 2^30).
FM_THR_HD double f1_value(double tp, double fp, double P) { return (2.0 * tp) / ((tp + fp) + P); }

FM_THR_HD bool f1_better(const Cand<uint64_t>& a, const Cand<uint64_t>& b, uint64_t P) {
  const uint64_t l = a.tp * (b.tp + b.fp + P), r = b.tp * (a.tp + a.fp + P);
  return l > r || (l == r && a.pos < b.pos);
}
FM_THR_HD bool f1_better(const Cand<double>& a, const Cand<double>& b, double P) {
  const double fa = f1_value(a.tp, a.fp, P), fb = f1_value(b.tp, b.fp, P);
  return fa > fb || (fa == fb && a.pos < b.pos);
}

// A precision target's best point among those that pass precision_ok: the greatest TP.
template <typename T>
FM_THR_HD bool tp_better(const Cand<T>& a, const Cand<T>& b) {
  return a.tp > b.tp || (a.tp == b.tp && a.pos < b.pos);
}

// The two target tests, in fp64 as written: one multiplication, one comparison.
FM_THR_HD bool precision_ok(double tp, double pp, double target) { return tp >= target * pp; }
FM_THR_HD bool recall_ok(double tp, double P, double target) { return tp >= target * P; }

// sum + w TP / PP: the quotient, the product and the sum each rounded once (never a fused multiply-add).
FM_THR_HD double ap_add(double sum, double w, double tp, double pp) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double q = tp / pp;
  const double t = w * q;
  return sum + t;
}

}  // namespace thr
}  // namespace fm
