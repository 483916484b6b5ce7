#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <numeric>
#include <type_traits>
#include <vector>

#include <omp.h>

#include "../hash64.h"
#include "../iso_hull.h"
#include "../rank_table.h"
#include "../score_key.h"
#include "../threshold_rule.h"
#include "../topk_order.h"

namespace fm {
namespace cpu {

namespace {

inline float bf16_to_f32(uint16_t h) {
  uint32_t u = static_cast<uint32_t>(h) << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

inline uint16_t f32_to_bf16(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u && (u & 0x7fffffu)) return static_cast<uint16_t>((u >> 16) | 0x40u);
  return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

inline void load_row(const void* v, long long off, int Kp, int dtype, float* dst) {
  if (dtype == 1) {
    const uint16_t* p = static_cast<const uint16_t*>(v) + off;
    for (int k = 0; k < Kp; ++k) dst[k] = bf16_to_f32(p[k]);
  } else {
    std::memcpy(dst, static_cast<const float*>(v) + off, sizeof(float) * Kp);
  }
}

inline void store_row(void* v, long long off, int Kp, int dtype, const float* src) {
  if (dtype == 1) {
    uint16_t* p = static_cast<uint16_t*>(v) + off;
    for (int k = 0; k < Kp; ++k) p[k] = f32_to_bf16(src[k]);
  } else {
    std::memcpy(static_cast<float*>(v) + off, src, sizeof(float) * Kp);
  }
}

inline void opt_step(const OptParams& o, float g, float& p, float& s0, float& s1) {
  if (o.type == 0) {
    s0 += g * g;
    p -= o.lr * g / std::sqrt(s0);
  } else if (o.type == 1) {
    const float n_new = s0 + g * g;
    const float sq_old = std::sqrt(s0), sq_new = std::sqrt(n_new);
    s1 += g - (sq_new - sq_old) / o.lr * p;
    s0 = n_new;
    const float quad = (o.beta + sq_new) / o.lr + 2.f * o.l2;
    p = std::fabs(s1) > o.l1 ? (std::copysign(o.l1, s1) - s1) / quad : 0.f;
  } else {
    p -= o.lr * g;
  }
}

inline void set_threads(int threads) {
  if (threads > 0) omp_set_num_threads(threads);
}

void update_row(const OptParams& opt, long long row, const float* g, float gw, int Kp, void* v, long long v_stride,
                float* w, long long w_stride, float* s0v, float* s1v, long long s_stride, float* s0w, float* s1w,
                int dtype, float* scratch) {
  load_row(v, row * v_stride, Kp, dtype, scratch);
  float* a0 = s0v + row * s_stride;
  float* a1 = s1v ? s1v + row * s_stride : nullptr;
  for (int k = 0; k < Kp; ++k) {
    float z = a1 ? a1[k] : 0.f;
    opt_step(opt, g[k], scratch[k], a0[k], z);
    if (a1) a1[k] = z;
  }
  store_row(v, row * v_stride, Kp, dtype, scratch);
  float& pw = w[row * w_stride];
  float z = s1w ? s1w[row] : 0.f;
  opt_step(opt, gw, pw, s0w[row], z);
  if (s1w) s1w[row] = z;
}

}  // namespace

FwdResult fwd(int B, const int* offsets, const int* rows, const float* vals, const void* v, long long v_stride,
              const float* w, long long w_stride, int Kp, int dtype, const float* labels, const float* weights,
              int loss_type, float grad_scale, float* pred, float* r1, float* dpred, int threads,
              const float* bias) {
  set_threads(threads);
  double loss_sum = 0, regv_sum = 0, regw_sum = 0;
#pragma omp parallel reduction(+ : loss_sum, regv_sum, regw_sum)
  {
    std::vector<float> s1(Kp), s2(Kp), row(Kp);
#pragma omp for schedule(static)
    for (int i = 0; i < B; ++i) {
      std::fill(s1.begin(), s1.end(), 0.f);
      std::fill(s2.begin(), s2.end(), 0.f);
      float lin = 0.f, rv = 0.f, rw = 0.f;
      for (int j = offsets[i]; j < offsets[i + 1]; ++j) {
        const long long r = rows[j];
        const float x = vals ? vals[j] : 1.f;
        load_row(v, r * v_stride, Kp, dtype, row.data());
        const float wv = w[r * w_stride];
        for (int k = 0; k < Kp; ++k) {
          const float xv = x * row[k];
          s1[k] += xv;
          s2[k] += xv * xv;
          rv += row[k] * row[k];
        }
        lin += x * wv;
        rw += wv * wv;
      }
      float part = 0.f;
      for (int k = 0; k < Kp; ++k) part += s1[k] * s1[k] - s2[k];
      const float p = lin + 0.5f * part + (bias ? bias[0] : 0.f);
      pred[i] = p;
      if (r1) std::memcpy(r1 + (long long)i * Kp, s1.data(), sizeof(float) * Kp);
      regv_sum += rv;
      regw_sum += rw;
      if (loss_type != 0) {
        const float y = labels[i];
        const float wt = weights ? weights[i] : 1.f;
        float l, d;
        if (loss_type == 1) {
          const float diff = p - y;
          l = wt * diff * diff;
          d = 2.f * wt * diff;
        } else {
          l = wt * (std::max(p, 0.f) - p * y + std::log1p(std::exp(-std::fabs(p))));
          d = wt * (1.f / (1.f + std::exp(-p)) - y);
        }
        loss_sum += l;
        if (dpred) dpred[i] = d * grad_scale;
      }
    }
  }
  return FwdResult{loss_sum, regv_sum, regw_sum};
}

void explain(int B, const int* offsets, const int* rows, const float* vals, const void* v, long long v_stride,
             const float* w, long long w_stride, int Kp, int dtype, const float* bias, float* contrib, float* pred,
             int threads) {
  set_threads(threads);
#pragma omp parallel
  {
    std::vector<float> S(Kp), row(Kp);
#pragma omp for schedule(static)
    for (int i = 0; i < B; ++i) {
      std::fill(S.begin(), S.end(), 0.f);
      for (int j = offsets[i]; j < offsets[i + 1]; ++j) {
        const float x = vals ? vals[j] : 1.f;
        load_row(v, (long long)rows[j] * v_stride, Kp, dtype, row.data());
        for (int k = 0; k < Kp; ++k) S[k] += x * row[k];
      }
      float total = 0.f;
      for (int j = offsets[i]; j < offsets[i + 1]; ++j) {
        const long long r = rows[j];
        const float x = vals ? vals[j] : 1.f;
        load_row(v, r * v_stride, Kp, dtype, row.data());
        float d = 0.f;
        for (int k = 0; k < Kp; ++k) {
          const float xv = x * row[k];
          d += xv * (S[k] - xv);
        }
        const float c = x * w[r * w_stride] + 0.5f * d;
        contrib[j] = c;
        total += c;
      }
      pred[i] = total + (bias ? bias[0] : 0.f);
    }
  }
}

int dedup(int n, const uint32_t* keys, uint32_t* skeys, int* perm, uint32_t* uniq, int* seg_start, int* inv,
          const int* ex_of_occ, int* sorted_ex, const float* vals, float* sorted_x) {
  if (n <= 0) {
    seg_start[0] = 0;
    return 0;
  }
  std::vector<uint64_t> kv(n);
  for (int j = 0; j < n; ++j) kv[j] = (static_cast<uint64_t>(keys[j]) << 32) | static_cast<uint32_t>(j);
  std::sort(kv.begin(), kv.end());  // (key, index) order == stable sort by key
  int U = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t key = static_cast<uint32_t>(kv[j] >> 32);
    const int p = static_cast<int>(kv[j] & 0xffffffffu);
    skeys[j] = key;
    perm[j] = p;
    if (j == 0 || key != skeys[j - 1]) {
      uniq[U] = key;
      seg_start[U] = j;
      ++U;
    }
    if (inv) inv[p] = U - 1;
    if (sorted_ex) sorted_ex[j] = ex_of_occ[p];
    if (sorted_x) sorted_x[j] = vals[p];
  }
  seg_start[U] = n;
  return U;
}

void bwd(int mode, int U, const int* seg_start, const int* uniq, const int* sorted_ex, const float* sorted_x,
         const float* dpred, const float* r1, int Kp, void* v, long long v_stride, float* w, long long w_stride,
         float* s0v, float* s1v, long long s_stride, float* s0w, float* s1w, float reg_v, float reg_w,
         OptParams opt, float* grad_out, long long g_stride, int dtype, int threads) {
  set_threads(threads);
#pragma omp parallel
  {
    std::vector<float> A(Kp), vv(Kp), g(Kp), scratch(Kp);
#pragma omp for schedule(dynamic, 256)
    for (int u = 0; u < U; ++u) {
      std::fill(A.begin(), A.end(), 0.f);
      float Scx = 0.f, Sc = 0.f;
      const int sa = seg_start[u], sb = seg_start[u + 1];
      for (int j = sa; j < sb; ++j) {
        const int ex = sorted_ex[j];
        const float x = sorted_x ? sorted_x[j] : 1.f;
        const float c = dpred[ex] * x;
        const float* rr = r1 + (long long)ex * Kp;
        for (int k = 0; k < Kp; ++k) A[k] += c * rr[k];
        Scx += c * x;
        Sc += c;
      }
      const long long row = mode == 0 ? (long long)uniq[u] : (long long)u;
      load_row(v, row * v_stride, Kp, mode == 0 ? dtype : 0, vv.data());
      const float wv = w[row * w_stride];
      const float n_u = static_cast<float>(sb - sa);
      for (int k = 0; k < Kp; ++k) g[k] = A[k] - Scx * vv[k] + reg_v * n_u * vv[k];
      const float gw = Sc + reg_w * n_u * wv;
      if (mode == 1) {
        float* dst = grad_out + (long long)u * g_stride;
        std::memcpy(dst, g.data(), sizeof(float) * Kp);
        dst[Kp] = gw;
      } else {
        update_row(opt, row, g.data(), gw, Kp, v, v_stride, w, w_stride, s0v, s1v, s_stride, s0w, s1w, dtype,
                   scratch.data());
      }
    }
  }
}

void gather_rows(int R, const int* req, const void* v, long long v_stride, const float* w, long long w_stride,
                 int Kp, int dtype, float* out, long long o_stride, int threads) {
  set_threads(threads);
#pragma omp parallel for schedule(static)
  for (int p = 0; p < R; ++p) {
    const long long row = req[p];
    float* dst = out + (long long)p * o_stride;
    load_row(v, row * v_stride, Kp, dtype, dst);
    dst[Kp] = w[row * w_stride];
    for (long long k = Kp + 1; k < o_stride; ++k) dst[k] = 0.f;
  }
}

void apply_rows(int U, const int* seg_start, const int* uniq, const int* perm, const float* grad_in,
                long long g_stride, int Kp, void* v, long long v_stride, float* w, long long w_stride, float* s0v,
                float* s1v, long long s_stride, float* s0w, float* s1w, OptParams opt, int dtype, int threads) {
  set_threads(threads);
#pragma omp parallel
  {
    std::vector<float> g(Kp), scratch(Kp);
#pragma omp for schedule(dynamic, 256)
    for (int u = 0; u < U; ++u) {
      std::fill(g.begin(), g.end(), 0.f);
      float gw = 0.f;
      for (int j = seg_start[u]; j < seg_start[u + 1]; ++j) {
        const float* src = grad_in + (long long)perm[j] * g_stride;
        for (int k = 0; k < Kp; ++k) g[k] += src[k];
        gw += src[Kp];
      }
      update_row(opt, uniq[u], g.data(), gw, Kp, v, v_stride, w, w_stride, s0v, s1v, s_stride, s0w, s1w, dtype,
                 scratch.data());
    }
  }
}

void csr_rows(int B, const int* offsets, int* ex_of_occ) {
  for (int i = 0; i < B; ++i)
    for (int j = offsets[i]; j < offsets[i + 1]; ++j) ex_of_occ[j] = i;
}

namespace {
// (score key << 32) | example index of every score (score_key.h: bit patterns, no arithmetic on the score);
// nans += the NaN scores.
std::vector<uint64_t> keyed_scores(int n, const float* scores, uint64_t& nans) {
  std::vector<uint64_t> kv(n > 0 ? n : 0);
  for (int j = 0; j < n; ++j) {
    uint32_t b;
    std::memcpy(&b, scores + j, 4);
    nans += score_is_nan(b);
    kv[j] = (static_cast<uint64_t>(score_key(b)) << 32) | static_cast<uint32_t>(j);
  }
  return kv;
}

// One pass over the (key, index) order: a run of equal keys with positive weight rp and negative weight rn
// after negatives of weight nlt adds rp * (nlt + (nlt + rn)).
template <typename T>
void auc_pass(const std::vector<uint64_t>& kv, const float* labels, const float* weights, uint64_t nans, T* out) {
  const size_t n = kv.size();
  T u2 = 0, p = 0, nlt = 0;
  for (size_t j = 0; j < n;) {
    const uint32_t key = static_cast<uint32_t>(kv[j] >> 32);
    T rp = 0, rn = 0;
    for (; j < n && static_cast<uint32_t>(kv[j] >> 32) == key; ++j) {
      const uint32_t i = static_cast<uint32_t>(kv[j]);
      const T w = weights ? static_cast<T>(weights[i]) : static_cast<T>(1);
      if (labels[i] > 0.f) rp += w;
      else rn += w;
    }
    const T nle = nlt + rn;
    u2 += rp * (nlt + nle);
    p += rp;
    nlt = nle;
  }
  out[0] = u2;
  out[1] = p;
  out[2] = nlt;
  out[3] = static_cast<T>(nans);
  out[4] = 0;
}
}  // namespace

void auc(int n, const float* scores, const float* labels, const float* weights, void* out) {
  uint64_t nans = 0;
  std::vector<uint64_t> kv = keyed_scores(n, scores, nans);
  std::sort(kv.begin(), kv.end());
  if (weights) auc_pass<double>(kv, labels, weights, nans, static_cast<double*>(out));
  else auc_pass<uint64_t>(kv, labels, weights, nans, static_cast<uint64_t*>(out));
}

namespace {
// Placement of every example from one pass over the (key, index) order: in a run of equal keys with rp positives
// and rn negatives after nlt negatives and plt positives, a positive gets nlt + (nlt + rn) and a negative
// (P - plt - rp) + (P - plt).  Returns U2, the sum of the positives' placements.
uint64_t delong_place(const std::vector<uint64_t>& kv, const float* labels, uint64_t P, uint32_t* pl) {
  const size_t n = kv.size();
  uint64_t u2 = 0, nlt = 0, plt = 0;
  for (size_t j = 0; j < n;) {
    const uint32_t key = static_cast<uint32_t>(kv[j] >> 32);
    const size_t j0 = j;
    uint64_t rp = 0, rn = 0;
    for (; j < n && static_cast<uint32_t>(kv[j] >> 32) == key; ++j)
      (labels[static_cast<uint32_t>(kv[j])] > 0.f ? rp : rn) += 1;
    const uint64_t a = nlt + (nlt + rn), b = (P - plt - rp) + (P - plt);
    for (size_t i = j0; i < j; ++i) {
      const uint32_t e = static_cast<uint32_t>(kv[i]);
      pl[e] = static_cast<uint32_t>(labels[e] > 0.f ? a : b);
    }
    u2 += rp * a;
    nlt += rn;
    plt += rp;
  }
  return u2;
}
}  // namespace

void delong_moments(int n, const uint32_t* pl_a, const uint32_t* pl_b, const float* labels, uint64_t* out) {
  for (int w = 0; w < 12; ++w) out[w] = 0;
  const auto add = [&](int w, uint32_t x, uint32_t y) {
    const uint64_t t = static_cast<uint64_t>(x) * y;
    out[w] += t >> 32;
    out[w + 1] += t & 0xffffffffull;
  };
  for (int e = 0; e < n; ++e) {
    const int c = labels[e] > 0.f ? 0 : 2;
    add(c, pl_a[e], pl_a[e]);
    if (pl_b) {
      add(4 + c, pl_b[e], pl_b[e]);
      add(8 + c, pl_a[e], pl_b[e]);
    }
  }
}

void auc_delong(int n, const float* scores_a, const float* scores_b, const float* labels, uint64_t* out) {
  uint64_t P = 0;
  for (int e = 0; e < n; ++e) P += labels[e] > 0.f;
  std::vector<uint32_t> pl[2];
  uint64_t u2[2] = {0, 0}, nans[2] = {0, 0};
  for (int m = 0; m < (scores_b ? 2 : 1); ++m) {
    std::vector<uint64_t> kv = keyed_scores(n, m ? scores_b : scores_a, nans[m]);
    std::sort(kv.begin(), kv.end());
    pl[m].resize(kv.size());
    u2[m] = delong_place(kv, labels, P, pl[m].data());
  }
  out[0] = u2[0];
  out[1] = u2[1];
  out[2] = P;
  out[3] = static_cast<uint64_t>(n > 0 ? n : 0) - P;
  delong_moments(n, pl[0].data(), scores_b ? pl[1].data() : nullptr, labels, out + 4);
  out[16] = nans[0];
  out[17] = nans[1];
  out[18] = scores_b ? 1 : 0;
  out[19] = 0;
}

namespace {
// One pass over the (complemented key, index) order, from the highest score down: at the end of every run of
// equal keys the candidate (TP, FP, last position) is tried for every selection (threshold_rule.h), then the
// run's positives add their AP terms.  P and N are the sums of the same terms in the same order (a pass before).
template <typename T>
void threshold_pass(const std::vector<uint64_t>& kv, const float* labels, const float* weights, uint64_t nans,
                    const thr::Targets& tg, T* out) {
  const size_t n = kv.size();
  const auto weight = [&](size_t j) {
    return weights ? static_cast<T>(weights[static_cast<uint32_t>(kv[j])]) : static_cast<T>(1);
  };
  const auto positive = [&](size_t j) { return labels[static_cast<uint32_t>(kv[j])] > 0.f; };
  T P = 0, N = 0;
  for (size_t j = 0; j < n; ++j) (positive(j) ? P : N) += weight(j);
  const double dP = static_cast<double>(P);
  thr::Cand<T> sel[thr::kSel];
  for (auto& c : sel) c = thr::no_cand<T>();
  thr::Cand<T> rc[thr::kMaxTargets];  // the first candidate that passes each recall target
  for (auto& c : rc) c = thr::no_cand<T>();
  double ap = 0;
  T tp = 0, fp = 0;
  for (size_t j = 0; j < n;) {
    const uint32_t key = static_cast<uint32_t>(kv[j] >> 32);
    const size_t j0 = j;
    for (; j < n && static_cast<uint32_t>(kv[j] >> 32) == key; ++j) (positive(j) ? tp : fp) += weight(j);
    const T pp = tp + fp;
    if (pp > static_cast<T>(0)) {
      const thr::Cand<T> c{tp, fp, static_cast<int>(j - 1)};
      const double dtp = static_cast<double>(tp), dpp = static_cast<double>(pp);
      if (thr::ks_better(c, sel[0], P, N)) sel[0] = c;
      if (thr::f1_better(c, sel[1], P)) sel[1] = c;
      for (int i = 0; i < tg.np; ++i)
        if (thr::precision_ok(dtp, dpp, tg.pt[i]) && thr::tp_better(c, sel[2 + i])) sel[2 + i] = c;
      for (int i = 0; i < tg.nr; ++i)
        if (rc[i].pos == thr::kNoPos && thr::recall_ok(dtp, dP, tg.rt[i])) rc[i] = c;
    }
    for (size_t i = j0; i < j; ++i) {
      const T w = weight(i);
      if (positive(i) && w > static_cast<T>(0))
        ap = thr::ap_add(ap, static_cast<double>(w), static_cast<double>(tp), static_cast<double>(pp));
    }
  }
  if constexpr (std::is_same<T, double>::value) {
    out[0] = ap;
  } else {
    uint64_t bits;
    std::memcpy(&bits, &ap, 8);
    out[0] = bits;
  }
  out[1] = P;
  out[2] = N;
  thr::Cand<T> pts[thr::kPoints];
  for (int s = 0; s < thr::kSel; ++s) pts[s] = sel[s];
  for (int i = 0; i < thr::kMaxTargets; ++i) pts[thr::kSel + i] = rc[i];
  for (int s = 0; s < thr::kPoints; ++s) {
    const bool ok = pts[s].pos != thr::kNoPos;
    T* o = out + thr::kPoint0 + 3 * s;
    o[0] = ok ? pts[s].tp : static_cast<T>(0);
    o[1] = ok ? pts[s].fp : static_cast<T>(0);
    o[2] = ok ? static_cast<T>(score_key_bits(~static_cast<uint32_t>(kv[pts[s].pos] >> 32))) : static_cast<T>(0);
  }
  out[thr::kRecWords - 2] = static_cast<T>(nans);
  out[thr::kRecWords - 1] = 0;
}
}  // namespace

bool threshold_metrics(int n, const float* scores, const float* labels, const float* weights, const double* pt,
                       int np, const double* rt, int nr, void* out) {
  if (np < 0 || np > thr::kMaxTargets || nr < 0 || nr > thr::kMaxTargets) return false;
  thr::Targets tg{};
  tg.np = np;
  tg.nr = nr;
  for (int i = 0; i < np; ++i) {
    if (!(pt[i] > 0.0 && pt[i] <= 1.0)) return false;
    tg.pt[i] = pt[i];
  }
  for (int i = 0; i < nr; ++i) {
    if (!(rt[i] > 0.0 && rt[i] <= 1.0)) return false;
    tg.rt[i] = rt[i];
  }
  uint64_t nans = 0;
  std::vector<uint64_t> kv = keyed_scores(n, scores, nans);
  for (auto& x : kv) x ^= 0xffffffff00000000ull;  // the complemented key: from the highest score down
  std::sort(kv.begin(), kv.end());
  if (weights) threshold_pass<double>(kv, labels, weights, nans, tg, static_cast<double*>(out));
  else threshold_pass<uint64_t>(kv, labels, weights, nans, tg, static_cast<uint64_t*>(out));
  return true;
}

namespace {
// One pass per group over the (group, key, index) order; a group's runs of equal keys as in auc_pass.
template <typename T>
void gauc_pass(const std::vector<std::pair<uint64_t, uint32_t>>& kv, long long G, const float* labels,
               const float* weights, uint64_t nans, void* out, T* rec) {
  const size_t n = kv.size();
  std::fill(rec, rec + 3 * static_cast<size_t>(G), static_cast<T>(0));
  double wa = 0.0;
  T wsum = 0;
  uint64_t valid = 0, exs = 0;
  for (size_t j = 0; j < n;) {
    const uint32_t g = static_cast<uint32_t>(kv[j].first >> 32);
    const size_t first = j;
    T u2 = 0, p = 0, nlt = 0;
    while (j < n && static_cast<uint32_t>(kv[j].first >> 32) == g) {
      const uint64_t gk = kv[j].first;
      T rp = 0, rn = 0;
      for (; j < n && kv[j].first == gk; ++j) {
        const uint32_t i = kv[j].second;
        const T w = weights ? static_cast<T>(weights[i]) : static_cast<T>(1);
        if (labels[i] > 0.f) rp += w;
        else rn += w;
      }
      const T nle = nlt + rn;
      u2 += rp * (nlt + nle);
      p += rp;
      nlt = nle;
    }
    T* r = rec + 3 * static_cast<size_t>(g);
    r[0] = u2;
    r[1] = p;
    r[2] = nlt;
    if (p > 0 && nlt > 0) {
      const T w = p + nlt;
      wa += static_cast<double>(w) *
            (static_cast<double>(u2) / (2.0 * static_cast<double>(p) * static_cast<double>(nlt)));
      wsum += w;
      ++valid;
      exs += j - first;
    }
  }
  unsigned char* o = static_cast<unsigned char*>(out);
  const uint64_t zero = 0;
  std::memcpy(o, &wa, 8);
  std::memcpy(o + 8, &wsum, 8);
  std::memcpy(o + 16, &valid, 8);
  std::memcpy(o + 24, &exs, 8);
  std::memcpy(o + 32, &nans, 8);
  std::memcpy(o + 40, &zero, 8);
}
}  // namespace

void gauc(int n, long long G, const float* scores, const float* labels, const float* weights, const int* groups,
          void* out, void* rec) {
  uint64_t nans = 0;
  const std::vector<uint64_t> ks = keyed_scores(n, scores, nans);
  std::vector<std::pair<uint64_t, uint32_t>> kv(ks.size());
  for (int j = 0; j < n; ++j) {
    const uint32_t g = static_cast<uint32_t>(groups[j]) < static_cast<uint64_t>(G) ? static_cast<uint32_t>(groups[j])
                                                                                  : static_cast<uint32_t>(G - 1);
    kv[j] = {(static_cast<uint64_t>(g) << 32) | (ks[j] >> 32), static_cast<uint32_t>(j)};
  }
  std::sort(kv.begin(), kv.end());
  if (weights) gauc_pass<double>(kv, G, labels, weights, nans, out, static_cast<double*>(rec));
  else gauc_pass<uint64_t>(kv, G, labels, weights, nans, out, static_cast<uint64_t*>(rec));
}

namespace {
// The (group, key of vals, index) order of the examples; nans += the NaN values.
std::vector<std::pair<uint64_t, uint32_t>> grouped_order(int n, long long G, const float* vals, const int* groups,
                                                         uint64_t& nans) {
  const std::vector<uint64_t> ks = keyed_scores(n, vals, nans);
  std::vector<std::pair<uint64_t, uint32_t>> kv(ks.size());
  for (int j = 0; j < n; ++j) {
    const uint32_t g = static_cast<uint32_t>(groups[j]) < static_cast<uint64_t>(G) ? static_cast<uint32_t>(groups[j])
                                                                                  : static_cast<uint32_t>(G - 1);
    kv[j] = {(static_cast<uint64_t>(g) << 32) | (ks[j] >> 32), static_cast<uint32_t>(j)};
  }
  std::sort(kv.begin(), kv.end());
  return kv;
}

// One pass per group over that order: a run [lb, ub) of equal keys in the group [first, end) occupies the ranks
// a = end - ub + 1 .. b = end - lb, and every member with a positive gain adds gain (D[min(b, k)] - D[min(a - 1,
// k)]) / (b - a + 1) to the cutoff's DCG -- into column dcg_col + 3 i of the group's record -- and, with hits,
// (min(b, k) - min(a - 1, k)) / (b - a + 1) to its hits and 1 to P_g.
void rank_pass(const std::vector<std::pair<uint64_t, uint32_t>>& kv, const std::vector<float>& gains, const double* D,
               const int* k, int nk, int dcg_col, bool hits, double* per) {
  const size_t n = kv.size(), ncol = 2 + 3 * static_cast<size_t>(nk);
  for (size_t j = 0; j < n;) {
    const uint32_t g = static_cast<uint32_t>(kv[j].first >> 32);
    size_t end = j;
    while (end < n && static_cast<uint32_t>(kv[end].first >> 32) == g) ++end;
    double* r = per + ncol * g;
    if (hits) r[0] = static_cast<double>(end - j);
    while (j < end) {
      size_t ub = j;
      while (ub < end && kv[ub].first == kv[j].first) ++ub;
      const long long a = static_cast<long long>(end - ub) + 1, b = static_cast<long long>(end - j);
      const double len = static_cast<double>(b - a + 1);
      for (; j < ub; ++j) {
        const float gain = gains[kv[j].second];
        if (!(gain > 0.f)) continue;
        if (hits) r[1] += 1.0;
        for (int i = 0; i < nk; ++i) {
          if (a > k[i]) continue;
          const long long lo = std::min<long long>(a - 1, k[i]), hi = std::min<long long>(b, k[i]);
          r[dcg_col + 3 * i] += static_cast<double>(gain) * ((D[hi] - D[lo]) / len);
          if (hits) r[4 + 3 * i] += static_cast<double>(hi - lo) / len;
        }
      }
    }
  }
}
}  // namespace

bool rank_metrics(int n, long long G, const float* scores, const float* labels, const int* groups, const int* k,
                  int nk, void* out, double* per) {
  if (!rank_cutoffs_ok(k, nk)) return false;
  static const std::vector<double> D = [] {
    std::vector<double> d(kRankMaxCutoff + 1);
    rank_dcg_table(d.data());
    return d;
  }();
  const size_t ncol = 2 + 3 * static_cast<size_t>(nk);
  std::fill(per, per + ncol * static_cast<size_t>(G), 0.0);
  std::vector<float> gains(n > 0 ? n : 0);
  for (int j = 0; j < n; ++j) gains[j] = labels[j] > 0.f ? labels[j] : 0.f;
  uint64_t nans = 0, ideal_nans = 0;
  rank_pass(grouped_order(n, G, scores, groups, nans), gains, D.data(), k, nk, 2, true, per);
  rank_pass(grouped_order(n, G, gains.data(), groups, ideal_nans), gains, D.data(), k, nk, 3, false, per);
  std::vector<double> sums(3 * static_cast<size_t>(nk), 0.0);
  uint64_t ranked = 0, exs = 0;
  for (long long g = 0; g < G; ++g) {
    const double* r = per + ncol * static_cast<size_t>(g);
    if (!(r[1] > 0)) continue;
    ++ranked;
    exs += static_cast<uint64_t>(r[0]);
    for (int i = 0; i < nk; ++i) {
      sums[3 * i] += r[2 + 3 * i] / r[3 + 3 * i];
      sums[3 * i + 1] += r[4 + 3 * i] / r[1];
      sums[3 * i + 2] += r[4 + 3 * i] / static_cast<double>(k[i]);
    }
  }
  unsigned char* o = static_cast<unsigned char*>(out);
  const uint64_t zero = 0;
  std::memcpy(o, sums.data(), 8 * sums.size());
  o += 8 * sums.size();
  std::memcpy(o, &ranked, 8);
  std::memcpy(o + 8, &exs, 8);
  std::memcpy(o + 16, &nans, 8);
  std::memcpy(o + 24, &zero, 8);
  return true;
}

void group_keys(int B, const int* offsets, const int* rows, int pos, int num_rows, int* keys) {
  for (int i = 0; i < B; ++i) {
    int k = -1;
    if (offsets[i] >= 0 && offsets[i + 1] - offsets[i] > pos) {
      const int r = rows[offsets[i] + pos];
      if (static_cast<unsigned>(r) < static_cast<unsigned>(num_rows)) k = r;
    }
    keys[i] = k;
  }
}

void group_plan(int n, const int* ids, int key_bits, int* sidx, int* first, int* end) {
  const uint32_t excl = (1u << key_bits) - 1u;
  std::vector<uint32_t> key(n > 0 ? n : 0);
  for (int e = 0; e < n; ++e)
    key[e] = (ids[e] < 0 || static_cast<uint32_t>(ids[e]) >= excl) ? excl : static_cast<uint32_t>(ids[e]);
  std::iota(sidx, sidx + n, 0);
  std::stable_sort(sidx, sidx + n, [&key](int a, int b) { return key[a] < key[b]; });
  for (int j = 0; j < n;) {
    const uint32_t k = key[sidx[j]];
    int e = j + 1;
    while (e < n && key[sidx[e]] == k) ++e;
    for (int q = j; q < e; ++q) {
      first[q] = k == excl ? q : j;
      end[q] = k == excl ? 0 : e;
    }
    j = e;
  }
}

double group_softmax(int n, const int* sidx, const int* first, const int* end, const float* scores,
                     const float* labels, const float* weights, double grad_scale, float* dpred) {
  double loss = 0.0;
  auto gain = [labels, weights](int ex) {
    return (weights ? static_cast<double>(weights[ex]) : 1.0) * (labels[ex] > 0.f ? static_cast<double>(labels[ex]) : 0.0);
  };
  for (int j = 0; j < n;) {
    if (end[j] == 0) {
      dpred[sidx[j]] = 0.f;
      ++j;
      continue;
    }
    const int e = end[j];
    double m = -std::numeric_limits<double>::infinity(), Z = 0.0, A = 0.0, T = 0.0;
    for (int q = j; q < e; ++q) m = std::fmax(m, static_cast<double>(scores[sidx[q]]));
    for (int q = j; q < e; ++q) {
      const double s = scores[sidx[q]], a = gain(sidx[q]);
      Z += std::exp(s - m);
      A += a;
      T += a * s;
    }
    for (int q = j; q < e; ++q) {
      const double s = scores[sidx[q]];
      const double d = A != 0.0 ? A * (std::exp(s - m) / Z) - gain(sidx[q]) : 0.0;
      dpred[sidx[q]] = static_cast<float>(grad_scale * d);
    }
    if (A != 0.0) loss += A * (m + std::log(Z)) - T;
    j = e;
  }
  return loss;
}

double group_pairwise(int n, const int* sidx, const int* first, const int* end, const float* scores,
                      const float* labels, const float* weights, double grad_scale, float* dpred) {
  double loss = 0.0;
  std::vector<double> cw;  // the group's signed class weights: +p, -q, 0
  for (int j = 0; j < n;) {
    if (end[j] == 0) {
      dpred[sidx[j]] = 0.f;
      ++j;
      continue;
    }
    const int e = end[j], m = e - j;
    cw.assign(m, 0.0);
    double P = 0.0, N = 0.0;
    for (int q = 0; q < m; ++q) {
      const int ex = sidx[j + q];
      const double w = weights ? static_cast<double>(weights[ex]) : 1.0;
      if (!(w > 0.0)) continue;
      if (labels[ex] > 0.f) {
        P += w;
        cw[q] = w;
      } else {
        N += w;
        cw[q] = -w;
      }
    }
    const bool valid = P > 0.0 && N > 0.0;
    const double c = valid ? (P + N) / (P * N) : 0.0;
    for (int q = 0; q < m; ++q) {
      const int ex = sidx[j + q];
      double d = 0.0;
      if (valid && cw[q] != 0.0) {
        const bool pos = cw[q] > 0.0;
        const double s = scores[ex];
        double sig = 0.0, sp = 0.0;
        for (int k = 0; k < m; ++k) {
          if (pos ? !(cw[k] < 0.0) : !(cw[k] > 0.0)) continue;
          const double sk = scores[sidx[j + k]];
          const double df = pos ? sk - s : s - sk;  // s_neg - s_pos
          const double t = std::exp(-std::fabs(df));
          const double aw = std::fabs(cw[k]);
          sig += aw * ((df >= 0.0 ? 1.0 : t) / (1.0 + t));
          if (pos) sp += aw * (std::fmax(df, 0.0) + std::log1p(t));
        }
        d = -(c * cw[q]) * sig;
        if (pos) loss += (c * cw[q]) * sp;
      }
      dpred[ex] = static_cast<float>(grad_scale * d);
    }
    j = e;
  }
  return loss;
}

namespace {
template <typename T>
void isotonic_pass(const std::vector<uint64_t>& kv, const float* labels, const float* weights, uint64_t nans,
                   float* lo, float* hi, T* W, T* Y, double* v, double* fitted, T* out, int tile) {
  const int n = static_cast<int>(kv.size());
  std::vector<T> cW(n + 1), cY(n + 1);
  std::vector<uint8_t> cand(n + 1);
  T w = 0, y = 0;
  for (int j = 0; j < n; ++j) {
    const uint32_t i = static_cast<uint32_t>(kv[j]);
    const T wi = weights ? static_cast<T>(weights[i]) : static_cast<T>(1);
    cW[j] = w;
    cY[j] = y;
    cand[j] = j == 0 || (kv[j - 1] >> 32) != (kv[j] >> 32);
    w += wi;
    if (labels[i] > 0.f) y += wi;
  }
  cW[n] = w;
  cY[n] = y;
  cand[n] = 1;
  std::vector<int> H(n + 1);
  int c = 0;
  if (tile < 2) {
    c = iso::leaf_hull<T>(cW.data(), cY.data(), cand.data(), n + 1, H.data());
  } else {
    const iso::Diagram<T> d{cW.data(), cY.data(), n};
    const int ntl = n / tile + 1;
    std::vector<int> A(static_cast<size_t>(ntl) * tile), B(A.size()), ca(ntl), cb(ntl);
    for (int t = 0; t < ntl; ++t) {
      const int base = t * tile, cnt = std::min(tile, n + 1 - base);
      ca[t] = iso::leaf_hull<T>(cW.data() + base, cY.data() + base, cand.data() + base, cnt, A.data() + base);
      for (int k = 0; k < ca[t]; ++k) A[base + k] += base;
    }
    int *src = A.data(), *dst = B.data(), *sc = ca.data(), *dc = cb.data();
    for (int level = 0; (1ll << level) < ntl; ++level) {
      for (long long k = 0; ((2 * k) << level) < ntl; ++k) {
        const long long tl = (2 * k) << level, tr = (2 * k + 1) << level;
        const int* L = src + tl * tile;
        const int nL = sc[tl];
        int nR = 0, a = nL - 1, b = 0;
        const int* R = L;
        if (tr < ntl) {
          R = src + tr * tile;
          nR = sc[tr];
          if (nL > 0 && nR > 0) iso::bridge<T>(d, L, nL, R, nR, a, b);
        }
        int* D = dst + tl * tile;
        std::copy(L, L + a + 1, D);
        std::copy(R + b, R + nR, D + a + 1);
        dc[tl] = a + 1 + nR - b;
      }
      std::swap(src, dst);
      std::swap(sc, dc);
    }
    c = sc[0];
    std::copy(src, src + c, H.begin());
  }
  const int m = c - 1;  // (H[0] = 0, H[m] = n)
  for (int b = 0; b < m; ++b) {
    const int p = H[b], q = H[b + 1];
    const uint32_t bl = score_key_bits(static_cast<uint32_t>(kv[p] >> 32));
    const uint32_t bh = score_key_bits(static_cast<uint32_t>(kv[q - 1] >> 32));
    std::memcpy(lo + b, &bl, 4);
    std::memcpy(hi + b, &bh, 4);
    W[b] = cW[q] - cW[p];
    Y[b] = cY[q] - cY[p];
    v[b] = static_cast<double>(Y[b]) / static_cast<double>(W[b]);
    if (fitted)
      for (int j = p; j < q; ++j) fitted[static_cast<uint32_t>(kv[j])] = v[b];
  }
  out[0] = static_cast<T>(m);
  out[1] = w;
  out[2] = y;
  out[3] = static_cast<T>(nans);
  out[4] = 0;
}
}  // namespace

void isotonic(int n, const float* scores, const float* labels, const float* weights, float* lo, float* hi, void* W,
              void* Y, double* v, double* fitted, void* out, int tile) {
  uint64_t nans = 0;
  std::vector<uint64_t> kv = keyed_scores(n, scores, nans);
  std::sort(kv.begin(), kv.end());
  if (weights)
    isotonic_pass<double>(kv, labels, weights, nans, lo, hi, static_cast<double*>(W), static_cast<double*>(Y), v,
                          fitted, static_cast<double*>(out), tile);
  else
    isotonic_pass<uint64_t>(kv, labels, weights, nans, lo, hi, static_cast<uint64_t*>(W), static_cast<uint64_t*>(Y),
                            v, fitted, static_cast<uint64_t*>(out), tile);
}

void calib_apply(long long n, const float* scores, const float* x, const float* y, int m2, float* out) {
  for (long long i = 0; i < n; ++i)
    out[i] = iso::calib_value(scores[i], x, y, m2, [](float t, float d, float v) { return std::fmaf(t, d, v); });
}

void topk(long long nq, long long nc, int Kp, int k, const float* Q, long long q_stride, const float* C,
          long long c_stride, const float* qb, const float* cb, int* idx, float* score, int threads) {
  set_threads(threads);
  std::vector<int> cols;  // pi(Kp)
  topk::for_each_col(Kp, [&](int c) { cols.push_back(c); });
#pragma omp parallel
  {
    std::vector<uint64_t> heap;  // min-heap of the best k keys so far
    std::vector<float> qv(cols.size());
    heap.reserve(k + 1);
    const auto gt = [](uint64_t a, uint64_t b) { return a > b; };
#pragma omp for schedule(dynamic, 1)
    for (long long q = 0; q < nq; ++q) {
      const float* qr = Q + q * q_stride;
      for (size_t i = 0; i < cols.size(); ++i) qv[i] = qr[cols[i]];
      heap.clear();
      for (long long c = 0; c < nc; ++c) {
        const float* cr = C + c * c_stride;
        float dot = 0.f;
        for (size_t i = 0; i < cols.size(); ++i) dot = std::fmaf(qv[i], cr[cols[i]], dot);
        // (two additions as written, then + 0.f: -0 becomes +0)
        volatile float base = qb[q] + cb[c];
        volatile float sum = base + dot;
        const float s = sum + 0.f;
        uint32_t bits;
        std::memcpy(&bits, &s, 4);
        const uint64_t key = topk::make_key(bits, (uint32_t)c);
        if ((int)heap.size() < k) {
          heap.push_back(key);
          std::push_heap(heap.begin(), heap.end(), gt);
        } else if (key > heap.front()) {
          std::pop_heap(heap.begin(), heap.end(), gt);
          heap.back() = key;
          std::push_heap(heap.begin(), heap.end(), gt);
        }
      }
      std::sort(heap.begin(), heap.end(), gt);
      for (int t = 0; t < k; ++t) {
        const uint64_t key = t < (int)heap.size() ? heap[t] : 0ull;
        const uint32_t sb = topk::key_score_bits(key);
        idx[q * k + t] = topk::key_index(key);
        std::memcpy(&score[q * k + t], &sb, 4);
      }
    }
  }
}

namespace {
inline float init_uniform(unsigned long long seed, long long gid, int col, float range) {
  const unsigned long long h =
      mix64(seed ^ mix64(static_cast<unsigned long long>(gid) * 0x100000001b3ull + static_cast<unsigned long long>(col)));
  const float u = static_cast<float>(h >> 40) * (1.0f / 16777216.0f);
  return range * (2.f * u - 1.f);
}
}  // namespace

void init_rows(void* v, long long v_stride, float* w, long long w_stride, long long rows, int K, int Kp, int dtype,
               long long gid_mul, long long gid_add, unsigned long long seed, float range, int threads) {
  set_threads(threads);
#pragma omp parallel for schedule(static)
  for (long long r = 0; r < rows; ++r) {
    const long long gid = r * gid_mul + gid_add;
    for (int c = 0; c < Kp; ++c) {
      const float val = c < K ? init_uniform(seed, gid, c + 1, range) : 0.f;
      if (dtype == 1)
        static_cast<uint16_t*>(v)[r * v_stride + c] = f32_to_bf16(val);
      else
        static_cast<float*>(v)[r * v_stride + c] = val;
    }
    w[r * w_stride] = init_uniform(seed, gid, 0, range);
  }
}

long long changed_rows(const void* v, long long v_stride, const float* w, long long w_stride, const float* s0v,
                        const float* s1v, long long s_stride, const float* s0w, const float* s1w, long long rows,
                        int K, int dtype, long long gid_mul, long long gid_add, unsigned long long seed, float range,
                        const uint32_t* sv_bits, const uint32_t* sw_bits, uint8_t* flags, int threads) {
  set_threads(threads);
  const auto bits = [](const float* p) {
    uint32_t b;
    std::memcpy(&b, p, 4);
    return b;
  };
  long long count = 0;
#pragma omp parallel for schedule(static) reduction(+ : count)
  for (long long r = 0; r < rows; ++r) {
    const long long gid = r * gid_mul + gid_add;
    const float w0 = init_uniform(seed, gid, 0, range);
    bool d = bits(w + r * w_stride) != bits(&w0);
    d = d || (s0w && bits(s0w + r) != sw_bits[0]) || (s1w && bits(s1w + r) != sw_bits[1]);
    for (int c = 0; c < K && !d; ++c) {
      const float val = init_uniform(seed, gid, c + 1, range);
      if (dtype == 1)
        d = static_cast<const uint16_t*>(v)[r * v_stride + c] != f32_to_bf16(val);
      else
        d = bits(static_cast<const float*>(v) + r * v_stride + c) != bits(&val);
      d = d || (s0v && bits(s0v + r * s_stride + c) != sv_bits[0]) ||
          (s1v && bits(s1v + r * s_stride + c) != sv_bits[1]);
    }
    flags[r] = d;
    count += d;
  }
  return count;
}

void changed_rows_emit(const uint8_t* flags, long long rows, long long* out) {
  long long n = 0;
  for (long long r = 0; r < rows; ++r)
    if (flags[r]) out[n++] = r;
}

}  // namespace cpu
}  // namespace fm
