// Host (CPU) implementations of the FM step kernels. They follow the same
// contracts as the gfx950 kernels in csrc/hip/ (same argument meaning, same
// row layouts) and back the world_size=1 CPU configuration and the gloo
// multi-process tests. They mirror the reference's CPU Eigen path
// (cc/fm_scorer_op.cc:79, cc/fm_grad_op.cc:88), but group occurrences per
// row instead of the CAS-loop float atomics of cc/fm_grad_op.h:4-15.
#pragma once
#include <cstdint>

namespace fm {
namespace cpu {

struct OptParams {
  int type;  // 0 adagrad, 1 ftrl, 2 sgd
  float lr, l1, l2, beta;
};

struct FwdResult {
  double loss_sum, regv_sum, regw_sum;
};

FwdResult fwd(int B, const int* offsets, const int* rows, const float* vals, const void* v, long long v_stride,
              const float* w, long long w_stride, int Kp, int dtype, const float* labels, const float* weights,
              int loss_type, float grad_scale, float* pred, float* r1, float* dpred, int threads,
              const float* bias = nullptr);

// Exact per-occurrence attributions of the score (hip/fm_explain.hip: same definition):
// contrib[j] = x_j w_j + 1/2 sum_f x_j v_jf (S_f - x_j v_jf); pred[i] = sum of example i's contributions + bias.
void explain(int B, const int* offsets, const int* rows, const float* vals, const void* v, long long v_stride,
             const float* w, long long w_stride, int Kp, int dtype, const float* bias, float* contrib, float* pred,
             int threads);

// The k best candidates of every query from FM profiles (hip/fm_topk.hip: same definition, bit for bit):
// s = ((qb[q] + cb[c]) + fmaf chain over pi(Kp)) + 0.f, greater s first, equal s by ascending candidate;
// idx = -1 / score = -inf where nc < k (../topk_order.h).
void topk(long long nq, long long nc, int Kp, int k, const float* Q, long long q_stride, const float* C,
          long long c_stride, const float* qb, const float* cb, int* idx, float* score, int threads);

// Stable sort of (key, occurrence) + run-length encoding. Returns U.
int dedup(int n, const uint32_t* keys, uint32_t* skeys, int* perm, uint32_t* uniq, int* seg_start, int* inv,
          const int* ex_of_occ, int* sorted_ex, const float* vals, float* sorted_x);

void bwd(int mode, int U, const int* seg_start, const int* uniq, const int* sorted_ex, const float* sorted_x,
         const float* dpred, const float* r1, int Kp, void* v, long long v_stride, float* w, long long w_stride,
         float* s0v, float* s1v, long long s_stride, float* s0w, float* s1w, float reg_v, float reg_w,
         OptParams opt, float* grad_out, long long g_stride, int dtype, int threads);

void gather_rows(int R, const int* req, const void* v, long long v_stride, const float* w, long long w_stride,
                 int Kp, int dtype, float* out, long long o_stride, int threads);

void apply_rows(int U, const int* seg_start, const int* uniq, const int* perm, const float* grad_in,
                long long g_stride, int Kp, void* v, long long v_stride, float* w, long long w_stride, float* s0v,
                float* s1v, long long s_stride, float* s0w, float* s1w, OptParams opt, int dtype, int threads);

void csr_rows(int B, const int* offsets, int* ex_of_occ);

// Exact weighted ROC AUC statistics (hip/auc.hip: same definition, same two modes): out[5] = U2, P, N, NaN
// scores, 0 -- uint64 when weights is null (exact), else fp64 summed in sorted order.
void auc(int n, const float* scores, const float* labels, const float* weights, void* out);

// DeLong statistics (hip/auc_delong.hip: same definitions, same record) of one model (scores_b null) or two on the
// same examples, unweighted: out[20] (uint64) = U2_a, U2_b, P, N, (hi, lo) of M_pos / M_neg of (a, a), (b, b),
// (a, b), NaN scores of a, of b, has_b, 0.
void auc_delong(int n, const float* scores_a, const float* scores_b, const float* labels, uint64_t* out);

// The 12 moment words of n placements (pl_b null: (a, a) only, the rest 0): every product t adds t >> 32 to its
// hi word and t & 0xffffffff to its lo word.
void delong_moments(int n, const uint32_t* pl_a, const uint32_t* pl_b, const float* labels, uint64_t* out);

// Threshold metrics (hip/threshold_metrics.hip: same definitions, same two modes, the rules of
// ../threshold_rule.h): out[thr::kRecWords], the record described there -- uint64 when weights is null (exact),
// else fp64 summed from the highest score down; word 0 holds fp64 bits in both.  pt[np] / rt[nr]: the precision /
// recall targets.  false: more than 4 targets of a kind or one outside (0, 1] (nothing is written).
bool threshold_metrics(int n, const float* scores, const float* labels, const float* weights, const double* pt,
                       int np, const double* rt, int nr, void* out);

// Grouped AUC statistics (hip/gauc.hip: same definition, same two modes) of n scores with group ids in [0, G)
// (ids outside it count as G - 1): rec[G, 3] = U2_g, P_g, N_g of every group (uint64 when weights is null, else
// fp64 summed in (group, score) order) and out[6], 64-bit words = sum over the valid groups of W_g AUC_g (fp64),
// their sum of W_g (uint64 / fp64), their number, their examples, the NaN scores, 0.
void gauc(int n, long long G, const float* scores, const float* labels, const float* weights, const int* groups,
          void* out, void* rec);

// Ranking statistics (hip/rank_metrics.hip: same definitions, the same discount table ../rank_table.h) of n scores
// with group ids in [0, G) (ids outside it count as G - 1) at nk cutoffs k (rank_cutoffs_ok): per[G, 2 + 3 nk]
// (fp64) = n_g, P_g, then DCG, IDCG, hits per cutoff, and out[3 nk + 4], 64-bit words = per cutoff the sums over
// the ranked groups of NDCG_g, recall_g, precision_g (fp64), then the ranked groups, their examples, the NaN
// scores, 0.  false: bad cutoffs (nothing is written).
bool rank_metrics(int n, long long G, const float* scores, const float* labels, const int* groups, const int* k,
                  int nk, void* out, double* per);

// Listwise ranking loss (hip/group_loss.hip: same definition, fp64, a plain sort and loop).
// group_keys: keys[i] = rows[offsets[i] + pos], -1 (excluded) for an example with fewer features or a row outside
// [0, num_rows).  group_plan: sidx[n] = the examples in (group, batch) order (ids < 0 or >= 2^key_bits - 1 are
// excluded and come last), first[n] / end[n] = every sorted position's group range (end == 0: excluded).
// group_softmax: dpred[n] (example order) = fp32(grad_scale (A_g softmax_g(s)_i - a_i)) with a_i = w_i max(y_i, 0);
// returns sum_g A_g (m_g + log Z_g) - T_g; a group with A_g == 0 and an excluded example add exactly 0.
void group_keys(int B, const int* offsets, const int* rows, int pos, int num_rows, int* keys);
void group_plan(int n, const int* ids, int key_bits, int* sidx, int* first, int* end);
double group_softmax(int n, const int* sidx, const int* first, const int* end, const float* scores,
                     const float* labels, const float* weights, double grad_scale, float* dpred);

// Pairwise ranking loss (hip/group_pair.hip: same definition, fp64, a loop over the plan's groups): positive iff
// y > 0, p = w of a positive, q = w of a non-positive, c = (P + N) / (P N); dpred[n] (example order) =
// fp32(grad_scale (-+) c w sum of the opposite class's weights times sigma(s_neg - s_pos)); returns sum_g c sum
// p_i q_j softplus(s_j - s_i).  A group without a positive or without a negative, an excluded example and an
// example of weight 0 add exactly 0 and get exactly 0, whatever their scores hold.
double group_pairwise(int n, const int* sidx, const int* first, const int* end, const float* scores,
                      const float* labels, const float* weights, double grad_scale, float* dpred);

// Exact isotonic regression (hip/isotonic.hip: same definition, same two modes) of n >= 1 scores, weights null
// or all > 0: the blocks' first / last score lo, hi, weight W, positive weight Y (uint64 when weights is null,
// else fp64 summed in sorted order) and value v = Y / W (fp64), [n] each; out[5] = blocks, total weight, positive
// weight, NaN scores, 0; fitted[n] (fp64, input order) unless null.  tile == 0: the serial stack; tile >= 2: the
// GPU's formulation, hulls of tiles of that many points merged pairwise by their bridges (the same vertex list).
void isotonic(int n, const float* scores, const float* labels, const float* weights, float* lo, float* hi, void* W,
              void* Y, double* v, double* fitted, void* out, int tile);

// out[i] = the calibrated probability of scores[i] from the thresholds x[m2] = lo_0, hi_0, lo_1, hi_1, ... and
// the values y[m2] = v_0, v_0, v_1, v_1, ... (hip/isotonic.hip calib_apply_kernel: the same formula).
void calib_apply(long long n, const float* scores, const float* x, const float* y, int m2, float* out);

// Counter-based U(-range, range) init, identical to the gfx950 init_rows kernel.
void init_rows(void* v, long long v_stride, float* w, long long w_stride, long long rows, int K, int Kp, int dtype,
               long long gid_mul, long long gid_add, unsigned long long seed, float range, int threads);

// Sparse checkpoints (hip/ckpt.hip: same definition): flags[r] = 1 when row r < rows differs, bitwise over
// columns 0 .. K-1, from what init_rows wrote (v, w) or from a slot's initial bit pattern (sv_bits / sw_bits:
// slot 0, slot 1; null slots are skipped).  fp32 and bf16 tables.  Returns the number of flagged rows;
// changed_rows_emit then lists them in ascending order.
long long changed_rows(const void* v, long long v_stride, const float* w, long long w_stride, const float* s0v,
                       const float* s1v, long long s_stride, const float* s0w, const float* s1w, long long rows,
                       int K, int dtype, long long gid_mul, long long gid_add, unsigned long long seed, float range,
                       const uint32_t* sv_bits, const uint32_t* sw_bits, uint8_t* flags, int threads);
void changed_rows_emit(const uint8_t* flags, long long rows, long long* out);

}  // namespace cpu
}  // namespace fm
