"""fp64 oracle of the LambdaRank loss (``ops.kernels.group_lambda_loss``), a plain numpy loop over the groups, and the
cases its CPU and GPU tests share.  ``G = max(y, 0)``; per group over its examples (id >= 0) the place ``r`` by
``lexsort`` on (example index, -score) with -0.0 normalised; ``c(r) = 1 / log2(r + 1)`` for ``r <= K`` (every r when
K = 0) else 0; ``IDCG`` over the gains descending; for ``G_i > G_j``: ``delta = (G_i - G_j) |c_i - c_j| / IDCG``,
``L += delta softplus(s_j - s_i)``, ``dL/ds_i -= delta sigma(s_j - s_i)``, ``dL/ds_j +=`` the same.  A group of one or
with ``IDCG == 0`` is skipped before its scores are read.

The bound of ``check`` is derived, not tuned.  A gradient is a difference of two sums of non-negative terms, so its
error is relative to the sum A of the absolute terms:  |got - ref| <= 2^-23 |ref| + 2^-52 ((n_g + 256) A + 2 C) + 2^-149
  * 2^-23: the one rounding to fp32; 2^-149: fp32's underflow step;
  * n_g 2^-52 A: a sum over at most n_g columns, and IDCG, a sum of at most n_g non-negative terms;
  * 256 (x 2^-52 A): the few ulp of exp / log1p / the divisions in either implementation and the inexact fp64
    ``s_j - s_i`` at the case list's score spread of 160 (tests/group_pair_oracle.py has the argument);
  * 2 x 2^-52 C, C the same sum with ``c_i + c_j`` in place of ``|c_i - c_j|``: each discount is a log2 (<= 1 ulp)
    and a division (1/2 ulp) in each of two implementations, 3 x 2^-53 <= 2 x 2^-52 relative to c, and that absolute
    error stays when two nearby discounts are subtracted (places 3000 and 3001 differ by 4e-6 of their value).
The loss has no cancellation: the same with A = the loss and ``n`` in place of ``n_g``."""

import functools
import zlib

import numpy as np

import group_loss_cases as cases

EPS32, EPS64, TINY32, LD = 2.0 ** -23, 2.0 ** -52, 2.0 ** -149, np.longdouble


def discount(place, K):
    c = 1.0 / np.log2(np.asarray(place, dtype=np.float64) + 1.0)
    return c if K == 0 else np.where(np.asarray(place) <= K, c, 0.0)


def group_lambda(groups, scores, labels, K, grad_scale=1.0):
    """(dpred [n], loss, gsize [n] (0: excluded), A [n], C [n], the loss's C) in fp64; A and C as above."""
    groups = np.asarray(groups)
    gain = np.maximum(np.asarray(labels, dtype=np.float64), 0.0)
    n = groups.shape[0]
    dpred, gsize, A, C = np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(n), np.zeros(n)
    loss, loss_c = LD(0), LD(0)
    for k in np.unique(groups[groups >= 0]):
        idx = np.nonzero(groups == k)[0]
        m = gsize[idx] = idx.size
        g = gain[idx]
        idcg = float(np.sum(np.sort(g)[::-1] * discount(np.arange(1, m + 1), K), dtype=LD))
        if m < 2 or not idcg > 0:
            continue
        s = np.asarray(scores, dtype=np.float64)[idx] + 0.0   # (-0.0 + 0.0 = +0.0)
        place = np.empty(m, dtype=np.int64)
        place[np.lexsort((idx, -s))] = np.arange(1, m + 1)
        c = discount(place, K)
        dg = g[:, None] - g[None, :]                # [i, j]; the pairs are those with dg > 0
        d = s[None, :] - s[:, None]                 # s_j - s_i
        t = np.exp(-np.abs(d))
        sig = np.where(d >= 0, 1.0, t) / (1.0 + t)
        w = np.where(dg > 0, dg, 0.0) / idcg
        lam, lam_c = w * np.abs(c[:, None] - c[None, :]), w * (c[:, None] + c[None, :])
        up, dn = np.sum(lam * sig, axis=1, dtype=LD), np.sum(lam * sig, axis=0, dtype=LD)
        dpred[idx] = grad_scale * (dn - up).astype(np.float64)
        A[idx] = abs(grad_scale) * (dn + up).astype(np.float64)
        C[idx] = abs(grad_scale) * (np.sum(lam_c * sig, axis=1, dtype=LD) + np.sum(lam_c * sig, axis=0, dtype=LD))
        sp = np.maximum(d, 0.0) + np.log1p(t)
        loss += np.sum(lam * sp, dtype=LD)
        loss_c += np.sum(lam_c * sp, dtype=LD)
    return dpred, float(loss), gsize, A, C, float(loss_c)


def check(dpred, loss, groups, scores, labels, K, grad_scale=1.0, what="", ref=None):
    """Assert the op's fp32 ``dpred`` / ``loss`` against the oracle (``ref``: its result, when the caller has it)."""
    ref_d, ref_l, gsize, A, C, loss_c = ref or group_lambda(groups, scores, labels, K, grad_scale)
    got = np.asarray(dpred, dtype=np.float64)
    assert got.shape == ref_d.shape, (what, got.shape, ref_d.shape)
    bound = EPS32 * np.abs(ref_d) + EPS64 * ((gsize + 256) * A + 2 * C) + TINY32
    bad = np.nonzero(~(np.abs(got - ref_d) <= bound))[0]
    assert bad.size == 0, (what, "dpred", int(bad[0]), float(got[bad[0]]), float(ref_d[bad[0]]), float(bound[bad[0]]))
    lbound = EPS32 * abs(ref_l) + EPS64 * ((got.shape[0] + 256) * abs(ref_l) + 2 * loss_c) + TINY32
    assert abs(float(loss) - ref_l) <= lbound, (what, "loss", float(loss), ref_l, lbound)


@functools.lru_cache(maxsize=None)
def case_ref(n, grouping, values, K):
    """The inputs of ``group_loss_cases.case`` (weights dropped) and the oracle's result, computed once a session."""
    g, s, y, _, gs = cases.case(n, grouping, values)
    return (g, s, y, gs), group_lambda(g, s, y, K, gs)


# Cases placed by the GPU op's geometry (hip/group_lambda.hip): name -> (group sizes in sorted order, pairs after, K)
ROWS, CHUNK, SLABS = 1024, 128, 16
GEOMETRY_CASES = {
    "head_crosses_chunk": ((70, 400), 31, CHUNK + 1),   # a group from column 70: its K head columns cross column 128
    "three_tiles": ((1, 1, 2 * ROWS + 298), 40, 10),    # tail tiles: one-chunk spans; head rows: all slabs; the carry
    "cutoff_above_every_group": ((5, 17, 64, 200), 30, 4096),
    "two_groups_one_tile": ((10, 390, 500), 50, 3),
    "equal_scores": ((3, 300, 40), 5, 3),               # one score per group: the places are the example order
}


def geometry_case(name):
    """(ids, scores, graded labels, K, grad_scale) of a GEOMETRY_CASES entry, the examples shuffled."""
    sizes, pairs, K = GEOMETRY_CASES[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    g = np.concatenate([np.repeat(np.arange(len(sizes)), sizes), len(sizes) + np.arange(2 * pairs + 1) // 2])
    s = rng.normal(0.0, 3.0, g.size)
    if name == "equal_scores":
        s = np.where(g < len(sizes), 0.75 - g, s)
    y = rng.integers(-1, 4, g.size).astype(np.float32)
    perm = rng.permutation(g.size)
    return g[perm].astype(np.int32), s[perm].astype(np.float32), y[perm], K, 1.0 / g.size


def exact_zeros_case():
    """(g, s, y, the live examples): NaN / inf scores at excluded examples, a singleton and a group of no gain."""
    nan, inf = np.nan, np.inf
    g = np.array([-1, 0, 1, 1, 1, 3, 3, 3, 3, -1], dtype=np.int32)
    s = np.array([nan, inf, nan, -inf, 2.0, 0.5, -1.0, 0.5, 3.0, inf], dtype=np.float32)
    y = np.array([1.0, 2.0, 0.0, -1.0, 0.0, 0.0, 2.0, 1.0, 0.0, 3.0], dtype=np.float32)
    return g, s, y, np.arange(5, 9)
