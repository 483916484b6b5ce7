"""fp64 oracle of the pairwise ranking loss (``ops.kernels.group_pairwise_loss``), group by group: numpy outer
differences per group, every sum in ``np.longdouble``.

Straight from the definition.  Example i is positive iff ``y_i > 0``; ``p_i = w_i`` for a positive (else 0), ``q_i =
w_i`` for a non-positive (else 0); per group g over its non-excluded examples (group id >= 0):

    P = sum p_i      N = sum q_j      c = (P + N) / (P N)
    L_g = c sum_{i: p_i > 0} sum_{j: q_j > 0} p_i q_j softplus(s_j - s_i)
    dL/ds_i = -c p_i sum_{j: q_j > 0} q_j sigma(s_j - s_i)         (positive i)
    dL/ds_j = +c q_j sum_{i: p_i > 0} p_i sigma(s_j - s_i)         (negative j)
    softplus(d) = max(d, 0) + log1p(exp(-|d|))      sigma(d) = 1 / (1 + exp(-d)) through t = exp(-|d|)

A group is valid iff P > 0 and N > 0.  An invalid group, an excluded example and an example of weight 0 add exactly 0
and get exactly 0: the oracle never reads their scores (a pair is formed only when ``p_i > 0`` and ``q_j > 0``).

The bound of ``check`` is derived, not tuned.  The op computes every term as a product of exact or correctly rounded
fp64 factors, sums non-negative terms only (no cancellation: a sum's relative error is at most its length times
2^-53 per addition), and rounds to fp32 once.  So for a position of a group of ``n_g`` examples

    |got - ref| <= (2^-23 + (n_g + 256) 2^-52) |ref| + 2^-149

and the same for the loss with ``n`` in place of ``n_g``:
  * 2^-23: the one rounding to fp32 (the figure of tests/group_loss_oracle.py);
  * n_g 2^-52: the summation over at most n_g columns and the factor c (P and N are sums of at most n_g weights);
  * 256 (x 2^-52): the few ulp of exp / log1p / the division in either implementation, and the inexact fp64
    ``s_j - s_i`` at the case list's score spread of 160 (|d| <= 160 < 2^8: an absolute error of 2^-45 in d, which
    is a relative one of at most 2^-45 in exp(-|d|) and in softplus(d) for d > 0);
  * 2^-149: fp32's underflow step (a sigma sum at a spread of 160 is ~1e-70, which fp32 rounds to 0).
Every example is compared; nothing is filtered.
"""

from __future__ import annotations

from collections import OrderedDict

import numpy as np

EPS32 = 2.0 ** -23
EPS64 = 2.0 ** -52
TINY32 = 2.0 ** -149
LD = np.longdouble


def class_weights(labels, weights):
    """(p, q) in fp64."""
    y = np.asarray(labels, dtype=np.float64)
    w = np.ones_like(y) if weights is None else np.asarray(weights, dtype=np.float64)
    pos = y > 0
    return np.where(pos, w, 0.0), np.where(pos, 0.0, w)


def _members(groups) -> "OrderedDict[int, np.ndarray]":
    groups = np.asarray(groups, dtype=np.int64)
    out: "OrderedDict[int, list]" = OrderedDict()
    for i, g in enumerate(groups):
        if g >= 0:
            out.setdefault(int(g), []).append(i)
    return OrderedDict((k, np.asarray(v, dtype=np.int64)) for k, v in out.items())


def _group(s, p, q, idx):
    """(L_g, ipos, dL/ds of ipos, ineg, dL/ds of ineg, W_g) of one group, None when it is invalid."""
    ipos, ineg = idx[p[idx] > 0], idx[q[idx] > 0]
    if ipos.size == 0 or ineg.size == 0:
        return None
    pp, qq = p[ipos], q[ineg]
    P, N = float(np.sum(pp, dtype=LD)), float(np.sum(qq, dtype=LD))
    c = (P + N) / (P * N)
    d = s[ineg][None, :] - s[ipos][:, None]     # [positives, negatives]: s_j - s_i
    t = np.exp(-np.abs(d))
    sig = np.where(d >= 0, 1.0, t) / (1.0 + t)
    sp = np.maximum(d, 0.0) + np.log1p(t)
    L = c * float(np.sum(pp[:, None] * qq[None, :] * sp, dtype=LD))
    dpos = -c * pp * np.sum(qq[None, :] * sig, axis=1, dtype=LD).astype(np.float64)
    dneg = c * qq * np.sum(pp[:, None] * sig, axis=0, dtype=LD).astype(np.float64)
    return L, ipos, dpos, ineg, dneg, P + N


def loss_only(groups, scores, p, q) -> float:
    """sum_g L_g in fp64; what the finite-difference check differentiates."""
    s = np.asarray(scores, dtype=np.float64)
    tot = LD(0)
    for idx in _members(groups).values():
        r = _group(s, p, q, idx)
        if r is not None:
            tot += LD(r[0])
    return float(tot)


def group_pairwise(groups, scores, labels, weights=None, grad_scale: float = 1.0):
    """(dpred [n] fp64, loss fp64, gsize [n]: the size of every example's group (0: excluded), per: {group id:
    (L_g, W_g)} of the valid groups)."""
    s = np.asarray(scores, dtype=np.float64)
    p, q = class_weights(labels, weights)
    n = s.shape[0]
    dpred = np.zeros(n, dtype=np.float64)
    gsize = np.zeros(n, dtype=np.int64)
    per = OrderedDict()
    tot = LD(0)
    for k, idx in _members(groups).items():
        gsize[idx] = idx.size
        r = _group(s, p, q, idx)
        if r is None:
            continue
        L, ipos, dpos, ineg, dneg, W = r
        dpred[ipos] = grad_scale * dpos
        dpred[ineg] = grad_scale * dneg
        per[k] = (L, W)
        tot += LD(L)
    return dpred, float(tot), gsize, per


def check(dpred, loss, groups, scores, labels, weights=None, grad_scale: float = 1.0, what: str = "") -> None:
    """Assert the op's fp32 ``dpred`` / ``loss`` against the oracle within the bound of the module docstring."""
    ref_d, ref_l, gsize, _ = group_pairwise(groups, scores, labels, weights, grad_scale)
    got = np.asarray(dpred, dtype=np.float64)
    assert got.shape == ref_d.shape, (what, got.shape, ref_d.shape)
    err = np.abs(got - ref_d)
    bound = (EPS32 + (gsize + 256) * EPS64) * np.abs(ref_d) + TINY32
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (what, "dpred", int(bad[0]), float(got[bad[0]]), float(ref_d[bad[0]]), float(bound[bad[0]]))
    lerr, lbound = abs(float(loss) - ref_l), (EPS32 + (got.shape[0] + 256) * EPS64) * abs(ref_l) + TINY32
    assert lerr <= lbound, (what, "loss", float(loss), ref_l, lerr, lbound)


def exact_zeros_case():
    """NaN and inf scores at: excluded examples (2, 7), singletons (0, 1), a group without a positive (id 2), a group
    without a negative (id 3), and the zero-weight members (12, 13) of the valid group 4, whose weighted members
    are 10, 11, 14.  Returns (g, s, y, w, the indices of the valid group's weighted members)."""
    nan, inf = np.nan, np.inf
    #             0    1     2    3    4     5    6    7     8     9    10   11    12    13   14
    g = np.array([0,   1,   -1,   2,   2,    2,   3,  -1,    3,    3,    4,   4,    4,    4,   4], dtype=np.int32)
    s = np.array([nan, -inf, nan, 1.0, inf,  nan, inf, inf,  nan,  2.0,  0.5, -1.0, nan,  inf, 0.25], dtype=np.float32)
    y = np.array([1.0, 0.0,  1.0, 0.0, -1.0, 0.0, 1.0, 1.0,  2.0,  1.0,  1.0, 0.0,  1.0,  0.0, 0.0], dtype=np.float32)
    w = np.array([1.0, 2.0,  1.0, 1.0, 1.0,  0.5, 1.0, 1.0,  1.0,  3.0,  1.5, 0.5,  0.0,  0.0, 2.0], dtype=np.float32)
    return g, s, y, w, np.array([10, 11, 14])
