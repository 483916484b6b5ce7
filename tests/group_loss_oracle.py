"""fp64 oracle of the listwise softmax loss (``ops.kernels.group_softmax_loss``), group by group with ``math.fsum``.

Straight from the definition: per group g over its non-excluded examples, with the gain ``a_i = w_i max(y_i, 0)``,

    m = max s_i      Z = sum exp(s_i - m)      A = sum a_i      T = sum a_i s_i
    L_g = A (m + log Z) - T                    dL/ds_i = A exp(s_i - m) / Z - a_i

A group id < 0 is an excluded example; a group with ``A == 0`` adds exactly 0 loss and 0 gradient.  Besides the loss
and the gradient it returns the two error scales the tests' bounds are written in.
"""

from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np

EPS32 = 2.0 ** -23
ABS = 1e-12
TINY32 = 2.0 ** -149  # fp32's smallest subnormal: what rounding a value below fp32's normal range once can cost


def gains(labels, weights):
    y = np.asarray(labels, dtype=np.float64)
    w = np.ones_like(y) if weights is None else np.asarray(weights, dtype=np.float64)
    return w * np.maximum(y, 0.0)


def loss_only(groups, scores, a) -> float:
    """sum_g L_g in fp64 (``a``: the gains); what the finite-difference check differentiates."""
    members: "OrderedDict[int, list]" = OrderedDict()
    for i, g in enumerate(groups):
        if g >= 0:
            members.setdefault(int(g), []).append(i)
    total = []
    for idx in members.values():
        A = math.fsum(a[i] for i in idx)
        if A == 0.0:
            continue
        m = max(scores[i] for i in idx)
        Z = math.fsum(math.exp(scores[i] - m) for i in idx)
        T = math.fsum(a[i] * scores[i] for i in idx)
        total.append(A * (m + math.log(Z)) - T)
    return math.fsum(total)


def group_softmax(groups, scores, labels, weights=None, grad_scale: float = 1.0):
    """(dpred [n] fp64, loss fp64, dscale [n], lscale): ``dscale_i = grad_scale (A_g p_i + a_i)`` and ``lscale =
    sum_g (A_g (|m_g| + |log Z_g|) + sum a_i |s_i|)``, the magnitudes the absolute parts of the bounds multiply."""
    groups = np.asarray(groups, dtype=np.int64)
    s = np.asarray(scores, dtype=np.float64)
    a = gains(labels, weights)
    n = s.shape[0]
    dpred = np.zeros(n, dtype=np.float64)
    dscale = np.zeros(n, dtype=np.float64)
    members: "OrderedDict[int, list]" = OrderedDict()
    for i in range(n):
        if groups[i] >= 0:
            members.setdefault(int(groups[i]), []).append(i)
    losses, lscale = [], []
    for idx in members.values():
        A = math.fsum(a[i] for i in idx)
        if A == 0.0:
            continue
        m = max(s[i] for i in idx)
        z = [math.exp(s[i] - m) for i in idx]
        Z = math.fsum(z)
        T = math.fsum(a[i] * s[i] for i in idx)
        losses.append(A * (m + math.log(Z)) - T)
        lscale.append(A * (abs(m) + abs(math.log(Z))) + math.fsum(a[i] * abs(s[i]) for i in idx))
        for i, zi in zip(idx, z):
            p = zi / Z
            dpred[i] = grad_scale * (A * p - a[i])
            dscale[i] = abs(grad_scale) * (A * p + a[i])
    return dpred, math.fsum(losses), dscale, math.fsum(lscale)


def check(dpred, loss, groups, scores, labels, weights=None, grad_scale: float = 1.0, what: str = "") -> None:
    """Assert the op's fp32 ``dpred`` / ``loss`` against the oracle within the derived bounds: the op computes in
    fp64 and rounds once, so |dpred - oracle| <= 2^-23 |oracle| + 1e-12 dscale and |loss - oracle| <= 2^-23
    |oracle| + 1e-12 lscale -- plus 2^-149 each, fp32's underflow step: with scores 160 apart in one group a
    softmax weight is ~1e-70, which no fp32 output holds to a relative 2^-23 (it rounds to 0).  Every example is
    compared; nothing is filtered."""
    ref_d, ref_l, dscale, lscale = group_softmax(groups, scores, labels, weights, grad_scale)
    got = np.asarray(dpred, dtype=np.float64)
    assert got.shape == ref_d.shape, (what, got.shape, ref_d.shape)
    err = np.abs(got - ref_d)
    bound = EPS32 * np.abs(ref_d) + ABS * dscale + TINY32
    bad = np.nonzero(~(err <= bound))[0]
    assert bad.size == 0, (what, "dpred", int(bad[0]), float(got[bad[0]]), float(ref_d[bad[0]]), float(bound[bad[0]]))
    lerr, lbound = abs(float(loss) - ref_l), EPS32 * abs(ref_l) + ABS * lscale + TINY32
    assert lerr <= lbound, (what, "loss", float(loss), ref_l, lerr, lbound)
