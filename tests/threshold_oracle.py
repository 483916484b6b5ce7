"""The threshold metrics' oracle, written from the definitions (not a port of the code under test): exact integer
arithmetic over a stable argsort of the complemented order-preserving key, cumulative sums from the top, and
``math.fsum`` where a value is a sum of rounded terms; and a brute-force check that loops over the distinct scores.

Every weight is an fp32 value, hence an integer multiple of 1 / ``scale`` for a power of two ``scale`` (1 without
weights and for integer weights): TP, FP, P and N are exact Python ints in units of 1 / scale, and every rate is
the correctly rounded quotient of two of them.

  candidate thresholds: the distinct scores t with PP(t) = TP(t) + FP(t) > 0, from the highest down
  AP = (1 / P) sum_{i positive} w_i TP(s_i) / PP(s_i);  KS = max_t |TP / P - FP / N|;  F1 = max_t 2 TP / (PP + P)
  precision target pi: the greatest TP among TP >= pi PP;  recall target rho: the highest t with TP >= rho P
  (equal maxima: the highest score; the two target tests in fp64 as written)
"""

from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

from auc_oracle import SPECIAL_LABELS, SPECIAL_SCORES, keys_of, make_case, rel_bound  # noqa: F401  (re-exported)


def _int_weights(weights, n: int):
    """(integer weights in units of 1 / scale, scale): int64 when scale == 1, else Python ints."""
    if weights is None:
        return np.ones(n, np.int64), 1
    w = np.asarray(weights, np.float32).astype(np.float64)
    if np.all(w == np.round(w)):
        return w.astype(np.int64), 1
    scale = max(float(x).as_integer_ratio()[1] for x in w)
    return np.array([int(Fraction(float(x)) * scale) for x in w], dtype=object), scale


class Oracle:
    """The candidate thresholds of one input from the highest score down: ``thr`` (fp32 values, +0.0 for either
    zero), ``tp`` / ``fp`` (Python ints in units of 1 / scale), and P, N, the NaN count."""

    def __init__(self, scores, labels, weights=None):
        s = np.ascontiguousarray(scores, np.float32)
        y = np.asarray(labels, np.float32)
        n = s.size
        self.n = n
        self.nans = int(np.isnan(s).sum())
        w, self.scale = _int_weights(weights, n)
        order = np.argsort(~keys_of(s), kind="stable")
        ks, pos, w = keys_of(s)[order], (y[order] > 0), w[order]
        zero = w.dtype.type(0) if w.dtype != object else 0
        ctp = np.cumsum(np.where(pos, w, zero)) if n else np.zeros(0, np.int64)
        cfp = np.cumsum(np.where(pos, zero, w)) if n else np.zeros(0, np.int64)
        self.P = int(ctp[-1]) if n else 0
        self.N = int(cfp[-1]) if n else 0
        end = np.flatnonzero(np.append(ks[1:] != ks[:-1], True)) if n else np.zeros(0, np.int64)
        start = np.append(0, end[:-1] + 1) if n else end
        self.thr, self.tp, self.fp, self.run_pos = [], [], [], []
        for a, e in zip(start.tolist(), end.tolist()):
            tp, fp = int(ctp[e]), int(cfp[e])
            if tp + fp > 0:
                t = np.float32(s[order[e]])
                self.thr.append(np.float32(0.0) if t == 0 else t)
                self.tp.append(tp)
                self.fp.append(fp)
                self.run_pos.append(int(ctp[e]) - (int(ctp[a - 1]) if a else 0))  # the run's positive weight

    @property
    def defined(self) -> bool:
        return not self.nans and self.P > 0 and self.N > 0

    # ---- the rates at candidate i, each the correctly rounded quotient of exact integers ------------------
    def precision(self, i: int) -> float:
        return self.tp[i] / (self.tp[i] + self.fp[i])

    def recall(self, i: int) -> float:
        return self.tp[i] / self.P

    def f1(self, i: int) -> float:
        return 2 * self.tp[i] / (self.tp[i] + self.fp[i] + self.P)

    def ks_at(self, i: int) -> float:
        return abs(self.tp[i] * self.N - self.fp[i] * self.P) / (self.P * self.N)

    def index_of(self, threshold: float) -> int:
        """The candidate whose score is ``threshold`` (ValueError when there is none)."""
        return [float(t) for t in self.thr].index(float(threshold))

    # ---- the metrics --------------------------------------------------------------------------------------
    def ap(self) -> float:
        if not self.defined:
            return float("nan")
        terms = [rp * tp / (tp + fp) for rp, tp, fp in zip(self.run_pos, self.tp, self.fp) if rp]
        return math.fsum(terms) / self.P

    def ks(self):
        """(value, candidate index): the first (highest score) of the exact maxima."""
        d = [abs(tp * self.N - fp * self.P) for tp, fp in zip(self.tp, self.fp)]
        i = d.index(max(d))
        return self.ks_at(i), i

    def best_f1(self):
        f = [Fraction(2 * tp, tp + fp + self.P) for tp, fp in zip(self.tp, self.fp)]
        i = f.index(max(f))
        return self.f1(i), i

    def at_precision(self, target: float):
        """Candidate index or None; the test TP >= target * PP in fp64 as written."""
        ok = [i for i in range(len(self.thr))
              if float(self.tp[i]) / self.scale >= target * (float(self.tp[i] + self.fp[i]) / self.scale)]
        if not ok:
            return None
        best = max(self.tp[i] for i in ok)
        return next(i for i in ok if self.tp[i] == best)

    def at_recall(self, target: float):
        for i in range(len(self.thr)):
            if float(self.tp[i]) / self.scale >= target * (float(self.P) / self.scale):
                return i
        return None

    def point(self, i):
        """(TP, FP, threshold) in weight units (ints when scale == 1), as ``ThresholdStats.stats()`` reports."""
        if i is None:
            return None
        if self.scale == 1:
            return self.tp[i], self.fp[i], float(self.thr[i])
        return self.tp[i] / self.scale, self.fp[i] / self.scale, float(self.thr[i])


def brute_force(scores, labels, weights=None):
    """For tiny n, the definitions threshold by threshold in Fractions: (AP, KS, its threshold, best F1, its
    threshold), None values when a class is empty."""
    s = np.asarray(scores, np.float32)
    y = np.asarray(labels, np.float32) > 0
    w = [Fraction(1)] * s.size if weights is None else [Fraction(float(x)) for x in np.asarray(weights, np.float32)]
    P = sum((w[i] for i in range(s.size) if y[i]), Fraction(0))
    N = sum((w[i] for i in range(s.size) if not y[i]), Fraction(0))
    if not P > 0 or not N > 0:
        return None, None, None, None, None

    def at(t):
        tp = sum((w[i] for i in range(s.size) if y[i] and s[i] >= t), Fraction(0))
        fp = sum((w[i] for i in range(s.size) if not y[i] and s[i] >= t), Fraction(0))
        return tp, fp

    ap = sum((w[i] * at(s[i])[0] / sum(at(s[i])) for i in range(s.size) if y[i] and w[i] > 0), Fraction(0)) / P
    ks = f1 = Fraction(-1)
    ks_t = f1_t = None
    for t in sorted(set(float(x) for x in s), reverse=True):  # (-0.0 == 0.0: one threshold)
        tp, fp = at(np.float32(t))
        if not tp + fp > 0:
            continue
        if abs(tp / P - fp / N) > ks:
            ks, ks_t = abs(tp / P - fp / N), t + 0.0
        if 2 * tp / (tp + fp + P) > f1:
            f1, f1_t = 2 * tp / (tp + fp + P), t + 0.0
    return ap, ks, ks_t, f1, f1_t


# ---- what the tests assert of a ``ThresholdStats`` against the oracle ------------------------------------------
PRECISION_TARGETS = (0.5, 0.9, 0.35, 1.0)
RECALL_TARGETS = (0.25, 0.5, 0.9, 1.0)


def _same_point(got, want) -> bool:
    """(TP, FP, threshold) equal, the threshold with its sign (a +-0 run reports +0.0)."""
    if got is None or want is None:
        return got is None and want is None
    return tuple(got) == tuple(want) and math.copysign(1.0, got[2]) == math.copysign(1.0, want[2])


def assert_exact(ts, o: Oracle, pt=(), rt=()) -> None:
    """Unweighted and integer weights: every integer and every selected threshold equal the oracle's; the AP
    within 3 rho_n (its numerator is an fp64 sum of n correctly rounded terms); every rate the same quotient."""
    assert o.scale == 1
    st = ts.stats()
    assert (st["P"], st["N"], st["nans"]) == (o.P, o.N, o.nans), (st, o.P, o.N)
    if not o.defined:
        assert all(math.isnan(v) for v in (ts.ap(), *ts.ks(), *ts.best_f1()))
        return
    tol = 3 * rel_bound(o.n)
    print("ap", ts.ap(), "oracle", o.ap(), "relative error", abs(ts.ap() - o.ap()) / o.ap(), "bound", tol)
    assert abs(ts.ap() - o.ap()) <= tol * o.ap()
    kv, ki = o.ks()
    assert _same_point(st["ks"], o.point(ki)), (st["ks"], o.point(ki))
    assert abs(ts.ks()[0] - kv) <= (2 * tol if ts.weighted else 0.0) and ts.ks()[1] == float(o.thr[ki])
    fv, fi = o.best_f1()
    assert _same_point(st["best_f1"], o.point(fi)), (st["best_f1"], o.point(fi))
    assert ts.best_f1() == (fv, float(o.thr[fi]), o.precision(fi), o.recall(fi))
    for kind, targets, find, read in (("precision", pt, o.at_precision, ts.at_precision),
                                      ("recall", rt, o.at_recall, ts.at_recall)):
        for j, target in enumerate(targets):
            i = find(target)
            assert _same_point(st[kind][j], o.point(i)), (kind, target, st[kind][j], o.point(i))
            if i is None:
                assert all(math.isnan(v) for v in read(target))
            else:
                assert read(target) == (float(o.thr[i]), o.precision(i), o.recall(i))


def _close(got: float, want: float, tol: float) -> bool:
    return abs(got - want) <= tol * abs(want)


def assert_real(ts, o: Oracle, pt=(), rt=()) -> None:
    """Real weights, rho_n = rel_bound(n): TP, FP and P are fixed-order sums of <= n non-negative fp64 terms, each
    within rho_n of the exact value, so a rate is within 2 rho_n plus two roundings and AP, best F1 and every
    reported precision and recall are held to 3 rho_n relative, KS (a difference of two rates <= 1) to 6 rho_n
    absolute.  A selected threshold may resolve a near-tie either way: the oracle's metric at the reported
    threshold is held to the same tolerance of the oracle's optimum.  A precision target's point has oracle
    precision >= pi (1 - 3 rho_n) and a recall not below, by more than 3 rho_n, the best oracle recall among the
    thresholds with precision >= pi (1 + 3 rho_n); a recall target's point, by the same reasoning, has oracle
    recall >= rho (1 - 3 rho_n) and lies no lower than the highest threshold with recall >= rho (1 + 3 rho_n)."""
    st = ts.stats()
    rho = rel_bound(o.n)
    tol = 3 * rho
    assert _close(st["P"], o.P / o.scale, rho) and _close(st["N"], o.N / o.scale, rho) and st["nans"] == o.nans
    if not o.defined:
        assert all(math.isnan(v) for v in (ts.ap(), *ts.ks(), *ts.best_f1()))
        return
    m = len(o.thr)
    print("ap", ts.ap(), "oracle", o.ap(), "relative error", abs(ts.ap() - o.ap()) / o.ap(), "bound", tol)
    assert _close(ts.ap(), o.ap(), tol)
    v, t = ts.ks()
    opt = o.ks()[0]
    print("ks", v, "oracle", opt, "at the reported threshold", o.ks_at(o.index_of(t)), "bound", 2 * tol)
    assert abs(v - opt) <= 2 * tol and o.ks_at(o.index_of(t)) >= opt - 2 * tol
    v, t, p, r = ts.best_f1()
    i, opt = o.index_of(t), o.best_f1()[0]
    print("best f1", v, "oracle", opt, "at the reported threshold", o.f1(i))
    assert _close(v, opt, tol) and o.f1(i) >= opt * (1 - tol)
    assert _close(p, o.precision(i), tol) and _close(r, o.recall(i), tol)
    for target in pt:
        t, p, r = ts.at_precision(target)
        strict = [i for i in range(m) if o.precision(i) >= target * (1 + tol)]
        if math.isnan(t):
            assert not strict, (target, strict[:3])
            continue
        i = o.index_of(t)
        assert o.precision(i) >= target * (1 - tol), (target, o.precision(i))
        assert _close(p, o.precision(i), tol) and _close(r, o.recall(i), tol)
        if strict:
            assert o.recall(i) >= max(o.recall(k) for k in strict) * (1 - tol)
    for target in rt:
        t, p, r = ts.at_recall(target)
        i = o.index_of(t)
        assert o.recall(i) >= target * (1 - tol), (target, o.recall(i))
        assert _close(p, o.precision(i), tol) and _close(r, o.recall(i), tol)
        strict = [k for k in range(m) if o.recall(k) >= target * (1 + tol)]
        assert not strict or i <= strict[0], (target, i, strict[0])
