"""Python-int oracle of ``K.auc_delong`` (DeLong, DeLong & Clarke-Pearson 1988): placements by sorted searches,
the variance / covariance formulas in ``fractions.Fraction``, a brute-force check from the P x N comparison matrix,
and the test cases.  Scores compare as float64 values of the fp32 inputs (-0.0 == +0.0, infinities ordinary)."""

from __future__ import annotations

import math
import statistics
from bisect import bisect_left, bisect_right
from fractions import Fraction

import numpy as np

MOMENTS = ("m_pos_aa", "m_neg_aa", "m_pos_bb", "m_neg_bb", "m_pos_ab", "m_neg_ab")
MASK = 0xFFFFFFFF


def make_case(n: int, seed: int, ties: bool = False, two: bool = True, rho: float = 0.8):
    """(scores_a, scores_b or None, labels): logistic labels (~40% positives) of continuous scores, or of scores
    rounded to sixteenths (tie runs cross tile borders); the second model is correlated with the first."""
    g = np.random.default_rng(seed)
    a = g.standard_normal(n)
    y = (g.random(n) < 1 / (1 + np.exp(-(1.1 * a - 0.4)))).astype(np.float32)
    b = rho * a + math.sqrt(1 - rho * rho) * g.standard_normal(n)
    if ties:
        a, b = np.round(16 * a) / 16, np.round(16 * b) / 16
    return a.astype(np.float32), (b.astype(np.float32) if two else None), y


def placements(scores, labels) -> list:
    """Every example's integer placement: a positive's Nlt + Nle, a negative's Pgt + Pge."""
    s = np.asarray(scores, np.float32).astype(np.float64)
    pos = np.asarray(labels, np.float64) > 0
    sn, sp = np.sort(s[~pos]), np.sort(s[pos])
    P = int(sp.size)
    if s.size > 4096:  # (the same searches, vectorised: exact comparisons of exact values)
        a = np.searchsorted(sn, s, "left") + np.searchsorted(sn, s, "right")
        b = (P - np.searchsorted(sp, s, "right")) + (P - np.searchsorted(sp, s, "left"))
        return [int(v) for v in np.where(pos, a, b)]
    sn, sp = sn.tolist(), sp.tolist()
    return [bisect_left(sn, x) + bisect_right(sn, x) if p else (P - bisect_right(sp, x)) + (P - bisect_left(sp, x))
            for x, p in zip(s.tolist(), pos.tolist())]


def split_sum(xs, ys) -> tuple:
    """(hi, lo) of sum x y: hi = sum (t >> 32), lo = sum (t & 0xffffffff)."""
    ts = [x * y for x, y in zip(xs, ys)]
    return sum(t >> 32 for t in ts), sum(t & MASK for t in ts)


class Oracle:
    def __init__(self, scores_a, labels, scores_b=None):
        y = np.asarray(labels)
        self.pos = [float(v) > 0 for v in y]
        self.P = sum(self.pos)
        self.N = len(self.pos) - self.P
        self.has_b = scores_b is not None
        self.nans = [int(np.isnan(np.asarray(s, np.float32)).sum()) if s is not None else 0
                     for s in (scores_a, scores_b)]
        self.pl = {"a": placements(scores_a, y), "b": placements(scores_b, y) if self.has_b else None}
        self.U2 = {}
        for m in "ab":
            pl = self.pl[m]
            if pl is None:
                self.U2[m] = 0
                continue
            up = sum(v for v, p in zip(pl, self.pos) if p)
            assert up == sum(v for v, p in zip(pl, self.pos) if not p)  # sum_pos a_i == sum_neg b_j
            self.U2[m] = up

    def _sel(self, m: str, positive: bool) -> list:
        return [v for v, p in zip(self.pl[m], self.pos) if p == positive]

    def words(self) -> list:
        """The 20 record words."""
        w = [self.U2["a"], self.U2["b"], self.P, self.N]
        for x, y in ("aa", "bb", "ab"):
            for positive in (True, False):
                w += list(split_sum(self._sel(x, positive), self._sel(y, positive))) if self.has_b or x + y == "aa" \
                    else [0, 0]
        return w + [self.nans[0], self.nans[1], int(self.has_b), 0]

    def moment(self, x: str, y: str, positive: bool) -> int:
        return sum(u * v for u, v in zip(self._sel(x, positive), self._sel(y, positive)))

    def theta(self, m: str = "a") -> Fraction:
        return Fraction(self.U2[m], 2 * self.P * self.N)

    def cov(self, x: str = "a", y: str = "a") -> Fraction:
        P, N = self.P, self.N
        uu = self.U2[x] * self.U2[y]
        s10 = Fraction(self.moment(x, y, True) * P - uu, 4 * N * N * P * (P - 1))
        s01 = Fraction(self.moment(x, y, False) * N - uu, 4 * P * P * N * (N - 1))
        return s10 / P + s01 / N

    def var_diff(self) -> Fraction:
        return self.cov("a", "a") + self.cov("b", "b") - 2 * self.cov("a", "b")

    def interval(self, level: float) -> tuple:
        t, se = float(self.theta()), math.sqrt(float(self.cov()))
        z = statistics.NormalDist().inv_cdf((1 + level) / 2)
        return max(0.0, t - z * se), min(1.0, t + z * se)

    def difference(self) -> tuple:
        d, v = self.theta("a") - self.theta("b"), self.var_diff()
        if v > 0:
            se = math.sqrt(float(v))
            z = float(d) / se
        else:
            se, z = 0.0, (0.0 if d == 0 else math.copysign(math.inf, d))
        return float(d), se, z, math.erfc(abs(z) / math.sqrt(2.0))


def brute_force(scores_a, labels, scores_b=None) -> dict:
    """DeLong from the P x N kernel matrix psi(pos, neg) = 1 / 0.5 / 0 (n <= 300): theta per model and the
    covariance matrix, as Fractions."""
    y = np.asarray(labels)
    pos = [i for i, v in enumerate(y) if float(v) > 0]
    neg = [i for i, v in enumerate(y) if not float(v) > 0]
    P, N = len(pos), len(neg)
    assert P + N <= 300 and P >= 2 and N >= 2
    half = Fraction(1, 2)
    theta, v10, v01 = [], [], []
    for s in (scores_a, scores_b):
        if s is None:
            continue
        s = [float(x) for x in np.asarray(s, np.float32)]
        psi = [[Fraction(1) if s[i] > s[j] else (half if s[i] == s[j] else Fraction(0)) for j in neg] for i in pos]
        v10.append([sum(row) / N for row in psi])
        v01.append([sum(psi[i][j] for i in range(P)) / P for j in range(N)])
        theta.append(sum(v10[-1]) / P)
    k = len(theta)
    cov = [[None] * k for _ in range(k)]
    for x in range(k):
        for z in range(k):
            s10 = sum((u - theta[x]) * (v - theta[z]) for u, v in zip(v10[x], v10[z])) / (P - 1)
            s01 = sum((u - theta[x]) * (v - theta[z]) for u, v in zip(v01[x], v01[z])) / (N - 1)
            cov[x][z] = s10 / P + s01 / N
    return {"theta": theta, "cov": cov}


def moments_case():
    """Placements of 2^31 - 1 (and a few smaller ones) on 3 * 2048 + 77 examples: the hi words carry."""
    n = 3 * 2048 + 77
    g = np.random.default_rng(11)
    big = 2**31 - 1
    pa = np.full(n, big, np.int64)
    pb = np.full(n, big, np.int64)
    pa[g.integers(0, n, 50)] = g.integers(0, big, 50)
    pb[g.integers(0, n, 50)] = g.integers(0, 2**16, 50)
    y = (g.random(n) < 0.5).astype(np.float32)
    return pa, pb, y


def expected_moments(pa, pb, y) -> list:
    w = []
    for x, z in ((pa, pa), (pb, pb), (pa, pb)):
        for positive in (True, False):
            keep = (y > 0) == positive
            w += list(split_sum(x[keep].tolist(), z[keep].tolist()))
    return w
