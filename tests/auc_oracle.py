"""The AUC tests' oracle: numpy int64 / fp64 over a stable argsort of the order-preserving key, cumsum and
searchsorted (not the code under test), its brute-force pairwise check, and the seeded inputs.

  P = sum_{pos} w,  N = sum_{neg} w,  positive iff label > 0
  U2 = sum_{i pos} w_i (Nlt(s_i) + Nle(s_i)),  AUC = U2 / (2 P N)
"""

from __future__ import annotations

import math

import numpy as np


def keys_of(scores: np.ndarray) -> np.ndarray:
    b = np.ascontiguousarray(scores, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0  # -0.0 == +0.0, by its bit pattern
    sign = np.uint32(0x80000000)
    return np.where((b & sign) != 0, ~b, b | sign).astype(np.uint32)


def oracle_stats(scores, labels, weights=None):
    """(U2, P, N, nans): Python ints without weights, floats (fp64 sums) with."""
    s = np.ascontiguousarray(scores, np.float32)
    y = np.asarray(labels, np.float32)
    nans = int(np.isnan(s).sum())
    k = keys_of(s)
    order = np.argsort(k, kind="stable")
    ks, pos = k[order], y[order] > 0
    if weights is None:
        w = np.ones(s.size, np.int64)
        zero = np.zeros(1, np.int64)
    else:
        w = np.asarray(weights, np.float32)[order].astype(np.float64)
        zero = np.zeros(1, np.float64)
    wneg = np.where(pos, 0, w).astype(w.dtype)
    nex = np.concatenate([zero, np.cumsum(wneg)])  # nex[j]: negative weight at sorted positions < j
    lb = np.searchsorted(ks, ks[pos], "left")
    ub = np.searchsorted(ks, ks[pos], "right")
    u2 = (w[pos] * (nex[lb] + nex[ub])).sum()
    p, n = w[pos].sum(), wneg.sum()
    conv = int if weights is None else float
    return conv(u2), conv(p), conv(n), nans


def value_of(stats) -> float:
    u2, p, n, nans = stats
    if nans or not p > 0 or not n > 0:
        return float("nan")
    return u2 / (2 * p * n)


def pairwise_stats(scores, labels, weights=None):
    """The definition, pair by pair, summed exactly (fsum of products that are exact in fp64)."""
    s = np.asarray(scores, np.float32)
    y = np.asarray(labels, np.float32)
    w = np.ones(s.size) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    pos, neg = np.flatnonzero(y > 0), np.flatnonzero(~(y > 0))
    c = 2.0 * (s[neg][None, :] < s[pos][:, None]) + 1.0 * (s[neg][None, :] == s[pos][:, None])
    terms = (w[pos][:, None] * w[neg][None, :]) * c
    return math.fsum(terms.ravel()), math.fsum(w[pos]), math.fsum(w[neg])


def make_case(n: int, seed: int, *, ties: bool = False, weights: str | None = None, pm1: bool = False):
    """Seeded (scores, labels, weights): continuous scores or scores rounded to one decimal (long tie runs,
    -0.0 among them), ~30% positives with at least one example of each class, weights None / "int" ({0..3})
    / "real" (uniform in (0.01, 1.01))."""
    rng = np.random.default_rng(seed)
    s = rng.standard_normal(n).astype(np.float32)
    if ties:
        s = np.round(s, 1)
    y = (rng.random(n) < 0.3).astype(np.float32)
    if n >= 2:
        y[0], y[1] = 1.0, 0.0
    w = None
    if weights == "int":
        w = rng.integers(0, 4, n).astype(np.float32)
        w[: min(n, 2)] = 1.0
    elif weights == "real":
        w = (rng.random(n) + 0.01).astype(np.float32)
    if pm1:
        y = 2.0 * y - 1.0
    return s, y, w


# -0.0 / +0.0 tie, both infinities are ordinary values, denormals keep their order around zero
SPECIAL_SCORES = np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, 1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 1e-42,
                           3e-42], np.float32)
SPECIAL_LABELS = np.array([1, 0, 1, 1, 1, 1, 0, 1, 0, 1, 0, 0, 0, 0], np.float32)


def rel_bound(n: int) -> float:
    """Relative error of a sum of n non-negative fp64 terms against another order of the same sum: the plain
    summation bound, 4 n 2^-53 (for U2, P and N alike)."""
    return 4.0 * n * 2.0 ** -53
