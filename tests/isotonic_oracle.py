"""Exact references for the isotonic fit (ops/kernels.py ``isotonic_fit``) and for applying one
(``calibrate_apply``), and the inputs the tests share.

The fit is the serial stack over the cumulative (weight, positive weight) diagram in exact arithmetic: Python
ints without weights; with weights every fp32 weight is taken as a ``fractions.Fraction`` and all of them are
scaled by their common (power of two) denominator, so the stack again runs on Python ints.  The apply rule is
evaluated in fp64 numpy scalars."""

import bisect
import math
from fractions import Fraction

import numpy as np


def sort_order(s):
    """Stable ascending order of fp32 scores by value (-0.0 == +0.0) and the values with -0.0 folded."""
    v = np.asarray(s, np.float32) + np.float32(0.0)  # (-0.0 + 0.0 = +0.0; numpy keeps denormals)
    order = np.argsort(v, kind="stable")
    return order, v[order]


def fit(s, y, w=None):
    """The exact fit: dict with the vertex list ``H`` (sorted positions), the blocks' ``lo`` / ``hi`` (fp32),
    ``W`` / ``Y`` (ints without weights, else Fractions), ``v`` (Fractions) and ``fitted`` (fp64, input order)."""
    s = np.asarray(s, np.float32)
    n = len(s)
    assert n >= 1 and not np.isnan(s).any()
    order, sv = sort_order(s)
    pos = np.asarray(y)[order] > 0
    if w is None:
        scale, wi = 1, [1] * n
    else:
        fr = [Fraction(float(x)) for x in np.asarray(w, np.float32)[order]]
        assert all(f > 0 for f in fr)
        scale = max(f.denominator for f in fr)
        wi = [int(f * scale) for f in fr]
    cW, cY = [0] * (n + 1), [0] * (n + 1)
    for j in range(n):
        cW[j + 1] = cW[j] + wi[j]
        cY[j + 1] = cY[j] + (wi[j] if pos[j] else 0)
    cand = [j for j in range(n + 1) if j == 0 or j == n or sv[j - 1] != sv[j]]

    def below(a, b, c):
        return (cY[b] - cY[a]) * (cW[c] - cW[b]) < (cY[c] - cY[b]) * (cW[b] - cW[a])

    st = []
    for c in cand:
        while len(st) >= 2 and not below(st[-2], st[-1], c):
            st.pop()
        st.append(c)
    m = len(st) - 1
    W = [cW[st[b + 1]] - cW[st[b]] for b in range(m)]
    Y = [cY[st[b + 1]] - cY[st[b]] for b in range(m)]
    v = [Fraction(Y[b], W[b]) for b in range(m)]
    assert all(v[b] < v[b + 1] for b in range(m - 1))
    fitted = np.empty(n, np.float64)
    for b in range(m):
        fitted[order[st[b]:st[b + 1]]] = float(v[b])
    if w is not None:
        W, Y = [Fraction(x, scale) for x in W], [Fraction(x, scale) for x in Y]
    return {"H": st, "lo": sv[[st[b] for b in range(m)]], "hi": sv[[st[b + 1] - 1 for b in range(m)]], "W": W,
            "Y": Y, "v": v, "fitted": fitted}


def calibrator(f):
    """(x, y) fp32 threshold lists of an oracle fit."""
    m = len(f["v"])
    x, y = np.empty(2 * m, np.float32), np.empty(2 * m, np.float32)
    x[0::2], x[1::2] = f["lo"], f["hi"]
    y[0::2] = y[1::2] = np.array([float(v) for v in f["v"]], np.float64).astype(np.float32)
    return x, y


def apply(s, x, y):
    """The apply rule in fp64: (values, in_gap) -- in_gap marks the scores strictly between two blocks."""
    x64, y64 = np.asarray(x, np.float64), np.asarray(y, np.float64)
    lo, hi, v = x64[0::2], x64[1::2], y64[0::2]
    m = len(v)
    out, gap = np.empty(len(s), np.float64), np.zeros(len(s), bool)
    for i, si in enumerate(np.asarray(s, np.float64)):
        if math.isnan(si):
            out[i] = math.nan
        elif si <= hi[0]:
            out[i] = v[0]
        elif si >= lo[m - 1]:
            out[i] = v[m - 1]
        else:
            b = bisect.bisect_right(lo.tolist(), si) - 1  # the last block with lo_b <= s
            if si <= hi[b]:
                out[i] = v[b]
                continue
            gap[i] = True
            if math.isinf(lo[b + 1]):
                t = 0.5 if math.isinf(hi[b]) else 0.0
            elif math.isinf(hi[b]):
                t = 1.0
            else:
                t = (si - hi[b]) / (lo[b + 1] - hi[b])
            out[i] = min(max(v[b] + t * (v[b + 1] - v[b]), v[b]), v[b + 1])
    return out, gap


def apply_grid(x):
    """Scores around a calibrator: every threshold, its fp32 neighbours on either side, the midpoint of every gap,
    values outside both ends, +-inf and NaN."""
    x = np.asarray(x, np.float32)
    g = [x, np.nextafter(x, np.float32(np.inf)), np.nextafter(x, np.float32(-np.inf))]
    hi, lo = x[1:-1:2].astype(np.float64), x[2::2].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        mid = (hi / 2 + lo / 2).astype(np.float32)
    g.append(mid[np.isfinite(mid)])
    fin = x[np.isfinite(x)]
    ends = [fin.min() - 1, fin.min() - 1e6, fin.max() + 1, fin.max() + 1e6] if len(fin) else []
    g.append(np.array(ends + [np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32))
    return np.ascontiguousarray(np.concatenate(g), np.float32)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
def logistic(n, seed, ties=False):
    """Random logistic data: scores N(0, 2), P(positive) = sigmoid(score + noise); ties: scores rounded to 1/8."""
    r = np.random.default_rng(seed)
    s = r.normal(0, 2, n).astype(np.float32)
    y = (r.random(n) < 1 / (1 + np.exp(-(0.7 * s + 0.3)))).astype(np.float32)
    if ties:
        s = (np.round(s * 8) / 8).astype(np.float32)
    return s, y


def dyadic_weights(n, seed):
    """Multiples of 1/64 in (0, 4]: every prefix sum and cross product of n <= 2^18 of them is exact in fp64."""
    return (np.random.default_rng(seed).integers(1, 257, n) / 64).astype(np.float32)


def general_weights(n, seed):
    return np.random.default_rng(seed).uniform(0.5, 2, n).astype(np.float32)


def farey(order):
    fr = sorted({Fraction(p, q) for q in range(1, order + 1) for p in range(q + 1)})
    return [(f.numerator, f.denominator) for f in fr]


def staircase(order, tied):
    """For every reduced fraction p/q, q <= order, ascending: a run of q examples with p positives.  tied: the run
    shares one score (its end is the only candidate); else increasing scores, the positives first (the run pools)."""
    s, y = [], []
    k = 0
    for r, (p, q) in enumerate(farey(order)):
        for i in range(q):
            s.append(r if tied else k)
            y.append(1.0 if i < p else 0.0)
            k += 1
    return np.array(s, np.float32), np.array(y, np.float32)


def one_score(n, seed=5):
    return np.full(n, 0.25, np.float32), (np.random.default_rng(seed).random(n) < 0.3).astype(np.float32)


def separated(n):
    s = np.random.default_rng(6).permutation(n).astype(np.float32)
    return s, (s >= n // 2).astype(np.float32)


def anti_sorted(n=3 * 2048 + 5):
    s = np.random.default_rng(7).permutation(n).astype(np.float32)
    return s, (s < n // 3).astype(np.float32)


def long_tie(n=4 * 2048 + 10, first=2048 - 100, last=3 * 2048 + 50, seed=8):
    """Untied scores but for one tie run that starts in one tile and ends two tiles later."""
    r = np.random.default_rng(seed)
    s = np.arange(n, dtype=np.float32)
    s[first:last + 1] = s[first]
    y = (r.random(n) < 1 / (1 + np.exp(-(np.arange(n) / n * 6 - 3)))).astype(np.float32)
    p = r.permutation(n)
    return s[p], y[p]


LAYOUTS = {
    "one_score": lambda: one_score(3 * 2048 + 5),
    "separated": lambda: separated(2 * 2048 + 3),
    "anti_sorted": anti_sorted,
    "farey32_tied": lambda: staircase(32, True),
    "farey32_untied": lambda: staircase(32, False),
    "farey48_untied": lambda: staircase(48, False),
    "long_tie": long_tie,
}
# (examples, blocks) where the layout fixes them
LAYOUT_BLOCKS = {"one_score": (3 * 2048 + 5, 1), "separated": (2 * 2048 + 3, 2), "anti_sorted": (3 * 2048 + 5, 1),
                 "farey32_tied": (7044, 325), "farey32_untied": (7044, 325), "farey48_untied": (22964, 713)}


# ---------------------------------------------------------------------------
# checks shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------
def check_exact(blocks, f):
    """Block arrays (lo, hi, W, Y, v as numpy) equal the oracle's: the positions through lo / hi, W and Y as exact
    numbers, v as the correctly rounded quotient."""
    lo, hi, W, Y, v = blocks
    assert len(v) == len(f["v"]), (len(v), len(f["v"]))
    assert lo.dtype == np.float32 and hi.dtype == np.float32 and v.dtype == np.float64
    assert np.array_equal(lo, f["lo"]) and np.array_equal(hi, f["hi"])
    if W.dtype == np.int64:
        assert W.tolist() == f["W"] and Y.tolist() == f["Y"]
    else:
        assert [Fraction(float(a)) for a in W] == f["W"] and [Fraction(float(a)) for a in Y] == f["Y"]
    assert v.tolist() == [float(a) for a in f["v"]]
    assert (np.diff(v) > 0).all()


def check_close(fitted, f, tol=1e-9):
    err = float(np.abs(np.asarray(fitted, np.float64) - f["fitted"]).max())
    print("largest fitted-value error", err)
    assert err <= tol
    assert (fitted >= 0).all() and (fitted <= 1).all()


def check_apply(got, s, x, y):
    """calibrate_apply's fp32 output against the fp64 rule: NaN for NaN, exactly v_b outside the gaps, inside a
    gap within [v_b, v_b+1] and within 2^-22 of the reference (three fp32 roundings of quantities <= 1)."""
    want, gap = apply(s, x, y)
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.sum() == np.isnan(s).sum()
    flat = ~nan & ~gap
    assert np.array_equal(got[flat].astype(np.float64), want[flat])
    if gap.any():
        y64 = np.asarray(y, np.float64)[0::2]
        lo64 = np.asarray(x, np.float64)[0::2]
        b = np.searchsorted(lo64, np.asarray(s, np.float64)[gap], side="right") - 1
        g = got[gap].astype(np.float64)
        assert (g >= y64[b]).all() and (g <= y64[b + 1]).all()
        err = float(np.abs(g - want[gap]).max())
        print("largest gap error", err, "of", int(gap.sum()), "gap scores")
        assert err <= 2.0 ** -22
