"""Oracles of the grouped AUC (ops/kernels.py ``gauc``), exact: weights are taken as the rationals their fp32
bit patterns denote (integers after scaling by 2^149), so every per-group statistic is an exact integer or
``Fraction`` and only the last conversion to a float rounds.

* ``brute_groups``: the definition, per group a pair count over (positive, negative) pairs, O(n_g^2);
* ``sorted_groups``: one pass over the (group, score) order, for the larger cases.

Both return ``[G]`` lists of ``(U2_g, P_g, N_g)`` (ints without weights, ``Fraction`` with them);
``summary`` turns them into (GAUC, valid groups, examples in valid groups).  NaN scores are not ordered here:
the callers check the NaN count and the NaN value only."""

import math
from fractions import Fraction

import numpy as np

_SCALE = 2 ** 149  # every finite fp32 times this is an integer


def _int_weights(n, w):
    if w is None:
        return [1] * n, 1
    return [int(Fraction(float(x)) * _SCALE) for x in np.asarray(w, np.float32)], _SCALE


def _finish(recs, scale, weighted):
    if not weighted:
        return recs
    return [(Fraction(u2, scale * scale), Fraction(p, scale), Fraction(ng, scale)) for u2, p, ng in recs]


def brute_groups(s, y, g, G, w=None):
    s = np.asarray(s, np.float32).astype(np.float64)  # (-0.0 == +0.0, denormals and infinities ordered)
    y = np.asarray(y, np.float32)
    g = np.asarray(g)
    W, scale = _int_weights(len(s), w)
    members = [[] for _ in range(G)]
    for i, gi in enumerate(g):
        members[int(gi)].append(i)
    recs = []
    for m in members:
        pos = [i for i in m if y[i] > 0]
        neg = [i for i in m if not y[i] > 0]
        u2 = 0
        for i in pos:
            for j in neg:
                if s[j] < s[i]:
                    u2 += 2 * W[i] * W[j]
                elif s[j] == s[i]:
                    u2 += W[i] * W[j]
        recs.append((u2, sum(W[i] for i in pos), sum(W[j] for j in neg)))
    return _finish(recs, scale, w is not None)


def sorted_groups(s, y, g, G, w=None):
    s = np.asarray(s, np.float32).astype(np.float64)
    y = np.asarray(y, np.float32)
    g = np.asarray(g).astype(np.int64)
    n = len(s)
    W, scale = _int_weights(n, w)
    order = np.lexsort((s, g))
    recs = [(0, 0, 0)] * G
    j = 0
    while j < n:
        gi = g[order[j]]
        u2 = p = nlt = 0
        while j < n and g[order[j]] == gi:
            sj = s[order[j]]
            rp = rn = 0
            while j < n and g[order[j]] == gi and s[order[j]] == sj:
                i = order[j]
                if y[i] > 0:
                    rp += W[i]
                else:
                    rn += W[i]
                j += 1
            u2 += rp * (2 * nlt + rn)
            p += rp
            nlt += rn
        recs[int(gi)] = (u2, p, nlt)
    return _finish(recs, scale, w is not None)


def summary(recs, g, G):
    """(GAUC, valid groups, examples in valid groups) of per-group records and the ids they came from."""
    sizes = np.bincount(np.asarray(g).astype(np.int64), minlength=G)
    terms, ws, valid, covered = [], [], 0, 0
    for k, (u2, p, ng) in enumerate(recs):
        if p > 0 and ng > 0:
            terms.append(float(Fraction(p + ng) * Fraction(u2) / (2 * Fraction(p) * Fraction(ng))))
            ws.append(float(p + ng))
            valid += 1
            covered += int(sizes[k])
    value = math.fsum(terms) / math.fsum(ws) if valid else float("nan")
    return value, valid, covered


def make_groups_case(n, G, seed, *, distinct=None, weights=False, sizes=None):
    """Random (scores, labels, groups, weights): scores continuous or from ``distinct`` values, weights in
    [0.5, 2]; ``sizes``: the groups' sizes (sum n), dealt to shuffled positions -- else uniform random ids."""
    r = np.random.default_rng(seed)
    if distinct:
        s = r.integers(0, distinct, n).astype(np.float32) * np.float32(0.5) - np.float32(0.5)
    else:
        s = r.standard_normal(n).astype(np.float32)
    y = (r.random(n) < 0.4).astype(np.float32)
    if sizes is None:
        g = r.integers(0, G, n).astype(np.int32)
    else:
        g = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        assert len(g) == n
        g = g[r.permutation(n)]
    w = r.uniform(0.5, 2.0, n).astype(np.float32) if weights else None
    return s, y, g, w
