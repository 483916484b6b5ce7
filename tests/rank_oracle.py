"""Pure-Python oracle of the ranking metrics (NDCG@k, recall@k, precision@k per group), independent of the
CPU twin: per group it sorts by score and applies the tie rule -- a run of equal scores at the ranks a..b gives
every member the mean position weight (C_k(b) - C_k(a - 1)) / (b - a + 1) -- with ``fractions.Fraction`` for the
hits, recall and precision and ``math.fsum`` over exactly computed, once-rounded terms for DCG and IDCG.  The
discount sums C_k(r) = D[min(r, k)] come from the table the definition names: D[r] = D[r - 1] + 1 / log2(r + 1),
one sequential fp64 loop.

``brute_group`` checks the definition itself: it enumerates every tie-breaking permutation of a small group and
averages the plain metric (position weights 1 / log2(j + 1) and [j <= k], no tie rule)."""

import itertools
import math
from fractions import Fraction

import numpy as np

MAX_CUTOFF = 4096


def dcg_table() -> list:
    d = [0.0] * (MAX_CUTOFF + 1)
    for j in range(1, MAX_CUTOFF + 1):
        d[j] = d[j - 1] + 1.0 / math.log2(j + 1.0)
    return d


D = dcg_table()


def score_keys(s) -> np.ndarray:
    """Order-preserving integer keys of fp32 scores: -0.0 == +0.0, infinities and denormals as IEEE orders them."""
    b = np.ascontiguousarray(s, np.float32).view(np.uint32).astype(np.int64)
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, 0xFFFFFFFF - b, b | 0x80000000)


def gains_of(y) -> np.ndarray:
    y = np.ascontiguousarray(y, np.float32)
    return np.where(y > 0, y, np.float32(0)).astype(np.float32)


def _runs(keys) -> list:
    """[(members, a, b)] of a group: the runs of equal keys from the top, with the ranks a..b they occupy."""
    order = sorted(range(len(keys)), key=lambda i: -keys[i])
    out, r = [], 0
    for _, grp in itertools.groupby(order, key=lambda i: keys[i]):
        members = list(grp)
        out.append((members, r + 1, r + len(members)))
        r += len(members)
    return out


def _dcg(runs, gains, cutoffs) -> list:
    """DCG@k per cutoff of a group with the tie runs ``runs``: fsum of gain (D[min(b, k)] - D[min(a - 1, k)]) /
    (b - a + 1), every term computed exactly and rounded once."""
    terms = [[] for _ in cutoffs]
    for members, a, b in runs:
        if a > cutoffs[-1]:
            break
        for c, k in enumerate(cutoffs):
            if a > k:
                continue
            cbar = (Fraction(D[min(b, k)]) - Fraction(D[min(a - 1, k)])) / (b - a + 1)
            terms[c] += [float(Fraction(gains[i]) * cbar) for i in members if gains[i] > 0]
    return [math.fsum(t) for t in terms]


def _record(keys, gains, gain_keys, cutoffs) -> list:
    runs = _runs(keys)
    dcg = _dcg(runs, gains, cutoffs)
    idcg = _dcg(_runs(gain_keys), gains, cutoffs)
    hits = [Fraction(0) for _ in cutoffs]
    for members, a, b in runs:
        if a > cutoffs[-1]:
            break
        pos = sum(1 for i in members if gains[i] > 0)
        for c, k in enumerate(cutoffs):
            if pos and a <= k:
                hits[c] += Fraction(pos * (min(b, k) - (a - 1)), b - a + 1)
    rec = [len(keys), sum(1 for v in gains if v > 0)]
    for c in range(len(cutoffs)):
        rec += [dcg[c], idcg[c], hits[c]]
    return rec


def group_record(s, y, cutoffs) -> list:
    """[n, P, then (DCG, IDCG, hits) per cutoff] of one group; DCG and IDCG floats, hits a Fraction."""
    gains = gains_of(y)
    return _record(score_keys(s).tolist(), gains.tolist(), score_keys(gains).tolist(), list(cutoffs))


def group_records(s, y, g, G, cutoffs) -> list:
    """The per-group records of a set: G rows, zeros for empty groups."""
    gains = gains_of(y)
    g = np.asarray(g)
    order = np.argsort(g, kind="stable")
    keys, gkeys, gains = score_keys(s)[order].tolist(), score_keys(gains)[order].tolist(), gains[order].tolist()
    bounds = np.searchsorted(g[order], np.arange(G + 1)).tolist()
    out = []
    for q in range(G):
        lo, hi = bounds[q], bounds[q + 1]
        out.append(_record(keys[lo:hi], gains[lo:hi], gkeys[lo:hi], list(cutoffs)) if hi > lo
                   else [0, 0] + [0.0, 0.0, Fraction(0)] * len(cutoffs))
    return out


def ratios(rec, cutoffs) -> list:
    """[(NDCG, recall, precision)] per cutoff of a ranked group's record, as Fractions."""
    return [(Fraction(rec[2 + 3 * c]) / Fraction(rec[3 + 3 * c]), rec[4 + 3 * c] / rec[1], rec[4 + 3 * c] / k)
            for c, k in enumerate(cutoffs)]


def summary(recs, cutoffs) -> tuple:
    """([(mean NDCG, mean recall, mean precision)] per cutoff or None without a ranked group, ranked groups,
    examples in ranked groups)."""
    ranked = [r for r in recs if r[1] > 0]
    if not ranked:
        return None, 0, 0
    sums = [[Fraction(0)] * 3 for _ in cutoffs]
    for r in ranked:
        for c, t in enumerate(ratios(r, cutoffs)):
            sums[c] = [a + b for a, b in zip(sums[c], t)]
    return [tuple(float(v / len(ranked)) for v in t) for t in sums], len(ranked), sum(r[0] for r in ranked)


def brute_group(s, y, cutoffs) -> list:
    """[(DCG, hits)] per cutoff of one small group, averaged over every ordering that breaks its ties: the plain
    metrics, no tie rule (DCG a float, hits a Fraction)."""
    gains = gains_of(y).tolist()
    runs = [m for m, _, _ in _runs(score_keys(s).tolist())]
    dcg = [[] for _ in cutoffs]
    hits = [Fraction(0) for _ in cutoffs]
    count = 0
    for perm in itertools.product(*[list(itertools.permutations(m)) for m in runs]):
        ranking = [i for part in perm for i in part]
        count += 1
        for c, k in enumerate(cutoffs):
            dcg[c].append(math.fsum(gains[i] / math.log2(j + 2.0) for j, i in enumerate(ranking[:k])))
            hits[c] += sum(1 for i in ranking[:k] if gains[i] > 0)
    return [(math.fsum(d) / count, h / count) for d, h in zip(dcg, hits)]
