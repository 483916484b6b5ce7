"""The case list of the ranking-metric tests (CPU twin and GPU chain against tests/rank_oracle.py), built once per
process: name -> (scores, labels, group ids, G, cutoffs, oracle records).  The shapes are the ones at which the
segmented chain can go wrong: a tile is 2048 sorted positions, a thread owns 8, a wave 512."""

import functools

import numpy as np

import rank_oracle as R

TILE = 2048
NAMES = ["one", "tile-2047", "tile-2048", "tile-2049", "all-equal", "tiny-groups", "same-scores", "empty-unranked",
         "graded", "signed", "special", "zipf"]


def _one_group_top_run(n, rng):
    """One group of n examples whose five highest scores are equal: in the sorted order that run ends at
    position n - 1, so with n = 2049 it straddles the first tile boundary."""
    s = rng.integers(0, 50, n).astype(np.float32)
    s[rng.choice(n, min(5, n), replace=False)] = 99.0
    y = (rng.random(n) < 0.3).astype(np.float32)
    y[np.argmax(s)] = 1.0
    return s, y, np.zeros(n, np.int32), 1, (1, 3, 10)


def _sizes_case(sizes, levels, rng, cutoffs, p=0.3):
    g = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
    n = g.size
    perm = rng.permutation(n)
    s = rng.integers(0, levels, n).astype(np.float32)
    y = (rng.random(n) < p).astype(np.float32)
    return s[perm], y[perm], g[perm], len(sizes), cutoffs


def zipf_sizes(n, rng):
    """Group sizes summing to n: one group of tens of thousands, a Zipf tail, thousands of singletons."""
    sizes = [n // 4]
    left = n - sizes[0] - 4000
    while left > 0:
        sizes.append(int(min(left, rng.zipf(1.3))))
        left -= sizes[-1]
    return sizes + [1] * 4000


def _build(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one":
        return np.array([0.25], np.float32), np.array([1.0], np.float32), np.zeros(1, np.int32), 1, (1, 10)
    if name.startswith("tile-"):
        return _one_group_top_run(int(name.split("-")[1]), rng)
    if name == "all-equal":  # every example gets D[k] / n; the run spans four tiles
        n = 3 * TILE + 17
        return (np.full(n, 0.5, np.float32), (rng.random(n) < 0.4).astype(np.float32), np.zeros(n, np.int32), 1,
                (1, 10, 4096))
    if name == "tiny-groups":  # several groups per wave, cutoffs larger than the groups
        return _sizes_case(rng.integers(1, 6, 1700).tolist(), 3, rng, (1, 5, 10, 100), p=0.5)
    if name == "same-scores":  # adjacent group ids hold the same score values: runs must not join
        sizes = rng.integers(3, 60, 40).tolist() + [TILE - 7, 30, TILE + 9]
        return _sizes_case(sizes, 2, rng, (1, 4, 20))
    if name == "empty-unranked":  # empty groups, groups without a positive, an all-positive group
        s, y, g, G, ks = _sizes_case(rng.integers(1, 40, 60).tolist(), 6, rng, (2, 7))
        g = g * 3 + 1  # ids 1, 4, 7, ...: two of three groups are empty, and so are the last ones
        y[(g // 3) % 4 == 0] = 0.0
        y[g == 7] = 1.0
        return s, y, g.astype(np.int32), 3 * G + 5, ks
    if name in ("graded", "signed"):
        s, y, g, G, ks = _sizes_case(rng.integers(1, 300, 50).tolist(), 9, rng, (1, 5, 10))
        levels = np.array([0, 0.5, 1, 3] if name == "graded" else [-1, 1, -1, 1], np.float32)
        return s, levels[rng.integers(0, 4, s.size)], g, G, ks
    if name == "special":  # -0.0 / +0.0, +-inf, denormals
        vals = np.array([-0.0, 0.0, np.inf, -np.inf, 1e-45, -1e-45, 1e-40, 1.0, -1.0], np.float32)
        s, y, g, G, ks = _sizes_case(rng.integers(1, 50, 80).tolist(), 2, rng, (1, 3, 10))
        return vals[rng.integers(0, vals.size, s.size)], y, g, G, ks
    if name == "zipf":
        n = 1 << 17
        s, y, g, G, ks = _sizes_case(zipf_sizes(n, rng), 16, rng, (1, 5, 10, 100), p=0.2)
        assert s.size == n
        return s, y, g, G, ks
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    s, y, g, G, ks = _build(name)
    return s, y, g, G, ks, R.group_records(s, y, g, G, ks)


def with_nan(name="special"):
    """The case with one NaN score (the oracle orders it by its bit pattern, as the score sort does)."""
    s, y, g, G, ks, _ = case(name)
    s = s.copy()
    s[s.size // 2] = np.nan
    return s, y, g, G, ks


def bound_m(recs) -> tuple:
    """(m of the per-group bound, m of the means' bound): the case's largest group size; the larger of that and
    its number of ranked groups."""
    big = max(r[0] for r in recs)
    return big, max(big, sum(1 for r in recs if r[1] > 0))


def check(st, recs, n, G, ks):
    """``st`` (a RankStats) against the oracle records: n_g, P_g and the counts exactly, every per-group value
    within (m + 8) 2^-52 relative with m the largest group size, every mean within the same with m the larger of
    that and the number of ranked groups."""
    eps = 2.0 ** -52
    m_group, m_mean = bound_m(recs)
    got = st.per_group().cpu().numpy()
    assert got.shape == (G, 2 + 3 * len(ks)) and got.dtype == np.float64
    want = np.array([[float(v) for v in r] for r in recs], np.float64).reshape(got.shape)
    assert (got[:, :2] == want[:, :2]).all()
    err = np.abs(got - want)
    print("largest per-group relative error / 2^-52:", float((err / np.maximum(want, 1e-300)).max() / eps),
          "bound", m_group + 8)
    assert (err <= (m_group + 8) * eps * want).all()
    means, ranked, covered = R.summary(recs, ks)
    assert st.ranked_groups() == ranked
    assert st.coverage() == covered / n
    for c, k in enumerate(ks):
        for which, fn in enumerate((st.ndcg, st.recall, st.precision)):
            v = fn(k)
            if not ranked:
                assert np.isnan(v)
                continue
            w = means[c][which]
            print(f"{fn.__name__}@{k}", v, "oracle", w, "relative error / 2^-52:", abs(v - w) / w / eps, "bound",
                  m_mean + 8)
            assert abs(v - w) <= (m_mean + 8) * eps * w
