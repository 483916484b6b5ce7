"""The case list of the listwise-loss tests (CPU twin and GPU op, against tests/group_loss_oracle.py).

Sizes: 1, 2, 63, 64, 65 (around a wave), TILE - 1, TILE, TILE + 1 (the GPU op's tile of sorted positions) and
3 TILE + 5.  Groupings at every size: all singletons; one group; pairs; a group that ends exactly on a tile
boundary of the sorted order; one group over three tiles between singletons; Zipf sizes; excluded examples
scattered through the batch; everything excluded; groups without a positive; groups of equal scores.  Every
(size, grouping) runs with three value sets: scores spread over +-80 with binary labels; graded and negative
labels; example weights with zeros among them.  Example order is shuffled: the sort has work to do.
"""

from __future__ import annotations

import zlib

import numpy as np

TILE = 1024  # hip/group_loss.hip kGlTile (tests/test_group_loss_gpu.py asserts it)
SIZES = (1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
GROUPINGS = ("singletons", "one_group", "pairs", "tile_boundary", "span_three_tiles", "zipf", "excluded_scattered",
             "all_excluded", "no_positive", "equal_scores")
VALUES = ("wide_scores", "graded_labels", "weights")
CASES = [(n, g) for n in SIZES for g in GROUPINGS]


def bits_for_ids(ids) -> int:
    """key_bits that leave every id below the sort's all-ones key."""
    top = int(max(int(np.max(ids)), 0)) + 2
    return max(1, int(np.ceil(np.log2(top))))


def _sorted_groups(n: int, grouping: str, rng) -> np.ndarray:
    """Group ids in sorted (ascending) order."""
    j = np.arange(n)
    if grouping == "singletons":
        return j
    if grouping == "one_group":
        return np.zeros(n, dtype=np.int64)
    if grouping == "pairs":
        return j // 2
    if grouping == "tile_boundary":  # [0, 5) | [5, TILE) ends on the boundary | pairs
        return np.where(j < 5, 0, np.where(j < TILE, 1, 2 + (j - TILE) // 2))
    if grouping == "span_three_tiles":  # two singletons, one group to n - 3, three singletons
        return np.where(j < 2, j, np.where(j < n - 3, 2, 3 + j - (n - 3)))
    if grouping in ("zipf", "excluded_scattered"):
        return np.sort(rng.zipf(1.3, n) % 997)
    if grouping == "all_excluded":
        return np.full(n, -1, dtype=np.int64)
    if grouping == "no_positive":
        return j // 4
    if grouping == "equal_scores":
        return j // 5
    raise KeyError(grouping)


def case(n: int, grouping: str, values: str):
    """(ids int32 [n], scores, labels, weights or None (fp32), grad_scale)."""
    rng = np.random.default_rng(zlib.crc32(f"{n}/{grouping}/{values}".encode()))
    g = _sorted_groups(n, grouping, rng).astype(np.int64)
    if grouping == "excluded_scattered":
        g = np.where(rng.random(n) < 0.2, -1, g)
    if values == "wide_scores":
        s = rng.uniform(-80.0, 80.0, n)
        y = (rng.random(n) < 0.3).astype(np.float64)
        w = None
    elif values == "graded_labels":
        s = rng.normal(0.0, 2.0, n)
        y = rng.integers(-1, 4, n).astype(np.float64)  # -1 (a negative in the -1 / +1 convention), 0, grades 1..3
        w = None
    else:
        s = rng.normal(0.0, 1.0, n)
        y = (rng.random(n) < 0.4).astype(np.float64)
        w = rng.uniform(0.25, 3.0, n)
        w[rng.random(n) < 0.2] = 0.0
    if grouping == "no_positive":
        y = np.where((g % 3) == 0, np.minimum(y, 0.0), y)   # every third group has no positive
    if grouping == "equal_scores":
        s = np.where((g % 2) == 0, np.float32(0.75) + (g % 7), s)  # every other group: one score for all
    perm = rng.permutation(n)
    f32 = lambda a: None if a is None else np.ascontiguousarray(a[perm], dtype=np.float32)  # noqa: E731
    return np.ascontiguousarray(g[perm], dtype=np.int32), f32(s), f32(y), f32(w), 1.0 / n


def key_width_case(key_bits: int, n: int = 3 * TILE + 5):
    """Ids at 0, at the largest id ``2^key_bits - 2`` and in between (key_bits 1: id 0 alone), some excluded."""
    rng = np.random.default_rng(key_bits)
    top = (1 << key_bits) - 2
    pool = np.unique(np.concatenate([[0, top], rng.integers(0, top + 1, 40)]))
    g = rng.choice(pool, n)
    g = np.where(rng.random(n) < 0.1, -1, g)
    g[:4] = [0, top, top, 0]
    s = rng.normal(0.0, 3.0, n).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    return g.astype(np.int32), s, y, None, 0.5
