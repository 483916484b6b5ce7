"""The dedup's grouping and chunk plan (hip/dedup.hip), written plainly in numpy, and the key
generators the CPU and GPU plan tests share.

``plan`` has no kernel-shaped structure -- no tiles, no strips, no scans over tile counts: a stable
argsort, two boolean flag arrays and cumulative sums over the whole array.
"""

from __future__ import annotations

from types import SimpleNamespace

import numpy as np

FIRST = 1 << 30      # hip/fm_common.h kChunkFirst: the chunk starts its segment
SINGLE = 1 << 31     # hip/fm_common.h kChunkSingle: the chunk is its segment's only one
SEG_MASK = FIRST - 1
SMALL_CHUNKS = 16    # hip/fm_bwd.hip kSmallChunks: rows over more chunks go to the workgroup combine


def plan(keys, CH: int, ex_of_occ=None, vals=None) -> SimpleNamespace:
    """Grouping of ``keys`` (non-negative, < 2^31) by value and the backward's chunk list for chunk
    length ``CH``: every segment (run of one key in the stably sorted order) is cut at the sorted
    positions that are multiples of CH."""
    keys = np.asarray(keys, dtype=np.int64)
    n = keys.size
    perm = np.argsort(keys, kind="stable")
    sk = keys[perm]
    pos = np.arange(n)
    head = np.ones(n, dtype=bool)
    head[1:] = sk[1:] != sk[:-1]
    cstart = head | (pos % CH == 0)
    U, C = int(head.sum()), int(cstart.sum())
    seg_of = np.cumsum(head) - 1            # segment of every sorted position
    chunk_of = np.cumsum(cstart) - 1        # chunk of every sorted position
    at = np.flatnonzero(cstart)             # sorted position of every chunk's start
    seg_chunk = np.append(chunk_of[head], C)
    chunks_of_seg = np.diff(seg_chunk)
    cseg = seg_of[at]
    flags = cseg.astype(np.int64) | (head[at].astype(np.int64) * FIRST) | ((chunks_of_seg[cseg] == 1) * SINGLE)
    i32 = np.int32
    p = SimpleNamespace(
        n=n, U=U, C=C, CH=CH,
        skeys=sk.astype(i32), perm=perm.astype(i32),
        uniq=sk[head].astype(i32),
        seg_start=np.append(np.flatnonzero(head), n).astype(i32),
        seg_chunk=seg_chunk.astype(i32),
        chunk_start=np.append(at, n).astype(i32),
        chunk_seg=flags.astype(np.uint32).view(i32),
        chunk_key=sk[at].astype(i32),
        counts=np.array([U, C, 0, 0, 0, 0, 0, 0], dtype=i32),
        inv=None, sorted_ex=None, sorted_x=None)
    inv = np.empty(n, dtype=i32)
    inv[perm] = seg_of
    p.inv = inv
    if ex_of_occ is not None:
        p.sorted_ex = np.asarray(ex_of_occ)[perm].astype(i32)
    if vals is not None:
        p.sorted_x = np.asarray(vals, dtype=np.float32)[perm]
    return p


def chunk_classes(p: SimpleNamespace) -> tuple[int, int, int]:
    """Rows of a plan by the backward path that finishes them: (one chunk: applied by the chunk kernel,
    2..SMALL_CHUNKS chunks: the lane-group combine, more: the workgroup combine)."""
    k = np.diff(p.seg_chunk.astype(np.int64))
    return int((k == 1).sum()), int(((k > 1) & (k <= SMALL_CHUNKS)).sum()), int((k > SMALL_CHUNKS).sum())


# ---------------------------------------------------------------------------
# key generators (int32 numpy arrays; every one takes a seed)
# ---------------------------------------------------------------------------
def distinct(n: int, seed: int = 0) -> np.ndarray:
    """n different keys in shuffled order: every segment is one occurrence, every chunk single."""
    rng = np.random.default_rng(seed)
    return (rng.permutation(n) * 3 + 1).astype(np.int32)


def all_equal(n: int, seed: int = 0) -> np.ndarray:
    """One key n times: a single segment cut into ceil(n / CH) chunks."""
    rng = np.random.default_rng(seed)
    return np.full(n, int(rng.integers(0, 1 << 20)), dtype=np.int32)


def zipf(n: int, V: int, seed: int = 0) -> np.ndarray:
    """Heavy-tailed keys in [0, V): a few hot keys with long runs, many that occur once."""
    rng = np.random.default_rng(seed)
    return ((rng.zipf(1.3, n) - 1) % V).astype(np.int32)


def ladder_lengths(CH: int) -> list[int]:
    c = CH
    return sorted({x for x in (1, 2, 3, 4, 5, c - 1, c, c + 1, 2 * c - 1, 2 * c, 2 * c + 1, 16 * c - 1, 16 * c,
                               16 * c + 1, 17 * c + 1, 40 * c + 3) if x > 0})


def ladder_runs(CH: int, shifts: int) -> list[int]:
    """Run lengths of ``ladder`` in key order: the ladder's lengths ``shifts`` times, repeat s followed
    by s % CH + 1 single-occurrence rows (which move the next repeat's run starts to other residues
    mod CH)."""
    runs: list[int] = []
    for s in range(shifts):
        runs += ladder_lengths(CH)
        runs += [1] * (s % CH + 1)
    return runs


def ladder(CH: int, shifts: int, seed: int = 0) -> np.ndarray:
    """Keys 0..R-1, key r occurring ``ladder_runs(CH, shifts)[r]`` times, in shuffled occurrence order:
    runs of every length around 1, CH, 2 CH and 16 CH (the one-chunk / lane-group / workgroup
    thresholds of the backward), starting at shifting residues mod CH."""
    rng = np.random.default_rng(seed)
    runs = np.asarray(ladder_runs(CH, shifts))
    keys = np.repeat(np.arange(runs.size), runs)
    return keys[rng.permutation(keys.size)].astype(np.int32)
