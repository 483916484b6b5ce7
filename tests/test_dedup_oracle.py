"""The numpy plan oracle (tests/dedup_oracle.py) against an independent per-segment definition, the
ladder generator's shape, and the CPU dedup (csrc/cpu/kernels.cpp) against the oracle.  No GPU."""

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K

import dedup_oracle as O

CHS = [1, 2, 3, 7, 16, 31, 32]
NS = [1, 7, 8, 9, 100, 2047, 2048, 2049, 5000]
RANGES = [1, 3, 50, 10 ** 6]


def _by_segment(keys, CH):
    """The plan by walking every run of the sorted keys: cut it at the multiples of CH, flag the pieces."""
    order = sorted(range(len(keys)), key=lambda i: (int(keys[i]), i))
    sk = [int(keys[i]) for i in order]
    n = len(sk)
    uniq, seg_start, seg_chunk, chunk_start, chunk_seg, chunk_key = [], [], [], [], [], []
    inv = [0] * n
    a = 0
    while a < n:
        b = a
        while b < n and sk[b] == sk[a]:
            b += 1
        u = len(uniq)
        uniq.append(sk[a])
        seg_start.append(a)
        seg_chunk.append(len(chunk_start))
        cuts = [a] + [j for j in range(a + 1, b) if j % CH == 0]
        for i, j in enumerate(cuts):
            chunk_start.append(j)
            chunk_key.append(sk[a])
            word = u | (O.FIRST if i == 0 else 0) | (O.SINGLE if len(cuts) == 1 else 0)
            chunk_seg.append(word - (1 << 32) if word >= 1 << 31 else word)
        for j in range(a, b):
            inv[order[j]] = u
        a = b
    seg_start.append(n)
    seg_chunk.append(len(chunk_start))
    chunk_start.append(n)
    return dict(skeys=sk, perm=order, uniq=uniq, seg_start=seg_start, seg_chunk=seg_chunk, chunk_start=chunk_start,
                chunk_seg=chunk_seg, chunk_key=chunk_key, inv=inv)


@pytest.mark.parametrize("CH", CHS)
def test_oracle_matches_per_segment_definition(CH):
    for n in NS:
        for hi in RANGES:
            keys = np.random.default_rng(n * 31 + hi % 97 + CH).integers(0, hi, n).astype(np.int32)
            p = O.plan(keys, CH)
            ref = _by_segment(keys, CH)
            for name, want in ref.items():
                got = getattr(p, name)
                assert got.dtype == np.int32 and got.tolist() == want, (name, n, hi)
            assert p.counts.tolist() == [len(ref["uniq"]), len(ref["chunk_key"]), 0, 0, 0, 0, 0, 0]
            assert (p.U, p.C) == (len(ref["uniq"]), len(ref["chunk_key"]))
            # no chunk is longer than CH or crosses a CH-aligned position
            cs = p.chunk_start.astype(np.int64)
            assert int(np.diff(cs).max()) <= CH and bool(((cs[1:] - 1) // CH == cs[:-1] // CH).all())


def test_oracle_empty_input():
    p = O.plan(np.zeros(0, np.int32), 7, ex_of_occ=np.zeros(0, np.int32), vals=np.zeros(0, np.float32))
    assert p.U == 0 and p.C == 0 and p.counts.tolist() == [0] * 8
    assert p.seg_start.tolist() == [0] and p.seg_chunk.tolist() == [0] and p.chunk_start.tolist() == [0]
    for name in ("uniq", "chunk_seg", "chunk_key", "skeys", "perm", "inv", "sorted_ex", "sorted_x"):
        assert getattr(p, name).size == 0


def test_oracle_payload_outputs():
    keys = O.zipf(999, 40, seed=2)
    rng = np.random.default_rng(0)
    ex = rng.integers(0, 77, 999).astype(np.int32)
    x = rng.random(999, dtype=np.float32)
    p = O.plan(keys, 7, ex_of_occ=ex, vals=x)
    assert np.array_equal(p.uniq[p.inv], keys)
    assert np.array_equal(p.sorted_ex, ex[p.perm]) and np.array_equal(p.sorted_x, x[p.perm])
    assert np.array_equal(keys[p.perm], p.skeys) and bool((np.diff(p.skeys.astype(np.int64)) >= 0).all())


@pytest.mark.parametrize("CH,n,U,C", [(32, 117_872, 1040, 4691), (7, 5747, None, None)])
def test_ladder_full_shifts_cover_every_residue(CH, n, U, C):
    keys = O.ladder(CH, CH, seed=1)
    p = O.plan(keys, CH)
    assert p.n == n and (U is None or (p.U, p.C) == (U, C))
    lens = np.diff(p.seg_start)
    starts = p.seg_start[:-1]
    # run starts walk through the residues mod CH: all of them over the whole ladder, and (the walk is
    # quadratic in the repeat, so not a permutation) more than half of them for every single run length
    assert set((starts % CH).tolist()) == set(range(CH))
    assert set((p.seg_start[1:][lens > 1] % CH).tolist()) == set(range(CH))  # (and run ends)
    for L in O.ladder_lengths(CH):
        assert len(set((starts[lens == L] % CH).tolist())) > CH // 2, L
    assert min(O.chunk_classes(p)) > 0


@pytest.mark.parametrize("CH,n,classes", [(32, 11_007, (20, 19, 15)), (1, 375, None), (7, 2457, None),
                                          (31, 10_665, None)])
def test_ladder_three_shifts_populate_every_backward_class(CH, n, classes):
    p = O.plan(O.ladder(CH, 3, seed=4), CH)
    assert n is None or p.n == n
    one, small, big = O.chunk_classes(p)
    assert one > 0 and small > 0 and big > 0 and one + small + big == p.U
    assert classes is None or (one, small, big) == classes
    assert p.n <= 11_007


def test_generators_are_seeded():
    for make in (lambda s: O.distinct(100, s), lambda s: O.zipf(100, 1000, s), lambda s: O.ladder(3, 3, s)):
        assert np.array_equal(make(5), make(5)) and not np.array_equal(make(5), make(6))
    assert np.unique(O.distinct(1000, 1)).size == 1000
    assert np.unique(O.all_equal(50, 1)).size == 1
    z = O.zipf(5000, 1 << 20, 3)
    assert z.min() >= 0 and z.max() < 1 << 20 and 1 < np.unique(z).size < 5000


def _cpu_cases():
    yield "empty", np.zeros(0, np.int32)
    yield "one", np.array([5], np.int32)
    yield "extremes", np.array([2 ** 31 - 1, 0, 7, 0, 2 ** 31 - 1, 2 ** 31 - 1], np.int32)
    for n in (7, 2049, 5000):
        yield f"zipf{n}", O.zipf(n, 300, seed=n)
        yield f"distinct{n}", O.distinct(n, seed=n)
        yield f"equal{n}", O.all_equal(n, seed=n)
    yield "ladder7", O.ladder(7, 7, seed=3)
    yield "ladder32", O.ladder(32, 3, seed=3)


@pytest.mark.parametrize("name,keys", list(_cpu_cases()), ids=[c[0] for c in _cpu_cases()])
def test_cpu_dedup_matches_oracle(name, keys):
    n = keys.size
    rng = np.random.default_rng(n)
    ex = rng.integers(0, max(n // 3, 1), n).astype(np.int32)
    x = rng.random(n, dtype=np.float32)
    p = O.plan(keys, 32, ex_of_occ=ex, vals=x)
    ws = K.DedupWorkspace(n + 5, torch.device("cpu"))
    mark = -0x5A5A5A5B
    for t in (ws.skeys, ws.perm, ws.uniq, ws.seg_start, ws.inv, ws.sorted_ex):
        t.fill_(mark)
    ws.sorted_x.fill_(float("nan"))
    dd = K.dedup(torch.from_numpy(keys), ws=ws, key_bits=32, ex_of_occ=torch.from_numpy(ex), vals=torch.from_numpy(x),
                 want_inv=True)
    U = dd.sync()
    assert U == p.U and int(dd.counts[0]) == p.U

    def eq(t, want, tail=True):
        want = torch.from_numpy(want)
        assert torch.equal(t[: want.numel()], want)
        assert not tail or bool((t[want.numel():] == mark).all())  # nothing written past the valid prefix

    eq(dd.skeys, p.skeys)
    eq(dd.perm, p.perm)
    eq(dd.uniq, p.uniq)
    eq(dd.seg_start, p.seg_start)
    eq(dd.inv, p.inv)
    eq(dd.sorted_ex, p.sorted_ex)
    eq(dd.sorted_x, p.sorted_x, tail=False)
    assert bool(torch.isnan(dd.sorted_x[n:]).all())
