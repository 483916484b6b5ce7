"""The dedup's RLE kernels (hip/dedup.hip rle_count_kernel / rle_emit_kernel) against the numpy plan
oracle (tests/dedup_oracle.py), bitwise: segments, the backward's chunk list with its first / single
bits, the counts word and the optional inverse map / sorted example / sorted value outputs, for chunk
lengths 1..32, sizes around the 8-element strips and 2048-element tiles, more tiles than a block has
threads, every payload mode and both sort backends.  Every run starts from poisoned buffers: nothing
past the valid prefix of an output may be written, and the counts word must come back whole."""

import functools

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K

import dedup_oracle as O

pytestmark = pytest.mark.gpu

CHS = [1, 3, 7, 16, 31, 32]
MARK = -0x5A5A5A5B
TILE = 2048
BIG_N = 257 * TILE + 11  # more tiles than rle_emit_kernel's block has threads (256)


def _poison(ws):
    for t in (ws.skeys, ws.perm, ws.uniq, ws.seg_start, ws.seg_chunk, ws.chunk_start, ws.chunk_seg, ws.chunk_key,
              ws.inv, ws.sorted_ex, ws.counts):
        t.fill_(MARK)
    ws.sorted_x.fill_(float("nan"))


def _workspace(n):
    ws = K.DedupWorkspace(n + 37, torch.device("cuda"))  # cap > n: room for a tail to be written into
    _poison(ws)
    return ws


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _eq(got, want, name):
    want = torch.from_numpy(want)
    assert got.dtype == want.dtype, name
    assert torch.equal(got[: want.numel()].cpu(), want), name


def _check_plan(dd, ws, p, tails=True):
    """Every plan field of ``dd`` == the oracle's on its valid prefix; the poison survives behind it."""
    torch.cuda.synchronize()
    assert ws.counts.cpu().tolist() == p.counts.tolist()
    n, U, C = p.n, p.U, p.C
    assert dd.n == n and dd.sync() == U
    for name in ("skeys", "uniq", "seg_start", "seg_chunk", "chunk_start", "chunk_seg", "chunk_key"):
        _eq(getattr(dd, name), getattr(p, name), name)
    if tails:
        for name, k in (("uniq", U), ("seg_start", U + 1), ("seg_chunk", U + 1), ("chunk_start", C + 1),
                        ("chunk_seg", C), ("chunk_key", C), ("skeys", n), ("perm", n)):
            assert bool((getattr(ws, name)[k:] == MARK).all()), name


def _check_occurrence_payload(dd, ws, p, tails=True):
    """``perm`` is the stable sort permutation, ``inv`` the occurrence -> segment map."""
    _eq(dd.perm, p.perm, "perm")
    _eq(dd.inv, p.inv, "inv")
    if tails:
        assert bool((ws.inv[p.n:] == MARK).all())


def _plain(keys, CH, key_bits, ws=None, tails=True):
    """dedup with the occurrence index as payload and the inverse map: all plan fields + perm + inv."""
    p = O.plan(keys, CH)
    ws = ws or _workspace(keys.size)
    dd = K.dedup(_dev(keys), ws=ws, key_bits=key_bits, CH=CH, want_inv=True)
    _check_plan(dd, ws, p, tails)
    _check_occurrence_payload(dd, ws, p, tails)
    assert dd.sorted_ex is None and dd.sorted_x is None
    return p, ws


@functools.lru_cache(maxsize=None)
def _ladder(CH):
    return O.ladder(CH, CH, seed=CH)


@functools.lru_cache(maxsize=None)
def _big_keys():
    return O.zipf(BIG_N, 1 << 20, seed=11)


@pytest.mark.parametrize("CH", CHS)
def test_sizes_around_strips_and_tiles(CH):
    """load8's vector and element paths, strips and tiles that straddle n, the empty plan."""
    for n in (0, 1, 7, 8, 9, TILE - 1, TILE, TILE + 1, 2 * TILE, 5 * TILE + 3):
        p, _ = _plain(O.zipf(n, 1000, seed=n + CH), CH, key_bits=10)
        assert (p.U, p.C) == (0, 0) if n == 0 else p.C >= p.U >= 1


@pytest.mark.parametrize("CH", CHS)
def test_distinct_keys_every_chunk_single(CH):
    for n in (9, TILE + 1, 3 * TILE + 3):
        p, _ = _plain(O.distinct(n, seed=n), CH, key_bits=15)
        assert p.U == p.C == n and bool((p.chunk_seg < 0).all())  # (bit 31: single)


@pytest.mark.parametrize("CH", CHS)
def test_one_key_one_segment(CH):
    for n in (9, TILE + 1, 3 * TILE + 3):
        p, _ = _plain(O.all_equal(n, seed=n), CH, key_bits=20)
        assert p.U == 1 and p.C == -(-n // CH)
        assert bool((p.chunk_seg < 0).any()) == (n <= CH)


@pytest.mark.parametrize("algo", ["fm", "rocprim"])
@pytest.mark.parametrize("CH", CHS)
def test_ladder_every_run_length_at_every_residue(CH, algo):
    """Runs of 1..5, CH-1..CH+1, 2CH-1..2CH+1, 16CH-1..16CH+1, 17CH+1 and 40CH+3 occurrences starting at
    every residue mod CH: a wrong single or first bit at a cut, or a cut next to a tile edge, shows here."""
    keys = _ladder(CH)
    was = K.set_sort_algo(algo)
    try:
        p, _ = _plain(keys, CH, key_bits=max(1, int(keys.max()).bit_length()))
    finally:
        K.set_sort_algo(was)
    one, small, big = O.chunk_classes(p)
    assert one > 0 and small > 0 and big > 0


@pytest.mark.parametrize("CH", [32, 7])
def test_more_tiles_than_threads(CH):
    """258 tiles: rle_emit_kernel's strided sum over the earlier tiles' counts takes a second round."""
    assert BIG_N == 526_347
    p, _ = _plain(_big_keys(), CH, key_bits=20)
    assert min(O.chunk_classes(p)) > 0


def test_workspace_reuse_leaves_no_stale_plan():
    """A 9-element plan in the workspace the 526,347-element one just used, without re-poisoning."""
    _, ws = _plain(_big_keys(), 32, key_bits=20)
    _plain(O.zipf(9, 4, seed=1), 32, key_bits=20, ws=ws, tails=False)
    _plain(np.zeros(0, np.int32), 32, key_bits=20, ws=ws, tails=False)


@pytest.mark.parametrize("CH", [7, 32])
def test_key_range_ends(CH):
    """Keys 0 and 2^31 - 1 (the RLE's out-of-range filler 0xffffffff is no key), full 32 key bits."""
    rng = np.random.default_rng(5)
    keys = rng.choice(np.array([0, 1, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 30, 12345], dtype=np.int32), 3 * TILE + 5)
    _plain(keys, CH, key_bits=32)
    _plain(np.array([2 ** 31 - 1] * 9, dtype=np.int32), CH, key_bits=32)
    _plain(np.array([2 ** 31 - 1, 0] * 5, dtype=np.int32), CH, key_bits=31)


@pytest.mark.parametrize("CH", [7, 32])
def test_smallest_key_bits_the_keys_allow(CH):
    keys = O.zipf(5 * TILE + 3, 1000, seed=9)
    assert int(keys.max()) >= 512
    _plain(keys, CH, key_bits=int(keys.max()).bit_length())
    _plain((keys & 1).astype(np.int32), CH, key_bits=1)


def _payload_inputs():
    n = 5 * TILE + 3
    rng = np.random.default_rng(21)
    keys = O.zipf(n, 3000, seed=21)
    lens = []
    while sum(lens) < n:  # examples of 0..11 features
        lens.append(int(rng.integers(0, 12)))
    lens[-1] -= sum(lens) - n
    lens += [0, 0]
    lens = np.asarray(lens)
    assert int((lens == 0).sum()) > 2 and int(lens.sum()) == n
    offsets = np.zeros(lens.size + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(lens)
    ex = np.repeat(np.arange(lens.size), lens).astype(np.int32)
    slot = (np.arange(n) - offsets[:-1][ex]).astype(np.int32)
    vals = rng.random(n, dtype=np.float32) * 2
    return n, keys, offsets, ex, slot, vals


def test_payload_occurrence_index_with_inverse_examples_and_values():
    n, keys, _, ex, _, vals = _payload_inputs()
    p = O.plan(keys, 7, ex_of_occ=ex, vals=vals)
    ws = _workspace(n)
    dd = K.dedup(_dev(keys), ws=ws, key_bits=12, CH=7, want_inv=True, ex_of_occ=_dev(ex), vals=_dev(vals))
    _check_plan(dd, ws, p)
    _check_occurrence_payload(dd, ws, p)
    assert dd.sorted_ex is ws.sorted_ex and dd.sorted_x is ws.sorted_x
    _eq(dd.sorted_ex, p.sorted_ex, "sorted_ex")
    _eq(dd.sorted_x, p.sorted_x, "sorted_x")
    assert bool((ws.sorted_ex[n:] == MARK).all()) and bool(torch.isnan(ws.sorted_x[n:]).all())


def test_payload_example_index():
    """Neither inverse map nor values: the sort carries the example index, no gather pass."""
    n, keys, _, ex, _, _ = _payload_inputs()
    p = O.plan(keys, 7, ex_of_occ=ex)
    ws = _workspace(n)
    dd = K.dedup(_dev(keys), ws=ws, key_bits=12, CH=7, ex_of_occ=_dev(ex))
    _check_plan(dd, ws, p)
    assert dd.sorted_ex is dd.perm and dd.inv is None and dd.sorted_x is None
    _eq(dd.sorted_ex, p.sorted_ex, "sorted_ex")
    # (the kernel was given no inverse / sorted example / sorted value output: all three stay untouched)
    assert bool((ws.inv == MARK).all()) and bool((ws.sorted_ex == MARK).all()) and bool(torch.isnan(ws.sorted_x).all())


def test_payload_packed_codes():
    """The sort carries example << s | slot; inverse map and values are indexed by the decoded
    occurrence offsets[example] + slot.  Offsets with empty examples."""
    n, keys, offsets, ex, slot, vals = _payload_inputs()
    s = 4
    assert int(slot.max()) < 1 << s
    codes = (ex << s) | slot
    p = O.plan(keys, 7, ex_of_occ=codes, vals=vals)
    ws = _workspace(n)
    d_off = _dev(offsets)
    d_codes = K.csr_rows(d_off, nnz=n, slot_bits=s)
    assert torch.equal(d_codes.cpu(), torch.from_numpy(codes))
    dd = K.dedup(_dev(keys), ws=ws, key_bits=12, CH=7, want_inv=True, ex_of_occ=d_codes, vals=_dev(vals), ex_shift=s,
                 offsets=d_off)
    _check_plan(dd, ws, p)
    assert dd.sorted_ex is dd.perm and dd.ex_shift == s
    _eq(dd.perm, p.sorted_ex, "perm (sorted codes)")
    _eq(dd.inv, p.inv, "inv")
    _eq(dd.sorted_x, p.sorted_x, "sorted_x")
    assert bool((ws.inv[n:] == MARK).all()) and bool(torch.isnan(ws.sorted_x[n:]).all())
    assert bool((ws.sorted_ex == MARK).all())


def test_non_default_stream():
    keys = O.zipf(3 * TILE + 5, 500, seed=3)
    p = O.plan(keys, 7)
    ws = _workspace(keys.size)
    d_keys = _dev(keys)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        dd = K.dedup(d_keys, ws=ws, key_bits=9, CH=7, want_inv=True)
    st.synchronize()
    _check_plan(dd, ws, p)
    _check_occurrence_payload(dd, ws, p)
