"""The pairwise ranking loss on the GPU (hip/group_pair.hip through ops/kernels.py ``group_pairwise_loss``) against the
fp64 oracle of tests/group_pair_oracle.py, within its derived bound (fp64 arithmetic rounded to fp32 once): the case
list of tests/group_loss_cases.py; a short list of cases placed by the kernel's geometry; key widths 1 and 27; the
exact zeros; bitwise repeatability -- two calls, a workspace filled with 0xFF and last used by a larger call, a
captured graph replayed on new inputs; and one plan feeding both group losses."""

import zlib

import numpy as np
import pytest
import torch

import group_loss_cases as C
import group_loss_oracle as SO
import group_pair_oracle as O
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

ROWS, CHUNK, SLABS = 1024, 128, 16   # hip/group_pair.hip: kGlTile, kGpChunk, kGpSlabs


def _t(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda")


def run(g, s, y, w, gs, key_bits=None, ws=None, pws=None):
    plan = K.group_plan(_t(g, np.int32), C.bits_for_ids(g) if key_bits is None else key_bits, ws=ws)
    d, loss = K.group_pairwise_loss(plan, _t(s), _t(y), _t(w), gs, ws=pws)
    return d.cpu().numpy(), loss.cpu().numpy()


def test_geometry():
    assert K.group_pair_geometry() == (ROWS, CHUNK, SLABS)
    assert ROWS == C.TILE == K.group_loss_tile()


@pytest.mark.parametrize("n,grouping", C.CASES)
def test_gpu_equals_oracle(n, grouping):
    for values in C.VALUES:
        g, s, y, w, gs = C.case(n, grouping, values)
        d, loss = run(g, s, y, w, gs)
        O.check(d, float(loss), g, s, y, w, gs, what=f"{n}/{grouping}/{values}")
        if grouping in ("all_excluded", "singletons"):
            assert not d.any() and float(loss) == 0.0
    K.check_device_errors()


def _runs(*sizes):
    """Group ids in sorted order: run k has sizes[k] positions."""
    return np.repeat(np.arange(len(sizes)), sizes)


def _tail(kind, n, first_id):
    j = np.arange(n)
    return first_id + (j if kind == "singletons" else j // (2 if kind == "pairs" else 3))


GEOMETRY_CASES = ("chunk_boundary", "two_slabs", "three_tiles_two_chunks_per_slab", "two_groups_one_tile",
                  "positives_in_last_tile")


def geometry_case(name):
    """Cases placed by (ROWS, CHUNK, SLABS); positions are those of the sorted order, the examples are shuffled.

    chunk_boundary: [0, 3) | [3, CHUNK) ends exactly where column chunk 0 ends | [CHUNK, CHUNK + 72) begins chunk 1
        | pairs: a row's walk stops at the chunk's last column, the next group's starts at a chunk's first.
    two_slabs: singletons | [100, 200) | pairs: the span of the one row tile has 3 chunks, one per slab, and the
        group's columns lie in chunks 0 and 1: every row of it adds two slab partials.
    three_tiles_two_chunks_per_slab: two singletons | [2, 2 ROWS + 300) | triples: the group touches row tiles 0, 1
        and 2, whose spans each hold its 19 column chunks -- more than SLABS, so a slab walks two chunks and the
        last slabs are empty; the tiles' partials of P and N go through the carry.
    two_groups_one_tile: [0, 10) | [10, 400) | [400, 900) | pairs: two medium groups in row tile 0, whose span
        holds both; a slab in the middle (chunk 3) serves the rows of both with different ranges.
    positives_in_last_tile: [0, 5) | [5, 2 ROWS + 300) with positives only at sorted positions >= 2 ROWS: the rows
        of tiles 0 and 1 are all negatives whose only columns sit in the last slabs; P comes from the last tile
        alone through the carry."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pos_from = None
    if name == "chunk_boundary":
        g = np.concatenate([_runs(3, CHUNK - 3, 72), _tail("pairs", 58, 3)])
    elif name == "two_slabs":
        g = np.concatenate([_tail("singletons", 100, 0), np.full(100, 100), _tail("pairs", 101, 101)])
    elif name == "three_tiles_two_chunks_per_slab":
        g = np.concatenate([_runs(1, 1, 2 * ROWS + 298), _tail("triples", 97, 3)])
    elif name == "two_groups_one_tile":
        g = np.concatenate([_runs(10, 390, 500), _tail("pairs", 101, 3)])
    elif name == "positives_in_last_tile":
        g = np.concatenate([_runs(5, 2 * ROWS + 295), _tail("pairs", 11, 2)])
        pos_from = 2 * ROWS
    else:
        raise KeyError(name)
    n = g.size
    s = rng.normal(0.0, 3.0, n)
    y = (rng.random(n) < 0.3).astype(np.float64)
    if pos_from is not None:
        y = np.where((g == 1) & (np.arange(n) < pos_from), 0.0, y)
        assert y[(g == 1) & (np.arange(n) >= pos_from)].sum() > 0
    w = rng.uniform(0.25, 3.0, n)
    w[rng.random(n) < 0.1] = 0.0
    # the plan's sort is stable, so sorted position k of a group is its k-th member of the batch: interleave the
    # groups at random, every group's members in their order (the labels above are placed by sorted position)
    slot_group = g[rng.permutation(n)]
    perm = np.empty(n, dtype=np.int64)
    perm[np.argsort(slot_group, kind="stable")] = np.arange(n)
    f32 = lambda a: np.ascontiguousarray(a[perm], dtype=np.float32)  # noqa: E731
    return np.ascontiguousarray(g[perm], dtype=np.int32), f32(s), f32(y), f32(w), 1.0 / n


@pytest.mark.parametrize("name", GEOMETRY_CASES)
def test_geometry_cases(name):
    g, s, y, w, gs = geometry_case(name)
    if name == "positives_in_last_tile":   # the placement the case is about
        sidx = K.group_plan(_t(g, np.int32), C.bits_for_ids(g)).sidx.cpu().numpy()
        ys, big = y[sidx], np.nonzero(g[sidx] == 1)[0]
        assert big[0] == 5 and not ys[big[big < 2 * ROWS]].any() and ys[big[big >= 2 * ROWS]].any()
    d, loss = run(g, s, y, w, gs)
    O.check(d, float(loss), g, s, y, w, gs, what=name)
    assert float(loss) > 0
    K.check_device_errors()


@pytest.mark.parametrize("key_bits", [1, 27])
def test_key_widths(key_bits):
    g, s, y, w, gs = C.key_width_case(key_bits)
    d, loss = run(g, s, y, w, gs, key_bits=key_bits)
    O.check(d, float(loss), g, s, y, w, gs, what=f"key_bits {key_bits}")
    K.check_device_errors()


def test_exact_zeros():
    """Excluded examples, singletons, a group without a positive, one without a negative and the zero-weight
    members of a valid group get exactly 0, whatever their scores hold; the valid group's result is the oracle's."""
    g, s, y, w, live = O.exact_zeros_case()
    d, loss = run(g, s, y, w, 0.5, key_bits=4)
    rest = np.setdiff1d(np.arange(g.size), live)
    assert (d[rest] == 0.0).all() and np.isfinite(d).all() and (d[live] != 0.0).all()
    O.check(d, float(loss), g, s, y, w, 0.5, what="exact zeros")
    d2, _ = run(g, s, y, None, 1.0, key_bits=4)
    assert (d2[g != 4] == 0.0).all()
    K.check_device_errors()


def test_repeatable_and_workspace_reuse():
    big = C.case(3 * C.TILE + 5, "zipf", "weights")
    small = C.case(C.TILE + 1, "excluded_scattered", "graded_labels")
    first = run(*small)
    again = run(*small)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    dev = torch.device("cuda")
    ws = K.group_loss_workspace(len(big[0]), dev)
    pws = K.group_pair_workspace(len(big[0]), dev)
    ws.fill_(0xFF)
    pws.fill_(0xFF)
    reused = run(*small, pws=pws)   # the pair workspace straight after the fill
    assert first[0].tobytes() == reused[0].tobytes() and first[1].tobytes() == reused[1].tobytes()
    run(*big, ws=ws, pws=pws)
    reused = run(*small, ws=ws, pws=pws)
    assert first[0].tobytes() == reused[0].tobytes() and first[1].tobytes() == reused[1].tobytes()
    O.check(reused[0], float(reused[1]), *small[:4], small[4], what="reused workspace")


def test_graph_replay_equals_eager():
    n = 3 * C.TILE + 5
    a = C.case(n, "zipf", "weights")
    b = C.case(n, "excluded_scattered", "weights")
    dev = torch.device("cuda")
    g, s, y, w = _t(a[0], np.int32), _t(a[1]), _t(a[2]), _t(a[3])
    ws = K.group_loss_workspace(n, dev)
    pws = K.group_pair_workspace(n, dev)
    dpred = torch.empty(n, dtype=torch.float32, device=dev)
    # eager once: the sort's self-check
    K.group_pairwise_loss(K.group_plan(g, 10, ws=ws), s, y, w, a[4], dpred=dpred, ws=pws)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, loss = K.group_pairwise_loss(K.group_plan(g, 10, ws=ws), s, y, w, a[4], dpred=dpred, ws=pws)
    for t, src, dt in ((g, b[0], np.int32), (s, b[1], np.float32), (y, b[2], np.float32), (w, b[3], np.float32)):
        t.copy_(_t(src, dt))
    graph.replay()
    torch.cuda.synchronize()
    got = dpred.cpu().numpy(), loss.cpu().numpy()
    del graph
    want = run(*b[:4], a[4], key_bits=10)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    O.check(got[0], float(got[1]), b[0], b[1], b[2], b[3], a[4], what="graph replay")
    K.check_device_errors()


@pytest.mark.parametrize("pair_first", [False, True])
def test_one_plan_feeds_both_losses(pair_first):
    g, s, y, w, gs = C.case(3 * C.TILE + 5, "zipf", "weights")
    plan = K.group_plan(_t(g, np.int32), C.bits_for_ids(g))
    before = [x.clone() for x in (plan.sidx, plan.first, plan.end)]
    ts, ty, tw = _t(s), _t(y), _t(w)
    if pair_first:
        dp, lp = K.group_pairwise_loss(plan, ts, ty, tw, gs)
        dsm, lsm = K.group_softmax_loss(plan, ts, ty, tw, gs)
    else:
        dsm, lsm = K.group_softmax_loss(plan, ts, ty, tw, gs)
        dp, lp = K.group_pairwise_loss(plan, ts, ty, tw, gs)
    torch.cuda.synchronize()
    for x, z in zip(before, (plan.sidx, plan.first, plan.end)):
        assert torch.equal(x, z)
    O.check(dp.cpu().numpy(), float(lp), g, s, y, w, gs, what="pairwise on a shared plan")
    SO.check(dsm.cpu().numpy(), float(lsm), g, s, y, w, gs, what="softmax on a shared plan")
    K.check_device_errors()
