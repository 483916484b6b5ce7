"""Recommend and place with every context's already-seen candidates left out, on the CPU: ``fm_topk`` / ``fm_place``
with ``seen`` (cpu/kernels.cpp, the twins of hip/fm_seen.hip) against the fp64 oracles with the seen columns removed,
on inputs whose every sum is exact in fp32: equality is bit for bit.  tests/test_seen_gpu.py shares the cases."""

import numpy as np
import pytest
import torch

import place_oracle as PO
import topk_oracle as TO
from fast_tffm_amd.ops import kernels as K

CPU = torch.device("cpu")


def seen_rows(S, slab, rot, k=10):
    """A list per row of S, the kinds rotating over the rows (from kind ``rot``): empty; the row's unfiltered top
    k; both sides of a slab cut and both ends; all but 3 candidates; everything; a fixed-seed random 30%."""
    nq, nc = S.shape
    top = TO.oracle_topk(S, k)[0]
    rng = np.random.default_rng(7)
    kinds = [lambda q: [],
             lambda q: top[q].tolist(),
             lambda q: [0, slab - 1, slab, nc - 1],
             lambda q: sorted(set(range(nc)) - {3, slab + 1, nc - 2}),
             lambda q: list(range(nc)),
             lambda q: np.flatnonzero(rng.random(nc) < 0.3).tolist()]
    return [kinds[(q + rot) % len(kinds)](q) for q in range(nq)]


def topk_case(Kp, k, nq=17):
    """(inputs, lists, expected idx, expected fp64 score): the oracle on the scores with row q's list at -inf."""
    slab = TO.slab_of(nq, k)
    inputs = TO.exact_inputs(nq, 3 * slab + 5, Kp, seed=Kp + k)
    S = TO.scores64(*inputs)
    rows = seen_rows(S, slab, 0, k)
    for q, r in enumerate(rows):
        S[q, r] = -np.inf
    want_i, want_s = TO.oracle_topk(S, k)
    want_i[np.isneginf(want_s)] = -1
    return inputs, rows, want_i, want_s


def run_topk(inputs, rows, k, device, **kw):
    seen = K.seen_lists(rows, inputs[2].shape[0], device)
    return tuple(o.cpu().numpy() for o in K.fm_topk(*(x.to(device) for x in inputs), k, seen=seen, **kw))


def place_cases(Kp, nq):
    """(inputs, targets, lists, expected counts) per rotation -- every kind of list occurs for every nq: counts64
    on each row's scores with its seen columns other than the target deleted."""
    slab = PO.slab_of(nq)
    inputs = TO.exact_inputs(nq, 3 * slab + 5, Kp, seed=Kp + nq)
    S = TO.scores64(*inputs)
    for rot in range(-(-6 // nq)):
        t = PO.targets(nq, S.shape[1], slab, rot, seed=rot)
        tn = t.numpy()
        rows = seen_rows(S, slab, rot * nq)
        want = np.zeros((nq, 2), dtype=np.int32)
        for q, r in enumerate(rows):
            keep = np.ones(S.shape[1], dtype=bool)
            keep[r] = False
            if tn[q] >= 0:
                keep[tn[q]] = True
                want[q] = PO.counts64(S[q:q + 1, keep], np.array([keep[:tn[q]].sum()]))[0]
        yield inputs, t, rows, want


def run_place(inputs, t, rows, device, **kw):
    seen = K.seen_lists(rows, inputs[2].shape[0], device)
    return K.fm_place(*(x.to(device) for x in inputs), t.to(device), seen=seen, **kw).counts().cpu().numpy()


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("Kp", [4, 64])
def test_topk_twin(Kp, k):
    inputs, rows, want_i, want_s = topk_case(Kp, k)
    idx, score = run_topk(inputs, rows, k, CPU)
    assert np.array_equal(idx, want_i) and np.array_equal(score.astype(np.float64), want_s)
    assert (idx[4] == -1).all() and (idx[3, :3] >= 0).all() and (idx[3, 3:] == -1).all()
    plain = K.fm_topk(*inputs, k)
    none = K.fm_topk(*inputs, k, seen=K.seen_lists([[]] * 17, inputs[2].shape[0], CPU))
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])


@pytest.mark.parametrize("Kp", [4, 64])
def test_place_twin(Kp):
    for inputs, t, rows, want in place_cases(Kp, 17):
        assert np.array_equal(run_place(inputs, t, rows, CPU), want)
        assert tuple(want[10]) == (0, 1) and t[4] == -1 and rows[4] and int(t[2]) in rows[2]
        none = K.seen_lists([[]] * 17, inputs[2].shape[0], CPU)
        assert torch.equal(K.fm_place(*inputs, t).counts(), K.fm_place(*inputs, t, seen=none).counts())


def test_seen_lists_and_arguments():
    off, idx = K.seen_lists([[5, 1, 5, 3], [], (2,)], 6, CPU)
    assert off.dtype == idx.dtype == torch.int32
    assert off.tolist() == [0, 3, 3, 4] and idx.tolist() == [1, 3, 5, 2]
    for bad in ([[0], [6]], [[0], [2, -1]]):
        with pytest.raises(ValueError, match="context 1"):
            K.seen_lists(bad, 6, CPU)
    Q, qb, C, cb = TO.exact_inputs(2, 6, 8, seed=1)
    t = torch.tensor([0, -1], dtype=torch.int32)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    # not ascending, a duplicate, out of range (twice); offsets not from 0, not to nnz, decreasing, too few
    for o, i in (([0, 2, 3], [3, 1, 0]), ([0, 2, 3], [1, 1, 0]), ([0, 1, 2], [1, 6]), ([0, 1, 2], [-1, 2]),
                 ([1, 1, 2], [1, 2]), ([0, 1, 1], [1, 2]), ([0, 3, 2], [1, 2]), ([0, 2], [1, 2])):
        for call in (lambda s: K.fm_topk(Q, qb, C, cb, 3, seen=s), lambda s: K.fm_place(Q, qb, C, cb, t, seen=s)):
            with pytest.raises(ValueError, match="seen"):
                call((i32(o), i32(i)))
    K.fm_topk(Q, qb, C, cb, 3, seen=(i32([0, 2, 3]), i32([4, 5, 0])))   # (a new context may start lower)
