"""``fm_topk`` / ``fm_place`` with ``shortlist`` on the CPU (the twins of hip/fm_shortlist.hip) against the fp64 oracles
on each row's listed scores; every sum is exact in fp32, so equality is bit for bit.  The GPU tests share the cases."""

import numpy as np
import pytest
import torch

import place_oracle as PO
import topk_oracle as TO
from fast_tffm_amd.ops import kernels as K

CPU = torch.device("cpu")
KINDS = 13


def short_rows(S, rot, k):
    """A list per row of S, the kinds rotating over the rows from kind ``rot``: 0, 1, 15 / 16 / 17 (a tile), 63 / 64 /
    65 (a step) and k - 1 / k + 1 random entries; the row's unrestricted top k; everything; a fixed-seed random 30%."""
    nq, nc = S.shape
    top = TO.oracle_topk(S, k)[0]
    rng = np.random.default_rng(11)
    pick = lambda n: (lambda q: rng.choice(nc, n, replace=False).tolist())
    kinds = [pick(n) for n in (0, 1, 15, 16, 17, 63, 64, 65, k - 1, k + 1)]
    kinds += [lambda q: top[q].tolist(), lambda q: list(range(nc)), pick(3 * nc // 10)]
    return [kinds[(q + rot) % KINDS](q) for q in range(nq)]


def restrict(S, rows):
    R = np.full_like(S, -np.inf)   # S with every score outside row q's list at -inf
    for q, r in enumerate(rows):
        R[q, r] = S[q, r]
    return R


def topk_cases(Kp, k, nq=17):
    """(inputs, lists, expected idx, expected fp64 score) per rotation -- every kind of list occurs for every nq."""
    inputs = TO.exact_inputs(nq, 3 * TO.slab_of(nq, k) + 5, Kp, seed=Kp + k + nq)
    S = TO.scores64(*inputs)
    for rot in range(-(-KINDS // nq)):
        rows = short_rows(S, rot * nq, k)
        want_i, want_s = TO.oracle_topk(restrict(S, rows), k)
        want_i[np.isneginf(want_s)] = -1
        yield inputs, rows, want_i, want_s


def run_topk(inputs, rows, k, device, **kw):
    sl = K.seen_lists(rows, inputs[2].shape[0], device)
    return tuple(o.cpu().numpy() for o in K.fm_topk(*(x.to(device) for x in inputs), k, shortlist=sl, **kw))


def place_cases(Kp, nq):
    """(inputs, targets, lists, expected counts) per rotation: counts64 on each row's listed scores and its target's."""
    slab = PO.slab_of(nq)
    inputs = TO.exact_inputs(nq, 3 * slab + 5, Kp, seed=Kp + nq)
    S = TO.scores64(*inputs)
    for rot in range(-(-KINDS // nq)):
        tn = PO.targets(nq, S.shape[1], slab, rot, seed=rot).numpy()
        rows = short_rows(S, rot * nq, 10)
        for q in range(0, nq, 3):   # every third ranked context's target is listed (as are those of "everything")
            if tn[q] >= 0 and rows[q]:
                rows[q][0] = int(tn[q])
        want = PO.counts64(restrict(S, [r + [int(t)] * int(t >= 0) for r, t in zip(rows, tn)]), tn)
        yield inputs, torch.from_numpy(tn), rows, want


def run_place(inputs, t, rows, device, **kw):
    sl = K.seen_lists(rows, inputs[2].shape[0], device)
    return K.fm_place(*(x.to(device) for x in inputs), t.to(device), shortlist=sl, **kw).counts().cpu().numpy()


@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("Kp", [4, 64])
def test_topk_twin(Kp, k):
    (inputs, rows, want_i, want_s), = topk_cases(Kp, k)
    idx, score = run_topk(inputs, rows, k, CPU)
    assert np.array_equal(idx, want_i) and np.array_equal(score.astype(np.float64), want_s)
    assert (idx[0] == -1).all() and idx[1, 0] == rows[1][0] and (idx[1, 1:] == -1).all() and idx[8, k - 1] == -1
    plain, none = K.fm_topk(*inputs, k), K.fm_topk(*inputs, k, shortlist=None)
    assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    assert np.array_equal(idx[10:12], plain[0][10:12].numpy())   # (the row's top k; everything)


@pytest.mark.parametrize("Kp", [4, 64])
def test_place_twin(Kp):
    (inputs, t, rows, want), = place_cases(Kp, 17)
    assert np.array_equal(run_place(inputs, t, rows, CPU), want) and t[4] == -1 and tuple(want[4]) == (0, 0)
    assert tuple(want[13]) == (0, 1) and not rows[13]   # (an empty list)
    assert 0 < sum(int(t[q]) in rows[q] for q in range(17)) < 16   # (targets listed and unlisted)
    plain = K.fm_place(*inputs, t).counts()
    assert torch.equal(plain, K.fm_place(*inputs, t, shortlist=None).counts()) and (want[11] == plain[11].numpy()).all()


def test_arguments():
    Q, qb, C, cb = TO.exact_inputs(2, 6, 8, seed=1)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    calls = (lambda **kw: K.fm_topk(Q, qb, C, cb, 3, **kw), lambda **kw: K.fm_place(Q, qb, C, cb, i32([0, -1]), **kw))
    good = K.seen_lists([[1, 2], [0]], 6, CPU)
    for call in calls:
        with pytest.raises(ValueError, match="seen and shortlist"):
            call(seen=good, shortlist=good)
        for o, i in (([0, 2, 3], [3, 1, 0]), ([0, 2, 3], [1, 1, 0]), ([0, 1, 2], [1, 6]), ([0, 1, 2], [-1, 2]),
                     ([1, 1, 2], [1, 2]), ([0, 1, 1], [1, 2]), ([0, 3, 2], [1, 2]), ([0, 2], [1, 2])):  # test_seen's
            with pytest.raises(ValueError, match="shortlist_"):
                call(shortlist=(i32(o), i32(i)))
    assert K.shortlist_plan(100_000, 20_000_000, 1 << 20) == 1 and K.shortlist_plan(1, 10**6, 1 << 20) == 512
    assert K.shortlist_plan(1, 900, 1100) == 4 and K.shortlist_plan(1024, 1_024_000, 1 << 20) == 2
