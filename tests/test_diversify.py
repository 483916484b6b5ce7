"""``fm_diversify`` (greedy MMR re-ranking of ``fm_topk``'s rows) on the CPU against a plain fp64 greedy loop, on
inputs for which every intermediate is exact in fp32 -- so the comparison needs no tolerance; the argument checks and
``diversify_scale``.  (tests/test_diversify_gpu.py runs the same cases on the GPU.)"""

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K

CPU = torch.device("cpu")
NC = 200
# (M, Kp, n, nq, lam, pad): M at and around the 16-position tiles and the 64-lane halves; Kp of one column group, a cut
# group, the last prefetching width's neighbours and the widest; n = 1, min(10, M), M.  pad: the last row's pool ends
# after n // 2 candidates.  Row 0 of a pool of 4 or more holds one candidate twice (positions 1 and 3).
CASES = [(1, 4, 1, 1, 0.5, False), (15, 20, 10, 3, 0.5, True), (16, 64, 16, 1, 0.0, False), (17, 20, 1, 3, 0.5, False),
         (17, 256, 17, 1, 0.5, True), (33, 4, 10, 3, 0.0, True), (33, 64, 33, 1, 1.0, False),
         (64, 64, 64, 1, 0.5, False), (64, 20, 10, 3, 1.0, True), (128, 64, 10, 3, 0.5, False),
         (128, 256, 128, 1, 0.5, True), (128, 4, 128, 3, 0.0, False)]


def exact_inputs(M, Kp, n, nq, pad, seed=0):
    """Profiles of small integers, scales powers of two, scores multiples of 1/8: sums and products exact in fp32."""
    rng = np.random.default_rng(seed + 1000 * M + Kp)
    C = rng.integers(-3, 4, (NC, Kp)).astype(np.float32)
    inv = (2.0 ** rng.integers(-2, 2, NC)).astype(np.float32)
    pidx = np.stack([rng.permutation(NC)[:M] for _ in range(nq)]).astype(np.int32)
    pscore = -np.sort(-rng.integers(-64, 65, (nq, M)), axis=1).astype(np.float32) / 8   # best first, ties included
    if M >= 4:
        pidx[0, 3] = pidx[0, 1]
    if pad:
        pidx[-1, n // 2:], pscore[-1, n // 2:] = -1, -np.inf
    return C, inv, pidx, pscore


def reference(C, inv, pidx, pscore, n, lam):
    """The definition in fp64, one context at a time; every sim and m is checked to be an fp32 number."""
    nq, M = pidx.shape
    idx, score, mmr = np.full((nq, n), -1, np.int32), np.full((nq, n), -np.inf), np.full((nq, n), -np.inf)
    exact = lambda x: np.array_equal(x.astype(np.float32).astype(np.float64), x)
    for q in range(nq):
        a = np.maximum(pidx[q], 0)
        P = C[a].astype(np.float64)
        sim = ((P @ P.T) * inv[a].astype(np.float64)[:, None]) * inv[a].astype(np.float64)[None, :]
        is_open, pen = pidx[q] >= 0, np.zeros(M)
        assert exact(sim)
        for t in range(min(n, int(is_open.sum()))):
            m = -(1.0 - lam) * pen + lam * np.where(is_open, pscore[q].astype(np.float64), 0.0)
            assert exact(m)
            s = int(np.argmax(np.where(is_open, m, -np.inf)))   # the first of the greatest: the lower position
            idx[q, t], score[q, t], mmr[q, t] = pidx[q, s], pscore[q, s], m[s]
            is_open[s] = False
            pen = sim[:, s] if t == 0 else np.maximum(pen, sim[:, s])
    return idx, score, mmr


def run(inputs, n, lam, dev):
    C, inv, pidx, pscore = (torch.from_numpy(x).to(dev) for x in inputs)
    return tuple(t.cpu().numpy() for t in K.fm_diversify(C, inv, pidx, pscore, n, lam))


def check_case(case, dev):
    M, Kp, n, nq, lam, pad = case
    inputs = exact_inputs(M, Kp, n, nq, pad)
    want, got = reference(*inputs, n, lam), run(inputs, n, lam, dev)
    for name, w, g in zip(("idx", "score", "mmr"), want, got):
        assert np.array_equal(g.astype(w.dtype), w), f"{name}: rows {np.flatnonzero((g != w).any(1))} differ"
    if lam == 1.0:
        assert np.array_equal(got[0], inputs[2][:, :n]) and np.array_equal(got[1], inputs[3][:, :n])
    if pad:
        assert (got[0][-1, n // 2:] == -1).all() and (got[0][-1, :n // 2] >= 0).all()
    return inputs, got


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-Kp%d-n%d-nq%d-lam%s-pad%d" % c)
def test_against_fp64_greedy(case):
    check_case(case, CPU)


def check_tie(dev):
    # lam = 0: m is -pen alone.  Positions 1 and 3 hold one candidate, so their sim and m tie at every step, and only
    # the score written tells them apart: position 1's comes first.  At t = 0 every m is +-0: position 0 is picked.
    C, inv, pidx, pscore = exact_inputs(16, 20, 16, 1, False)
    pscore[0] = -np.arange(16, dtype=np.float32) / 8
    idx, score, _ = run((C, inv, pidx, pscore), 16, 0.0, dev)
    twice = np.flatnonzero(idx[0] == pidx[0, 1])
    assert idx[0, 0] == pidx[0, 0] and len(twice) == 2 and score[0, twice].tolist() == [pscore[0, 1], pscore[0, 3]]


def test_twice_listed_candidate_ties_to_the_lower_position():
    check_tie(CPU)


def test_arguments_and_scale():
    C, inv, pidx, pscore = (torch.from_numpy(x) for x in exact_inputs(16, 8, 4, 2, False))
    for bad in (dict(n=17), dict(n=0), dict(lam=1.5), dict(lam=-0.1)):
        with pytest.raises(ValueError, match="fm_diversify"):
            K.fm_diversify(C, inv, pidx, pscore, **{"n": 4, "lam": 0.5, **bad})
    wide = torch.zeros((2, 129), dtype=torch.int32)
    with pytest.raises(ValueError, match="1..128"):
        K.fm_diversify(C, inv, wide, wide.float(), 4, 0.5)
    with pytest.raises(ValueError, match="c_inv"):
        K.fm_diversify(C, inv[:-1], pidx, pscore, 4, 0.5)
    C[5] = 0
    cos, dot = K.diversify_scale(C), K.diversify_scale(C, "dot")
    norm = np.sqrt((C.numpy().astype(np.float64) ** 2).sum(1))
    assert cos[5] == 0 and np.allclose(np.delete(cos.numpy() * norm, 5), 1.0, rtol=1e-6) and bool((dot == 1).all())
