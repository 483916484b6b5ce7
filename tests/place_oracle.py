"""Shared cases and fp64 references of the place tests (tests/test_place.py on the CPU, tests/test_place_gpu.py
on the GPU): the held-out candidate's (greater, equal) among all candidates, and the metrics they imply."""

import math
from fractions import Fraction

import numpy as np
import torch

from fast_tffm_amd.ops import kernels as K
from topk_oracle import exact_inputs, scores64

EXACT_KPS = [4, 12, 64, 100, 256]   # one group, a group cut short, the last prefetching width, no prefetch, the maximum
EXACT_NQS = [1, 17, 65]             # a partial tile, idle waves, a second query block
CUTOFFS = (1, 10, 4096)


def slab_of(nq: int) -> int:
    """The slab length of a small call (every nc up to 4 slabs): from the kernel's own plan."""
    slab, parts = K.place_plan(nq, 500)
    assert parts == -(-500 // slab)
    return slab


def targets(nq: int, nc: int, slab: int, rot: int, seed: int) -> torch.Tensor:
    """Candidate 0, the last one, a slab's last row, the next slab's first row and one -1 (those that exist), the
    rest random; ``rot`` chooses which of them a call of fewer queries than that holds."""
    special = [t for t in (0, nc - 1, slab - 1, slab, -1) if t < nc]
    t = torch.randint(0, nc, (nq,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    part = special[rot * nq:(rot + 1) * nq]
    t[:len(part)] = torch.tensor(part, dtype=torch.int32)
    return t


def counts64(S: np.ndarray, t: np.ndarray) -> np.ndarray:
    out = np.zeros((S.shape[0], 2), dtype=np.int32)
    for q in np.flatnonzero(t >= 0):
        out[q] = ((S[q] > S[q, t[q]]).sum(), (S[q] == S[q, t[q]]).sum())
    return out


def check_exact(Kp: int, nq: int, device):
    """counts == the fp64 reference on profiles whose every sum is exact in fp32 (plenty of ties)."""
    slab = slab_of(nq)
    for nc in (1, 33, slab + 1, 3 * slab + 5):
        assert K.place_plan(nq, nc) == (slab, -(-nc // slab))
        Q, qb, C, cb = exact_inputs(nq, nc, Kp, seed=Kp + nq + nc)
        S = scores64(Q, qb, C, cb)
        for rot in range(-(-5 // nq)):
            t = targets(nq, nc, slab, rot, seed=nc + rot)
            ps = K.fm_place(Q.to(device), qb.to(device), C.to(device), cb.to(device), t.to(device), CUTOFFS)
            got = ps.counts().cpu().numpy()
            want = counts64(S, t.numpy())
            wrong = np.flatnonzero((got != want).any(1))
            assert wrong.size == 0, f"Kp={Kp} nq={nq} nc={nc} rot={rot}: rows {wrong}"
            assert ps.ranked() == int((t >= 0).sum())


# ---- metrics ------------------------------------------------------------------------------------------------
# (greater, equal): equal = 1 at, before and after a cutoff; tie runs straddling 10 and 4096; runs entirely past a
# cutoff; a place past 4096; an unranked row
METRIC_ROWS = [(0, 1), (9, 1), (10, 1), (5, 10), (3, 3), (0, 2), (20, 5), (4090, 10), (5000, 1), (100000, 50),
               (0, 0), (7, 1), (0, 5000)]


def metrics_ref(rows, cutoffs):
    """(ranked, sum of a + b, {(name, k): mean}) with Fractions and fp64 log2."""
    ranked = [(g, e) for g, e in rows if e > 0]
    ab = sum(2 * g + e + 1 for g, e in ranked)
    out = {}
    for k in cutoffs:
        hit, mrr, ndcg = Fraction(0), Fraction(0), 0.0
        for g, e in ranked:
            places = range(g + 1, min(g + e, k) + 1)
            hit += Fraction(len(places), e)
            mrr += sum(Fraction(1, j) for j in places) / e
            ndcg += math.fsum(1.0 / math.log2(j + 1.0) for j in places) / e
        n = len(ranked)
        means = (float(hit / n), float(mrr / n), ndcg / n) if n else (math.nan,) * 3
        out["hit", k], out["mrr", k], out["ndcg", k] = means
    return len(ranked), ab, out


def check_metrics(device):
    for rows in (METRIC_ROWS, [(0, 0), (0, 0)]):
        ps = K.place_metrics(torch.tensor(rows, dtype=torch.int32, device=device), CUTOFFS)
        ranked, ab, want = metrics_ref(rows, CUTOFFS)
        assert ps.ranked() == ranked and ps.stats()[1] == ab
        assert ps.mean_place() == ab / (2 * ranked) if ranked else math.isnan(ps.mean_place())
        for (name, k), w in want.items():
            got = getattr(ps, name)(k)
            print(f"{name}@{k}: {got!r} want {w!r}")
            # every term lies in [0, 1] and fewer than 1000 are added in fp64: the error is below 1000 * 2^-52
            assert abs(got - w) <= 1e-12 if ranked else math.isnan(got), (name, k, got, w)
