"""The place of a held-out candidate among all candidates on the CPU: ``ops.kernels.fm_place`` /
``place_metrics`` (cpu/kernels.cpp, the twin of hip/fm_place.hip) against fp64 references."""

import pytest
import torch

import place_oracle as PO
from fast_tffm_amd.ops import kernels as K
from topk_oracle import exact_inputs

CPU = torch.device("cpu")


@pytest.mark.parametrize("nq", PO.EXACT_NQS)
@pytest.mark.parametrize("Kp", PO.EXACT_KPS)
def test_exact_counts(Kp, nq):
    PO.check_exact(Kp, nq, CPU)


def test_metrics():
    PO.check_metrics(CPU)


def test_arguments():
    Q, qb, C, cb = exact_inputs(3, 7, 8, seed=1)
    t = torch.tensor([0, 6, -1], dtype=torch.int32)
    bad = [
        lambda: K.fm_place(Q, qb, C[:, :4].contiguous(), cb, t),      # widths differ
        lambda: K.fm_place(Q, qb, C, cb, t.long()),                   # int32 targets
        lambda: K.fm_place(Q, qb, C, cb, torch.tensor([0, 7, -1], dtype=torch.int32)),
        lambda: K.fm_place(Q, qb, C, cb, torch.tensor([0, -2, 1], dtype=torch.int32)),
        lambda: K.fm_place(Q, qb, C, cb, t, (10, 5)),                 # ascending cutoffs
        lambda: K.fm_place(Q, qb, C, cb, t, (0,)),
        lambda: K.fm_place(Q, qb, C, cb, t, (4097,)),
        lambda: K.fm_place(Q, qb, C, cb, t, (1, 2, 3, 4, 5)),
    ]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(KeyError):
        K.fm_place(Q, qb, C, cb, t, (5,)).hit(10)
    for q, c in ((Q[:0], C), (Q, C[:0])):   # nothing to rank: everything unranked
        ps = K.fm_place(q, qb[:q.shape[0]], c, cb[:c.shape[0]], torch.full((q.shape[0],), -1, dtype=torch.int32))
        assert ps.ranked() == 0 and not ps.counts().any() and ps.hit(10) != ps.hit(10)
