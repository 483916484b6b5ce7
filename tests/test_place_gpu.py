"""The place of a held-out candidate among all candidates on the GPU: hip/fm_place.hip through
``ops.kernels.fm_place`` / ``place_metrics`` and ``FactorizationMachine.place``, against fp64 references, the CPU
twin and ``fm_topk``."""

import numpy as np
import pytest
import torch

import place_oracle as PO
from fast_tffm_amd.ops import kernels as K
from topk_oracle import exact_batches, exact_model, random_inputs, scores64, tol64

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("nq", PO.EXACT_NQS)
@pytest.mark.parametrize("Kp", PO.EXACT_KPS)
def test_exact_counts(Kp, nq):
    PO.check_exact(Kp, nq, DEV)


@pytest.mark.parametrize("Kp", [8, 64, 100])
def test_random_profiles(Kp):
    nq = 33
    slab = PO.slab_of(nq)
    nc = 3 * slab + 5
    Q, qb, C, cb = random_inputs(nq, nc, Kp, seed=Kp)
    t = PO.targets(nq, nc, slab, 0, seed=Kp)
    dev = [x.to(DEV) for x in (Q, qb, C, cb)]
    ws = K.place_workspace(nq, nc, 1, DEV)
    got = K.fm_place(*dev, t.to(DEV), ws=ws).counts().cpu().numpy()
    assert np.array_equal(got, K.fm_place(Q, qb, C, cb, t).counts().numpy()), "the CPU twin's counts differ"
    assert np.array_equal(got, K.fm_place(*dev, t.to(DEV), ws=ws).counts().cpu().numpy()), "not repeatable"
    with pytest.raises(ValueError):
        K.fm_place(*dev, t.to(DEV), ws=ws[:-8])
    S, T = scores64(Q, qb, C, cb), tol64(Q, qb, C, cb)
    idx, _ = K.fm_topk(*dev, 10)
    idx = idx.cpu().numpy()
    for q, tq in enumerate(t.tolist()):
        gt, eq = got[q]
        if tq < 0:
            assert gt == 0 and eq == 0
            continue
        assert eq >= 1, f"query {q}: the target pass and the matrix pass differ in s_t"
        rest = np.arange(nc) != tq
        lo = (S[q, rest] - T[q, rest] > S[q, tq] + T[q, tq]).sum()
        hi = (S[q, rest] + T[q, rest] >= S[q, tq] - T[q, tq]).sum()
        assert lo <= gt <= hi, f"query {q}: greater {gt} outside [{lo}, {hi}]"
        if gt + eq <= 10:
            assert tq in idx[q]
        if gt >= 10:
            assert tq not in idx[q]


def test_metrics():
    PO.check_metrics(DEV)
    # more than one tile of 1024 contexts: the same bits as the CPU's sums
    c = torch.randint(0, 3000, (2500, 2), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    assert K.place_metrics(c.to(DEV), PO.CUTOFFS).stats() == K.place_metrics(c, PO.CUTOFFS).stats()


def test_model_place():
    bq, bc = exact_batches()
    t = torch.randint(0, bc.B, (bq.B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    t[3] = -1
    want = exact_model("cpu").place(bq, bc, t, (5, 10)).counts().numpy()
    assert (want[:, 1] >= 1).sum() == bq.B - 1
    m = exact_model(DEV)
    assert np.array_equal(m.place(bq.to(DEV), bc.to(DEV), t.to(DEV), (5, 10)).counts().cpu().numpy(), want)
    prof = m.profile(bc.to(DEV))
    assert np.array_equal(m.place(bq.to(DEV), prof, t.to(DEV), (5, 10)).counts().cpu().numpy(), want)
