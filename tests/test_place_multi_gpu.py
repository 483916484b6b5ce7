"""Several held-out targets per context on the GPU: hip/fm_place_multi.hip through ``ops.kernels.fm_place`` with a
target pair and ``place_metrics(offsets=)``, against fp64 references and the CPU twin (cases: test_place_multi.py)."""

import pytest
import torch

import place_oracle as PO
import test_place_multi as PM
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.ops import native
from topk_oracle import random_inputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("with_seen", [False, True])
@pytest.mark.parametrize("nq", PO.EXACT_NQS)
@pytest.mark.parametrize("Kp", PO.EXACT_KPS)
def test_exact_counts(Kp, nq, with_seen):
    PM.check_exact(Kp, nq, DEV, with_seen)


def test_single_target_lists():
    PM.check_single(DEV)


def test_metrics():
    assert PM.S == native.hip().PLACE_SEGMENT
    PM.check_metrics(DEV)


@pytest.mark.parametrize("Kp", [8, 64, 100])
def test_cpu_twin_and_repeat(Kp):
    """Random fp32 profiles: counts and record word for word the CPU twin's, and again from the same workspace."""
    nq = 1100 if Kp == 8 else 33   # (more than one metric tile once)
    slab = PO.slab_of(nq)
    nc = 3 * slab + 5
    Q, qb, C, cb = random_inputs(nq, nc, Kp, seed=Kp)
    lists = PM.target_lists(nq, nc, slab, seed=Kp)
    seen = [sorted({(5 * q + j) % nc for j in range(q % 7)} | set(lists[q][:1])) for q in range(nq)]
    want = K.fm_place(Q, qb, C, cb, K.seen_lists(lists, nc, PM.CPU), PO.CUTOFFS, seen=K.seen_lists(seen, nc, PM.CPU))
    dev = [x.to(DEV) for x in (Q, qb, C, cb)]
    pair, sn = K.seen_lists(lists, nc, DEV), K.seen_lists(seen, nc, DEV)
    ws = K.place_workspace(nq, nc, len(PO.CUTOFFS), DEV, entries=pair[1].numel())
    for _ in range(2):
        got = K.fm_place(*dev, pair, PO.CUTOFFS, ws=ws, seen=sn)
        assert torch.equal(got.counts().cpu(), want.counts())
        assert torch.equal(got.rec.cpu(), want.rec)
    with pytest.raises(ValueError):
        K.fm_place(*dev, pair, PO.CUTOFFS, ws=ws[:-8])
