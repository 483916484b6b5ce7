"""Recommend and place with the already-seen candidates left out on the GPU: hip/fm_seen.hip (the filtered slab pass
of ``fm_topk``, the correction pass of ``fm_place``) against the fp64 references and the CPU twins of
tests/test_seen.py, bit for bit, and ``FactorizationMachine.recommend`` / ``.place`` against the CPU model."""

import numpy as np
import pytest
import torch

import topk_oracle as TO
from fast_tffm_amd.ops import kernels as K
from test_seen import CPU, place_cases, run_place, run_topk, topk_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("Kp", [4, 64, 100])   # one column group; the last prefetching width; no prefetch, a cut group
def test_topk_seen(Kp, k):
    inputs, rows, want_i, want_s = topk_case(Kp, k)
    ws = K.topk_workspace(17, inputs[2].shape[0], k, DEV)
    idx, score = run_topk(inputs, rows, k, DEV, ws=ws)
    assert np.array_equal(idx, want_i), "idx differs from the reference"
    assert np.array_equal(score.astype(np.float64), want_s), "score differs from the reference"
    for other in (run_topk(inputs, rows, k, CPU), run_topk(inputs, rows, k, DEV, ws=ws)):   # the twin; repeatable
        assert np.array_equal(idx, other[0]) and np.array_equal(score.view(np.uint32), other[1].view(np.uint32))


@pytest.mark.parametrize("nq", [1, 17, 65])    # a partial tile; idle lane groups; a second query block
@pytest.mark.parametrize("Kp", [4, 64, 100])
def test_place_seen(Kp, nq):
    for inputs, t, rows, want in place_cases(Kp, nq):
        ws = K.place_workspace(nq, inputs[2].shape[0], 1, DEV)
        got = run_place(inputs, t, rows, DEV, ws=ws)
        assert np.array_equal(got, want), f"rows {np.flatnonzero((got != want).any(1))} differ from the reference"
        assert np.array_equal(got, run_place(inputs, t, rows, CPU)), "the CPU twin's counts differ"
        assert np.array_equal(got, run_place(inputs, t, rows, DEV, ws=ws)), "not repeatable"


def test_model_seen():
    bq, bc = TO.exact_batches()
    t = torch.randint(0, bc.B, (bq.B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    t[3] = -1
    cpu, gpu = TO.exact_model("cpu"), TO.exact_model(DEV)
    plain = cpu.recommend(bq, bc, 10)[0]
    # every context has seen its plain answer, the odd ones their target too
    rows = [plain[q].tolist() + [int(t[q])] * (q % 2 and int(t[q]) >= 0) for q in range(bq.B)]
    want_i, want_s = cpu.recommend(bq, bc, 10, seen=K.seen_lists(rows, bc.B, CPU))
    assert not any(set(want_i[q].tolist()) & set(rows[q]) for q in range(bq.B))
    seen = K.seen_lists(rows, bc.B, DEV)
    idx, score = gpu.recommend(bq.to(DEV), bc.to(DEV), 10, seen=seen)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(score.cpu(), want_s)
    want = cpu.place(bq, bc, t, (5, 10), seen=K.seen_lists(rows, bc.B, CPU)).counts()
    assert torch.equal(gpu.place(bq.to(DEV), bc.to(DEV), t.to(DEV), (5, 10), seen=seen).counts().cpu(), want)
