"""hip/fm_shortlist.hip against the fp64 references and the CPU twins of tests/test_shortlist.py, bit for bit; against
``seen`` = the lists' complement on random profiles; in a captured graph; and the model's methods against the CPU's."""

import numpy as np
import pytest
import torch

import topk_oracle as TO
from fast_tffm_amd.ops import kernels as K
from test_shortlist import CPU, place_cases, restrict, run_place, run_topk, topk_cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
same_bits = lambda a, b: np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("nq", [1, 17, 65])    # one context per call; every kind in one call; more waves than kinds
@pytest.mark.parametrize("k", [1, 10, 128])
@pytest.mark.parametrize("Kp", [4, 64, 100])   # one column group; the last prefetching width; no prefetch, a cut group
def test_topk_shortlist(Kp, k, nq):
    for inputs, rows, want_i, want_s in topk_cases(Kp, k, nq):
        ws = K.shortlist_workspace(nq, sum(map(len, rows)), inputs[2].shape[0], k, DEV)
        idx, score = run_topk(inputs, rows, k, DEV, ws=ws)
        assert np.array_equal(idx, want_i) and np.array_equal(score.astype(np.float64), want_s), "not the reference's"
        for other in (run_topk(inputs, rows, k, CPU), run_topk(inputs, rows, k, DEV, ws=ws)):   # the twin; repeatable
            assert same_bits((idx, score), other)


@pytest.mark.parametrize("nq", [1, 17, 65])
@pytest.mark.parametrize("Kp", [4, 64, 100])
def test_place_shortlist(Kp, nq):
    for inputs, t, rows, want in place_cases(Kp, nq):
        ws = K.shortlist_workspace(nq, sum(len(set(r)) for r in rows), inputs[2].shape[0], 1, DEV)
        got = run_place(inputs, t, rows, DEV, ws=ws)
        assert np.array_equal(got, want), f"rows {np.flatnonzero((got != want).any(1))} differ from the reference"
        assert all(np.array_equal(got, run_place(inputs, t, rows, d, ws=w)) for d, w in ((CPU, None), (DEV, ws)))


@pytest.mark.parametrize("Kp", [64, 100])
def test_parts_of_one_list(Kp):
    # 900 entries in 3 full parts and a remainder; the best are candidates 0, nc - 1 and both neighbours of every cut
    nc, k = 1100, 10
    Q, qb, C, cb = TO.exact_inputs(1, nc, Kp, seed=Kp)
    row = np.sort(np.r_[0, nc - 1, np.random.default_rng(3).choice(np.arange(1, nc - 1), 898, replace=False)])
    edges = [row[p] for p in (0, 255, 256, 511, 512, 767, 768, 899)]
    cb[edges] += 1024.0   # (still exact in fp32: quarters below 2^11)
    inputs, rows = (Q, qb, C, cb), [row.tolist()]
    want_i, want_s = TO.oracle_topk(restrict(TO.scores64(*inputs), rows), k)
    got = run_topk(inputs, rows, k, DEV)
    assert np.array_equal(got[0], want_i) and np.array_equal(got[1].astype(np.float64), want_s)
    assert set(edges) <= set(got[0][0].tolist()) and K.shortlist_plan(1, 900, nc) == 4
    t = torch.tensor([int(row[256])], dtype=torch.int32)
    assert np.array_equal(run_place(inputs, t, rows, DEV), run_place(inputs, t, rows, CPU))


@pytest.mark.parametrize("Kp", [64, 100])
def test_score_is_fm_topk_s(Kp):
    # random normal profiles, whose sums round: the same bits as the slab pass with the list's complement left out
    nq, k = 17, 10
    nc = 3 * TO.slab_of(nq, k) + 5
    inputs = [x.to(DEV) for x in TO.random_inputs(nq, nc, Kp, seed=Kp)]
    rng = np.random.default_rng(5)
    rows = [np.flatnonzero(rng.random(nc) < 0.3).tolist() for _ in range(nq)]
    sl = K.seen_lists(rows, nc, DEV)
    rest = K.seen_lists([sorted(set(range(nc)) - set(r)) for r in rows], nc, DEV)
    a, b = K.fm_topk(*inputs, k, shortlist=sl), K.fm_topk(*inputs, k, seen=rest)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    t = torch.randint(0, nc, (nq,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).to(DEV)
    t[::2] = torch.tensor([r[3] for r in rows[::2]], dtype=torch.int32).to(DEV)   # listed targets too
    assert torch.equal(K.fm_place(*inputs, t, shortlist=sl).counts(), K.fm_place(*inputs, t, seen=rest).counts())


def test_graph_capture():
    (inputs, rows, want_i, _), = topk_cases(64, 10)
    inputs = [x.to(DEV) for x in inputs]
    sl = K.seen_lists(rows, inputs[2].shape[0], DEV)
    ws = K.shortlist_workspace(17, sl[1].numel(), inputs[2].shape[0], 10, DEV)
    idx, score = K.fm_topk(*inputs, 10, shortlist=sl, ws=ws)
    torch.cuda.synchronize()
    g_idx, g_score, g = torch.empty_like(idx), torch.empty_like(score), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.fm_topk(*inputs, 10, shortlist=sl, ws=ws, idx=g_idx, score=g_score)
    for _ in range(3):
        g_idx.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(g_idx, idx) and torch.equal(g_score.view(torch.int32), score.view(torch.int32))
        assert np.array_equal(g_idx.cpu().numpy(), want_i)


def test_model_shortlist():
    bq, bc = TO.exact_batches()
    t = torch.randint(0, bc.B, (bq.B,), generator=torch.Generator().manual_seed(2), dtype=torch.int32)
    t[3] = -1   # (the lists below: a random 40 candidates, the odd contexts' with their target)
    cpu, gpu, rng = TO.exact_model("cpu"), TO.exact_model(DEV), np.random.default_rng(8)
    rows = [rng.choice(bc.B, 40, replace=False).tolist() + [int(x)] * (q % 2 and int(x) >= 0) for q, x in enumerate(t)]
    want_i, want_s = cpu.recommend(bq, bc, 10, shortlist=K.seen_lists(rows, bc.B, CPU))
    sl = K.seen_lists(rows, bc.B, DEV)
    idx, score = gpu.recommend(bq.to(DEV), bc.to(DEV), 10, shortlist=sl)
    assert torch.equal(idx.cpu(), want_i) and torch.equal(score.cpu(), want_s)
    want = cpu.place(bq, bc, t, (5, 10), shortlist=K.seen_lists(rows, bc.B, CPU)).counts()
    assert torch.equal(gpu.place(bq.to(DEV), bc.to(DEV), t.to(DEV), (5, 10), shortlist=sl).counts().cpu(), want)
