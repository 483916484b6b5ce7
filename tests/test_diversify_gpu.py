"""hip/fm_diversify.hip against the fp64 greedy loop of tests/test_diversify.py on the exact inputs, and against the
CPU twin bit for bit on random float inputs (eagerly, repeated, and replayed from a captured graph)."""

import pytest
import torch

from fast_tffm_amd.ops import kernels as K
from test_diversify import CASES, check_case, check_tie

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "M%d-Kp%d-n%d-nq%d-lam%s-pad%d" % c)
def test_against_fp64_greedy(case):
    check_case(case, DEV)


def test_twice_listed_candidate_ties_to_the_lower_position():
    check_tie(DEV)


@pytest.mark.parametrize("M,Kp,n", [(128, 64, 40), (17, 20, 17)])
def test_bitwise_the_cpu_twin(M, Kp, n):
    nq, nc, lam = 5, 300, 0.3
    g = torch.Generator().manual_seed(M)
    C = torch.randn((nc, Kp), generator=g)
    C[nc // 2:] = C[:nc // 2] + 0.05 * torch.randn((nc // 2, Kp), generator=g)   # near-copies: sims close to 1
    inv = K.diversify_scale(C)
    pidx = torch.stack([torch.randperm(nc, generator=g)[:M] for _ in range(nq)]).to(torch.int32)
    pscore = torch.randn((nq, M), generator=g).sort(dim=1, descending=True).values
    pidx[2, n // 2:], pscore[2, n // 2:] = -1, float("-inf")
    want = K.fm_diversify(C, inv, pidx, pscore, n, lam)
    dev = [t.to(DEV) for t in (C, inv, pidx, pscore)]
    got = K.fm_diversify(*dev, n, lam)
    bits = lambda ts: [t.cpu().contiguous().view(torch.int32) for t in ts]
    assert all(torch.equal(a, b) for a, b in zip(bits(got), bits(want)))
    assert len(set(want[0][0].tolist())) == n and (want[0][2, n // 2:] == -1).all()
    torch.cuda.synchronize()
    out, graph = tuple(torch.empty_like(t) for t in got), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        K.fm_diversify(*dev, n, lam, out=out)
    for _ in range(3):
        out[0].fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(bits(out), bits(want)))
