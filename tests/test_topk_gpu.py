"""Top-k recommendation on the GPU (hip/fm_topk.hip): the fp64 oracle's exact grid and slab placements, random
profiles bit for bit against the CPU twin and within the rounding bounds, the score identity against the
scorer, inputs and outputs, and ``FactorizationMachine.recommend`` on a GPU model against the CPU model."""

import numpy as np
import pytest
import torch

import topk_oracle as O
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

CPU = torch.device("cpu")


def _dev():
    return torch.device("cuda:0")


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))


@pytest.mark.parametrize("i_kp", range(len(O.KPS)), ids=[f"Kp{v}" for v in O.KPS])
def test_exact_grid(i_kp):
    O.check_exact_grid(i_kp, _dev())


def test_placement_across_slabs():
    O.check_placement(_dev())


@pytest.mark.parametrize("Kp,k", O.RANDOM_CASES)
def test_random_profiles_equal_the_cpu_twin_and_meet_the_bounds(Kp, k):
    Q, qb, C, cb = O.random_case(Kp, k)
    gpu = O.run(Q, qb, C, cb, k, _dev())
    cpu = O.run(Q, qb, C, cb, k, CPU)
    assert _same(gpu, cpu), f"Kp={Kp} k={k}: GPU and CPU twin differ"
    O.assert_within_bounds(gpu[0], gpu[1], Q, qb, C, cb, k, what=f"gpu Kp={Kp} k={k}")


def test_many_slabs_and_query_tiles_equal_the_cpu_twin():
    """200 queries against 50000 candidates: 13 query tiles, and as many slabs as the plan allows."""
    nq, nc, Kp, k = 200, 50000, 16, 10
    slab, parts = K.topk_plan(nq, nc, k)
    assert parts > 100
    Q, qb, C, cb = O.random_inputs(nq, nc, Kp, seed=11)
    assert _same(O.run(Q, qb, C, cb, k, _dev()), O.run(Q, qb, C, cb, k, CPU))


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_identity_against_the_scorer(dtype, bias):
    with O.make_model(dtype, bias, device=_dev()) as m:
        O.check_identity(m, what=f"gpu {dtype} bias={bias}")


def test_repeatable_strided_given_outputs_and_workspace():
    dev = _dev()
    Q, qb, C, cb = O.random_inputs(17, 3 * O.slab_of(17, 10) + 5, 12, seed=2)
    a = O.run(Q, qb, C, cb, 10, dev)
    for _ in range(3):
        assert _same(a, O.run(Q, qb, C, cb, 10, dev))
    assert _same(a, O.run(Q, qb, C, cb, 10, CPU))
    # row strides greater than Kp
    Qw, Cw = torch.full((17, 20), 7.0), torch.full((C.shape[0], 16), -7.0)
    Qw[:, :12], Cw[:, :12] = Q, C
    assert _same(a, O.run(Qw.to(dev)[:, :12], qb, Cw.to(dev)[:, :12], cb, 10, dev))
    # caller-provided outputs and workspace
    idx = torch.empty((17, 10), dtype=torch.int32, device=dev)
    score = torch.empty((17, 10), device=dev)
    ws = K.topk_workspace(17, C.shape[0], 10, dev)
    gi, gs = K.fm_topk(Q.to(dev), qb.to(dev), C.to(dev), cb.to(dev), 10, idx=idx, score=score, ws=ws)
    assert gi.data_ptr() == idx.data_ptr() and gs.data_ptr() == score.data_ptr()
    assert _same(a, (idx.cpu().numpy(), score.cpu().numpy()))
    with pytest.raises(ValueError):
        K.fm_topk(Q.to(dev), qb.to(dev), C.to(dev), cb.to(dev), 10, ws=ws[:64])


def test_argument_checks_and_empty_inputs():
    dev = _dev()
    Q, qb, C, cb = (t.to(dev) for t in O.random_inputs(5, 40, 8, seed=1))
    for k in (0, 129):
        with pytest.raises(ValueError):
            K.fm_topk(Q, qb, C, cb, k)
    with pytest.raises(ValueError):
        K.fm_topk(Q[:, :6], qb, C[:, :6], cb, 3)                 # Kp = 6
    with pytest.raises(ValueError):
        K.fm_topk(Q.double(), qb, C, cb, 3)                      # dtype mismatch
    with pytest.raises(ValueError):
        K.fm_topk(Q, qb, C.cpu(), cb.cpu(), 3)                   # tensors on mixed devices
    with pytest.raises(ValueError):
        K.fm_topk(Q, qb.cpu(), C, cb, 3)
    idx, score = K.fm_topk(Q[:0], qb[:0], C, cb, 3)
    assert tuple(idx.shape) == (0, 3) == tuple(score.shape)
    idx, score = K.fm_topk(Q, qb, C[:0], cb[:0], 3)
    assert (idx == -1).all() and torch.isneginf(score).all() and tuple(idx.shape) == (5, 3)


def test_fp8_table_is_refused():
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig

    bq, bc = O.identity_batches(1013)
    with FactorizationMachine(FMConfig(vocabulary_size=1013, factor_num=16, dtype=K.FP8), device=_dev()) as m:
        with pytest.raises(NotImplementedError, match="bf16"):
            m.profile(bq.to(_dev()))
        with pytest.raises(NotImplementedError):
            m.recommend(bq.to(_dev()), bc.to(_dev()), 3)


def test_model_recommend_equals_the_cpu_model():
    """The exact-integer table: every score is exact in fp32 in any order, so the executors agree bit for bit."""
    bq, bc = O.exact_batches()
    with O.exact_model(CPU) as mc, O.exact_model(_dev()) as mg:
        want = mc.recommend(bq, bc, 10)
        got = mg.recommend(bq.to(_dev()), bc.to(_dev()), 10)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
        index = mg.profile(bc.to(_dev()))
        got = mg.recommend(bq.to(_dev()), index, 10)
        assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])
