"""The segmented backward (hip/fm_bwd.hip) on plans with chunk lengths below 32: one training step on
a ladder batch (tests/dedup_oracle.py: rows of 1..5, CH-1..CH+1, 2CH-1..2CH+1, 16CH-1..16CH+1, 17CH+1
and 40CH+3 occurrences, so the chunk kernel's direct apply, the lane-group combine and the workgroup
combine all run) against the fp64 autograd oracle, for dedup_chunk 1, 7, 31 and the usual 32 (the
control leg), every row width's chunk kernel, with and without feature values; run-to-run determinism
(the combine lists are filled through atomics); and the row-sharded step's EMIT kernels against the
local step on the same batches."""

import functools
import os

import numpy as np
import pytest
import torch

from fast_tffm_amd.data.batch import Batch
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.ops import kernels as K

import dedup_oracle as O
from oracle import fm_objective, ftrl_step, reference_train_step, touched_rows

pytestmark = pytest.mark.gpu

CHS = [1, 7, 31, 32]
SPARE = 64  # table rows no occurrence touches
LR, LAMBDA, BATCH_CFG = 0.05, 0.01, 512
FTRL = K.OptConfig("ftrl", lr=0.1, l1=0.01, l2=0.02, beta=1.0, initial_accumulator=0.1)


@functools.lru_cache(maxsize=None)
def _ladder_batch(CH: int, with_vals: bool, seed: int = 0):
    """(cpu batch, vocabulary size, touched-row mask): the ladder's occurrences, in their shuffled
    order, dealt into examples of 0..~70 features; its keys mapped, in order, onto a random subset of
    the U + SPARE table rows (the sorted layout -- so every row's chunk count -- is the ladder's)."""
    rng = np.random.default_rng(1000 * CH + seed)
    keys = O.ladder(CH, 3, seed=CH + seed)
    p = O.plan(keys, CH)
    one, small, big = O.chunk_classes(p)
    assert one > 0 and small > 0 and big > 0, (CH, one, small, big)  # all three backward paths run
    assert p.n <= 11_007
    V = p.U + SPARE
    rows = np.sort(rng.choice(V, p.U, replace=False))
    ids = rows[keys].astype(np.int32)
    assert O.chunk_classes(O.plan(ids, CH)) == (one, small, big)
    lens = [0, 1, 70]
    while sum(lens) < p.n:
        lens.append(int(rng.integers(0, 41)))
    lens[-1] -= sum(lens) - p.n
    lens = np.asarray(lens)[rng.permutation(len(lens))]
    assert int(lens.sum()) == p.n and (lens == 0).any() and (lens == 1).any() and lens.max() > 64
    offsets = np.zeros(lens.size + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(lens)
    labels = (rng.random(lens.size) < 0.3).astype(np.float32)
    vals = None
    if with_vals:  # in (0, 2)
        vals = torch.from_numpy(np.clip(rng.random(p.n) * 2, 1e-3, 2 - 1e-3).astype(np.float32))
    b = Batch(torch.from_numpy(labels), torch.from_numpy(offsets), torch.from_numpy(ids), vals, None, p.n,
              max_feats=int(lens.max()))
    touched = torch.zeros(V, dtype=torch.bool)
    touched[torch.from_numpy(rows)] = True
    return b, V, touched


def _model(V, k, dtype, CH, opt=None, dist=None, **kw):
    if dtype == K.FP8:
        kw.setdefault("stochastic_rounding", False)  # the requantisation bound is round-to-nearest's
    cfg = FMConfig(vocabulary_size=V, factor_num=k, loss_type="logistic", init_value_range=0.05, seed=3,
                   opt=opt or K.OptConfig("adagrad", lr=LR), batch_size=BATCH_CFG, factor_lambda=LAMBDA,
                   bias_lambda=LAMBDA, dtype=dtype, dedup_chunk=CH, **kw)
    return FactorizationMachine(cfg, device="cuda", dist=dist)


def _raw_state(m):
    """Every stored array of the table, as bytes."""
    t = m.table
    return {n: x.detach().clone().contiguous().view(torch.uint8).reshape(x.shape[0], -1).cpu()
            for n, x in (("v", t.v), ("w", t.wx if t.wx is not None else t.w), ("s0v", t.s0v), ("s0w", t.s0w),
                         ("s1v", t.s1v), ("s1w", t.s1w)) if x is not None}


def _assert_untouched_rows_keep_their_bits(before, after, touched):
    for n in before:
        assert torch.equal(before[n][~touched], after[n][~touched]), n
    assert not torch.equal(before["v"][touched], after["v"][touched])


def _check_rows(m, dtype, got, want):
    if dtype == torch.float32:
        torch.testing.assert_close(got, want, rtol=2e-4, atol=5e-6)
    elif dtype == torch.bfloat16:
        torch.testing.assert_close(got, want, rtol=2e-2, atol=2e-3)
    else:  # fp8: w stays fp32; v within the final requantisation of the row
        torch.testing.assert_close(got[:, 0], want[:, 0], rtol=2e-4, atol=5e-6)
        scale = m.table.scale.double().cpu()[:, None]
        err = (got[:, 1:] - want[:, 1:]).abs()
        assert bool((err <= 16.0 * scale * 1.01 + 1e-7).all()), float((err / scale).max())


# k, dtype: the chunk kernel instantiated (4 table elements per lane)
#   16 fp32 / 16 bf16: 4-lane rows, the flat walk (fewer lanes than r1 rows in flight)
#   64 fp32: 16-lane rows;  100 fp32: padded Kp, inactive lanes
#   128 bf16: 32-lane rows, the short block for chunks of <= 4
#   128 fp8: the wide kernels, 8 values per lane
CONFIGS = [(16, torch.float32), (64, torch.float32), (100, torch.float32), (16, torch.bfloat16),
           (128, torch.bfloat16), (128, K.FP8)]


@pytest.mark.parametrize("with_vals", [False, True], ids=["nox", "x"])
@pytest.mark.parametrize("k,dtype", CONFIGS, ids=[f"k{k}-{str(d).split('.')[-1]}" for k, d in CONFIGS])
@pytest.mark.parametrize("CH", CHS)
def test_adagrad_step_on_ladder_batch_matches_oracle(CH, k, dtype, with_vals):
    from fast_tffm_amd.ops import native

    cpu_b, V, touched = _ladder_batch(CH, with_vals)
    m = _model(V, k, dtype, CH)
    p0 = m.table.reference_rows().double().cpu()
    before = _raw_state(m)
    wide0 = native.hip().bwd_wide_launches()
    m.train_step(cpu_b.to("cuda"))
    torch.cuda.synchronize()
    if dtype == K.FP8:
        assert native.hip().bwd_wide_launches() == wide0 + 1
    p1, _, _ = reference_train_step(p0, torch.full_like(p0, 0.1), cpu_b, "logistic", LR, LAMBDA, LAMBDA, BATCH_CFG)
    assert torch.equal(p1[~touched], p0[~touched])
    _assert_untouched_rows_keep_their_bits(before, _raw_state(m), touched)
    _check_rows(m, dtype, m.table.reference_rows().double().cpu(), p1)


@pytest.mark.parametrize("with_vals", [False, True], ids=["nox", "x"])
@pytest.mark.parametrize("CH", CHS)
def test_ftrl_step_on_ladder_batch_matches_oracle(CH, with_vals):
    cpu_b, V, touched = _ladder_batch(CH, with_vals)
    m = _model(V, 64, torch.float32, CH, opt=FTRL)
    p0 = m.table.reference_rows().double().cpu()
    before = _raw_state(m)
    m.train_step(cpu_b.to("cuda"))
    torch.cuda.synchronize()
    pr = p0.clone().requires_grad_(True)
    obj, _, _ = fm_objective(pr, cpu_b, "logistic", LAMBDA, LAMBDA, BATCH_CFG)
    (gr,) = torch.autograd.grad(obj, pr)
    assert torch.equal(touched_rows(cpu_b, V), touched)
    p1, _, _ = ftrl_step(p0, torch.full_like(gr, FTRL.initial_accumulator), torch.zeros_like(gr), gr, touched,
                         FTRL.lr, FTRL.l1, FTRL.l2, FTRL.beta)
    _assert_untouched_rows_keep_their_bits(before, _raw_state(m), touched)
    _check_rows(m, torch.float32, m.table.reference_rows().double().cpu(), p1)


@pytest.mark.parametrize("k,dtype", [(64, torch.float32), (16, torch.bfloat16)], ids=["k64-float32", "k16-bfloat16"])
@pytest.mark.parametrize("CH", [1, 7])
def test_step_does_not_depend_on_the_combine_lists_order(CH, k, dtype):
    """The chunk kernel appends multi-chunk rows to the two combine lists with atomics: whatever the
    order, two fresh models end bitwise equal."""
    cpu_b, V, _ = _ladder_batch(CH, True)
    b = cpu_b.to("cuda")
    runs = []
    for _ in range(2):
        m = _model(V, k, dtype, CH)
        m.train_step(b)
        torch.cuda.synchronize()
        t = m.table
        runs.append([x.clone() for x in (t.v, t.w, t.s0v, t.s0w)])
    for x, y in zip(*runs):
        assert torch.equal(x, y)


@pytest.fixture(scope="module")
def rccl_ctx():
    from ports import free_port

    from fast_tffm_amd.parallel import dist as fmdist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    ctx = fmdist.init_distributed(backend="nccl", rank=0, world=1, device="cuda:0", force_pg=True)
    yield ctx
    fmdist.shutdown()


@pytest.mark.parametrize("with_vals", [False, True], ids=["nox", "x"])
@pytest.mark.parametrize("k,dtype", [(64, torch.float32), (16, torch.bfloat16)], ids=["k64-float32", "k16-bfloat16"])
@pytest.mark.parametrize("CH", [1, 7])
def test_sharded_emit_step_matches_local_on_ladder_batches(rccl_ctx, CH, k, dtype, with_vals, monkeypatch):
    """The EMIT chunk kernels (the row-sharded step's compute path, run at world 1) walk the same short-chunk
    plans: two steps, tables against the local step's."""
    monkeypatch.setenv("FM_SHARD_W1_LOCAL", "0")
    b0, V, _ = _ladder_batch(CH, with_vals)
    b1, V1, _ = _ladder_batch(CH, with_vals, 1)
    assert V1 == V
    batches = [b0.to("cuda"), b1.to("cuda")]
    loc = _model(V, k, dtype, CH, mode="local")
    dm = _model(V, k, dtype, CH, mode="shard", dist=rccl_ctx)
    for i, b in enumerate(batches):
        l1 = loc.train_step(b).mean_loss()
        l2 = dm.train_step(b, batches[i + 1] if i + 1 < len(batches) else None).mean_loss()
        assert abs(l1 - l2) <= 1e-5 * max(1.0, abs(l1))
    torch.cuda.synchronize()
    tol = dict(rtol=1e-5, atol=1e-7) if dtype == torch.float32 else dict(rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dm.table.reference_rows(), loc.table.reference_rows(), **tol)
    dm.close()
