"""Top-k recommendation on the CPU: the kernel's twin against the fp64 oracle (exact grid, placement across
slabs, random profiles), the score identity against the scorer, argument checks, and the layers above it:
``FactorizationMachine.profile`` / ``recommend``, ``ServingModel.index`` / ``recommend``, ``run.py recommend``
alone and on two gloo ranks, and ``forward(want_r1=True)`` through the exchanges."""

import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import topk_oracle as O
from fast_tffm_amd import cli
from fast_tffm_amd.ops import kernels as K

CPU = torch.device("cpu")


@pytest.mark.parametrize("i_kp", range(len(O.KPS)), ids=[f"Kp{v}" for v in O.KPS])
def test_exact_grid(i_kp):
    O.check_exact_grid(i_kp, CPU)


def test_placement_across_slabs():
    O.check_placement(CPU)


@pytest.mark.parametrize("Kp,k", O.RANDOM_CASES)
def test_random_profiles_within_bounds(Kp, k):
    Q, qb, C, cb = O.random_case(Kp, k)
    idx, score = O.run(Q, qb, C, cb, k, CPU, threads=2)
    O.assert_within_bounds(idx, score, Q, qb, C, cb, k, what=f"cpu Kp={Kp} k={k}")


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_identity_against_the_scorer(dtype, bias):
    with O.make_model(dtype, bias) as m:
        O.check_identity(m, what=f"cpu {dtype} bias={bias}")


def test_repeatable_strided_and_given_outputs():
    Q, qb, C, cb = O.random_inputs(17, 600, 12, seed=2)
    a = O.run(Q, qb, C, cb, 10, CPU)
    b = O.run(Q, qb, C, cb, 10, CPU, threads=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    # row strides greater than Kp
    Qw, Cw = torch.full((17, 20), 7.0), torch.full((600, 16), -7.0)
    Qw[:, :12], Cw[:, :12] = Q, C
    c = O.run(Qw[:, :12], qb, Cw[:, :12], cb, 10, CPU)
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1].view(np.uint32), c[1].view(np.uint32))
    # caller-provided outputs
    idx, score = torch.empty((17, 10), dtype=torch.int32), torch.empty((17, 10))
    gi, gs = K.fm_topk(Q, qb, C, cb, 10, idx=idx, score=score)
    assert gi.data_ptr() == idx.data_ptr() and gs.data_ptr() == score.data_ptr()
    assert np.array_equal(idx.numpy(), a[0]) and np.array_equal(score.numpy(), a[1])


def test_argument_checks_and_empty_inputs():
    Q, qb, C, cb = O.random_inputs(5, 40, 8, seed=1)
    for k in (0, 129):
        with pytest.raises(ValueError):
            K.fm_topk(Q, qb, C, cb, k)
    with pytest.raises(ValueError):
        K.fm_topk(Q[:, :6], qb, C[:, :6], cb, 3)                 # Kp = 6
    with pytest.raises(ValueError):
        K.fm_topk(torch.zeros(5, 260), qb, torch.zeros(40, 260), cb, 3)   # Kp > 256
    with pytest.raises(ValueError):
        K.fm_topk(Q.double(), qb, C, cb, 3)                      # dtype mismatch
    with pytest.raises(ValueError):
        K.fm_topk(Q, qb, C, cb.double(), 3)
    with pytest.raises(ValueError):
        K.fm_topk(Q, qb[:4], C, cb, 3)                           # one base per row
    with pytest.raises(ValueError):
        K.fm_topk(Q, qb, C, cb, 3, idx=torch.empty((5, 3), dtype=torch.int64))
    with pytest.raises(ValueError):
        K.fm_topk(Q.to("meta"), qb, C, cb, 3)                    # tensors on mixed devices
    idx, score = K.fm_topk(Q[:0], qb[:0], C, cb, 3)
    assert tuple(idx.shape) == (0, 3) == tuple(score.shape)
    idx, score = K.fm_topk(Q, qb, C[:0], cb[:0], 3)
    assert (idx == -1).all() and torch.isneginf(score).all() and tuple(idx.shape) == (5, 3)


def test_plan_covers_the_candidates():
    for nq, nc, k in [(1, 1 << 20, 10), (64, 1 << 20, 10), (1024, 1 << 20, 10), (33, 1000, 128), (100000, 50, 1),
                      (1, (1 << 31) - 1, 128)]:
        slab, parts = K.topk_plan(nq, nc, k)
        assert slab % 32 == 0 and slab * (parts - 1) < nc <= slab * parts and 1 <= parts <= 512
    assert K.topk_plan(1, 1 << 20, 10)[1] == 512     # one query still spreads over the chip


# ---- model ------------------------------------------------------------------------------------------------
def test_model_recommend_is_topk_over_its_profiles():
    bq, bc = O.identity_batches(1013)
    with O.make_model(torch.float32, True) as m:
        q_pred, q_prof = m.profile(bq)
        c_pred, c_prof = m.profile(bc)
        assert torch.equal(q_pred, m.predict(bq)) and q_prof.shape == (bq.B, m.Kp) and q_prof.dtype == torch.float32
        assert torch.equal(q_prof[0], torch.zeros(m.Kp))          # (the empty context)
        want = K.fm_topk(q_prof, q_pred, c_prof, c_pred - m.gbias, 7)
        for cand in (bc, (c_pred, c_prof)):
            got = m.recommend(bq, cand, 7)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with O.make_model(torch.float32, False) as m:
        c_pred, c_prof = m.profile(bc)
        q_pred, q_prof = m.profile(bq)
        want = K.fm_topk(q_prof, q_pred, c_prof, c_pred, 30)      # k > candidates
        got = m.recommend(bq, bc, 30)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and (got[0][:, bc.B:] == -1).all()


def test_fp8_table_is_refused():
    """fp8 tables exist on the GPU only (tests/test_topk_gpu.py builds one); here a bare model object with
    an fp8 configuration: ``profile`` refuses by the configured dtype before it touches a table."""
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig

    m = object.__new__(FactorizationMachine)
    m.closed = True  # (nothing to release)
    m.cfg = FMConfig(vocabulary_size=100, factor_num=8, dtype=K.FP8)
    with pytest.raises(NotImplementedError, match="bf16"):
        m.profile(None)
    with pytest.raises(NotImplementedError):
        m.recommend(None, (None, None), 3)


# ---- CLI ----------------------------------------------------------------------------------------------------
LINES, CANDS = 60, 150


def _copy_lines(src, dst, start, n):
    with open(src, "rb") as f, open(dst, "wb") as g:
        for i, line in enumerate(f):
            if i >= start + n:
                break
            if i >= start:
                g.write(line)


def _write_cfg(workdir, mode="auto"):
    text = f"""[General]
vocabulary_size = 5003
vocabulary_block_num = 2
factor_num = 6
hash_feature_id = True
log_dir = {workdir}/log
device = cpu
global_bias = true

[Train]
batch_size = 100
init_value_range = 0.3
factor_lambda = 0
bias_lambda = 0
epoch_num = 1
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
loss_type = logistic
train_files = {workdir}/data/train_0

[Predict]
predict_files = {workdir}/data/test_0

[Distributed]
mode = {mode}
"""
    p = os.path.join(workdir, f"run_{mode}.cfg")
    with open(p, "w") as f:
        f.write(text)
    return p


@pytest.fixture(scope="module")
def trained(tmp_path_factory, ref_data_dir):
    """A tiny model trained for a few steps through the CLI, then ``recommend`` of test_0's head over a
    candidate file cut from further down test_0."""
    wd = str(tmp_path_factory.mktemp("recommend_cli"))
    os.makedirs(os.path.join(wd, "data"))
    _copy_lines(os.path.join(ref_data_dir, "train_0"), os.path.join(wd, "data", "train_0"), 0, 600)
    _copy_lines(os.path.join(ref_data_dir, "test_0"), os.path.join(wd, "data", "test_0"), 0, LINES)
    cands = os.path.join(wd, "data", "candidates")
    _copy_lines(os.path.join(ref_data_dir, "test_0"), cands, LINES, CANDS)
    cfg = _write_cfg(wd)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["train", cfg, "--max-steps", "4"]) == 0
        assert cli.main(["recommend", cfg, "--candidates", cands]) == 0
    return wd, cfg, cands


def _trainer(cfg_path):
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.trainer import Trainer

    tr = Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None)
    assert tr.restore()
    return tr


def _load(tr, path):
    from fast_tffm_amd.data.reader import load_file_batch

    c = tr.cfg
    return load_file_batch([path], None, c.vocabulary_size, c.hash_feature_id, c.parse_threads)


def _expected_lines(idx, score):
    return [" ".join(f"{c}:{str(np.float32(s))}" for c, s in zip(ri, rs) if c >= 0) for ri, rs in zip(idx, score)]


def test_cli_recommend_file(trained):
    wd, cfg, cands = trained
    out = os.path.join(wd, "data", "test_0_recommend")
    got = open(out).read().splitlines()
    assert len(got) == LINES
    with _trainer(cfg) as tr:
        assert float(tr.model.gbias) != 0.0
        idx, score = tr.model.recommend(_load(tr, os.path.join(wd, "data", "test_0")), _load(tr, cands), 10)
    assert got == _expected_lines(idx.numpy(), score.numpy())
    for ln in got:
        toks = [t.split(":") for t in ln.split()]
        assert len(toks) == 10 and all(0 <= int(c) < CANDS for c, _ in toks)
        s = [np.float32(x) for _, x in toks]
        assert all(a >= b for a, b in zip(s, s[1:]))
    # --top N, and its range
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["recommend", cfg, "--candidates", cands, "--top", "3"]) == 0
    assert open(out).read().splitlines() == [" ".join(ln.split()[:3]) for ln in got]
    for bad in ("0", "129"):
        with pytest.raises(ValueError), contextlib.redirect_stdout(io.StringIO()):
            cli.main(["recommend", cfg, "--candidates", cands, "--top", bad])
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        cli.main(["recommend", cfg])


def test_cli_profiles_candidates_in_batches(trained, monkeypatch):
    """More candidates than one profile batch: the same file."""
    from fast_tffm_amd import trainer

    wd, cfg, cands = trained
    out = os.path.join(wd, "data", "test_0_recommend")
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["recommend", cfg, "--candidates", cands]) == 0
    want = open(out).read()
    monkeypatch.setattr(trainer, "RECOMMEND_PROFILE_BATCH", 64)
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["recommend", cfg, "--candidates", cands]) == 0
    assert open(out).read() == want


def _rank_worker(rank, world, port, cfg_path, cands):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    with Trainer(load_config(cfg_path, echo=False), ctx, printer=lambda *a, **k: None) as tr:
        tr.recommend(cands)
    fmdist.shutdown()


def test_two_row_sharded_ranks_write_the_same_file(trained):
    from ports import free_port

    wd, cfg, cands = trained
    out = os.path.join(wd, "data", "test_0_recommend")
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["recommend", cfg, "--candidates", cands]) == 0
    want = open(out).read()
    os.remove(out)
    cfg2 = _write_cfg(wd, mode="shard")
    mp.spawn(_rank_worker, args=(2, free_port(), cfg2, cands), nprocs=2, join=True)
    assert open(out).read() == want


def _r1_worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
    from fast_tffm_amd.parallel import dist as fmdist

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")

    def cfg(mode):
        return FMConfig(vocabulary_size=997, factor_num=8, init_value_range=0.3, seed=11, mode=mode, threads=1,
                        global_bias=True)

    b = random_batch(24, 997, max_feats=10, seed=50 + rank)
    with FactorizationMachine(cfg("local"), device="cpu") as local:
        want = local.forward(b, want_r1=True)
        assert want.r1 is not None and local.forward(b).r1 is None
    for mode in ("shard", "dp", "dp_dense"):
        m = FactorizationMachine(cfg(mode), device="cpu", dist=ctx)
        fo = m.forward(b, want_r1=True)
        assert fo.r1 is not None and torch.equal(fo.r1, want.r1), mode
        assert torch.equal(fo.pred, want.pred), mode
        assert m.forward(b).r1 is None, mode
        m.close()
    fmdist.shutdown()


def test_forward_want_r1_through_the_exchanges():
    from ports import free_port

    mp.spawn(_r1_worker, args=(2, free_port()), nprocs=2, join=True)


# ---- serving --------------------------------------------------------------------------------------------------
def test_serving_recommend_lines_and_index(trained, tmp_path):
    from fast_tffm_amd.data.batch import Batch
    from fast_tffm_amd.serving import ServingModel, export_model, parse_serving_lines
    from fast_tffm_amd.utils.checkpoint import latest_checkpoint

    wd, cfg, _ = trained
    with _trainer(cfg) as tr:
        export = str(tmp_path / "export")
        export_model(latest_checkpoint(tr.cfg.log_dir), export, vocabulary_block_num=2, hash_feature_id=True,
                     loss_type="logistic")
        sm = ServingModel.load(export, device="cpu")
        ctx_lines = ["3:1 17:0.5 3:2", "4999:1", "12:1 13:1 14:-1.5 5002:0.25"]
        cand_lines = [f"{7 * i + 1}:1 {3 * i}:0.5 17:{i % 3}" for i in range(40)]
        a = sm.recommend(ctx_lines, cand_lines, top=5)
        index = sm.index(cand_lines)
        assert len(index) == 40
        b = sm.recommend(ctx_lines, index, top=5)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert a[0].shape == (3, 5) and a[0].dtype == np.int32 and a[1].dtype == np.float32

        def batch(lines):
            o, i, v = parse_serving_lines(lines, 5003, True)
            return Batch(torch.zeros(len(lines)), o, i, v, None, int(o[-1]))

        idx, score = tr.model.recommend(batch(ctx_lines), batch(cand_lines), 5)
        assert np.array_equal(a[0], idx.numpy()) and np.array_equal(a[1], score.numpy())
