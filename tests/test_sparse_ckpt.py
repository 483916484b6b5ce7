"""Sparse checkpoints on the CPU: ``FMTable.changed_rows`` (cpu/kernels.cpp, the twin of hip/ckpt.hip)
against a torch comparison with a second, freshly initialised table; the sparse checkpoint format's
round trips (same layout, re-sharded, back to dense), the offline readers' dense view, the unchanged
default, and the CLI.  Every comparison is bitwise."""

import contextlib
import io
import json
import os
import types

import numpy as np
import pytest
import torch
from safetensors import safe_open

from fast_tffm_amd import cli
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.synthetic import random_batch
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.models.table import FMTable
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.utils import checkpoint as ckpt

from sparse_ckpt_oracle import T, assert_same_state, flip, torch_changed_rows

DTYPES = [torch.float32, torch.bfloat16]
OPTS = ["adagrad", "ftrl", "sgd"]


def _table(rows=200, Kf=6, dtype=torch.float32, opt="adagrad", world=1, rank=0, seed=3, vocab=None):
    return FMTable(rows * world if vocab is None else vocab, Kf, world=world, rank=rank, dtype=dtype,
                   opt=K.OptConfig(opt, lr=0.1), seed=seed, device="cpu")


def _check(table, want=None):
    got = table.changed_rows()
    assert got.dtype == torch.int64 and got.device.type == table.device.type
    ref = torch_changed_rows(table)
    assert torch.equal(got, ref)
    if want is not None:
        assert got.tolist() == sorted(want)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", OPTS)
@pytest.mark.parametrize("Kf", [1, 4, 6, 100])
def test_fresh_table_reports_nothing(dtype, opt, Kf):
    t = _table(130, Kf, dtype, opt)
    assert t.init_seed == 3
    _check(t, [])
    t.reinit(seed=77)
    assert t.init_seed == 77 and t.init_range == 0.01
    _check(t, [])
    assert K.changed_rows(t, seed=3).numel() == t.real_rows  # (another seed: every row differs)


@pytest.mark.parametrize("dtype", DTYPES)
def test_targeted_edits(dtype):
    Kf = 6
    t = _table(200, Kf, dtype, "ftrl")
    assert t.Kp > Kf
    edits = [("v", (17, 0)), ("v", (18, Kf - 1)), ("w", (3,)), ("s0v", (150, Kf - 1)), ("s0w", (64,)),
             ("s1v", (63, 0)), ("s1w", (199,))]
    for name, idx in edits:
        t = _table(200, Kf, dtype, "ftrl")
        flip(getattr(t, name), *idx)
        _check(t, [idx[0]])
    t = _table(200, Kf, dtype, "ftrl")
    for name, idx in edits:
        flip(getattr(t, name), *idx)
    flip(t.v, 17, 3)  # (a second element of an already changed row)
    _check(t, [i[0] for _, i in edits])
    # pad columns are not looked at
    t = _table(200, Kf, dtype, "ftrl")
    flip(t.v, 40, Kf)
    flip(t.s0v, 41, t.Kp - 1)
    _check(t, [])


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 2 * T + 37])
@pytest.mark.parametrize("case", ["none", "all", "first", "last"])
def test_row_counts(rows, case):
    t = _table(rows, 4, torch.float32, "adagrad")
    if case == "all":
        t.w += 1.0
        want = list(range(rows))
    elif case == "none":
        want = []
    else:
        want = [0 if case == "first" else rows - 1]
        flip(t.s0w, want[0])
    _check(t, want)


def test_shard_offsets():
    V = 3 * 100 + 2  # ranks 0 and 1 own 101 rows, rank 2 owns 100
    for rank in range(3):
        t = _table(Kf=4, world=3, rank=rank, vocab=V)
        assert t.real_rows == (101 if rank < 2 else 100)
        _check(t, [])
        flip(t.v, t.real_rows - 1, 1)
        flip(t.w, 0)
        _check(t, [0, t.real_rows - 1])
    # more allocated rows than real ones: the dead rows are not reported (they are zero, not their init)
    t = FMTable(10, 4, seed=1, rows_multiple=8)
    assert t.rows == 16 and t.real_rows == 10
    _check(t, [])
    # an empty shard
    t = _table(Kf=4, world=3, rank=2, vocab=2)
    assert t.real_rows == 0 and t.rows == 1
    t.w += 1.0
    assert t.changed_rows().numel() == 0


def _model(dtype=torch.float32, opt="adagrad", gbias=False, seed=5, V=5000, Kf=6):
    cfg = FMConfig(vocabulary_size=V, factor_num=Kf, loss_type="logistic", batch_size=64, seed=seed, dtype=dtype,
                   global_bias=gbias, opt=K.OptConfig(opt, lr=0.1))
    return FactorizationMachine(cfg, device="cpu")


def _train(m, steps=3, V=5000):
    seen = []
    for s in range(steps):
        b = random_batch(64, V, max_feats=8, seed=s)
        seen.append(b.ids)
        m.train_step(b)
    return torch.unique(torch.cat(seen))


@pytest.mark.parametrize("dtype,opt", [(torch.float32, "adagrad"), (torch.bfloat16, "ftrl"), (torch.float32, "sgd")])
def test_after_training_steps(dtype, opt):
    m = _model(dtype, opt)
    seen = _train(m)
    got = m.table.changed_rows()
    assert torch.equal(got, torch_changed_rows(m.table))
    assert 0 < got.numel() <= seen.numel()
    assert bool(torch.isin(got, seen).all())


def _shard_file(path):
    return [os.path.join(path, f) for f in sorted(os.listdir(path)) if f.endswith(".safetensors")]


@pytest.mark.parametrize("dtype,opt,gbias", [(torch.float32, "ftrl", True), (torch.bfloat16, "adagrad", False),
                                             (torch.float32, "sgd", False)])
def test_round_trip(tmp_path, monkeypatch, dtype, opt, gbias):
    monkeypatch.setattr(ckpt, "CHUNK_BYTES", 3000)  # (many chunks)
    m = _model(dtype, opt, gbias)
    _train(m)
    n = int(torch_changed_rows(m.table).numel())
    path = ckpt.save_checkpoint(m, str(tmp_path / "sparse"), m.global_step, table_format="sparse")
    dense = ckpt.save_checkpoint(m, str(tmp_path / "dense"), m.global_step)
    meta = ckpt.read_meta(path)
    assert meta["table_format"] == "sparse" and meta["init_seed"] == 5 and meta["init_range"] == 0.01
    assert meta["slot_init"] == [0.1 if opt != "sgd" else 0.0, 0.0]
    (sf,), (df,) = _shard_file(path), _shard_file(dense)
    with safe_open(sf, framework="pt") as f, safe_open(df, framework="pt") as g:
        assert set(f.keys()) == set(g.keys()) | {"rows"}
        assert f.get_slice("rows").get_shape() == [n]
        assert torch.equal(f.get_tensor("rows"), torch_changed_rows(m.table))
        for k in g.keys():
            if k.startswith("gbias"):
                continue
            assert f.get_slice(k).get_shape() == [n] + g.get_slice(k).get_shape()[1:], k
            assert f.get_slice(k).get_dtype() == g.get_slice(k).get_dtype(), k
    assert n < m.table.real_rows / 2 and os.path.getsize(sf) < os.path.getsize(df)

    m2 = _model(dtype, opt, gbias, seed=1234)  # (another config seed: the checkpoint's is used)
    ckpt.restore_checkpoint(m2, path)
    assert_same_state(m.table, m2.table)
    assert m2.global_step == m.global_step and m2.table.init_seed == 5
    if gbias:
        for k in ("gbias", "gbias_s0", "gbias_s1"):
            assert torch.equal(getattr(m, k), getattr(m2, k)), k
    # sparse -> restore -> dense save -> restore
    path2 = ckpt.save_checkpoint(m2, str(tmp_path / "dense2"), m2.global_step)
    m3 = _model(dtype, opt, gbias, seed=99)
    ckpt.restore_checkpoint(m3, path2)
    assert_same_state(m.table, m3.table)


def _shard_model(m, world, rank):
    """A stand-in for rank ``rank`` of a row-sharded model: what save / restore touch."""
    t = FMTable(m.table.vocab_size, m.table.K, world=world, rank=rank, dtype=m.table.dtype, opt=m.table.opt,
                seed=4321, device="cpu")
    return types.SimpleNamespace(table=t, mode="shard", cfg=m.cfg, global_step=0)


@pytest.mark.parametrize("dtype,opt", [(torch.float32, "ftrl"), (torch.bfloat16, "adagrad")])
def test_reshard_round_trip(tmp_path, dtype, opt):
    m = _model(dtype, opt, V=5003)
    _train(m, V=5003)
    one = ckpt.save_checkpoint(m, str(tmp_path / "w1"), m.global_step, table_format="sparse")
    # 1 -> 2
    ranks = [_shard_model(m, 2, r) for r in range(2)]
    gid = torch.arange(5003)
    for r, sm in enumerate(ranks):
        ckpt.restore_checkpoint(sm, one)
        mine = gid[gid % 2 == r]
        for name in ("v", "w", "s0v", "s0w", "s1v", "s1w"):
            a, b = getattr(m.table, name), getattr(sm.table, name)
            if a is not None:
                assert torch.equal(a[mine], b[: mine.numel()]), (r, name)
        assert torch.equal(sm.table.changed_rows(), torch_changed_rows(sm.table))
    # 2 -> 1
    for sm in ranks:
        two = ckpt.save_checkpoint(sm, str(tmp_path / "w2"), sm.global_step, table_format="sparse")
    assert len(_shard_file(two)) == 2
    back = _model(dtype, opt, seed=77, V=5003)
    ckpt.restore_checkpoint(back, two)
    assert_same_state(m.table, back.table)
    assert back.global_step == m.global_step


def test_empty_sparse_checkpoint(tmp_path):
    m = _model()
    path = ckpt.save_checkpoint(m, str(tmp_path / "log"), 0, table_format="sparse")
    with safe_open(_shard_file(path)[0], framework="pt") as f:
        assert f.get_slice("rows").get_shape() == [0] and f.get_slice("v").get_shape() == [0, 6]
    m2 = _model(seed=8)
    ckpt.restore_checkpoint(m2, path)
    assert_same_state(m.table, m2.table)


@pytest.mark.parametrize("dtype,opt", [(torch.float32, "adagrad"), (torch.bfloat16, "ftrl")])
def test_offline_view_equals_dense(tmp_path, monkeypatch, dtype, opt):
    monkeypatch.setattr(ckpt, "CHUNK_BYTES", 5000)
    m = _model(dtype, opt)
    _train(m)
    outs = {}
    for fmt in ("dense", "sparse"):
        path = ckpt.save_checkpoint(m, str(tmp_path / fmt), m.global_step, table_format=fmt)
        ckpt.export_reference_blocks(path, str(tmp_path / f"ref_{fmt}"), 3)
        outs[fmt] = str(tmp_path / f"ref_{fmt}")
    names = sorted(f for f in os.listdir(outs["dense"]) if f.endswith(".npy"))
    assert len(names) == 6 and names == sorted(f for f in os.listdir(outs["sparse"]) if f.endswith(".npy"))
    for f in names:
        want, got = (open(os.path.join(outs[k], f), "rb").read() for k in ("dense", "sparse"))
        assert want == got, f


def test_default_format_unchanged(tmp_path):
    m = _model(opt="ftrl", gbias=True)
    _train(m)
    path = ckpt.save_checkpoint(m, str(tmp_path / "log"), m.global_step)
    n, Kf = m.table.saved_rows, m.table.K
    want = {"w": [n], "v": [n, Kf], "s0w": [n], "s0v": [n, Kf], "s1w": [n], "s1v": [n, Kf], "gbias": [1],
            "gbias_s0": [1], "gbias_s1": [1]}
    with safe_open(_shard_file(path)[0], framework="pt") as f:
        assert {k: f.get_slice(k).get_shape() for k in f.keys()} == want
    assert "table_format" not in ckpt.read_meta(path)
    with pytest.raises(ValueError):
        ckpt.save_checkpoint(m, str(tmp_path / "log"), m.global_step, table_format="bitmap")


# ---------------------------------------------------------------------------------------------
def _write_cfg(d, log, extra=""):
    text = f"""[General]
vocabulary_size = 20000
vocabulary_block_num = 2
factor_num = 4
hash_feature_id = False
log_dir = {log}
device = cpu

[Train]
batch_size = 100
init_value_range = 0.01
factor_lambda = 0.0001
bias_lambda = 0.0001
epoch_num = 1
learning_rate = 0.05
adagrad.initial_accumulator = 0.1
save_steps = 2
loss_type = logistic
shuffle = false
train_files = {d}/train
{extra}

[Predict]
predict_files = {d}/test
"""
    p = os.path.join(d, f"{os.path.basename(log)}.cfg")
    with open(p, "w") as f:
        f.write(text)
    return p


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def test_config_key(tmp_path):
    d = str(tmp_path)
    open(os.path.join(d, "train"), "w").write("1 3:1\n")
    assert load_config(_write_cfg(d, os.path.join(d, "a")), echo=False).checkpoint_format == "dense"
    c = load_config(_write_cfg(d, os.path.join(d, "b"), "checkpoint_format = Sparse"), echo=False)
    assert c.checkpoint_format == "sparse"
    with pytest.raises(ConfigError):
        load_config(_write_cfg(d, os.path.join(d, "c"), "checkpoint_format = bitmap"), echo=False)


def test_cli_train_resume_predict(tmp_path):
    from fast_tffm_amd.data.synthetic import write_libsvm

    d = str(tmp_path)
    write_libsvm(os.path.join(d, "train"), 600, vocab_size=20000, seed=1)
    write_libsvm(os.path.join(d, "test"), 200, vocab_size=20000, seed=2)
    scores = {}
    for fmt in ("dense", "sparse"):
        log = os.path.join(d, f"log_{fmt}")
        cfg = _write_cfg(d, log, f"checkpoint_format = {fmt}")
        rc, out = _run(["train", cfg, "--max-steps", "3"])
        assert rc == 0, out
        last = ckpt.latest_checkpoint(log)
        assert last.endswith("model.ckpt-3")
        with safe_open(_shard_file(last)[0], framework="pt") as f:
            assert ("rows" in f.keys()) == (fmt == "sparse")
        assert json.load(open(os.path.join(last, "meta.json"))).get("table_format", "dense") == fmt
        rc, out = _run(["train", cfg])
        assert rc == 0 and "Restored checkpoint" in out, out
        assert ckpt.latest_checkpoint(log).endswith("model.ckpt-6")
        rc, out = _run(["predict", cfg])
        assert rc == 0, out
        scores[fmt] = open(os.path.join(d, "test_score"), "rb").read()
    assert scores["dense"] == scores["sparse"] and len(scores["dense"].splitlines()) == 200
    assert np.isfinite(np.loadtxt(io.BytesIO(scores["sparse"]))).all()
