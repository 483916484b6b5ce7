"""Exact per-feature attributions on the CPU: the kernel against the fp64 oracle, the sum identity against
``fm_forward``, ``feature_importance`` against a numpy group-by, ``run.py explain`` end to end, two gloo
ranks (row-sharded, replicated) against one process, and ``ServingModel.explain``."""

import contextlib
import io
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from explain_oracle import (ROWS, check_bias, check_case, check_importance, check_sum_identity, example_sums,
                            explain_oracle, group_by, make_batch, make_table, table_f64)
from fast_tffm_amd import cli
from fast_tffm_amd.ops import kernels as K

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _t(a):
    return None if a is None else torch.from_numpy(a)


@pytest.mark.parametrize("with_vals", [True, False], ids=["vals", "novals"])
@pytest.mark.parametrize("Kf", [1, 10, 64])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_cpu_kernel_against_oracle(dtype, Kf, with_vals):
    off, rows, vals = make_batch(seed=Kf, with_vals=with_vals)
    v, w, Kp = make_table(DTYPES[dtype], Kf)
    what = f"cpu {dtype} k{Kf}"
    contrib, pred = K.fm_explain(_t(off), _t(rows), _t(vals), v, w, Kp, threads=2)
    assert contrib.shape == (rows.size,) and pred.shape == (off.size - 1,)
    c, tol = check_case(off, rows, vals, v, w, Kp, contrib, pred, what=what)
    # the forward's score obeys the same identity
    fo = K.fm_forward(_t(off), _t(rows), _t(vals), v, w, Kp, want_r1=False, threads=2)
    check_sum_identity(off, c, tol, fo.pred, what + " fm_forward")
    bias = torch.tensor([0.375])
    _, pred_b = K.fm_explain(_t(off), _t(rows), _t(vals), v, w, Kp, bias=bias, threads=2)
    check_bias(off, pred_b, pred, 0.375, what)
    fo_b = K.fm_forward(_t(off), _t(rows), _t(vals), v, w, Kp, want_r1=False, threads=2, bias=bias)
    check_bias(off, fo_b.pred, fo.pred, 0.375, what + " fm_forward")


def test_outputs_into_given_buffers_and_argument_checks(monkeypatch):
    monkeypatch.setattr(K, "_DEBUG", True)  # (index range checks)
    off, rows, vals = make_batch(seed=3)
    v, w, Kp = make_table(torch.float32, 10)
    cbuf, pbuf = torch.empty(rows.size), torch.empty(off.size - 1)
    contrib, pred = K.fm_explain(_t(off), _t(rows), _t(vals), v, w, Kp, contrib=cbuf, pred=pbuf)
    assert contrib.data_ptr() == cbuf.data_ptr() and pred.data_ptr() == pbuf.data_ptr()
    with pytest.raises(ValueError):
        K.fm_explain(_t(off), _t(rows).long(), _t(vals), v, w, Kp)
    with pytest.raises(ValueError):
        K.fm_explain(_t(off), _t(rows), _t(vals), v, w[: ROWS - 1], Kp)
    with pytest.raises(ValueError):
        K.fm_explain(_t(off), _t(rows + ROWS), _t(vals), v, w, Kp)  # (row range)
    with pytest.raises(ValueError):
        K.fm_explain(_t(off), _t(rows), _t(vals), v.t().contiguous().t(), w, Kp)


def test_feature_importance_against_group_by():
    rng = np.random.default_rng(5)
    ids = np.minimum(rng.zipf(1.3, 5000), 400).astype(np.int32) - 1
    c = torch.from_numpy(rng.normal(size=5000).astype(np.float32))
    dd = K.dedup(_t(ids), want_perm=True)
    check_importance(ids, c.numpy(), K.feature_importance(c, dd))
    empty = K.feature_importance(torch.empty(0), K.dedup(torch.empty(0, dtype=torch.int32), want_perm=True))
    assert [t.numel() for t in empty] == [0, 0, 0, 0]


# ---- CLI ------------------------------------------------------------------------------------------------
LINES = 200


def _copy_head(src, dst, n):
    with open(src, "rb") as f, open(dst, "wb") as g:
        for i, line in enumerate(f):
            if i >= n:
                break
            g.write(line)


def _write_cfg(workdir, mode="auto", extra=""):
    text = f"""[General]
vocabulary_size = 5003
vocabulary_block_num = 2
factor_num = 6
hash_feature_id = True
log_dir = {workdir}/log
device = cpu
{extra}

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
    """A tiny model trained for a few steps through the CLI, then ``predict`` and ``explain`` on test_0's head."""
    wd = str(tmp_path_factory.mktemp("explain_cli"))
    os.makedirs(os.path.join(wd, "data"))
    _copy_head(os.path.join(ref_data_dir, "train_0"), os.path.join(wd, "data", "train_0"), 600)
    _copy_head(os.path.join(ref_data_dir, "test_0"), os.path.join(wd, "data", "test_0"), LINES)
    cfg = _write_cfg(wd, extra="global_bias = true")
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["train", cfg, "--max-steps", "4"]) == 0
        assert cli.main(["predict", cfg]) == 0
        assert cli.main(["explain", cfg]) == 0
    return wd, cfg


def _read_contrib(path):
    out = []
    for ln in open(path):
        t = ln.split()
        out.append((t[0], [tok.split(":") for tok in t[1:]]))
    return out


def _model_and_batch(cfg_path):
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.data.reader import load_file_batch
    from fast_tffm_amd.trainer import Trainer

    cfg = load_config(cfg_path, echo=False)
    tr = Trainer(cfg, None, printer=lambda *a, **k: None)
    assert tr.restore()
    b = load_file_batch(cfg.predict_files, None, cfg.vocabulary_size, cfg.hash_feature_id, cfg.parse_threads)
    return tr, b


def test_cli_contrib_file(trained):
    wd, cfg = trained
    test0 = os.path.join(wd, "data", "test_0")
    lines = _read_contrib(test0 + "_contrib")
    scores = open(test0 + "_score").read().split()
    assert len(lines) == LINES == len(scores)
    tr, b = _model_and_batch(cfg)
    with tr:
        bias = float(tr.model.gbias)
        assert bias != 0.0
        t = tr.model.table
        off = b.offsets.numpy()
        ids = b.ids.numpy()
        vals = None if b.vals is None else b.vals.numpy()
        V, wv, n2 = table_f64(t.v, t.w, t.Kp)
        c, tol = explain_oracle(off, ids, vals, V, wv, n2)
    for i, (score, toks) in enumerate(lines):
        assert score == scores[i]                                   # the score predict writes
        assert [int(k) for k, _ in toks] == ids[off[i]:off[i + 1]].tolist()  # ids in input order
        got = np.array([np.float32(x) for _, x in toks], dtype=np.float64)
        assert (np.abs(got - c[off[i]:off[i + 1]]) <= tol[off[i]:off[i + 1]]).all()
    # the tokens add up to the score less the bias
    sums = np.array([sum(np.float64(np.float32(x)) for _, x in toks) for _, toks in lines])
    sc = np.array([np.float32(s) for s in scores], dtype=np.float64)
    gap = np.abs(sc - bias - sums)
    print("max token-sum gap / bound =", float((gap / np.maximum(example_sums(off, tol), 1e-300)).max()))
    assert (gap <= example_sums(off, tol)).all()


def test_cli_top_and_importance(trained):
    wd, cfg = trained
    test0 = os.path.join(wd, "data", "test_0")
    full = _read_contrib(test0 + "_contrib")
    imp = [ln.split() for ln in open(test0 + "_importance")]
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["explain", cfg, "--top", "3"]) == 0
    top = _read_contrib(test0 + "_contrib")
    assert [ln.split() for ln in open(test0 + "_importance")] == imp   # --top does not touch the importance
    for (score, toks), (score3, toks3) in zip(full, top):
        assert score == score3
        a = np.abs(np.array([np.float32(x) for _, x in toks]))
        order = sorted(range(len(toks)), key=lambda j: (-a[j], j))[:3]   # descending |c|, then position
        assert toks3 == [toks[j] for j in order] and len(toks3) == min(3, len(toks))
    # importance: id count mean_abs mean, by descending sum |c| then ascending id; counts sum to nnz
    ids = np.array([int(k) for _, toks in full for k, _ in toks])
    c = np.array([np.float32(x) for _, toks in full for _, x in toks])
    uniq, cnt, sa, sm = group_by(ids, c)
    assert sum(int(r[1]) for r in imp) == ids.size and len(imp) == uniq.size
    want = np.lexsort((uniq, -sa))
    # (the file's sums come from the unrounded fp32 contributions, the same numbers the tokens print exactly)
    assert [int(r[0]) for r in imp] == uniq[want].tolist()
    assert [int(r[1]) for r in imp] == cnt[want].tolist()
    assert [r[2] for r in imp] == [str(np.float32(sa[k] / cnt[k])) for k in want]
    assert [r[3] for r in imp] == [str(np.float32(sm[k] / cnt[k])) for k in want]


# ---- two row-sharded ranks --------------------------------------------------------------------------------
def _shard_worker(rank, world, port, cfg_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    with Trainer(load_config(cfg_path, echo=False), ctx, printer=lambda *a, **k: None) as tr:
        tr.explain()
    fmdist.shutdown()


@pytest.mark.parametrize("mode", ["shard", "dp"])
def test_two_ranks_equal_one_process(trained, mode):
    """Two gloo ranks, row-sharded (fp32 table, fp32 wire) or replicated: rank 0's files equal the
    single-process ones exactly."""
    from ports import free_port

    wd, cfg = trained
    test0 = os.path.join(wd, "data", "test_0")
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["explain", cfg]) == 0
    want = open(test0 + "_contrib").read(), open(test0 + "_importance").read()
    os.remove(test0 + "_contrib")
    os.remove(test0 + "_importance")
    cfg2 = _write_cfg(wd, mode=mode, extra="global_bias = true")
    mp.spawn(_shard_worker, args=(2, free_port(), cfg2), nprocs=2, join=True)
    assert open(test0 + "_contrib").read() == want[0]
    got_imp = [ln.split() for ln in open(test0 + "_importance")]
    want_imp = [ln.split() for ln in want[1].splitlines()]
    # counts and order are exact; the merged fp64 sums may differ from one process's in the last place
    assert [r[:2] for r in got_imp] == [r[:2] for r in want_imp]
    for g, w_ in zip(got_imp, want_imp):
        assert abs(float(g[2]) - float(w_[2])) <= 2.0 ** -22 * abs(float(w_[2]))
        assert abs(float(g[3]) - float(w_[3])) <= 2.0 ** -22 * abs(float(w_[2]))


# ---- serving ----------------------------------------------------------------------------------------------
def test_serving_explain_equals_model_explain(trained, tmp_path):
    from fast_tffm_amd.data.batch import Batch
    from fast_tffm_amd.serving import ServingModel, export_model, parse_serving_lines
    from fast_tffm_amd.utils.checkpoint import latest_checkpoint

    wd, cfg = trained
    tr, _ = _model_and_batch(cfg)
    with tr:
        export = str(tmp_path / "export")
        export_model(latest_checkpoint(tr.cfg.log_dir), export, vocabulary_block_num=2, hash_feature_id=True,
                     loss_type="logistic")
        lines = ["3:1 17:0.5 3:2", "4999:1", "12:1 13:1 14:-1.5 5002:0.25"]
        sm = ServingModel.load(export, device="cpu")
        scores, off, ids, contrib = sm.explain(lines)
        o, i, v = parse_serving_lines(lines, 5003, True)
        b = Batch(torch.zeros(3), o, i, v, None, int(o[-1]))
        c2, p2 = tr.model.explain(b)
        assert np.array_equal(off, o.numpy()) and np.array_equal(ids, i.numpy().astype(ids.dtype))
        assert np.array_equal(contrib, c2.numpy()) and np.array_equal(scores, p2.numpy())
        assert contrib.dtype == np.float32 and contrib.shape == (int(o[-1]),) and scores.shape == (3,)
