"""Validation AUC through the CLI on the golden sample (CPU): the ``validation auc at step`` line after the
unchanged loss line, metrics.jsonl, the AUC early stop, and no AUC output without the key."""

import contextlib
import io
import json
import os
import re

import pytest

from auc_oracle import oracle_stats, value_of
from fast_tffm_amd import cli
from fast_tffm_amd.config import load_config
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.trainer import Trainer


def _copy_head(src, dst, n):
    with open(src, "rb") as f, open(dst, "wb") as g:
        for i, line in enumerate(f):
            if i >= n:
                break
            g.write(line)


@pytest.fixture()
def workdir(tmp_path, ref_data_dir):
    d = tmp_path / "data"
    d.mkdir()
    for i in range(2):
        _copy_head(os.path.join(ref_data_dir, f"train_{i}"), d / f"train_{i}", 3000)
        _copy_head(os.path.join(ref_data_dir, f"weight_{i}"), d / f"weight_{i}", 3000)
    _copy_head(os.path.join(ref_data_dir, "test_0"), d / "test_0", 1500)
    return tmp_path


def _write_cfg(workdir, extra_train="", log_dir="log", device="cpu"):
    text = f"""[General]
vocabulary_size = 200000
vocabulary_block_num = 4
factor_num = 8
hash_feature_id = False
log_dir = {workdir / log_dir}
save_summaries_steps = 1
device = {device}

[Train]
batch_size = 1000
init_value_range = 0.01
factor_lambda = 0.0001
bias_lambda = 0.0001
epoch_num = 2
learning_rate = 0.05
adagrad.initial_accumulator = 0.1
save_steps = 3
loss_type = logistic
train_files = {workdir}/data/train_*
weight_files = {workdir}/data/weight_*
validation_files = {workdir}/data/test_0
tolerance = 0.0
{extra_train}
"""
    p = workdir / "run.cfg"
    p.write_text(text)
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def test_validation_auc_line_metrics_and_value(workdir):
    cfg_path = _write_cfg(workdir, "validation_auc = true")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    assert rc == 0
    m = re.search(r"^validation loss at step 3: ([0-9.]+)\nvalidation auc at step 3: ([0-9.]+)$", out, re.M)
    assert m, out
    recs = [json.loads(ln) for ln in open(workdir / "log" / "metrics.jsonl")]
    logged = [r["validation_auc"] for r in recs if "validation_auc" in r]
    assert len(logged) == 1 and "%.8f" % logged[0] == m.group(2)
    assert [r["step"] for r in recs if "validation_loss" in r] == [3]

    # the same model state, restored: validation_metrics against the oracle on the predict scores
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.model.global_step == 3
        vb = tr.load_validation()
        loss, auc = tr.validation_metrics(vb)
        assert loss == tr.validation_loss(vb) and "%.8f" % loss == m.group(1)
        scores = tr.model.predict(vb)
        want = oracle_stats(scores.numpy(), vb.labels.numpy())
        assert (want[1], want[2]) == (310, 1190)  # test_0's 1500-line head
        assert K.auc(scores, vb.labels).stats() == want
        assert auc == value_of(want) and "%.8f" % auc == m.group(2)
        assert 0.0 < auc < 1.0


def test_auc_tolerance_stops_at_first_validation(workdir):
    cfg_path = _write_cfg(workdir, "validation_auc = true\nauc_tolerance = 0.0", log_dir="log_es")
    rc, out = _run(["train", cfg_path])
    assert rc == 0
    assert re.search(r"validation auc at step 3: [0-9.]+\nAUC on validation data set is above tolerance. "
                     r"Training completed.", out), out
    assert "Loss on validation data set is below tolerance" not in out
    assert "-- Global Step: 4;" not in out


def test_no_auc_output_without_the_key(workdir):
    cfg_path = _write_cfg(workdir, log_dir="log_off")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    assert rc == 0 and re.search(r"validation loss at step 3: [0-9.]+", out)
    assert "validation auc" not in out and "validation_auc" not in out and "AUC" not in out
    assert "validation_auc" not in open(workdir / "log_off" / "metrics.jsonl").read()
