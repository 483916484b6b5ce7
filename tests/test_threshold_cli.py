"""Threshold metrics through the CLI on tiny generated data (CPU): ``train`` with ``validation_ap`` prints and logs
its line and stops at ``ap_tolerance``; ``evaluate`` with the ``[Predict]`` keys appends its fields and writes
``<file>_thresholds`` with the oracle's values on ``predict``'s scores, and is unchanged without them."""

import contextlib
import io
import json
import math
import re

import numpy as np
import pytest

from fast_tffm_amd import cli
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.reader import load_file_batch
from fast_tffm_amd.trainer import Trainer
from threshold_oracle import Oracle

VOCAB = 500


def _write_data(path, n, seed):
    """n lines: the label follows feature 0..9 three times out of four (learnable, not separable)."""
    r = np.random.default_rng(seed)
    with open(path, "w") as f:
        for _ in range(n):
            sig = int(r.integers(0, 10))
            y = int((sig < 5) != (r.random() < 0.25))
            feats = [sig] + [int(x) for x in r.integers(60, VOCAB, 4)]
            f.write(f"{y} " + " ".join(f"{k}:1" for k in feats) + "\n")


@pytest.fixture()
def workdir(tmp_path):
    _write_data(tmp_path / "train_0", 600, 1)
    _write_data(tmp_path / "valid_0", 300, 2)
    np.savetxt(tmp_path / "valid_0.w", np.random.default_rng(5).integers(1, 4, 300), fmt="%d")
    return tmp_path


def _write_cfg(workdir, extra_train="", extra_predict="", log_dir="log", validation=True):
    valid = f"validation_files = {workdir}/valid_0\nvalidation_weight_files = {workdir}/valid_0.w\ntolerance = 0.0"
    text = f"""[General]
vocabulary_size = {VOCAB}
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
log_dir = {workdir / log_dir}
save_summaries_steps = 1
device = cpu

[Train]
batch_size = 100
init_value_range = 0.01
factor_lambda = 0.0001
bias_lambda = 0.0001
epoch_num = 2
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
save_steps = 3
loss_type = logistic
train_files = {workdir}/train_0
{valid if validation else ""}
{extra_train}

[Predict]
predict_files = {workdir}/valid_0
{extra_predict}
"""
    p = workdir / "run.cfg"
    p.write_text(text)
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def test_train_prints_and_logs_the_validation_ap(workdir):
    cfg_path = _write_cfg(workdir, "validation_auc = true\nvalidation_ap = true")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    assert rc == 0
    m = re.search(r"^validation loss at step 3: [0-9.]+\nvalidation auc at step 3: [0-9.]+\n"
                  r"validation ap at step 3: ([0-9.]+)$", out, re.M)
    assert m, out
    recs = [json.loads(ln) for ln in open(workdir / "log" / "metrics.jsonl")]
    logged = [r["validation_ap"] for r in recs if "validation_ap" in r]
    assert len(logged) == 1 and "%.8f" % logged[0] == m.group(1)
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.model.global_step == 3
        b = load_file_batch([str(workdir / "valid_0")], [str(workdir / "valid_0.w")], VOCAB, False, 1)
        o = Oracle(tr.model.predict(b).numpy(), b.labels.numpy(), b.weights.numpy())  # the validation weights
        assert 0 < o.ap() < 1 and abs(logged[0] - o.ap()) <= 1e-12 * o.ap()
        assert o.ap() != Oracle(tr.model.predict(b).numpy(), b.labels.numpy()).ap()


def test_ap_line_alone_and_no_line_without_the_key(workdir):
    rc, out = _run(["train", _write_cfg(workdir, "validation_ap = true", log_dir="log_a"), "--max-steps", "3"])
    assert rc == 0 and re.search(r"^validation loss at step 3: [0-9.]+\nvalidation ap at step 3: [0-9.]+$", out, re.M)
    assert "validation auc" not in out
    rc, out = _run(["train", _write_cfg(workdir, log_dir="log_b"), "--max-steps", "3"])
    assert rc == 0 and "validation ap" not in out and "Average precision" not in out
    assert "validation_ap" not in open(workdir / "log_b" / "metrics.jsonl").read()


def test_ap_tolerance_stops_at_first_validation(workdir):
    cfg_path = _write_cfg(workdir, "validation_ap = true\nap_tolerance = 0.0", log_dir="log_es")
    rc, out = _run(["train", cfg_path])
    assert rc == 0
    assert re.search(r"validation ap at step 3: [0-9.]+\nAverage precision on validation data set is above "
                     r"tolerance. Training completed.", out), out
    assert "-- Global Step: 4;" not in out


def _f32(v) -> str:
    return str(np.float32(v))


def test_evaluate_appends_the_fields_and_writes_the_thresholds_file(workdir):
    plain = _write_cfg(workdir)
    assert _run(["train", plain, "--max-steps", "5"])[0] == 0
    assert _run(["predict", plain])[0] == 0
    path = str(workdir / "valid_0")
    scores = np.loadtxt(path + "_score", dtype=np.float32)
    rc, before = _run(["evaluate", plain])
    assert rc == 0 and re.search(r"^evaluate \S+valid_0: examples 300 loss [0-9.]+ auc [0-9.]+$", before, re.M)
    assert not (workdir / "valid_0_thresholds").exists()

    cfg_path = _write_cfg(workdir, extra_predict="precision_targets = 0.5, 0.999\nrecall_targets = 0.8")
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0
    line = [ln for ln in out.splitlines() if ln.startswith("evaluate ")][0]
    base = [ln for ln in before.splitlines() if ln.startswith("evaluate ")][0]
    assert line.startswith(base + " ap ")  # the fields come at the end of today's line
    b = load_file_batch([path], None, VOCAB, False, 1)
    o = Oracle(scores, b.labels.numpy())  # unit weights
    ks, ki = o.ks()
    f1, fi = o.best_f1()
    p5, p999, r8 = o.at_precision(0.5), o.at_precision(0.999), o.at_recall(0.8)
    assert p5 is not None and r8 is not None
    want = " ap %.8f ks %.8f best_f1 %.8f recall@p0.5 %.8f recall@p0.999 %.8f precision@r0.8 %.8f" % (
        o.ap(), ks, f1, o.recall(p5), float("nan") if p999 is None else o.recall(p999), o.precision(r8))
    assert line == base + want, (line, want)

    def row(kind, target, i):
        if i is None:
            return "%s %s nan nan nan nan nan nan" % (kind, target)
        return " ".join([kind, target, _f32(o.thr[i]), _f32(o.precision(i)), _f32(o.recall(i)), _f32(o.f1(i)),
                         str(o.tp[i]), str(o.fp[i])])

    assert open(path + "_thresholds").read().splitlines() == [
        row("ks", "-", ki), row("best_f1", "-", fi), row("precision", "0.5", p5), row("precision", "0.999", p999),
        row("recall", "0.8", r8)]
    assert np.array_equal(np.loadtxt(path + "_score", dtype=np.float32), scores)  # predict's output is left alone

    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        r = tr.evaluate()[path]
    assert {"ap", "ks", "best_f1", "recall@p0.5", "recall@p0.999", "precision@r0.8", "thresholds_file"} <= set(r)
    assert r["ap"] == pytest.approx(o.ap(), rel=1e-12) and r["ks"] == ks and r["best_f1"] == f1
    assert r["recall@p0.5"] == o.recall(p5) and r["precision@r0.8"] == o.precision(r8)
    assert math.isnan(r["recall@p0.999"]) == (p999 is None)


def test_threshold_metrics_key_without_targets(workdir):
    cfg_path = _write_cfg(workdir, extra_predict="threshold_metrics = true")
    assert _run(["train", cfg_path, "--max-steps", "3"])[0] == 0
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0 and re.search(r"auc [0-9.]+ ap [0-9.]+ ks [0-9.]+ best_f1 [0-9.]+$", out, re.M), out
    rows = open(str(workdir / "valid_0_thresholds")).read().splitlines()
    assert [r.split()[0] for r in rows] == ["ks", "best_f1"] and all(len(r.split()) == 8 for r in rows)


def test_config_errors(workdir):
    for extra in ("ap_tolerance = 0.5", "validation_ap = false\nap_tolerance = 0.5"):
        with pytest.raises(ConfigError, match="ap_tolerance needs validation_ap"):
            load_config(_write_cfg(workdir, extra), echo=False)
    with pytest.raises(ConfigError, match="ap_tolerance needs validation_ap"):
        load_config(_write_cfg(workdir, "validation_ap = true\nap_tolerance = 0.5", validation=False), echo=False)
    for key in ("precision_targets", "recall_targets"):
        for bad in ("0", "1.5", "0.1,0.2,0.3,0.4,0.5", "high", "-0.5"):
            with pytest.raises(ConfigError, match=key):
                load_config(_write_cfg(workdir, extra_predict=f"{key} = {bad}"), echo=False)
    c = load_config(_write_cfg(workdir, extra_predict="recall_targets = 0.9, 1"), echo=False)
    assert c.threshold_metrics and c.recall_targets == [0.9, 1.0] and c.precision_targets == []
    c = load_config(_write_cfg(workdir), echo=False)
    assert not c.threshold_metrics and not c.validation_ap and c.ap_tolerance is None
