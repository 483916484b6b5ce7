"""Calibration through the CLI on tiny generated data (CPU): ``calibrate`` fits the checkpoint's scores on the
validation files, writes ``calibration.json`` into the checkpoint's directory and the reliability table into the
log directory, both as the oracle fit of ``predict``'s scores gives them; ``predict --calibrated`` adds
``<file>_prob`` and leaves ``<file>_score`` alone; the serving export carries the calibrator."""

import contextlib
import glob
import io
import json
import math
import os
import re

import numpy as np
import pytest
import torch

import isotonic_oracle as O
from fast_tffm_amd import cli
from fast_tffm_amd.calibration import Calibrator
from fast_tffm_amd.serving import ServingModel

VOCAB = 500


def _write_data(path, wpath, n, seed):
    """n lines: the label follows feature 0..9 three times out of four (learnable, not separable)."""
    r = np.random.default_rng(seed)
    with open(path, "w") as f, open(wpath, "w") as w:
        for _ in range(n):
            sig = int(r.integers(0, 10))
            y = int((sig < 5) != (r.random() < 0.25))
            feats = [sig, 10 + int(r.integers(0, 50))] + [int(x) for x in r.integers(60, VOCAB, 4)]
            f.write(f"{y} " + " ".join(f"{k}:1" for k in feats) + "\n")
            w.write(f"{int(r.integers(1, 9)) / 4}\n")


@pytest.fixture()
def workdir(tmp_path):
    _write_data(tmp_path / "train_0", tmp_path / "train_0.w", 600, 1)
    _write_data(tmp_path / "valid_0", tmp_path / "valid_0.w", 300, 2)
    return tmp_path


def _write_cfg(workdir, log_dir="log", loss="logistic", validation=True, weights=False):
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
loss_type = {loss}
train_files = {workdir}/train_0
{f"validation_files = {workdir}/valid_0" if validation else ""}
{"tolerance = 0.0" if validation else ""}
{f"validation_weight_files = {workdir}/valid_0.w" if validation and weights else ""}

[Predict]
predict_files = {workdir}/valid_0
"""
    p = workdir / f"run_{log_dir}.cfg"
    p.write_text(text)
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def _newest_ckpt(log_dir):
    return max(glob.glob(os.path.join(log_dir, "model.ckpt-*")), key=lambda p: int(p.rsplit("-", 1)[1]))


def _labels(path):
    return np.array([float(ln.split()[0]) for ln in open(path)], np.float32)


LINE = re.compile(r"^calibrate: examples (\d+) blocks (\d+) loss ([0-9.]+) -> ([0-9.]+) ratio ([0-9.]+) -> 1\.00000000 "
                  r"\(in-sample\)$", re.M)


@pytest.mark.parametrize("weights", [False, True])
def test_calibrate_then_predict_calibrated(workdir, weights):
    cfg = _write_cfg(workdir, weights=weights)
    valid = str(workdir / "valid_0")
    assert _run(["train", cfg, "--max-steps", "5"])[0] == 0
    assert _run(["predict", cfg])[0] == 0
    plain = open(valid + "_score", "rb").read()
    assert not os.path.exists(valid + "_prob")
    scores = np.array([float(x) for x in plain.split()], np.float32)
    labels = _labels(valid)
    w = np.array([float(x) for x in open(valid + ".w")], np.float32) if weights else None

    rc, out = _run(["calibrate", cfg])
    assert rc == 0
    m = LINE.search(out)
    assert m, out
    f = O.fit(scores, labels, w)
    assert int(m.group(1)) == 300 and int(m.group(2)) == len(f["v"]) > 2
    ckpt = _newest_ckpt(workdir / "log")
    assert sorted(glob.glob(str(workdir / "log" / "model.ckpt-*" / "calibration.json"))) == [
        os.path.join(ckpt, "calibration.json")]
    cal = Calibrator.load(os.path.join(ckpt, "calibration.json"))
    ox, oy = O.calibrator(f)
    assert np.array_equal(cal.x.numpy(), ox) and np.array_equal(cal.y.numpy(), oy)
    meta = json.load(open(os.path.join(ckpt, "meta.json")))
    assert cal.meta["global_step"] == meta["global_step"] and cal.meta["examples"] == 300
    assert cal.meta["blocks"] == len(f["v"]) and cal.meta["weighted"] is weights
    assert cal.meta["positives"] == float(sum(f["Y"])) and cal.meta["total_weight"] == float(sum(f["W"]))
    # the reliability table: score_lo score_hi probability weight positives
    rows = [ln.split() for ln in open(workdir / "log" / "calibration_blocks.txt")]
    assert len(rows) == len(f["v"])
    for b, r in enumerate(rows):
        assert r[:3] == [str(np.float32(f["lo"][b])), str(np.float32(f["hi"][b])), str(np.float32(float(f["v"][b])))]
        assert float(r[3]) == float(f["W"][b]) and float(r[4]) == float(f["Y"][b])
    # the line's figures: the loss of the fitted values is below the model's, which the trainer reports as
    # the weighted loss sum over the number of examples
    w64 = np.ones(300) if w is None else w.astype(np.float64)
    s64, y64 = scores.astype(np.float64), (labels > 0).astype(np.float64)
    before = float((w64 * (np.logaddexp(0, s64) - y64 * s64)).sum() / 300)
    fv = np.clip(f["fitted"], 1e-300, 1 - 1e-16)
    inner = (f["fitted"] > 0) & (f["fitted"] < 1)
    after = float(-(w64 * (y64 * np.log(fv) + (1 - y64) * np.log1p(-fv)))[inner].sum() / 300)
    ratio = float((w64 / (1 + np.exp(-s64))).sum() / (w64 * y64).sum())
    assert abs(float(m.group(3)) - before) <= 2e-6 and abs(float(m.group(4)) - after) <= 1e-7
    assert abs(float(m.group(5)) - ratio) <= 1e-7 and float(m.group(4)) < float(m.group(3))

    rc, out = _run(["predict", cfg, "--calibrated"])
    assert rc == 0
    assert open(valid + "_score", "rb").read() == plain
    probs = np.array([np.float32(x) for x in open(valid + "_prob").read().split()], np.float32)
    O.check_apply(probs, scores, ox, oy)
    assert probs.shape == (300,) and (probs >= 0).all() and (probs <= 1).all()
    # in sample, every score sits inside a block: the probability is the fitted value
    assert np.array_equal(probs, f["fitted"].astype(np.float32))


def test_refusals(workdir):
    cfg = _write_cfg(workdir, log_dir="log_r")
    assert _run(["train", cfg, "--max-steps", "3"])[0] == 0
    rc, out = _run(["predict", cfg, "--calibrated"])
    assert rc == 1 and "no calibration.json" in out and "calibrate" in out
    assert not os.path.exists(str(workdir / "valid_0") + "_prob")
    rc, out = _run(["calibrate", _write_cfg(workdir, log_dir="log_r", validation=False)])
    assert rc == 1 and "validation_files" in out
    mse = _write_cfg(workdir, log_dir="log_m", loss="mse")
    assert _run(["train", mse, "--max-steps", "3"])[0] == 0
    rc, out = _run(["calibrate", mse])
    assert rc == 1 and "loss_type = logistic" in out and "mse" in out
    assert not glob.glob(str(workdir / "log_m" / "model.ckpt-*" / "calibration.json"))


def test_serving_export_carries_the_calibrator(workdir):
    cfg = _write_cfg(workdir, log_dir="log_s")
    assert _run(["train", cfg, "--max-steps", "5"])[0] == 0
    assert _run(["generate", cfg, "--export_path", str(workdir / "export_plain")])[0] == 0
    assert _run(["calibrate", cfg])[0] == 0
    assert _run(["generate", cfg, "--export_path", str(workdir / "export_cal")])[0] == 0
    lines = [ln.split(None, 1)[1].strip() for ln in open(workdir / "valid_0")][:64]
    plain = ServingModel.load(str(workdir / "export_plain"), "cpu")
    assert plain.calibrator is None
    with pytest.raises(RuntimeError, match="calibration.json"):
        plain.predict_proba(lines)
    sm = ServingModel.load(str(workdir / "export_cal"), "cpu")
    cal = Calibrator.load(os.path.join(_newest_ckpt(workdir / "log_s"), "calibration.json"))
    assert torch.equal(sm.calibrator.x, cal.x) and torch.equal(sm.calibrator.y, cal.y)
    scores = sm.predict(lines)
    assert np.array_equal(scores, plain.predict(lines))
    got = sm.predict_proba(lines)
    assert got.dtype == np.float32 and np.array_equal(got, cal(scores).numpy())
    assert (np.diff(got[np.argsort(scores, kind="stable")]) >= 0).all()


def test_calibrator_round_trip(tmp_path):
    x = np.array([-np.inf, -1.5, -1.25, 1e-45, 0.1, 0.1, 3e38, np.inf], np.float32)
    y = np.array([0.0, 0.0, 1 / 3, 1 / 3, 0.7, 0.7, 1.0, 1.0], np.float32)
    cal = Calibrator(x, y, {"examples": 9, "global_step": 4, "weighted": False})
    back = Calibrator.load(cal.save(str(tmp_path / "c.json")))
    assert np.array_equal(back.x.numpy(), x) and np.array_equal(back.y.numpy(), y) and back.meta == cal.meta
    assert back.blocks == 4
    got = back(np.array([-2, 0.05, math.nan, np.inf], np.float32)).tolist()
    assert got[0] == 0.0 and got[1] > y[2] and got[1] < y[4] and math.isnan(got[2]) and got[3] == 1.0
    for bad in ((x[::-1].copy(), y), (x[:3], y[:3]), (x, y[::-1].copy())):
        with pytest.raises(ValueError):
            Calibrator(*bad)
