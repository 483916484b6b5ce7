"""DeLong intervals and the paired test through the CLI on tiny generated data (CPU): two runs of different length,
the first one's ``predict`` scores as the second's ``baseline_score_files``; ``evaluate`` appends the fields with
the oracle's values and is unchanged without the keys."""

import contextlib
import io
import re

import numpy as np
import pytest

from fast_tffm_amd import cli
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.reader import load_file_batch
from fast_tffm_amd.trainer import Trainer
from delong_oracle import Oracle

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


def _write_cfg(workdir, log_dir, extra_predict="", name="run.cfg"):
    text = f"""[General]
vocabulary_size = {VOCAB}
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
log_dir = {workdir / log_dir}
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

[Predict]
predict_files = {workdir}/valid_0
{extra_predict}
"""
    p = workdir / name
    p.write_text(text)
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def _line(out: str) -> str:
    return [ln for ln in out.splitlines() if ln.startswith("evaluate ")][0]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two trained runs (2 and 6 steps), each one's ``predict`` scores kept beside the data, and today's
    ``evaluate`` line of the second."""
    wd = tmp_path_factory.mktemp("delong_cli")
    _write_data(wd / "train_0", 600, 1)
    _write_data(wd / "valid_0", 300, 2)
    scores = {}
    for log_dir, steps in (("log_a", 2), ("log_b", 6)):
        cfg = _write_cfg(wd, log_dir)
        assert _run(["train", cfg, "--max-steps", str(steps)])[0] == 0
        assert _run(["predict", cfg])[0] == 0
        (wd / "valid_0_score").rename(wd / f"{log_dir}_score")
        scores[log_dir] = np.loadtxt(wd / f"{log_dir}_score", dtype=np.float32)
    rc, plain = _run(["evaluate", _write_cfg(wd, "log_b")])
    assert rc == 0
    labels = load_file_batch([str(wd / "valid_0")], None, VOCAB, False, 1).labels.numpy()
    return wd, scores, labels, _line(plain)


def test_line_without_the_keys_is_todays(runs):
    _, _, _, plain = runs
    assert re.fullmatch(r"evaluate \S+valid_0: examples 300 loss [0-9.]+ auc [0-9.]+", plain)


def test_evaluate_prints_the_oracles_values(runs):
    wd, scores, labels, plain = runs
    assert not np.array_equal(scores["log_a"], scores["log_b"])
    cfg = _write_cfg(wd, "log_b", f"auc_interval = 0.9\nbaseline_score_files = {wd}/log_a_score")
    rc, out = _run(["evaluate", cfg])
    assert rc == 0
    o = Oracle(scores["log_b"], labels, scores["log_a"])
    lo, hi = o.interval(0.9)
    d, se, z, p = o.difference()
    want = " auc_se %.8f auc_lo %.8f auc_hi %.8f" % (float(o.cov()) ** 0.5, lo, hi)
    want += " baseline_auc %.8f auc_diff %.8f diff_se %.8f z %.4f p %.6g" % (float(o.theta("b")), d, se, z, p)
    assert _line(out) == plain + want
    assert 0 < lo < float(o.theta()) < hi < 1 and se > 0 and 0 < p <= 1
    with Trainer(load_config(cfg, echo=False), None, printer=lambda *a, **k: None) as tr:
        r = tr.evaluate()[str(wd / "valid_0")]
    assert (r["auc_se"], r["auc_lo"], r["auc_hi"]) == (float(o.cov()) ** 0.5, lo, hi)
    assert (r["baseline_auc"], r["auc_diff"], r["diff_se"], r["z"], r["p"]) == (float(o.theta("b")), d, se, z, p)
    assert r["auc"] == float(o.theta())


def test_own_scores_as_baseline(runs):
    wd, _, _, plain = runs
    rc, out = _run(["evaluate", _write_cfg(wd, "log_b", f"baseline_score_files = {wd}/log_b_score")])
    assert rc == 0
    line = _line(out)
    assert line.startswith(plain + " baseline_auc ") and "auc_se" not in line  # no interval without its key
    assert line.endswith(" auc_diff 0.00000000 diff_se 0.00000000 z 0.0000 p 1")
    assert line.split()[line.split().index("baseline_auc") + 1] == plain.split()[-1]


def test_interval_alone(runs):
    wd, scores, labels, plain = runs
    rc, out = _run(["evaluate", _write_cfg(wd, "log_b", "auc_interval = 0.95")])
    assert rc == 0
    o = Oracle(scores["log_b"], labels)
    assert _line(out) == plain + " auc_se %.8f auc_lo %.8f auc_hi %.8f" % (float(o.cov()) ** 0.5, *o.interval(0.95))


def test_wrong_counts_and_levels(runs):
    wd, scores, _, _ = runs
    with pytest.raises(ConfigError, match="baseline score files"):  # two files for one predict file
        load_config(_write_cfg(wd, "log_b", f"baseline_score_files = {wd}/log_a_score, {wd}/log_b_score"), echo=False)
    with pytest.raises(ConfigError, match="baseline score files"):  # no such file
        load_config(_write_cfg(wd, "log_b", f"baseline_score_files = {wd}/nothing_score"), echo=False)
    for bad in ("0", "1", "1.5", "-0.1", "wide", "nan"):
        with pytest.raises(ConfigError, match="auc_interval"):
            load_config(_write_cfg(wd, "log_b", f"auc_interval = {bad}"), echo=False)
    short = wd / "short_score"
    short.write_text("".join(f"{s}\n" for s in scores["log_a"][:-1]))
    with pytest.raises(ValueError, match="299 lines"):
        _run(["evaluate", _write_cfg(wd, "log_b", f"baseline_score_files = {short}")])
    c = load_config(_write_cfg(wd, "log_b"), echo=False)
    assert c.auc_interval is None and c.baseline_score_files == []
