"""Grouped AUC through the CLI on tiny generated data (CPU): ``train`` with ``validation_gauc`` prints and logs
its line and stops at ``gauc_tolerance``; ``evaluate`` reports the loss and AUC that ``validation_metrics``
gives on the same file, writes ``<file>_gauc`` as the oracle orders it and leaves ``predict``'s output alone."""

import contextlib
import io
import json
import re

import numpy as np
import pytest

from gauc_oracle import brute_groups, summary
from fast_tffm_amd import cli
from fast_tffm_amd.config import load_config
from fast_tffm_amd.data.groups import load_group_files
from fast_tffm_amd.data.reader import load_file_batch
from fast_tffm_amd.trainer import Trainer

VOCAB = 500


def _write_data(path, gpath, n, seed, users):
    """n lines: the label follows feature 0..9 three times out of four (learnable, not separable), the group
    key is a user name; a few users have one class only."""
    r = np.random.default_rng(seed)
    with open(path, "w") as f, open(gpath, "w") as g:
        for i in range(n):
            u = int(r.integers(0, users))
            sig = int(r.integers(0, 10))
            y = int((sig < 5) != (r.random() < 0.25)) if u % 7 else 1
            feats = [sig, 10 + u % 50] + [int(x) for x in r.integers(60, VOCAB, 4)]
            f.write(f"{y} " + " ".join(f"{k}:1" for k in feats) + "\n")
            g.write(f"user{u}\n")


@pytest.fixture()
def workdir(tmp_path):
    _write_data(tmp_path / "train_0", tmp_path / "train_0.grp", 600, 1, 40)
    _write_data(tmp_path / "valid_0", tmp_path / "valid_0.grp", 300, 2, 40)
    _write_data(tmp_path / "valid_1", tmp_path / "valid_1.grp", 120, 3, 25)
    return tmp_path


def _write_cfg(workdir, extra_train="", log_dir="log", groups=True, device="cpu"):
    text = f"""[General]
vocabulary_size = {VOCAB}
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
log_dir = {workdir / log_dir}
save_summaries_steps = 1
device = {device}

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
validation_files = {workdir}/valid_0
tolerance = 0.0
{extra_train}

[Predict]
predict_files = {workdir}/valid_0, {workdir}/valid_1
{f"predict_group_files = {workdir}/valid_0.grp, {workdir}/valid_1.grp" if groups else ""}
"""
    p = workdir / "run.cfg"
    p.write_text(text)
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


def _oracle(tr, path, gpath):
    """(oracle records, GroupIndex, labels) of the restored model's scores on one file."""
    b = load_file_batch([path], None, VOCAB, False, 1)
    gi = load_group_files([gpath], [path])
    scores = tr.model.predict(b).numpy()
    return brute_groups(scores, b.labels.numpy(), gi.ids, gi.num_groups), gi, b


GAUC_KEYS = "validation_group_files = {d}/valid_0.grp\nvalidation_gauc = true\n"


def test_train_prints_and_logs_the_validation_gauc(workdir):
    cfg_path = _write_cfg(workdir, GAUC_KEYS.format(d=workdir) + "validation_auc = true")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    assert rc == 0
    m = re.search(r"^validation loss at step 3: [0-9.]+\nvalidation auc at step 3: [0-9.]+\n"
                  r"validation gauc at step 3: ([0-9.]+)$", out, re.M)
    assert m, out
    recs = [json.loads(ln) for ln in open(workdir / "log" / "metrics.jsonl")]
    logged = [r["validation_gauc"] for r in recs if "validation_gauc" in r]
    assert len(logged) == 1 and "%.8f" % logged[0] == m.group(1)
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.model.global_step == 3
        recs_o, gi, _ = _oracle(tr, str(workdir / "valid_0"), str(workdir / "valid_0.grp"))
        value, valid, _ = summary(recs_o, gi.ids, gi.num_groups)
        assert 0 < valid < gi.num_groups and abs(logged[0] - value) <= 1e-10 * value


def test_gauc_line_without_the_auc_key_and_no_line_without_gauc(workdir):
    rc, out = _run(["train", _write_cfg(workdir, GAUC_KEYS.format(d=workdir), log_dir="log_a"), "--max-steps", "3"])
    assert rc == 0 and re.search(r"^validation loss at step 3: [0-9.]+\nvalidation gauc at step 3: [0-9.]+$", out, re.M)
    assert "validation auc" not in out
    rc, out = _run(["train", _write_cfg(workdir, log_dir="log_b"), "--max-steps", "3"])
    assert rc == 0 and "validation gauc" not in out and "GAUC" not in out
    assert "validation_gauc" not in open(workdir / "log_b" / "metrics.jsonl").read()


def test_gauc_tolerance_stops_at_first_validation(workdir):
    cfg_path = _write_cfg(workdir, GAUC_KEYS.format(d=workdir) + "gauc_tolerance = 0.0", log_dir="log_es")
    rc, out = _run(["train", cfg_path])
    assert rc == 0
    assert re.search(r"validation gauc at step 3: [0-9.]+\nGAUC on validation data set is above tolerance. "
                     r"Training completed.", out), out
    assert "-- Global Step: 4;" not in out


def test_evaluate_matches_validation_metrics_and_the_oracle(workdir):
    cfg_path = _write_cfg(workdir)
    assert _run(["train", cfg_path, "--max-steps", "5"])[0] == 0
    assert _run(["predict", cfg_path])[0] == 0
    before = [open(str(workdir / f) + "_score").read() for f in ("valid_0", "valid_1")]
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore()
        for name in ("valid_0", "valid_1"):
            path, gpath = str(workdir / name), str(workdir / name) + ".grp"
            recs, gi, b = _oracle(tr, path, gpath)
            loss, auc = tr.validation_metrics(b)
            value, valid, covered = summary(recs, gi.ids, gi.num_groups)
            m = re.search(r"^evaluate %s: examples (\d+) loss ([0-9.]+) auc ([0-9.]+) gauc ([0-9.]+) "
                          r"valid_groups (\d+)/(\d+) coverage ([0-9.]+)$" % re.escape(path), out, re.M)
            assert m, out
            assert (int(m.group(1)), m.group(2), m.group(3)) == (b.B, "%.8f" % loss, "%.8f" % auc)
            assert (m.group(4), int(m.group(5)), int(m.group(6))) == ("%.8f" % value, valid, gi.num_groups)
            assert m.group(7) == "%.8f" % (covered / b.B) and 0 < valid < gi.num_groups
            # <file>_gauc: ascending AUC then key, the invalid groups last (by key) with nan
            sizes = np.bincount(gi.ids, minlength=gi.num_groups)
            rows = []
            for g, (u2, p, n) in enumerate(recs):
                ok = p > 0 and n > 0
                rows.append((not ok, u2 / (2 * p * n) if ok else 0.0, gi.keys[g],
                             "nan" if not ok else str(np.float32(u2 / (2 * p * n))), p, n, sizes[g]))
            want = ["%s %s %d %d %d" % (key, a, p, n, sz) for _, _, key, a, p, n, sz in sorted(rows)]
            assert open(path + "_gauc").read().splitlines() == want
    after = [open(str(workdir / f) + "_score").read() for f in ("valid_0", "valid_1")]
    assert before == after
    assert _run(["predict", cfg_path])[0] == 0
    assert [open(str(workdir / f) + "_score").read() for f in ("valid_0", "valid_1")] == before


def test_evaluate_without_group_files_and_the_returned_metrics(workdir):
    cfg_path = _write_cfg(workdir, groups=False)
    assert _run(["train", cfg_path, "--max-steps", "3"])[0] == 0
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0 and re.search(r"^evaluate \S+valid_1: examples 120 loss [0-9.]+ auc [0-9.]+$", out, re.M)
    assert not (workdir / "valid_1_gauc").exists()
    with Trainer(load_config(_write_cfg(workdir), echo=False), None, printer=lambda *a, **k: None) as tr:
        res = tr.evaluate()
    r = res[str(workdir / "valid_1")]
    assert set(r) == {"examples", "loss", "auc", "gauc", "valid_groups", "groups", "coverage", "gauc_file"}
    assert r["examples"] == 120 and 0 < r["valid_groups"] < r["groups"] and 0 < r["gauc"] < 1
