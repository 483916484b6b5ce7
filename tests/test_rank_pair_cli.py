"""The pairwise loss through the CLI on tiny generated files (CPU): ``train`` with ``loss_type = rank_pairwise`` prints
finite, falling ``Avg loss`` and ``validation loss`` lines, the checkpoint records the loss string, ``evaluate`` on
the validation file prints the loss the last validation printed and a GAUC, ``predict`` writes one score per line,
and ``calibrate`` refuses the loss with its usual message."""

import contextlib
import glob
import io
import json
import os
import re

import numpy as np

from fast_tffm_amd import cli

VOCAB = 600


def _write_data(path, users, seed, groups=None):
    """8 lines per user, a user's lines together: ``label user:1 item:1``; items 100..119 are liked more often.
    ``groups``: a parallel file with the user of every line."""
    r = np.random.default_rng(seed)
    with open(path, "w") as f, open(groups or os.devnull, "w") as gf:
        for u in users:
            for it in r.choice(40, 8, replace=False):
                y = int(r.random() < (0.6 if it < 20 else 0.1))
                f.write(f"{y} {u}:1 {100 + int(it)}:1\n")
                gf.write(f"{u}\n")


def _write_cfg(d, loss="rank_pairwise", epochs=4):
    p = d / f"run_{loss}_{epochs}.cfg"
    p.write_text(f"""[General]
vocabulary_size = {VOCAB}
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
log_dir = {d}/log_{loss}
save_summaries_steps = 1
device = cpu

[Train]
batch_size = 64
init_value_range = 0.01
factor_lambda = 0
bias_lambda = 0
epoch_num = {epochs}
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
save_steps = 3
shuffle = false
loss_type = {loss}
rank_group_feature = 0
train_files = {d}/train_0
validation_files = {d}/valid_0
tolerance = 0.0

[Predict]
predict_files = {d}/valid_0
predict_group_files = {d}/valid_0_groups
""")
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


STEP = re.compile(r"^-- Global Step: (\d+); Avg loss: ([0-9.]+);", re.M)
VALID = re.compile(r"^validation loss at step (\d+): ([0-9.]+)$", re.M)
EVAL = re.compile(r"^evaluate \S+: examples (\d+) loss ([0-9.]+) auc ([0-9.]+) gauc ([0-9.]+) valid_groups (\d+)/(\d+)",
                  re.M)


def test_train_evaluate_predict_calibrate(tmp_path):
    _write_data(tmp_path / "train_0", range(48), 1)       # 384 lines: 6 batches of 64, 8 users each
    _write_data(tmp_path / "valid_0", range(48, 68), 2, tmp_path / "valid_0_groups")   # 160 lines, whole groups
    cfg = _write_cfg(tmp_path)
    rc, out = _run(["train", cfg])
    assert rc == 0, out
    steps = [(int(s), float(v)) for s, v in STEP.findall(out)]
    assert [s for s, _ in steps] == list(range(1, 25))
    assert all(np.isfinite(v) and v > 0 for _, v in steps)
    # near-zero scores at step 1: the loss sum is sum_g W_g ln 2 over the batch's valid users (8 lines each), the
    # trainer divides by B
    lines = [ln.split() for ln in open(tmp_path / "train_0")][:64]
    valid_users = sum(0 < sum(int(ln[0]) for ln in lines[u: u + 8]) < 8 for u in range(0, 64, 8))
    assert abs(steps[0][1] - valid_users * 8 * np.log(2.0) / 64) < 2e-3
    # falling: every batch is lower at its last visit than at its first (4 epochs of the same 6 batches)
    assert all(steps[18 + k][1] < steps[k][1] for k in range(6))
    valid = VALID.findall(out)
    assert valid and all(np.isfinite(float(v)) and float(v) > 0 for _, v in valid)
    ckpts = glob.glob(str(tmp_path / "log_rank_pairwise" / "model.ckpt-*"))
    assert ckpts
    newest = max(ckpts, key=lambda p: int(p.rsplit("-", 1)[1]))
    assert json.load(open(os.path.join(newest, "meta.json")))["loss_type"] == "rank_pairwise"
    at = int(newest.rsplit("-", 1)[1])

    rc, ev = _run(["evaluate", cfg])
    assert rc == 0, ev
    m = EVAL.search(ev)
    assert m and int(m.group(1)) == 160, ev
    last = [v for s, v in valid if int(s) == at]
    assert last and abs(float(m.group(2)) - float(last[-1])) <= 1e-7, (valid, ev)
    gauc, vg, ng = float(m.group(4)), int(m.group(5)), int(m.group(6))
    assert ng == 20 and 0 < vg <= 20 and 0.5 < gauc <= 1.0
    # the same loss rule and the same weighting: L / ln 2 >= sum_valid W_g (1 - AUC_g) = 8 valid_groups (1 - GAUC)
    assert float(m.group(2)) * 160 / np.log(2.0) >= 8 * vg * (1.0 - gauc) * (1.0 - 1e-6)

    rc, pr = _run(["predict", cfg])
    assert rc == 0, pr
    scores = [float(x) for x in open(str(tmp_path / "valid_0") + "_score")]
    assert len(scores) == 160 and np.isfinite(scores).all() and np.std(scores) > 0

    rc, out3 = _run(["calibrate", cfg])
    assert rc == 1 and "loss_type = logistic" in out3 and "rank_pairwise" in out3
