"""The listwise loss through the CLI on tiny generated files (CPU): ``train`` with ``loss_type = rank_softmax``
prints its ``Avg loss`` and ``validation loss`` lines and resumes from its checkpoint, ``evaluate`` on the validation
file prints the loss the last validation printed, the checkpoint records the loss string, and ``calibrate`` refuses
the loss with its usual message."""

import contextlib
import glob
import io
import json
import os
import re

import numpy as np

from fast_tffm_amd import cli

VOCAB = 600


def _write_data(path, users, seed):
    """8 lines per user, a user's lines together: ``label user:1 item:1``; items 100..119 are liked more often."""
    r = np.random.default_rng(seed)
    with open(path, "w") as f:
        for u in users:
            for it in r.choice(40, 8, replace=False):
                y = int(r.random() < (0.6 if it < 20 else 0.1))
                f.write(f"{y} {u}:1 {100 + int(it)}:1\n")


def _write_cfg(d, loss="rank_softmax", epochs=1, extra=""):
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
{extra}
train_files = {d}/train_0
validation_files = {d}/valid_0
tolerance = 0.0

[Predict]
predict_files = {d}/valid_0
""")
    return str(p)


def _run(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = cli.main(argv)
    return rc, buf.getvalue()


STEP = re.compile(r"^-- Global Step: (\d+); Avg loss: ([0-9.]+);", re.M)
VALID = re.compile(r"^validation loss at step (\d+): ([0-9.]+)$", re.M)
EVAL = re.compile(r"^evaluate \S+: examples (\d+) loss ([0-9.]+) auc", re.M)


def test_train_resume_evaluate_calibrate(tmp_path):
    _write_data(tmp_path / "train_0", range(48), 1)       # 384 lines: 6 batches of 64, 8 users each
    _write_data(tmp_path / "valid_0", range(48, 68), 2)   # 160 lines: one validation batch, whole groups
    cfg = _write_cfg(tmp_path, extra="rank_group_feature = 0")
    rc, out = _run(["train", cfg])
    assert rc == 0, out
    steps = STEP.findall(out)
    assert [int(s) for s, _ in steps] == [1, 2, 3, 4, 5, 6]
    # near-zero scores at step 1: the loss sum is sum_g A_g log 8 over the batch's 8 users, the trainer divides by B
    lines = [ln.split() for ln in open(tmp_path / "train_0")][:64]
    pos = sum(int(ln[0]) for ln in lines)
    assert abs(float(steps[0][1]) - pos * np.log(8) / 64) < 2e-3
    valid = VALID.findall(out)
    assert valid and all(float(v) > 0 for _, v in valid)
    ckpts = glob.glob(str(tmp_path / "log_rank_softmax" / "model.ckpt-*"))
    assert ckpts
    newest = max(ckpts, key=lambda p: int(p.rsplit("-", 1)[1]))
    assert json.load(open(os.path.join(newest, "meta.json")))["loss_type"] == "rank_softmax"
    at = int(newest.rsplit("-", 1)[1])

    rc, ev = _run(["evaluate", cfg])
    assert rc == 0, ev
    m = EVAL.search(ev)
    assert m and int(m.group(1)) == 160
    last = [v for s, v in valid if int(s) == at]
    assert last and abs(float(m.group(2)) - float(last[-1])) <= 1e-7, (valid, ev)

    # a second run with more epochs resumes from the checkpoint: the step numbers go on
    rc, out2 = _run(["train", _write_cfg(tmp_path, epochs=2, extra="rank_group_feature = 0")])
    assert rc == 0, out2
    more = [int(s) for s, _ in STEP.findall(out2)]
    assert more and more[0] == at + 1 and more[-1] == 12

    rc, out3 = _run(["calibrate", cfg])
    assert rc == 1 and "loss_type = logistic" in out3 and "rank_softmax" in out3
