"""The LambdaRank loss through the config and the CLI (CPU), on the configs and files of tests/test_group_pair.py and
tests/test_rank_pair_cli.py: the config accepts the loss and its cutoff and refuses the cutoff without the loss, a
cutoff out of range, ``weight_files`` with the loss and the non-local modes; ``train`` prints finite ``Avg loss`` and
``validation loss`` lines (the pair weights move with the places, so the printed value is no fixed function of the
scores and need not fall), the checkpoint records the loss string, and ``calibrate`` refuses the loss."""

import glob
import json
import os
import re

import numpy as np
import pytest

from fast_tffm_amd.config import ConfigError, load_config
from test_group_pair import _cfg
from test_rank_pair_cli import _run, _write_cfg, _write_data


def test_config(tmp_path):
    c = load_config(_cfg(tmp_path, "rank_lambda"), echo=False)
    assert c.loss_type == "rank_lambda" and c.rank_lambda_cutoff == 10 and c.fm_config().rank_lambda_cutoff == 10
    c = load_config(_cfg(tmp_path, "rank_lambda", "rank_lambda_cutoff = 0\nrank_group_feature = 1", "mode = local"),
                    echo=False)
    assert c.rank_lambda_cutoff == 0 and c.fm_config().rank_lambda_cutoff == 0 and c.rank_group_feature == 1
    for loss, extra, dist, match in (("rank_pairwise", "rank_lambda_cutoff = 3", "", "rank_lambda_cutoff"),
                                     ("rank_lambda", "rank_lambda_cutoff = 4097", "", "rank_lambda_cutoff"),
                                     ("rank_lambda", "rank_lambda_cutoff = -1", "", "rank_lambda_cutoff"),
                                     ("rank_lambda", f"weight_files = {tmp_path}/train", "", "weight_files"),
                                     ("rank_lambda", "", "mode = shard", "loss_type"),
                                     ("rank_lambda", "", "mode = dp", "loss_type"),
                                     ("rank_lambda", "", "mode = dp_dense", "loss_type")):
        with pytest.raises(ConfigError, match=match):
            load_config(_cfg(tmp_path, loss, extra, dist), echo=False)


def test_train_and_calibrate(tmp_path):
    _write_data(tmp_path / "train_0", range(48), 1)       # 384 lines: 6 batches of 64, 8 users each
    _write_data(tmp_path / "valid_0", range(48, 68), 2, tmp_path / "valid_0_groups")
    cfg = _write_cfg(tmp_path, "rank_lambda")
    with open(cfg) as f:
        text = f.read()
    with open(cfg, "w") as f:
        f.write(text.replace("loss_type = rank_lambda", "loss_type = rank_lambda\nrank_lambda_cutoff = 3"))
    rc, out = _run(["train", cfg])
    assert rc == 0, out
    steps = [float(v) for v in re.findall(r"^-- Global Step: \d+; Avg loss: ([0-9.]+);", out, re.M)]
    assert len(steps) == 24 and all(np.isfinite(v) and v > 0 for v in steps)
    valid = re.findall(r"^validation loss at step \d+: ([0-9.]+)$", out, re.M)
    assert valid and all(np.isfinite(float(v)) and float(v) > 0 for v in valid)
    newest = max(glob.glob(str(tmp_path / "log_rank_lambda" / "model.ckpt-*")), key=lambda p: int(p.rsplit("-", 1)[1]))
    assert json.load(open(os.path.join(newest, "meta.json")))["loss_type"] == "rank_lambda"
    rc, out = _run(["calibrate", cfg])
    assert rc == 1 and "loss_type = logistic" in out and "rank_lambda" in out
