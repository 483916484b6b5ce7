"""``calibrate`` across ranks (CPU, gloo, world 2): every rank scores ``rank::2`` of the validation set, all
gather the scores, and rank 0 writes the ``calibration.json`` a single process writes for the same checkpoint."""

import os
import shutil

import torch.multiprocessing as mp

from test_calibrate_cli import _newest_ckpt, _run, _write_cfg, _write_data
from fast_tffm_amd.calibration import Calibrator


def _worker(rank, world, port, cfg_path):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    with Trainer(load_config(cfg_path, echo=False), ctx, printer=lambda *a, **k: None) as tr:
        res = tr.calibrate()
        assert ("file" in res) == (rank == 0)
    fmdist.shutdown()


def test_world_2_writes_the_single_process_calibrator(tmp_path):
    from ports import free_port

    _write_data(tmp_path / "train_0", tmp_path / "train_0.w", 600, 1)
    _write_data(tmp_path / "valid_0", tmp_path / "valid_0.w", 300, 2)
    cfg = _write_cfg(tmp_path, log_dir="log", weights=True)
    assert _run(["train", cfg, "--max-steps", "5"])[0] == 0
    shutil.copytree(tmp_path / "log", tmp_path / "log2")
    assert _run(["calibrate", cfg])[0] == 0
    one = Calibrator.load(os.path.join(_newest_ckpt(tmp_path / "log"), "calibration.json"))
    cfg2 = _write_cfg(tmp_path, log_dir="log2", weights=True)
    mp.spawn(_worker, args=(2, free_port(), cfg2), nprocs=2, join=True)
    two = Calibrator.load(os.path.join(_newest_ckpt(tmp_path / "log2"), "calibration.json"))
    assert one.blocks > 2 and two.x.tolist() == one.x.tolist() and two.y.tolist() == one.y.tolist()
    for k in ("examples", "total_weight", "positives", "blocks", "global_step", "weighted", "loss_after"):
        assert two.meta[k] == one.meta[k], k
    assert abs(two.meta["loss_before"] - one.meta["loss_before"]) <= 1e-6  # (fp32 loss sums of two halves)
    assert open(tmp_path / "log2" / "calibration_blocks.txt").read() == open(
        tmp_path / "log" / "calibration_blocks.txt").read()
