"""Threshold metrics across ranks (CPU, gloo): every rank holds ``rank::world`` of one seeded vector (uneven
slices); the record on every rank equals single-process ``K.threshold_metrics`` on the full vector, exactly."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from fast_tffm_amd.ops import kernels as K
from threshold_oracle import PRECISION_TARGETS, RECALL_TARGETS, Oracle, assert_exact, make_case

N = 1001
KW = dict(precision_targets=PRECISION_TARGETS, recall_targets=RECALL_TARGETS)


def _case(weighted):
    s, y, w = make_case(N, 78, ties=True, weights="int" if weighted else None)
    t = torch.from_numpy
    return t(s), t(y), None if w is None else t(w)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.parallel import dist as fmdist

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    res = {}
    for weighted in (False, True):
        full = _case(weighted)
        mine = [None if t is None else t[rank::world].contiguous() for t in full]
        res[weighted] = K.threshold_metrics(*fmdist.gather_dealt(ctx, mine), **KW).rec.view(torch.int64).tolist()
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    fmdist.shutdown()


@pytest.mark.parametrize("world", [2, 3])
def test_merged_record_equals_single_process(tmp_path, world):
    from ports import free_port

    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    for weighted in (False, True):
        full = _case(weighted)
        want = K.threshold_metrics(*full, **KW)
        assert_exact(want, Oracle(*[None if t is None else t.numpy() for t in full]), PRECISION_TARGETS,
                     RECALL_TARGETS)
        for r in range(world):
            got = torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)[weighted]
            assert got == want.rec.view(torch.int64).tolist(), (r, weighted)


def _trainer_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import FMRunConfig
    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer, _take

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    cfg = FMRunConfig(vocabulary_size=997, factor_num=8, loss_type="logistic", batch_size=32, init_value_range=0.5,
                      seed=3, validation_ap=True)
    with Trainer(cfg, ctx, printer=lambda *a, **k: None) as tr:
        full = random_batch(101, 997, max_feats=10, seed=41)  # the whole validation set, on every rank
        full.weights = torch.arange(101, dtype=torch.float32) % 4
        vb = _take(full, torch.arange(rank, full.B, world))   # load_validation's split
        loss, _, _, ts = tr.validation_report(vb, False, thresholds=((0.5,), (0.9,)))
        scores = tr.model.predict(full)[: full.B].clone()      # (collective: every rank scores the whole set)
        torch.save({"loss": loss, "rec": ts.rec.view(torch.int64).tolist(), "scores": scores, "labels": full.labels,
                    "weights": full.weights}, os.path.join(out_dir, f"tr{rank}.pt"))
    fmdist.shutdown()


def test_trainer_validation_report_across_ranks(tmp_path):
    """Two ranks, each holding its rank::2 slice of one validation set: both report the whole set's record."""
    from ports import free_port

    mp.spawn(_trainer_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"tr{r}.pt"), weights_only=False) for r in range(2)]
    want = K.threshold_metrics(got[0]["scores"], got[0]["labels"], got[0]["weights"], precision_targets=(0.5,),
                               recall_targets=(0.9,))
    assert_exact(want, Oracle(got[0]["scores"].numpy(), got[0]["labels"].numpy(), got[0]["weights"].numpy()),
                 (0.5,), (0.9,))
    assert 0.0 < want.ap() < 1.0
    for g in got:
        assert g["rec"] == want.rec.view(torch.int64).tolist() and g["loss"] == got[0]["loss"]
