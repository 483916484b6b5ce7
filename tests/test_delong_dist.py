"""DeLong statistics across ranks (CPU, gloo): every rank holds ``rank::world`` of one seeded pair of score vectors
(uneven slices) and the whole baseline; the record and the values on every rank equal single-process
``K.auc_delong`` on the full vectors, exactly."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from fast_tffm_amd.ops import kernels as K
from delong_oracle import Oracle, make_case

N = 1001


def _case():
    a, b, y = make_case(N, 78, ties=True)
    return torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(y)


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.parallel import dist as fmdist

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    a, b, y = _case()
    scores, labels = fmdist.gather_dealt(ctx, [a[rank::world].contiguous(), y[rank::world].contiguous()])
    ds = K.auc_delong(scores, labels, b)  # (the baseline is whole on every rank, as evaluate reads it)
    torch.save({"rec": ds.rec.tolist(), "values": (ds.auc(), ds.interval(0.9), ds.difference())},
               os.path.join(out_dir, f"rank{rank}.pt"))
    fmdist.shutdown()


@pytest.mark.parametrize("world", [2, 3])
def test_every_rank_reports_the_single_process_values(tmp_path, world):
    from ports import free_port

    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    a, b, y = _case()
    want = K.auc_delong(a, y, b)
    o = Oracle(a.numpy(), y.numpy(), b.numpy())
    assert want.rec.tolist() == o.words() and want.difference() == o.difference()
    for r in range(world):
        got = torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)
        assert got["rec"] == want.rec.tolist(), r
        assert got["values"] == (want.auc(), want.interval(0.9), want.difference()), r


def _trainer_worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import FMRunConfig
    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer, _take

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    cfg = FMRunConfig(vocabulary_size=997, factor_num=8, loss_type="logistic", batch_size=32, init_value_range=0.5,
                      seed=3)
    with Trainer(cfg, ctx, printer=lambda *a, **k: None) as tr:
        full = random_batch(101, 997, max_feats=10, seed=41)  # the whole file, on every rank
        full.weights = torch.ones(101)  # evaluate's unit weights
        base = torch.sin(torch.arange(101, dtype=torch.float32))  # a baseline's scores, whole on every rank
        vb = _take(full, torch.arange(rank, full.B, world))   # evaluate's deal
        loss, v_auc, _, ds = tr.validation_report(vb, True, delong=(base,))
        scores = tr.model.predict(full)[: full.B].clone()      # (collective: every rank scores the whole set)
        torch.save({"loss": loss, "auc": v_auc, "rec": ds.rec.tolist(), "scores": scores, "labels": full.labels,
                    "base": base}, os.path.join(out_dir, f"tr{rank}.pt"))
    fmdist.shutdown()


def test_trainer_validation_report_across_ranks(tmp_path):
    """Two ranks, each holding its rank::2 slice of one file: both report the whole file's record."""
    from ports import free_port

    mp.spawn(_trainer_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"tr{r}.pt"), weights_only=False) for r in range(2)]
    want = K.auc_delong(got[0]["scores"], got[0]["labels"], got[0]["base"])
    assert want.rec.tolist() == Oracle(got[0]["scores"].numpy(), got[0]["labels"].numpy(),
                                       got[0]["base"].numpy()).words()
    assert 0.0 < want.auc() < 1.0 and want.stats()["has_b"] == 1
    for g in got:
        assert g["rec"] == want.rec.tolist() and g["loss"] == got[0]["loss"] and g["auc"] == want.auc()
