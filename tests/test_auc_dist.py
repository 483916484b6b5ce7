"""AUC across ranks (CPU, gloo): every rank holds ``rank::world`` of one seeded vector (uneven slices);
the merged statistics on every rank equal single-process ``K.auc`` on the full vector, exactly."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from auc_oracle import make_case, oracle_stats
from fast_tffm_amd.ops import kernels as K

N = 1001


def _case(weighted):
    s, y, w = make_case(N, 77, ties=True, weights="int" if weighted else None)
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
        got = fmdist.gather_dealt(ctx, mine)
        res[weighted] = (K.auc(*got).stats(), all(g is None if f is None else torch.equal(g, f)
                                                   for g, f in zip(got, full)))
    torch.save(res, os.path.join(out_dir, f"rank{rank}.pt"))
    fmdist.shutdown()


@pytest.mark.parametrize("world", [2, 3])
def test_merged_stats_equal_single_process(tmp_path, world):
    from ports import free_port

    mp.spawn(_worker, args=(world, free_port(), str(tmp_path)), nprocs=world, join=True)
    for weighted in (False, True):
        full = _case(weighted)
        want = K.auc(*full).stats()
        assert want == oracle_stats(*[None if t is None else t.numpy() for t in full])
        for r in range(world):
            stats, same = torch.load(os.path.join(tmp_path, f"rank{r}.pt"), weights_only=False)[weighted]
            assert stats == want and same, (r, weighted)


def _trainer_worker(rank, world, port, weighted, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import FMRunConfig
    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer, _take

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    cfg = FMRunConfig(vocabulary_size=997, factor_num=8, loss_type="logistic", batch_size=32, init_value_range=0.5,
                      seed=3, validation_auc=True)
    with Trainer(cfg, ctx, printer=lambda *a, **k: None) as tr:
        full = random_batch(101, 997, max_feats=10, seed=41)  # the whole validation set, on every rank
        if weighted:
            full.weights = torch.arange(101, dtype=torch.float32) % 4
        vb = _take(full, torch.arange(rank, full.B, world))   # load_validation's split
        loss, auc = tr.validation_metrics(vb)
        scores = tr.model.predict(full)[: full.B].clone()      # (collective: every rank scores the whole set)
        torch.save({"loss": loss, "same_loss": loss == tr.validation_loss(vb), "auc": auc, "scores": scores,
                    "labels": full.labels, "weights": full.weights}, os.path.join(out_dir, f"tr{rank}.pt"))
    fmdist.shutdown()


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_trainer_validation_metrics_across_ranks(tmp_path, weighted):
    """Two ranks, each holding its rank::2 slice of one validation set: both report the AUC of the whole set."""
    from auc_oracle import value_of
    from ports import free_port

    mp.spawn(_trainer_worker, args=(2, free_port(), weighted, str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"tr{r}.pt"), weights_only=False) for r in range(2)]
    w = got[0]["weights"]
    want = value_of(oracle_stats(got[0]["scores"].numpy(), got[0]["labels"].numpy(), None if w is None else w.numpy()))
    assert 0.0 < want < 1.0
    for g in got:
        assert g["auc"] == want and g["same_loss"] and g["loss"] == got[0]["loss"]


def test_single_rank_is_a_pass_through():
    from fast_tffm_amd.parallel import dist as fmdist

    parts = [torch.ones(3), None]
    out = fmdist.gather_dealt(None, parts)
    assert out[0] is parts[0] and out[1] is None
