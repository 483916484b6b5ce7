"""Grouped AUC across ranks (CPU, gloo, world 2): every rank holds ``rank::2`` of one validation set and of its
group ids; both report the GAUC single-process ``K.gauc`` gives on the whole set."""

import os

import pytest
import torch
import torch.multiprocessing as mp

from gauc_oracle import brute_groups, summary
from fast_tffm_amd.ops import kernels as K

N, G = 101, 13


def _groups():
    return (torch.arange(N, dtype=torch.int32) * 7) % G


def _trainer_worker(rank, world, port, weighted, out_dir):
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
        full = random_batch(N, 997, max_feats=10, seed=41)  # the whole validation set, on every rank
        if weighted:
            full.weights = 0.5 + (torch.arange(N, dtype=torch.float32) % 4) / 2
        idx = torch.arange(rank, full.B, world)              # load_validation's split
        vb, ids = _take(full, idx), _groups()[idx].contiguous()
        loss, auc, st = tr.validation_report(vb, True, (ids, G))
        _, none, st_only = tr.validation_report(vb, False, (ids, G))
        scores = tr.model.predict(full)[: full.B].clone()    # (collective: every rank scores the whole set)
        torch.save({"loss": loss, "auc": auc, "gauc": st.value(), "valid": st.valid_groups(), "cov": st.coverage(),
                    "per_group": st.per_group(), "same": none is None and st_only.value() == st.value(),
                    "auc_alone": tr.validation_metrics(vb)[1], "scores": scores, "labels": full.labels,
                    "weights": full.weights}, os.path.join(out_dir, f"tr{rank}.pt"))
    fmdist.shutdown()


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_both_ranks_report_the_single_process_gauc(tmp_path, weighted):
    from ports import free_port

    mp.spawn(_trainer_worker, args=(2, free_port(), weighted, str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"tr{r}.pt"), weights_only=False) for r in range(2)]
    s, y, w = got[0]["scores"], got[0]["labels"], got[0]["weights"]
    want = K.gauc(s, y, _groups(), G, w)
    value, valid, covered = summary(brute_groups(s.numpy(), y.numpy(), _groups().numpy(), G,
                                                 None if w is None else w.numpy()), _groups().numpy(), G)
    assert 0.0 < value < 1.0 and valid > 1 and abs(want.value() - value) <= 1e-10 * value
    for g in got:
        assert g["gauc"] == want.value() and g["valid"] == valid and g["cov"] == covered / N
        assert torch.equal(g["per_group"], want.per_group())
        assert g["same"] and g["auc"] == g["auc_alone"] == K.auc(s, y, w).value() and g["loss"] == got[0]["loss"]
