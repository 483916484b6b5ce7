"""Ranking metrics across ranks (CPU, gloo, world 2): every rank holds ``rank::2`` of one validation set and of its
group ids, and ``evaluate`` deals a predict file the same way; both ranks report the numbers single-process
``K.rank_metrics`` gives on the whole set, and rank 0 writes ``<file>_rank``."""

import os

import torch
import torch.multiprocessing as mp

import rank_oracle as R
from test_gauc_cli import VOCAB, _write_data
from fast_tffm_amd.ops import kernels as K

N, G, KS = 101, 13, (1, 3, 10)


def _groups():
    return (torch.arange(N, dtype=torch.int32) * 7) % G


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    from fast_tffm_amd.config import FMRunConfig
    from fast_tffm_amd.data.reader import load_file_batch
    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.trainer import Trainer, _take

    ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
    path = os.path.join(out_dir, "pred_0")
    cfg = FMRunConfig(vocabulary_size=VOCAB, factor_num=8, loss_type="logistic", batch_size=32, init_value_range=0.5,
                      seed=3, log_dir=os.path.join(out_dir, "log"), predict_files=[path],
                      predict_group_files=[path + ".grp"], rank_cutoffs=list(KS))
    with Trainer(cfg, ctx, printer=lambda *a, **k: None) as tr:
        full = random_batch(N, VOCAB, max_feats=10, seed=41)  # the whole validation set, on every rank
        full.labels[_groups().long() % 4 == 1] = 0.0          # (groups without a positive)
        idx = torch.arange(rank, full.B, world)               # load_validation's split
        vb, ids = _take(full, idx), _groups()[idx].contiguous()
        loss, auc, gst, rst = tr.validation_report(vb, True, (ids, G), rank_cutoffs=KS)
        _, none, no_gauc, alone = tr.validation_report(vb, False, (ids, G), rank_cutoffs=KS, want_gauc=False)
        plain = tr.validation_report(vb, True, (ids, G))
        scores = tr.model.predict(full)[: full.B].clone()     # (collective: every rank scores the whole set)
        tr.save()
        res = tr.evaluate()[path]
        fb = load_file_batch([path], None, VOCAB, False, 1)
        torch.save({"loss": loss, "auc": auc, "gauc": gst.value(), "rec": rst.rec, "per_group": rst.per_group(),
                    "same": none is None and no_gauc is None and torch.equal(alone.rec, rst.rec),
                    "plain": len(plain) == 3 and plain[:2] == (loss, auc) and plain[2].value() == gst.value(),
                    "scores": scores, "labels": full.labels, "eval": res,
                    "file_scores": tr.model.predict(fb)[: fb.B].clone(), "file_labels": fb.labels},
                   os.path.join(out_dir, f"tr{rank}.pt"))
    fmdist.shutdown()


def test_both_ranks_report_the_single_process_numbers(tmp_path):
    from ports import free_port
    from fast_tffm_amd.data.groups import load_group_files

    path = str(tmp_path / "pred_0")
    _write_data(path, path + ".grp", 150, 5, 20)
    mp.spawn(_worker, args=(2, free_port(), str(tmp_path)), nprocs=2, join=True)
    got = [torch.load(os.path.join(tmp_path, f"tr{r}.pt"), weights_only=False) for r in range(2)]
    s, y = got[0]["scores"], got[0]["labels"]
    want = K.rank_metrics(s, y, _groups(), G, KS)
    means, ranked, _ = R.summary(R.group_records(s.numpy(), y.numpy(), _groups().numpy(), G, KS), KS)
    assert 1 < ranked < G and abs(want.ndcg(3) - means[1][0]) <= 1e-12 * means[1][0]
    gi = load_group_files([path + ".grp"], [path])
    ev = K.rank_metrics(got[0]["file_scores"], got[0]["file_labels"], torch.from_numpy(gi.ids), gi.num_groups, KS)
    for g in got:
        assert torch.equal(g["rec"], want.rec) and torch.equal(g["per_group"], want.per_group())
        assert g["same"] and g["plain"] and g["loss"] == got[0]["loss"]
        for k in KS:
            assert g["eval"]["ndcg@%d" % k] == ev.ndcg(k) and g["eval"]["recall@%d" % k] == ev.recall(k)
            assert g["eval"]["precision@%d" % k] == ev.precision(k)
        assert g["eval"]["ranked_groups"] == ev.ranked_groups() > 0
    assert "rank_file" in got[0]["eval"] and "rank_file" not in got[1]["eval"]
    assert len(open(path + "_rank").read().splitlines()) == gi.num_groups
