"""``run.py recommend --diversity``: without the flag the file's bytes are what they were; with it every line's picks
come from that context's ``--top pool`` list and are ``ServingModel.recommend(..., diversity=)``'s (test_place_cli's
model)."""

import contextlib
import io
import os

from fast_tffm_amd import cli
from fast_tffm_amd.serving import ServingModel, export_model
from fast_tffm_amd.utils.checkpoint import latest_checkpoint
from test_place_cli import _recommend, workdir  # noqa: F401  (the fixture)
from test_topk import _trainer


def test_recommend_with_diversity(workdir, tmp_path):  # noqa: F811
    wd, cfg, _, cands, _ = workdir
    rec = os.path.join(wd, "data", "test_0_recommend")

    def tokens(*flags):
        with contextlib.redirect_stdout(io.StringIO()):
            assert cli.main(["recommend", cfg, "--candidates", cands, "--top", "5", *flags]) == 0
        return [[tok.split(":") for tok in ln.split()] for ln in open(rec).read().splitlines()]

    _recommend(cfg, cands)
    plain = open(rec, "rb").read()
    tr = _trainer(cfg)
    tr.recommend(cands, top=5, diversity=None)
    assert open(rec, "rb").read() == plain
    export = str(tmp_path / "export")
    export_model(latest_checkpoint(tr.cfg.log_dir), export, vocabulary_block_num=2, hash_feature_id=True,
                 loss_type="logistic")
    tr.close()

    pool = tokens("--top", "12")
    got = tokens("--diversity", "0.5", "--pool", "12")
    assert len(got) == len(pool) and all(len(g) == 5 and set(map(tuple, g)) <= set(map(tuple, p))
                                         for g, p in zip(got, pool))
    assert got != [p[:5] for p in pool], "lambda = 0.5 re-ranked nothing"
    assert tokens("--diversity", "1", "--pool", "12") == [p[:5] for p in pool]
    lines = lambda path: [ln.split(None, 1)[1].strip() for ln in open(path)]   # (without the label column)
    sm = ServingModel.load(export, device="cpu")
    idx, score = sm.recommend(lines(os.path.join(wd, "data", "test_0")), lines(cands), top=5, diversity=0.5, pool=12)
    assert [[int(c) for c, _ in g] for g in got] == idx.tolist()
    assert [[s for _, s in g] for g in got] == [[str(s) for s in row] for row in score]
    assert tokens("--diversity", "0.5") == [[[str(c), str(s)] for c, s in zip(ri, rs)] for ri, rs in zip(
        *sm.recommend(lines(os.path.join(wd, "data", "test_0")), lines(cands), top=5, diversity=0.5))]
