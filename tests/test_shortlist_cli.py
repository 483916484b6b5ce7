"""``run.py recommend`` with ``[Predict] recommend_shortlist_files``: both files are the Python API's, the printed tail,
the refusal with ``recommend_seen_files``, bad lines, the same bytes without the key (test_place_cli's model)."""

import contextlib
import io
import os
import re

import pytest
import torch

from fast_tffm_amd import cli
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.trainer import Trainer, load_file_batch
from test_place_cli import _recommend, workdir  # noqa: F401  (the fixture)
from test_seen_cli import _outputs
from test_topk import CANDS, LINES


@pytest.fixture(scope="module")
def short_cfg(workdir):  # noqa: F811
    wd, _, cfg_t, cands, _ = workdir
    short, cfg_s = os.path.join(wd, "data", "shortlist"), os.path.join(wd, "shortlist.cfg")
    with open(cfg_s, "w") as f:
        f.write(open(cfg_t).read().replace("[Distributed]", f"recommend_shortlist_files = {short}\n\n[Distributed]"))
    return wd, cfg_t, cfg_s, cands, short


def test_recommend_with_shortlist(short_cfg):
    wd, cfg_t, cfg_s, cands, short = short_cfg
    files = lambda: [open(os.path.join(wd, "data", "test_0" + s), "rb").read() for s in ("_recommend", "_places")]
    plain_out, plain_files, plain_places = _recommend(cfg_t, cands), files(), _outputs(wd)[1]
    # line i: every third candidate, unsorted, with a duplicate, its target on even lines; 7 empty, 8 shorter than --top
    lists = [[] if i == 7 else [1, 0] if i == 8 else list(range(i % 3, CANDS, 3))[::-1] + [i % 3]
             + ([t] if i % 2 == 0 and t >= 0 else []) for i, (t, _, _) in enumerate(plain_places)]
    with open(short, "w") as f:
        f.write("".join(" ".join(map(str, row)) + "\n" for row in lists))
    printed = _recommend(cfg_s, cands)
    got_rec, got_places = _outputs(wd)
    entries = sum(len(set(row)) for row in lists)
    assert re.search(r"recommend .*test_0: contexts .* mean_place \S+ shortlist %d\n" % entries, printed)
    c = load_config(cfg_s)
    tr = Trainer(c, None)
    assert tr.restore()
    bq, bc = (load_file_batch([p], None, c.vocabulary_size, c.hash_feature_id, 1) for p in (c.predict_files[0], cands))
    t = torch.tensor([p[0] for p in plain_places], dtype=torch.int32)
    sl = K.seen_lists(lists, CANDS, "cpu")
    assert got_rec == [[i for i in r if i >= 0] for r in tr.model.recommend(bq, bc, 5, shortlist=sl)[0].tolist()]
    assert got_rec[7] == [] and sorted(got_rec[8]) == [0, 1] and all(set(r) <= set(s) for r, s in zip(got_rec, lists))
    want = tr.model.place(bq, bc, t, (5,), shortlist=sl).counts()
    assert [p[1:] for p in got_places] == [tuple(r) for r in want.tolist()] and [p[0] for p in got_places] == t.tolist()
    assert got_places[7][1:] == (0, 1) and got_places[4] == (-1, 0, 0)
    with open(cfg_s + ".both", "w") as f:
        f.write(open(cfg_s).read().replace("[Distributed]", f"recommend_seen_files = {short}\n\n[Distributed]"))
    with pytest.raises(ConfigError, match="recommend_shortlist_files and recommend_seen_files"):
        load_config(cfg_s + ".both")
    assert _recommend(cfg_t, cands).split("=====")[-1] == plain_out.split("=====")[-1] and files() == plain_files


@pytest.mark.parametrize("line,text", [(3, "1 x"), (2, f"0 {CANDS}"), (LINES, None)])
def test_malformed_shortlist(short_cfg, line, text):
    _, _, cfg_s, cands, short = short_cfg
    lines = ["1 2"] * LINES
    lines[line - 1:line] = [text] if text is not None else []   # (None: a line short)
    with open(short, "w") as f:
        f.write("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match=re.escape(short) + f", line {line}:"), \
            contextlib.redirect_stdout(io.StringIO()):
        cli.main(["recommend", cfg_s, "--candidates", cands, "--top", "5"])
