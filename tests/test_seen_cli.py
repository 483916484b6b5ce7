"""``run.py recommend`` with ``[Predict] recommend_seen_files``: no listed candidate is recommended, ``<file>_places``
is ``fm_place(..., seen=...)``'s, the printed line ends with the list entries; without the key the run is what it
was.  (The trained model, the target file and its config are tests/test_place_cli.py's.)"""

import contextlib
import io
import os
import re

import pytest
import torch

from fast_tffm_amd import cli
from fast_tffm_amd.config import load_config
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.trainer import Trainer, load_file_batch
from test_place_cli import _recommend, workdir  # noqa: F401  (the fixture)
from test_topk import CANDS, LINES


@pytest.fixture(scope="module")
def seen_cfg(workdir):  # noqa: F811
    wd, _, cfg_t, cands, _ = workdir
    seen, cfg_s = os.path.join(wd, "data", "seen"), os.path.join(wd, "seen.cfg")
    with open(cfg_s, "w") as f:
        f.write(open(cfg_t).read().replace("[Distributed]", f"recommend_seen_files = {seen}\n\n[Distributed]"))
    return wd, cfg_t, cfg_s, cands, seen


def _outputs(wd):
    rec, pl = (open(os.path.join(wd, "data", "test_0" + s)).read().splitlines() for s in ("_recommend", "_places"))
    return [[int(tok.split(":")[0]) for tok in ln.split()] for ln in rec], [tuple(map(int, ln.split())) for ln in pl]


def test_recommend_with_seen(seen_cfg):
    wd, cfg_t, cfg_s, cands, seen = seen_cfg
    _recommend(cfg_t, cands)
    plain_rec, plain_places = _outputs(wd)
    # line i: its plain recommendations, unsorted and with a duplicate, its target on every third line; line 7 empty
    lists = [[] if i == 7 else rec[::-1] + rec[:1] + ([t] if i % 3 == 0 and t >= 0 else [])
             for i, (rec, (t, _, _)) in enumerate(zip(plain_rec, plain_places))]
    with open(seen, "w") as f:
        f.write("".join(" ".join(map(str, row)) + "\n" for row in lists))
    printed = _recommend(cfg_s, cands)
    got_rec, got_places = _outputs(wd)
    assert got_rec[7] == plain_rec[7] and all(len(r) == 5 and not set(r) & set(s) for r, s in zip(got_rec, lists))
    entries = sum(len(set(row)) for row in lists)
    assert re.search(r"recommend .*test_0: contexts .* mean_place \S+ seen %d\n" % entries, printed)
    # the places are fm_place's with the lists, and no worse than without them
    c = load_config(cfg_s)
    tr = Trainer(c, None)
    assert tr.restore()
    bq, bc = (load_file_batch([p], None, c.vocabulary_size, c.hash_feature_id, 1) for p in (c.predict_files[0], cands))
    t = torch.tensor([p[0] for p in plain_places], dtype=torch.int32)
    want = tr.model.place(bq, bc, t, (5,), seen=K.seen_lists(lists, CANDS, "cpu")).counts()
    assert [p[1:] for p in got_places] == [tuple(r) for r in want.tolist()] and [p[0] for p in got_places] == t.tolist()
    assert all(gt <= gt0 for (_, gt, _), (_, gt0, _) in zip(got_places, plain_places))
    assert any(gt < gt0 for (_, gt, _), (_, gt0, _) in zip(got_places, plain_places))
    _recommend(cfg_t, cands)   # without the key again: the same files as before
    assert _outputs(wd) == (plain_rec, plain_places)


@pytest.mark.parametrize("line,text", [(3, "1 x"), (2, f"0 {CANDS}"), (1, "-1"), (LINES, None)])
def test_malformed_seen(seen_cfg, line, text):
    _, _, cfg_s, cands, seen = seen_cfg
    lines = ["1 2"] * LINES
    lines[line - 1:line] = [text] if text is not None else []   # (None: a line short)
    with open(seen, "w") as f:
        f.write("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match=re.escape(seen) + f", line {line}:"), \
            contextlib.redirect_stdout(io.StringIO()):
        cli.main(["recommend", cfg_s, "--candidates", cands, "--top", "5"])
