"""``run.py recommend`` with ``[Predict] recommend_target_files``: the ``<file>_places`` file, the printed
metrics and their agreement with ``<file>_recommend``; without the key the run is what it was."""

import contextlib
import io
import os
import re

import pytest

from fast_tffm_amd import cli
from test_topk import CANDS, LINES, _copy_lines, _write_cfg


@pytest.fixture(scope="module")
def workdir(tmp_path_factory, ref_data_dir):
    wd = str(tmp_path_factory.mktemp("place_cli"))
    os.makedirs(os.path.join(wd, "data"))
    _copy_lines(os.path.join(ref_data_dir, "train_0"), os.path.join(wd, "data", "train_0"), 0, 600)
    _copy_lines(os.path.join(ref_data_dir, "test_0"), os.path.join(wd, "data", "test_0"), 0, LINES)
    cands = os.path.join(wd, "data", "candidates")
    _copy_lines(os.path.join(ref_data_dir, "test_0"), cands, LINES, CANDS)
    cfg = _write_cfg(wd)
    targets = os.path.join(wd, "data", "targets")
    with open(targets, "w") as f:
        f.write("".join(f"{-1 if i == 4 else (37 * i) % CANDS}\n" for i in range(LINES)))
    with open(cfg) as f:
        text = f.read()
    cfg_t = os.path.join(wd, "targets.cfg")
    with open(cfg_t, "w") as f:
        f.write(text.replace("[Distributed]", f"recommend_target_files = {targets}\n\n[Distributed]"))
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["train", cfg, "--max-steps", "4"]) == 0
    return wd, cfg, cfg_t, cands, targets


def _recommend(cfg, cands):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        assert cli.main(["recommend", cfg, "--candidates", cands, "--top", "5"]) == 0
    return out.getvalue()


def test_recommend_with_targets(workdir):
    wd, cfg, cfg_t, cands, targets = workdir
    rec, places = (os.path.join(wd, "data", "test_0" + s) for s in ("_recommend", "_places"))
    plain = _recommend(cfg, cands)
    before = open(rec, "rb").read()
    assert not os.path.exists(places) and "hit@" not in plain
    printed = _recommend(cfg_t, cands)
    assert open(rec, "rb").read() == before
    mark = "======== recommend"   # (before it the config is echoed, which names the key)
    report = re.search(r"recommend .*test_0: contexts.*\n", printed).group(0)
    assert printed[printed.index(mark):].replace(report, "") == plain[plain.index(mark):]
    rows = [tuple(map(int, ln.split())) for ln in open(places).read().splitlines()]
    assert [r[0] for r in rows] == [int(x) for x in open(targets).read().split()] and len(rows) == LINES
    hit, ranked = 0.0, 0
    for (t, gt, eq), ln in zip(rows, before.decode().splitlines()):
        listed = [int(tok.split(":")[0]) for tok in ln.split()]
        if t < 0:
            assert (gt, eq) == (0, 0)
            continue
        assert eq >= 1 and 0 <= gt < CANDS
        ranked += 1
        hit += (min(gt + eq, 5) - min(gt, 5)) / eq
        if gt + eq <= 5:
            assert t in listed
        if gt >= 5:
            assert t not in listed
    m = re.search(r"contexts (\d+) ranked (\d+) hit@5 (\S+) ndcg@5 (\S+) mrr@5 (\S+) mean_place (\S+)", printed)
    assert (int(m.group(1)), int(m.group(2))) == (LINES, ranked) == (LINES, LINES - 1)
    assert float(m.group(3)) == float("%.8f" % (hit / ranked))
    assert float(m.group(6)) == float("%.8g" % (sum(2 * gt + eq + 1 for t, gt, eq in rows if t >= 0) / (2 * ranked)))


@pytest.mark.parametrize("line,text", [(3, "x"), (2, str(CANDS)), (1, "-2"), (LINES, None)])
def test_malformed_targets(workdir, line, text):
    wd, _, cfg_t, cands, targets = workdir
    good = open(targets).read()
    lines = good.splitlines()
    lines[line - 1:line] = [text] if text is not None else []   # (None: a line short)
    try:
        with open(targets, "w") as f:
            f.write("\n".join(lines) + "\n")
        with pytest.raises(ValueError, match=re.escape(targets) + f", line {line}:"), \
                contextlib.redirect_stdout(io.StringIO()):
            cli.main(["recommend", cfg_t, "--candidates", cands, "--top", "5"])
    finally:
        with open(targets, "w") as f:
            f.write(good)
