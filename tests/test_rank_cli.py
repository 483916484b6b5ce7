"""Ranking metrics through the CLI on tiny generated data (CPU): ``evaluate`` with ``rank_cutoffs`` prints the
per-cutoff fields and writes ``<file>_rank``, both as the oracle gives them on the model's scores, and prints and
writes what it always did without the key; ``train`` with ``validation_ndcg`` prints and logs its line and stops at
``ndcg_tolerance``; the config errors."""

import json
import re

import pytest

import rank_oracle as R
from test_gauc_cli import VOCAB, _run, _write_cfg, _write_data
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.groups import load_group_files
from fast_tffm_amd.data.reader import load_file_batch
from fast_tffm_amd.trainer import Trainer

KS = (1, 3, 10)
REL = 1e-12  # groups of <= 300 examples, <= 40 ranked groups: (300 + 8) 2^-52 < 1e-13


@pytest.fixture()
def workdir(tmp_path):
    """test_gauc_cli's files, with every label of the users 3, 8, 13, ... set to 0: groups without a positive."""
    for name, n, seed, users in (("train_0", 600, 1, 40), ("valid_0", 300, 2, 40), ("valid_1", 120, 3, 25)):
        path, gpath = tmp_path / name, tmp_path / (name + ".grp")
        _write_data(path, gpath, n, seed, users)
        keys = gpath.read_text().splitlines()
        lines = path.read_text().splitlines()
        path.write_text("".join(("0" + ln[1:] if int(k[4:]) % 5 == 3 else ln) + "\n" for ln, k in zip(lines, keys)))
    return tmp_path


def _cfg(workdir, extra_train="", predict="", **kw):
    """_write_cfg, then ``predict`` appended to the [Predict] section (the file's last)."""
    path = _write_cfg(workdir, extra_train, **kw)
    with open(path, "a") as f:
        f.write(predict + "\n")
    return path


def _oracle(tr, path, gpath, ks):
    b = load_file_batch([path], None, VOCAB, False, 1)
    gi = load_group_files([gpath], [path])
    return R.group_records(tr.model.predict(b).numpy(), b.labels.numpy(), gi.ids, gi.num_groups, ks), gi, b


def test_evaluate_prints_the_fields_and_writes_the_rank_file(workdir):
    cfg_path = _cfg(workdir, predict="rank_cutoffs = 1, 3,10")
    assert _run(["train", cfg_path, "--max-steps", "5"])[0] == 0
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore()
        for name in ("valid_0", "valid_1"):
            path = str(workdir / name)
            recs, gi, b = _oracle(tr, path, path + ".grp", KS)
            means, ranked, _ = R.summary(recs, KS)
            fields = "".join(r" ndcg@%d ([0-9.]+) recall@%d ([0-9.]+) precision@%d ([0-9.]+)" % (k, k, k) for k in KS)
            m = re.search(r"^evaluate %s: examples \d+ loss [0-9.]+ auc [0-9.]+ gauc [0-9.]+ valid_groups \d+/\d+ "
                          r"coverage [0-9.]+%s ranked_groups (\d+)/(\d+)$" % (re.escape(path), fields), out, re.M)
            assert m, out
            got = [float(v) for v in m.groups()[:9]]
            want = [v for t in means for v in t]
            assert all(abs(a - w) <= 0.5e-8 + REL * w for a, w in zip(got, want)), (got, want)
            assert (int(m.group(10)), int(m.group(11))) == (ranked, gi.num_groups) and 0 < ranked < gi.num_groups
            # <file>_rank: ascending NDCG at the first cutoff then key, the unranked groups last (by key) with nan
            lines = [ln.split() for ln in open(path + "_rank").read().splitlines()]
            assert len(lines) == gi.num_groups and all(len(ln) == 3 + 3 * len(KS) for ln in lines)
            by_key = {gi.keys[g]: r for g, r in enumerate(recs)}
            assert sorted(ln[0] for ln in lines) == sorted(by_key)
            order = []
            for ln in lines:
                r = by_key[ln[0]]
                assert (int(ln[1]), int(ln[2])) == (r[0], r[1])
                if r[1] == 0:
                    assert ln[3:] == ["nan"] * (3 * len(KS))
                    order.append((True, 0.0, ln[0]))
                    continue
                want = [float(v) for t in R.ratios(r, KS) for v in t]
                assert all(abs(float(a) - w) <= 2.0 ** -23 * w for a, w in zip(ln[3:], want)), (ln, want)
                order.append((False, float(ln[3]), ln[0]))
            # (the order is that of the written fp32 values: the last bits of an fp64 ratio order nothing)
            assert order == sorted(order)
        res = tr.evaluate()[str(workdir / "valid_1")]
    assert {"ndcg@1", "recall@3", "precision@10", "ranked_groups", "rank_file", "gauc"} <= set(res)
    assert res["rank_file"] == str(workdir / "valid_1") + "_rank"


def test_evaluate_without_rank_cutoffs_is_unchanged(workdir):
    cfg_path = _cfg(workdir)
    assert _run(["train", cfg_path, "--max-steps", "3"])[0] == 0
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0 and " ndcg@" not in out and "ranked_groups" not in out
    assert re.search(r"^evaluate \S+valid_1: examples 120 loss [0-9.]+ auc [0-9.]+ gauc [0-9.]+ valid_groups \d+/\d+ "
                     r"coverage [0-9.]+$", out, re.M), out
    assert not (workdir / "valid_0_rank").exists() and not (workdir / "valid_1_rank").exists()
    assert (workdir / "valid_1_gauc").exists()
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        r = tr.evaluate()[str(workdir / "valid_1")]
    assert set(r) == {"examples", "loss", "auc", "gauc", "valid_groups", "groups", "coverage", "gauc_file"}


NDCG_KEYS = "validation_group_files = {d}/valid_0.grp\nvalidation_ndcg = 3\n"


def test_train_prints_and_logs_the_validation_ndcg(workdir):
    cfg_path = _cfg(workdir, NDCG_KEYS.format(d=workdir) + "validation_gauc = true")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    assert rc == 0
    m = re.search(r"^validation loss at step 3: [0-9.]+\nvalidation gauc at step 3: [0-9.]+\n"
                  r"validation ndcg@3 at step 3: ([0-9.]+)$", out, re.M)
    assert m, out
    recs = [json.loads(ln) for ln in open(workdir / "log" / "metrics.jsonl")]
    logged = [r["validation_ndcg"] for r in recs if "validation_ndcg" in r]
    assert len(logged) == 1 and "%.8f" % logged[0] == m.group(1)
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.model.global_step == 3
        recs_o, _, _ = _oracle(tr, str(workdir / "valid_0"), str(workdir / "valid_0.grp"), (3,))
        means, ranked, _ = R.summary(recs_o, (3,))
        assert ranked and abs(logged[0] - means[0][0]) <= REL * means[0][0]


def test_ndcg_line_alone_and_no_line_without_the_key(workdir):
    rc, out = _run(["train", _cfg(workdir, NDCG_KEYS.format(d=workdir), log_dir="log_a"), "--max-steps", "3"])
    assert rc == 0 and re.search(r"^validation loss at step 3: [0-9.]+\nvalidation ndcg@3 at step 3: [0-9.]+$", out,
                                 re.M), out
    assert "validation gauc" not in out and "validation auc" not in out
    rc, out = _run(["train", _cfg(workdir, log_dir="log_b"), "--max-steps", "3"])
    assert rc == 0 and "validation ndcg" not in out and " ndcg@" not in out and "NDCG" not in out
    assert "validation_ndcg" not in open(workdir / "log_b" / "metrics.jsonl").read()


def test_ndcg_tolerance_stops_at_first_validation(workdir):
    cfg_path = _cfg(workdir, NDCG_KEYS.format(d=workdir) + "ndcg_tolerance = 0.0", log_dir="log_es")
    rc, out = _run(["train", cfg_path])
    assert rc == 0
    assert re.search(r"validation ndcg@3 at step 3: [0-9.]+\nNDCG on validation data set is above tolerance. "
                     r"Training completed.", out), out
    assert "-- Global Step: 4;" not in out


@pytest.mark.parametrize("train,predict,groups,msg", [
    ("", "rank_cutoffs = 1,5", False, "rank_cutoffs needs predict_group_files"),
    ("", "rank_cutoffs = 5,1", True, "rank_cutoffs must be"),
    ("", "rank_cutoffs = 0", True, "rank_cutoffs must be"),
    ("", "rank_cutoffs = 1,2,3,4,5", True, "rank_cutoffs must be"),
    ("", "rank_cutoffs = ten", True, "rank_cutoffs must be"),
    ("validation_ndcg = 3", "", True, "validation_ndcg needs validation_group_files"),
    ("validation_group_files = {d}/valid_0.grp\nvalidation_ndcg = 1,3", "", True, "validation_ndcg must be one int"),
    ("validation_group_files = {d}/valid_0.grp\nvalidation_ndcg = 5000", "", True, "validation_ndcg must be"),
    ("validation_group_files = {d}/valid_0.grp\nndcg_tolerance = 0.5", "", True, "ndcg_tolerance needs validation_n"),
])
def test_config_errors(workdir, train, predict, groups, msg):
    with pytest.raises(ConfigError, match=msg):
        load_config(_cfg(workdir, train.format(d=workdir), predict, groups=groups), echo=False)


def test_config_reads_the_keys(workdir):
    c = load_config(_cfg(workdir, NDCG_KEYS.format(d=workdir) + "ndcg_tolerance = 0.9", "rank_cutoffs = 2, 20"),
                    echo=False)
    assert (c.rank_cutoffs, c.validation_ndcg, c.ndcg_tolerance) == ([2, 20], 3, 0.9)
    d = load_config(_cfg(workdir), echo=False)
    assert (d.rank_cutoffs, d.validation_ndcg, d.ndcg_tolerance) == ([], None, None)
