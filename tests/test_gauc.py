"""Grouped AUC on the CPU: the twin (csrc/cpu/kernels.cpp ``gauc`` through ops/kernels.py) against both oracles,
the group-file reader and the config keys' validation."""

import math

import numpy as np
import pytest
import torch

from gauc_oracle import brute_groups, make_groups_case, sorted_groups, summary
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.groups import load_group_files
from fast_tffm_amd.ops import kernels as K

REL = 1e-10  # fp64 sums of <= 2^17 non-negative terms in another order: n 2^-52 ~ 3e-11


def _t(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype))


def run(s, y, g, G, w=None, device="cpu"):
    return K.gauc(_t(s).to(device), _t(y).to(device), _t(g, np.int32).to(device), G,
                  None if w is None else _t(w).to(device))


def check(st, recs, g, G, weighted):
    """A GaucStats against oracle records: exact without weights, 1e-10 relative with them."""
    got = st.per_group().cpu()
    value, valid, covered = summary(recs, g, G)
    assert got.shape == (G, 3)
    if not weighted:
        assert got.dtype == torch.int64 and got.tolist() == [list(r) for r in recs]
    else:
        want = np.array([[float(x) for x in r] for r in recs], np.float64).reshape(G, 3)
        err = np.abs(got.numpy() - want)
        print("largest relative record error", float((err / np.maximum(want, 1e-300)).max()))
        assert (err <= REL * want).all()
    assert st.valid_groups() == valid
    assert st.coverage() == covered / len(g)
    if valid:
        print("value", st.value(), "oracle", value)
        assert abs(st.value() - value) <= REL * value
    else:
        assert math.isnan(st.value())


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("distinct", [None, 3], ids=["continuous", "ties"])
@pytest.mark.parametrize("n,G", [(1, 1), (2, 1), (2, 2), (50, 1), (300, 7), (300, 300), (200, 450)])
def test_twin_equals_both_oracles(n, G, distinct, weighted):
    s, y, g, w = make_groups_case(n, G, 11 * n + G, distinct=distinct, weights=weighted)
    brute = brute_groups(s, y, g, G, w)
    assert brute == sorted_groups(s, y, g, G, w)
    check(run(s, y, g, G, w), brute, g, G, weighted)


def test_twin_skewed_against_sorted_oracle():
    sizes = [4500] + list(np.random.default_rng(3).integers(1, 4, 500))
    n, G = int(sum(sizes)), len(sizes)
    for weighted in (False, True):
        s, y, g, w = make_groups_case(n, G, 5, distinct=40, weights=weighted, sizes=sizes)
        check(run(s, y, g, G, w), sorted_groups(s, y, g, G, w), g, G, weighted)


def test_one_group_equals_auc():
    s, y, g, w = make_groups_case(5000, 1, 9, distinct=50, weights=True)
    st = run(s, y, g, 1)
    assert tuple(st.per_group()[0].tolist()) == K.auc(_t(s), _t(y)).stats()[:3]
    assert st.value() == pytest.approx(K.auc(_t(s), _t(y)).value(), rel=1e-14)
    sw = run(s, y, g, 1, w)
    assert tuple(sw.per_group()[0].tolist()) == K.auc(_t(s), _t(y), _t(w)).stats()[:3]


def test_nan_empty_and_argument_checks():
    s, y, g, _ = make_groups_case(100, 4, 2)
    s[17] = np.nan
    st = run(s, y, g, 4)
    assert math.isnan(st.value()) and st.stats()[4] == 1
    st = K.gauc(torch.empty(0), torch.empty(0), torch.empty(0, dtype=torch.int32), 3)
    assert math.isnan(st.value()) and st.valid_groups() == 0 and st.per_group().tolist() == [[0, 0, 0]] * 3
    with pytest.raises(ValueError, match="groups"):
        K.gauc(_t(s), _t(y), _t(g, np.int64), 4)
    with pytest.raises(ValueError, match="num_groups"):
        K.gauc(_t(s), _t(y), _t(g, np.int32), 0)
    with pytest.raises(ValueError, match="groups: needs >= 100"):
        K.gauc(_t(s), _t(y), _t(g[:50], np.int32), 4)
    with pytest.raises(ValueError, match="one label / group"):
        K.gauc(_t(s), _t(y), _t(np.concatenate([g, g]), np.int32), 4)
    was = K.debug_checks()
    K.set_debug_checks(True)
    try:
        with pytest.raises(ValueError, match="num_groups"):
            run(s, y, g, 3)
    finally:
        K.set_debug_checks(was)


def test_zero_weights_make_a_group_invalid():
    s = np.array([0.1, 0.9, 0.5, 0.2, 0.7], np.float32)
    y = np.array([1, 0, 1, 0, 1], np.float32)
    g = np.array([0, 0, 1, 1, 1], np.int32)
    w = np.array([0, 1, 1, 2, 0.5], np.float32)  # group 0: its only positive weighs nothing
    st = run(s, y, g, 2, w)
    check(st, brute_groups(s, y, g, 2, w), g, 2, True)
    assert st.valid_groups() == 1 and st.coverage() == 3 / 5 and st.value() == 1.0


# ---------------------------------------------------------------------------
def test_group_file_reader(tmp_path):
    (tmp_path / "d0").write_text("1 1:1\n0 2:1\n1 3:1\n")
    (tmp_path / "d1").write_text("0 1:1\n1 2:1\n")
    (tmp_path / "g0").write_text("u7\nu3\nu7\n")
    (tmp_path / "g1").write_text("u9\r\nu3\n")
    gi = load_group_files([str(tmp_path / "g0"), str(tmp_path / "g1")], [str(tmp_path / "d0"), str(tmp_path / "d1")])
    assert gi.ids.dtype == np.int32 and gi.ids.tolist() == [0, 1, 0, 2, 1]
    assert gi.keys == ["u7", "u3", "u9"] and gi.num_groups == 3
    (tmp_path / "g1").write_text("u9\n")
    with pytest.raises(ValueError) as e:
        load_group_files([str(tmp_path / "g0"), str(tmp_path / "g1")], [str(tmp_path / "d0"), str(tmp_path / "d1")])
    assert str(tmp_path / "g1") in str(e.value) and str(tmp_path / "d1") in str(e.value)
    with pytest.raises(ValueError, match="numbers of data files and group files"):
        load_group_files([str(tmp_path / "g0")], [str(tmp_path / "d0"), str(tmp_path / "d1")])


CFG = """[General]
vocabulary_size = 100
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False

[Train]
batch_size = 10
init_value_range = 0.01
factor_lambda = 0
bias_lambda = 0
epoch_num = 1
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
loss_type = logistic
train_files = {d}/data
{train}

[Predict]
{predict}
"""


def _cfg(tmp_path, train="", predict=""):
    for name in ("data", "val", "grp"):
        (tmp_path / name).write_text("1 1:1\n")
    p = tmp_path / "run.cfg"
    p.write_text(CFG.format(d=tmp_path, train=train.format(d=tmp_path), predict=predict.format(d=tmp_path)))
    return str(p)


def test_config_keys_and_their_errors(tmp_path):
    val = "validation_files = {d}/val\ntolerance = 0\n"
    c = load_config(_cfg(tmp_path), echo=False)
    assert (c.validation_group_files, c.validation_gauc, c.gauc_tolerance, c.predict_group_files) == ([], False, None,
                                                                                                      [])
    c = load_config(_cfg(tmp_path, val + "validation_group_files = {d}/grp\nvalidation_gauc = true\n"
                         "gauc_tolerance = 0.75\n", "predict_files = {d}/val\npredict_group_files = {d}/grp\n"),
                    echo=False)
    assert c.validation_group_files == [str(tmp_path / "grp")] and c.validation_gauc and c.gauc_tolerance == 0.75
    assert c.predict_group_files == [str(tmp_path / "grp")]
    for train, predict, what in (
            ("validation_group_files = {d}/grp\n", "", "validation_group_files needs validation_files"),
            (val + "validation_group_files = {d}/grp, {d}/data\n", "", "validation group files do not match"),
            (val + "validation_gauc = true\n", "", "validation_gauc needs validation_group_files"),
            (val + "validation_group_files = {d}/grp\ngauc_tolerance = 0.7\n", "", "gauc_tolerance needs"),
            ("", "predict_files = {d}/val\npredict_group_files = {d}/grp, {d}/data\n",
             "predict group files do not match")):
        with pytest.raises(ConfigError, match=what):
            load_config(_cfg(tmp_path, train, predict), echo=False)
