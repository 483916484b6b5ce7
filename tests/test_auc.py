"""Exact weighted ROC AUC (ops/kernels.py ``auc``) on the CPU: the numpy oracle against the pairwise
definition, the CPU kernel against the oracle (exact without weights and with integer weights, within the
summation bound with real ones), special values, edge cases and the config keys."""

import math

import numpy as np
import pytest
import torch

from auc_oracle import (SPECIAL_LABELS, SPECIAL_SCORES, make_case, oracle_stats, pairwise_stats, rel_bound,
                        value_of)
from fast_tffm_amd.config import ConfigError, FMRunConfig, load_config
from fast_tffm_amd.ops import kernels as K


def _auc(s, y, w=None, device="cpu"):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)  # noqa: E731
    return K.auc(t(s), t(y), t(w))


def _close(got, want, n):
    return all(abs(g - x) <= rel_bound(n) * x for g, x in zip(got[:3], want[:3]))


@pytest.mark.parametrize("weights", [None, "int", "real"])
@pytest.mark.parametrize("ties", [False, True])
@pytest.mark.parametrize("n", [2, 3, 17, 300])
def test_oracle_matches_pairwise(n, ties, weights):
    s, y, w = make_case(n, 100 + n, ties=ties, weights=weights)
    got, want = oracle_stats(s, y, w), pairwise_stats(s, y, w)
    if weights == "real":
        assert _close(got, want, n), (got, want)
    else:
        assert got[:3] == want


def test_oracle_special_values_match_pairwise():
    assert oracle_stats(SPECIAL_SCORES, SPECIAL_LABELS)[:3] == pairwise_stats(SPECIAL_SCORES, SPECIAL_LABELS)


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "continuous"])
@pytest.mark.parametrize("n", [1, 2, 65, 1000, 100_003])
def test_cpu_unweighted_exact(n, ties):
    s, y, _ = make_case(n, n, ties=ties)
    st = _auc(s, y)
    want = oracle_stats(s, y)
    assert st.stats() == want
    assert all(isinstance(v, int) for v in st.stats())
    v = st.value()
    assert (math.isnan(v) and n == 1) or v == value_of(want)


def test_special_values():
    st = _auc(SPECIAL_SCORES, SPECIAL_LABELS)
    assert st.stats() == oracle_stats(SPECIAL_SCORES, SPECIAL_LABELS)
    # -0.0 against +0.0 is a tie
    assert _auc([0.0, -0.0], [1, 0]).value() == 0.5
    assert _auc([-0.0, 0.0], [1, 0]).value() == 0.5
    # a denormal is above zero and below its neighbour denormal; the infinities are ordinary values
    assert _auc([1e-42, 0.0], [1, 0]).value() == 1.0
    assert _auc([-1e-42, -0.0], [1, 0]).value() == 0.0
    assert _auc([1e-42, 3e-42], [1, 0]).value() == 0.0
    assert _auc([np.inf, 3e38, -np.inf], [1, 0, 0]).value() == 1.0
    assert _auc([np.inf, np.inf, -np.inf, -np.inf], [1, 0, 1, 0]).value() == 0.5


def test_edge_cases():
    n = 1000
    y = make_case(n, 5)[1]
    assert _auc(np.full(n, 0.25, np.float32), y).value() == 0.5
    assert _auc(np.where(y > 0, 2.0, -1.0) + np.arange(n) * 1e-4, y).value() == 1.0
    assert _auc(np.where(y > 0, -1.0, 2.0) + np.arange(n) * 1e-4, y).value() == 0.0
    s = make_case(n, 6)[0]
    for labels in (np.zeros(n, np.float32), np.ones(n, np.float32)):  # one class only: undefined, no error
        st = _auc(s, labels)
        assert math.isnan(st.value()) and st.stats() == oracle_stats(s, labels)
    s[17] = np.nan
    st = _auc(s, y)
    assert math.isnan(st.value()) and st.stats()[3] == 1
    st = K.auc(torch.empty(0), torch.empty(0))  # nothing to launch
    assert math.isnan(st.value()) and st.stats() == (0, 0, 0, 0)


def test_pm1_labels_equal_01_labels():
    s, y, _ = make_case(1000, 9, ties=True)
    assert _auc(s, 2.0 * y - 1.0).stats() == _auc(s, y).stats()
    sw, yw, w = make_case(1000, 9, ties=True, weights="int", pm1=True)
    assert _auc(sw, yw, w).stats() == _auc(sw, (yw > 0).astype(np.float32), w).stats()


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "continuous"])
@pytest.mark.parametrize("n", [2, 65, 1000, 100_003])
def test_cpu_integer_weights_exact(n, ties):
    s, y, w = make_case(n, 3 * n, ties=ties, weights="int")
    st = _auc(s, y, w)
    want = oracle_stats(s, y, w)
    assert st.stats() == want and st.value() == value_of(want)
    assert all(isinstance(v, float) for v in st.stats()[:3])


@pytest.mark.parametrize("ties", [True, False], ids=["ties", "continuous"])
@pytest.mark.parametrize("n", [2, 65, 3000, 100_003])
def test_cpu_real_weights_within_summation_bound(n, ties):
    s, y, w = make_case(n, 7 * n, ties=ties, weights="real")
    got, want = _auc(s, y, w).stats(), oracle_stats(s, y, w)
    print("relative errors", [abs(g - x) / x for g, x in zip(got[:3], want[:3])], "bound", rel_bound(n))
    assert _close(got, want, n), (got, want)


def test_weighted_equals_unweighted_with_unit_weights():
    s, y, _ = make_case(1000, 21, ties=True)
    u = _auc(s, y).stats()
    assert _auc(s, y, np.ones(1000, np.float32)).stats() == tuple(float(v) for v in u[:3]) + (0,)


def test_negative_weight_raises_under_debug_checks():
    s, y, w = make_case(100, 4, weights="real")
    w[50] = -0.5
    was = K.debug_checks()
    K.set_debug_checks(True)
    try:
        with pytest.raises(ValueError, match="weights"):
            _auc(s, y, w)
    finally:
        K.set_debug_checks(was)


def test_argument_checks():
    s, y, _ = make_case(10, 1)
    with pytest.raises(ValueError):
        K.auc(torch.from_numpy(s).double(), torch.from_numpy(y))
    with pytest.raises(ValueError):
        K.auc(torch.from_numpy(s), torch.from_numpy(y[:5].copy()))


def _cfg_text(tmp_path, extra=""):
    (tmp_path / "train_0").write_text("1 1:1\n")
    (tmp_path / "valid_0").write_text("0 1:1\n")
    p = tmp_path / "c.cfg"
    p.write_text(f"""[General]
vocabulary_size = 10
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
[Train]
batch_size = 1
init_value_range = 0.01
factor_lambda = 0
bias_lambda = 0
epoch_num = 1
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
loss_type = logistic
train_files = {tmp_path}/train_0
{extra}
""")
    return str(p)


def test_config_defaults_and_keys(tmp_path):
    assert FMRunConfig().validation_auc is False and FMRunConfig().auc_tolerance is None
    c = load_config(_cfg_text(tmp_path), echo=False)
    assert c.validation_auc is False and c.auc_tolerance is None
    lines = []
    valid = f"validation_files = {tmp_path}/valid_0\ntolerance = 0.0\n"
    c = load_config(_cfg_text(tmp_path, valid + "validation_auc = true\nauc_tolerance = 0.75"), printer=lines.append)
    assert c.validation_auc is True and c.auc_tolerance == 0.75
    assert "  validation_auc = true" in lines and "  auc_tolerance = 0.75" in lines


def test_auc_tolerance_needs_validation_auc(tmp_path):
    valid = f"validation_files = {tmp_path}/valid_0\ntolerance = 0.0\n"
    with pytest.raises(ConfigError):
        load_config(_cfg_text(tmp_path, valid + "auc_tolerance = 0.75"), echo=False)
    with pytest.raises(ConfigError):
        load_config(_cfg_text(tmp_path, valid + "validation_auc = false\nauc_tolerance = 0.75"), echo=False)
    with pytest.raises(ConfigError):  # no validation files
        load_config(_cfg_text(tmp_path, "validation_auc = true\nauc_tolerance = 0.75"), echo=False)
