"""Threshold metrics on the CPU (csrc/cpu/kernels.cpp ``threshold_metrics``, the twin of hip/threshold_metrics.hip)
against the numpy / Python-int oracle, scikit-learn and scipy, and the degenerate inputs."""

import math

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K
from threshold_oracle import (PRECISION_TARGETS, RECALL_TARGETS, SPECIAL_LABELS, SPECIAL_SCORES, Oracle, assert_exact,
                              assert_real, brute_force, make_case, rel_bound)

PT, RT = PRECISION_TARGETS, RECALL_TARGETS
SIZES = [1, 2, 63, 65, 2049, 8193]


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32))


def _run(s, y, w=None, pt=PT, rt=RT):
    return K.threshold_metrics(_t(s), _t(y), _t(w), precision_targets=pt, recall_targets=rt)


@pytest.mark.parametrize("weights", [None, "int"], ids=["unweighted", "int"])
@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_twin_equals_the_oracle_in_every_integer_and_threshold(n, ties, weights):
    s, y, w = make_case(n, 5 * n + 1, ties=ties, weights=weights)
    ts = _run(s, y, w)
    assert_exact(ts, Oracle(s, y, w), PT, RT)
    assert ts.rec.dtype == (torch.int64 if w is None else torch.float64)


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_real_weights_within_the_derived_bounds(n, ties):
    s, y, w = make_case(n, 7 * n, ties=ties, weights="real")
    assert_real(_run(s, y, w), Oracle(s, y, w), PT, RT)


@pytest.mark.parametrize("weights", [None, "int", "real"])
@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
def test_oracle_equals_the_definitions_threshold_by_threshold(ties, weights):
    s, y, w = make_case(40, 9, ties=ties, weights=weights)
    o = Oracle(s, y, w)
    ap, ks, ks_t, f1, f1_t = brute_force(s, y, w)
    assert abs(o.ap() - float(ap)) <= 1e-15 and o.ks()[0] == float(ks) and o.best_f1()[0] == float(f1)
    assert float(o.thr[o.ks()[1]]) == ks_t and float(o.thr[o.best_f1()[1]]) == f1_t
    ap, ks, ks_t, f1, f1_t = brute_force(SPECIAL_SCORES, SPECIAL_LABELS)
    o = Oracle(SPECIAL_SCORES, SPECIAL_LABELS)
    assert abs(o.ap() - float(ap)) <= 1e-15 and (o.ks()[0], float(o.thr[o.ks()[1]])) == (float(ks), ks_t)
    assert_exact(_run(SPECIAL_SCORES, SPECIAL_LABELS), o, PT, RT)


def test_against_scikit_learn_and_scipy():
    metrics = pytest.importorskip("sklearn.metrics")
    stats = pytest.importorskip("scipy.stats")
    for ties, weights in ((False, None), (True, None), (True, "real")):
        s, y, w = make_case(3001, 17, ties=ties, weights=weights)
        ts = _run(s, y, w)
        want = metrics.average_precision_score(y > 0, s, sample_weight=w)
        assert abs(ts.ap() - want) <= 1e-12 * want
        if w is None:  # the two-sample KS statistic: the greatest distance between the classes' score CDFs
            want = stats.ks_2samp(s[y > 0], s[~(y > 0)]).statistic
            assert abs(ts.ks()[0] - want) <= 1e-12
        p, r, _ = metrics.precision_recall_curve(y > 0, s, sample_weight=w)
        f1 = np.max(2 * p * r / np.maximum(p + r, 1e-300))
        assert abs(ts.best_f1()[0] - f1) <= 1e-12


def test_one_class_nan_score_and_tiny_n():
    s, y, _ = make_case(100, 3)
    for labels in (np.zeros(100, np.float32), np.ones(100, np.float32)):
        ts = _run(s, labels)
        assert_exact(ts, Oracle(s, labels), PT, RT)
        assert math.isnan(ts.ap()) and math.isnan(ts.at_recall(1.0)[0]) and math.isnan(ts.at_precision(0.5)[0])
    s[7] = np.nan
    ts = _run(s, y)
    assert ts.stats()["nans"] == 1
    assert all(math.isnan(v) for v in (ts.ap(), *ts.ks(), *ts.best_f1(), *ts.at_precision(0.5), *ts.at_recall(0.5)))
    ts = K.threshold_metrics(torch.empty(0), torch.empty(0), precision_targets=PT, recall_targets=RT)
    assert math.isnan(ts.ap()) and ts.stats()["P"] == 0 and ts.n == 0
    assert math.isnan(_run([0.5], [1.0]).ap())
    ts = _run([0.25, 0.5], [1.0, 0.0])  # the positive ranks last: precision 1/2 at recall 1
    assert ts.ap() == 0.5 and ts.ks() == (1.0, 0.5) and ts.best_f1() == (2 / 3, 0.25, 0.5, 1.0)


def test_all_scores_equal():
    y = make_case(500, 4)[1]
    s = np.full(500, 1.5, np.float32)
    p = int((y > 0).sum())
    ts = _run(s, y)
    tol = 3 * rel_bound(500)  # (the numerator is a sum of P rounded terms: the AP's bound, not equality)
    assert abs(ts.ap() - p / 500) <= tol * p / 500 and ts.ks() == (0.0, 1.5) and len(Oracle(s, y).thr) == 1
    assert ts.best_f1() == (2 * p / (500 + p), 1.5, p / 500, 1.0)
    w = np.full(500, 0.5, np.float32)
    assert abs(_run(s, y, w).ap() - (p * 0.5) / (500 * 0.5)) <= tol * p / 500  # AP = P / W


def test_zero_weight_run_at_the_top_is_no_candidate():
    s = np.array([3.0, 3.0, 2.0, 1.0, 0.5], np.float32)
    y = np.array([1, 0, 1, 0, 1], np.float32)
    w = np.array([0, 0, 2, 1, 1], np.float32)
    ts = _run(s, y, w)
    assert_exact(ts, Oracle(s, y, w), PT, RT)
    assert ts.at_precision(1.0) == (2.0, 1.0, 2 / 3) and ts.ks()[1] == 2.0
    assert ts.ap() == (2 * 1.0 + 1 * 0.75) / 3


def test_targets_nobody_reaches_and_full_recall():
    s = np.array([0.9, 0.8, 0.7, 0.6], np.float32)
    y = np.array([0, 1, 0, 1], np.float32)
    ts = _run(s, y, pt=(0.75, 0.5), rt=(1.0, 0.5))
    assert all(math.isnan(v) for v in ts.at_precision(0.75)) and ts.stats()["precision"][0] is None
    assert ts.at_precision(0.5) == (np.float32(0.6), 0.5, 1.0)  # the greatest recall, not the first to qualify
    assert ts.at_recall(1.0) == (np.float32(0.6), 0.5, 1.0) and ts.at_recall(0.5) == (np.float32(0.8), 0.5, 0.5)
    with pytest.raises(ValueError, match="not one of"):
        ts.at_recall(0.9)


def test_zero_threshold_is_reported_as_plus_zero():
    t, p, r = _run([0.0, -0.0, -1.0], [1, 0, 0], pt=(), rt=(1.0,)).at_recall(1.0)
    assert (t, p, r) == (0.0, 0.5, 1.0) and math.copysign(1.0, t) == 1.0


def test_target_validation():
    s, y, _ = make_case(10, 1)
    for bad in ((0.0,), (1.5,), (-0.1,), (0.1, 0.2, 0.3, 0.4, 0.5), (float("nan"),)):
        with pytest.raises(ValueError, match="precision_targets"):
            _run(s, y, pt=bad, rt=())
        with pytest.raises(ValueError, match="recall_targets"):
            _run(s, y, pt=(), rt=bad)
    with pytest.raises(ValueError):  # the twin's own check
        K.native.cpu().threshold_metrics(n=10, scores=_t(s).data_ptr(), labels=_t(y).data_ptr(), weights=0,
                                         precision_targets=[], recall_targets=[2.0],
                                         out=torch.empty(35, dtype=torch.int64).data_ptr())
    assert _run(s, y, pt=0.5, rt=1).precision_targets == (0.5,)  # a single number is one target
    with pytest.raises(ValueError, match="workspace"):
        K.threshold_metrics(_t(s), _t(y), ws=torch.empty(8, dtype=torch.uint8))
    with pytest.raises(ValueError, match="labels"):
        K.threshold_metrics(_t(s), _t(y)[:5])
