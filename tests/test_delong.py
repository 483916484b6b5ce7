"""``K.auc_delong`` on the CPU twin against the Python-int oracle (delong_oracle.py) and, for small inputs, a brute
force from the P x N comparison matrix: the record word for word, the derived values, every edge case."""

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K
from delong_oracle import MOMENTS, Oracle, brute_force, expected_moments, make_case, moments_case

SIZES = [2, 3, 64, 2049, 8193]


def _t(a, device="cpu"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _run(a, y, b=None, device="cpu", **kw):
    return K.auc_delong(_t(a, device), _t(y, device), _t(b, device), **kw)


def _words(st) -> list:
    return st.rec.cpu().tolist()


def _nan(*vals) -> bool:
    return all(isinstance(v, float) and math.isnan(v) for v in vals)


@pytest.mark.parametrize("seed", range(20))
def test_oracle_equals_brute_force(seed):
    n = 40 + 13 * seed
    a, b, y = make_case(n, 100 + seed, ties=seed % 2 == 1)
    o, bf = Oracle(a, y, b), brute_force(a, y, b)
    assert [o.theta("a"), o.theta("b")] == bf["theta"]  # (rationals: exactly)
    assert [[o.cov("a", "a"), o.cov("a", "b")], [o.cov("a", "b"), o.cov("b", "b")]] == bf["cov"]
    assert o.var_diff() >= 0


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_record_equal_to_oracle(n, ties, two):
    a, b, y = make_case(n, n + 7, ties=ties, two=two)
    if n <= 3:
        y[:2] = [1, 0]
    o = Oracle(a, y, b)
    ds = _run(a, y, b)
    assert _words(ds) == o.words()
    st = ds.stats()
    assert all(isinstance(v, int) for v in st.values())
    assert (st["U2_a"], st["P"], st["N"], st["has_b"]) == (o.U2["a"], o.P, o.N, int(two))
    assert st["m_pos_aa"] == o.moment("a", "a", True) and st["m_neg_aa"] == o.moment("a", "a", False)
    assert ds.auc() == float(o.theta()) == K.auc(_t(a), _t(y)).value()
    if two:
        assert st["m_pos_ab"] == o.moment("a", "b", True) and st["m_neg_bb"] == o.moment("b", "b", False)
        assert ds.auc_other() == float(o.theta("b"))
    if o.P >= 2 and o.N >= 2:
        assert ds.variance() == float(o.cov()) and ds.std_error() == math.sqrt(float(o.cov()))
        assert ds.interval(0.9) == o.interval(0.9) and ds.interval() == o.interval(0.95)
        if two:
            assert ds.covariance() == float(o.cov("a", "b")) and ds.difference() == o.difference()


def test_sum_of_placements_is_the_same_over_both_classes():
    a, b, y = make_case(2049, 3, ties=True)
    o = Oracle(a, y, b)  # (asserts the identity for both models)
    for m, s in (("a", a), ("b", b)):
        neg = sum(v for v, p in zip(o.pl[m], o.pos) if not p)
        assert neg == o.U2[m] == K.auc(_t(s), _t(y)).stats()[0]


def test_other_equal_to_scores():
    a, _, y = make_case(2049, 4, ties=True)
    ds = _run(a, y, a)
    assert ds.difference() == (0.0, 0.0, 0.0, 1.0)
    assert ds.covariance() == ds.variance() and ds.auc() == ds.auc_other()


def test_other_negated():
    a, _, y = make_case(2049, 5, ties=True)
    ds = _run(a, y, -a)
    st = ds.stats()
    assert st["U2_b"] == 2 * st["P"] * st["N"] - st["U2_a"]
    assert Fraction(st["U2_b"], 2 * st["P"] * st["N"]) == 1 - Fraction(st["U2_a"], 2 * st["P"] * st["N"])
    assert ds.covariance() == -ds.variance()


def test_separable():
    y = np.array([0, 0, 0, 1, 1, 1, 1], np.float32)
    s = np.array([-3, -2, -1, 1, 2, 3, 4], np.float32)
    ds = _run(s, y, -s)
    assert (ds.auc(), ds.variance(), ds.std_error(), ds.interval()) == (1.0, 0.0, 0.0, (1.0, 1.0))
    d, se, z, p = ds.difference()  # no variance, unequal AUCs
    assert (d, se, z, p) == (1.0, 0.0, math.inf, 0.0)
    assert _run(-s, y, s).difference() == (-1.0, 0.0, -math.inf, 0.0)


def test_small_classes():
    s = np.array([0.5, 0.25, 0.75, 0.1], np.float32)
    for y in ([0, 0, 0, 0], [1, 1, 1, 1]):  # P or N of 0: nothing is defined
        ds = _run(s, np.array(y, np.float32), s)
        assert _nan(ds.auc(), ds.auc_other(), ds.variance(), ds.std_error(), *ds.interval(), ds.covariance(),
                    *ds.difference())
    for y in ([1, 0, 0, 0], [0, 1, 1, 1]):  # P or N of 1: the AUCs alone
        y = np.array(y, np.float32)
        ds = _run(s, y, -s)
        o = Oracle(s, y, -s)
        assert ds.auc() == float(o.theta()) and ds.auc_other() == float(o.theta("b"))
        assert _nan(ds.variance(), ds.std_error(), *ds.interval(), ds.covariance(), *ds.difference()[1:])
        assert ds.difference()[0] == float(o.theta() - o.theta("b"))
        assert _words(ds) == o.words()


def test_nan_scores_per_model():
    a, b, y = make_case(300, 6)
    bad = a.copy()
    bad[[5, 200]] = np.nan
    for ds, counts in ((_run(bad, y, b), (2, 0)), (_run(a, y, bad), (0, 2)), (_run(bad, y), (2, 0))):
        st = ds.stats()
        assert (st["nans_a"], st["nans_b"]) == counts
        assert _nan(ds.auc(), ds.variance(), ds.std_error(), *ds.interval())
        if st["has_b"]:
            assert _nan(ds.auc_other(), ds.covariance(), *ds.difference())


def test_zeros_and_infinities():
    y = np.array([1, 0, 1, 0, 1, 0, 0, 1], np.float32)
    a = np.array([0.0, -0.0, np.inf, -np.inf, -0.0, 0.0, np.inf, 1e-45], np.float32)
    b = np.array([-np.inf, -np.inf, 0.0, 3.0, np.inf, -0.0, 1.0, -1.0], np.float32)
    o = Oracle(a, y, b)
    ds = _run(a, y, b)
    assert _words(ds) == o.words() and ds.stats()["nans_a"] == 0
    assert o.pl["a"][0] == o.pl["a"][4] == 1 + 3  # (+-0: one run with the two negative zeros; -inf below)
    assert ds.difference() == o.difference()


def test_empty_input():
    e = torch.empty(0)
    ds = K.auc_delong(e, e)
    assert _nan(ds.auc(), ds.variance(), *ds.interval()) and ds.stats()["P"] == 0 and not ds.stats()["has_b"]
    with pytest.raises(ValueError):
        ds.auc_other()
    assert _nan(*K.auc_delong(e, e, e).difference())


def test_argument_checks():
    a, b, y = make_case(64, 9)
    ds = _run(a, y)
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError):
            ds.interval(bad)
    for call in (ds.auc_other, ds.covariance, ds.difference):
        with pytest.raises(ValueError):  # no other model
            call()
    with pytest.raises(ValueError):
        K.auc_delong(_t(a), _t(y), _t(b[:63]))
    with pytest.raises(ValueError):
        K.auc_delong(_t(a), _t(y), _t(b).double())
    with pytest.raises(TypeError):
        K.auc_delong(_t(a), _t(y), weights=_t(y))  # no weights: see the docstring
    with pytest.raises(ValueError):
        K.auc_delong(_t(a), _t(y), ws=torch.empty(8, dtype=torch.uint8))  # the workspace is a GPU argument


def test_placement_moments_near_2_31():
    pa, pb, y = moments_case()
    ta, tb = torch.from_numpy(pa.astype(np.int32)), torch.from_numpy(pb.astype(np.int32))
    want = expected_moments(pa, pb, y)
    assert want[0] > 2**31 * 1000  # (the hi word of M_pos(a, a): about n / 2 terms of 2^30 each)
    assert K.placement_moments(ta, tb, _t(y)).tolist() == want
    assert K.placement_moments(ta, None, _t(y)).tolist() == want[:4] + [0] * 8
    for name, i in zip(MOMENTS, range(6)):
        keep = (y > 0) == (i % 2 == 0)
        x, z = ((pa, pa), (pb, pb), (pa, pb))[i // 2]
        whole = sum(u * v for u, v in zip(x[keep].tolist(), z[keep].tolist()))
        assert (want[2 * i] << 32) + want[2 * i + 1] == whole, name
