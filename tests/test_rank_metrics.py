"""Ranking metrics on the CPU: the twin (csrc/cpu/kernels.cpp ``rank_metrics`` through ops/kernels.py) against the
pure-Python oracle on the case list the GPU chain is tested on, the oracle's tie rule against a brute-force
average over every tie-breaking permutation, the argument errors and the empty set.

Tolerance of twin against oracle: tests/rank_cases.py ``check`` -- (m + 8) 2^-52 relative, counts exact.  Oracle
against brute force: hits are equal Fractions; the DCGs differ by the rounding of the table (D[r] for r <= 6 is a
sum of <= 6 terms) against directly rounded 1 / log2(j + 1) and by the average over <= 720 permutations, so they
agree within 1e-13 relative."""

import itertools
import math

import numpy as np
import pytest
import torch

import rank_cases as C
import rank_oracle as R
from fast_tffm_amd.ops import native
from fast_tffm_amd.ops import kernels as K


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype))


def run(s, y, g, G, ks, device="cpu", **kw):
    return K.rank_metrics(_t(s).to(device), _t(y).to(device), _t(g, np.int32).to(device), G, ks, **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_twin_equals_oracle(name):
    s, y, g, G, ks, recs = C.case(name)
    C.check(run(s, y, g, G, ks), recs, len(s), G, ks)


def test_table_bits_are_shared():
    d = torch.empty(R.MAX_CUTOFF + 1, dtype=torch.float64)
    native.cpu().rank_dcg_table(out=d.data_ptr())
    assert d.tolist() == R.D


def test_nan_score_gives_nan_means_and_is_counted():
    s, y, g, G, ks = C.with_nan()
    st = run(s, y, g, G, ks)
    assert st.stats()[3] == 1
    assert all(math.isnan(f(k)) for k in ks for f in (st.ndcg, st.recall, st.precision))
    assert st.ranked_groups() == R.summary(C.case("special")[5], ks)[1]  # (the labels decide what is ranked)


def test_all_equal_scores_share_the_discount_mass():
    s, y, g, G, ks, _ = C.case("all-equal")
    per = run(s, y, g, G, ks).per_group()[0].tolist()
    n, pos = len(s), int((y > 0).sum())
    assert per[:2] == [n, pos]
    for c, k in enumerate(ks):
        assert per[2 + 3 * c] == pytest.approx(pos * R.D[k] / n, rel=1e-12)
        assert per[4 + 3 * c] == pytest.approx(pos * k / n, rel=1e-12)


def _multisets(size):
    kinds = list(itertools.product((0.0, 1.0, 2.0), (0.0, 1.0, 2.0)))  # (score, label)
    return itertools.combinations_with_replacement(kinds, size)


@pytest.mark.parametrize("size", range(1, 7))
def test_oracle_tie_rule_equals_the_average_over_tie_breaks(size):
    """Every group of ``size`` examples over a 3-level score alphabet and labels {0, 1, 2} (the metrics do not
    depend on the input order, so one arrangement per multiset covers them all)."""
    ks = (1, 3, 8)
    for group in _multisets(size):
        s, y = [e[0] for e in group], [e[1] for e in group]
        rec = R.group_record(s, y, ks)
        for c, (dcg, hits) in enumerate(R.brute_group(s, y, ks)):
            assert rec[4 + 3 * c] == hits
            assert rec[2 + 3 * c] == pytest.approx(dcg, rel=1e-13, abs=0)
        ideal = R.brute_group(y, y, ks)
        for c in range(len(ks)):
            assert rec[3 + 3 * c] == pytest.approx(ideal[c][0], rel=1e-13, abs=0)


def test_input_order_does_not_matter():
    s, y, g, G, ks, _ = C.case("same-scores")
    p = np.random.default_rng(5).permutation(len(s))
    a, b = run(s, y, g, G, ks), run(s[p], y[p], g[p], G, ks)
    assert (a.per_group()[:, :2] == b.per_group()[:, :2]).all()
    assert torch.allclose(a.per_group(), b.per_group(), rtol=1e-12, atol=0)


@pytest.mark.parametrize("ks", [(), (0,), (4097,), (5, 5), (10, 5), (1, 2, 3, 4, 5), (1.5,), (True,)])
def test_bad_cutoffs(ks):
    with pytest.raises(ValueError):
        run([0.0, 1.0], [1.0, 0.0], [0, 0], 1, ks)


def test_native_twin_rejects_bad_cutoffs():
    z = torch.zeros(8, dtype=torch.float64)
    with pytest.raises(ValueError):
        native.cpu().rank_metrics(n=0, G=1, scores=0, labels=0, groups=0, cutoffs=[3, 2], out=z.data_ptr(),
                                  per=z.data_ptr())


def test_argument_errors():
    s, y, g = _t([0.0, 1.0]), _t([1.0, 0.0]), _t([0, 0], np.int32)
    with pytest.raises(ValueError):
        K.rank_metrics(s, y[:1], g, 1, (1,))
    with pytest.raises(ValueError):
        K.rank_metrics(s, y, g.to(torch.int64), 1, (1,))
    with pytest.raises(ValueError):
        K.rank_metrics(s.double(), y, g, 1, (1,))
    with pytest.raises(ValueError):
        K.rank_metrics(s, y, g, 0, (1,))
    with pytest.raises(ValueError):
        K.rank_metrics(s, y, g, 1, (1,), ws=torch.empty(16, dtype=torch.uint8))
    st = K.rank_metrics(s, y, g, 1, (1, 5))
    with pytest.raises(KeyError):
        st.ndcg(2)
    with pytest.raises(ValueError):
        st.recall(1.0)
    assert st.ndcg(1) == 0.0 and st.recall(5) == 1.0 and st.precision(5) == 0.2


def test_out_of_range_ids_count_as_the_last_group():
    def twin(ids):  # (the native entry: FM_DEBUG_CHECKS=1 makes the op reject such ids)
        s, y, g = _t([1.0, 2.0, 3.0]), _t([1.0, 0.0, 1.0]), _t(ids, np.int32)
        rec, per = torch.empty(7, dtype=torch.int64), torch.empty((2, 5), dtype=torch.float64)
        native.cpu().rank_metrics(n=3, G=2, scores=s.data_ptr(), labels=y.data_ptr(), groups=g.data_ptr(),
                                  cutoffs=[1], out=rec.data_ptr(), per=per.data_ptr())
        return rec, per

    a, b = twin([0, 7, -1]), twin([0, 1, 1])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_empty_set():
    e = torch.empty(0)
    st = K.rank_metrics(e, e, e.to(torch.int32), 3, (1, 10))
    assert math.isnan(st.ndcg(1)) and math.isnan(st.recall(10)) and math.isnan(st.precision(10))
    assert st.ranked_groups() == 0 and math.isnan(st.coverage())
    assert st.per_group().shape == (3, 8) and not st.per_group().any()
