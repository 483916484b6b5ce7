"""The isotonic fit's CPU twin (csrc/cpu/kernels.cpp ``isotonic`` / ``calib_apply`` through ops/kernels.py)
against the exact oracle of tests/isotonic_oracle.py, and the oracle against scipy where it imports.

Criteria: without weights, and with weights that are multiples of 1/64 in (0, 4] (every prefix sum and cross
product of n <= 2^18 such weights is exact in fp64), the block arrays equal the oracle's exactly.  With general
fp32 weights in [0.5, 2] the per-example fitted values are within 1e-9 of the oracle's: the values lie in [0, 1],
the fp64 sums of <= 2^17 terms err by <= n 2^-53 ~ 1.5e-11, and a near-tie between neighbouring slopes that the
rounded predicate decides the other way moves the values by no more than that."""

import numpy as np
import pytest
import torch

import isotonic_oracle as O
from fast_tffm_amd.ops import kernels as K


def _t(a, device="cpu"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def run(s, y, w=None, device="cpu", **kw):
    return K.isotonic_fit(_t(s, device), _t(y, device), _t(w, device), **kw)


def blocks_np(fit):
    return tuple(a.cpu().numpy() for a in fit.blocks())


CASES = {
    "logistic": lambda: O.logistic(5000, 1),
    "logistic_ties": lambda: O.logistic(5000, 2, ties=True),
    **O.LAYOUTS,
    "zeros": lambda: (np.array([-0.0, 0.0, -0.0, 0.0, 1.0, -1.0], np.float32),
                      np.array([1, 0, 0, 1, 1, 0], np.float32)),
    "inf": lambda: (np.array([np.inf, -np.inf, 0.5, np.inf, -np.inf, -2, 3e38, -3e38], np.float32),
                    np.array([1, 0, 1, 0, 1, 0, 1, 0], np.float32)),
    "denormal": lambda: (np.array([1e-45, -1e-45, 3e-45, 0.0, 2e-45, -3e-45, 1e-40, -1e-40], np.float32),
                         np.array([0, 1, 1, 0, 0, 0, 1, 1], np.float32)),
    "n1": lambda: (np.array([0.3], np.float32), np.array([1], np.float32)),
    "n2": lambda: (np.array([0.3, -0.3], np.float32), np.array([0, 1], np.float32)),
    "n2_up": lambda: (np.array([0.3, -0.3], np.float32), np.array([1, 0], np.float32)),
    "all_negative": lambda: (O.logistic(300, 3)[0], np.zeros(300, np.float32)),
    "all_positive": lambda: (O.logistic(300, 4, ties=True)[0], np.ones(300, np.float32)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_unweighted_blocks_are_exact(name):
    s, y = CASES[name]()
    f = O.fit(s, y)
    fit = run(s, y, want_fitted=True)
    O.check_exact(blocks_np(fit), f)
    assert fit.count() == len(f["v"]) and fit.totals() == (len(s), int((y > 0).sum()))
    assert np.array_equal(fit.fitted().numpy(), f["fitted"])
    if name in O.LAYOUT_BLOCKS:
        assert (len(s), fit.count()) == O.LAYOUT_BLOCKS[name]
    if name == "zeros":
        assert fit.count() == 3 and fit.blocks()[2].tolist() == [1, 4, 1]  # -0.0 and +0.0: one tie run
    if name in ("all_negative", "all_positive"):
        assert fit.blocks()[4].tolist() == [0.0 if name == "all_negative" else 1.0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_dyadic_weights_blocks_are_exact(name):
    s, y = CASES[name]()
    w = O.dyadic_weights(len(s), 11)
    fit = run(s, y, w, want_fitted=True)
    f = O.fit(s, y, w)
    O.check_exact(blocks_np(fit), f)
    assert np.array_equal(fit.fitted().numpy(), f["fitted"])


@pytest.mark.parametrize("name", ["logistic", "logistic_ties", "farey32_untied", "long_tie"])
def test_general_weights_fitted_values(name):
    s, y = CASES[name]()
    w = O.general_weights(len(s), 12)
    fit = run(s, y, w, want_fitted=True)
    O.check_close(fit.fitted().numpy(), O.fit(s, y, w))
    v = fit.blocks()[4].numpy()
    assert (np.diff(v) > 0).all()


@pytest.mark.parametrize("tile", [2, 3, 8, 64])
@pytest.mark.parametrize("name", ["logistic", "logistic_ties", "farey32_tied", "farey32_untied", "anti_sorted",
                                  "one_score", "long_tie", "n1", "n2", "zeros"])
def test_tile_hulls_and_bridges_give_the_serial_hull(name, tile):
    """The GPU's formulation (hulls of small tiles merged pairwise by their bridges) on the host."""
    s, y = CASES[name]()
    want = blocks_np(run(s, y))
    got = blocks_np(run(s, y, _cpu_tile=tile))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    w = O.dyadic_weights(len(s), 13)
    want = blocks_np(run(s, y, w))
    got = blocks_np(run(s, y, w, _cpu_tile=tile))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))


def test_nan_score_raises():
    s, y = O.logistic(100, 5)
    s[17] = np.nan
    fit = run(s, y)
    for reader in (fit.count, fit.blocks, fit.calibrator, fit.totals):
        with pytest.raises(ValueError, match="NaN"):
            reader()


def test_zero_weight_examples_are_dropped():
    s, y = O.logistic(2000, 6, ties=True)
    w = O.dyadic_weights(len(s), 14)
    w[::3] = 0
    keep = w > 0
    fit = run(s, y, w, want_fitted=True)
    ref = run(s[keep], y[keep], w[keep], want_fitted=True)
    assert all(torch.equal(a, b) for a, b in zip(fit.blocks(), ref.blocks()))
    full = fit.fitted().numpy()
    assert full.shape == s.shape and np.array_equal(full[keep], ref.fitted().numpy())
    x, yy = ref.calibrator()
    assert np.array_equal(full[~keep], K.calibrate_apply(_t(s[~keep]), x, yy).double().numpy())
    none = run(s, y, np.zeros(len(s), np.float32))
    assert none.count() == 0 and all(a.numel() == 0 for a in none.blocks())
    empty = K.isotonic_fit(torch.empty(0), torch.empty(0))
    assert empty.count() == 0
    with pytest.raises(ValueError):
        run(s, y, -w)


def test_argument_checks():
    s, y = O.logistic(10, 7)
    with pytest.raises(ValueError):
        K.isotonic_fit(_t(s).double(), _t(y))
    with pytest.raises(ValueError):
        K.isotonic_fit(_t(s), _t(y[:5]))
    with pytest.raises(ValueError):
        K.calibrate_apply(_t(s), torch.zeros(3), torch.zeros(3))
    with pytest.raises(ValueError):
        run(s, y).fitted()


@pytest.mark.parametrize("name", ["logistic", "farey32_tied", "separated", "one_score", "inf", "denormal"])
def test_calibrate_apply_against_the_fp64_rule(name):
    s, y = CASES[name]()
    fit = run(s, y)
    x, yy = fit.calibrator()
    ox, oy = O.calibrator(O.fit(s, y))
    assert np.array_equal(x.numpy(), ox) and np.array_equal(yy.numpy(), oy)
    grid = O.apply_grid(ox)
    got = K.calibrate_apply(_t(grid), x, yy).numpy()
    O.check_apply(got, grid, ox, oy)
    order = np.argsort(grid[~np.isnan(grid)], kind="stable")
    assert (np.diff(got[~np.isnan(grid)][order]) >= 0).all()  # monotone in the score


def test_apply_infinite_gap_ends():
    x = _t(np.array([-np.inf, -np.inf, 0, 1, np.inf, np.inf]))
    y = _t(np.array([0.1, 0.1, 0.5, 0.5, 0.9, 0.9]))
    got = K.calibrate_apply(_t(np.array([-np.inf, -5, 0, 0.5, 1, 7, np.inf])), x, y).tolist()
    assert got == [np.float32(v) for v in (0.1, 0.5, 0.5, 0.5, 0.5, 0.5, 0.9)]
    x = _t(np.array([-np.inf, -np.inf, np.inf, np.inf]))
    y = _t(np.array([0.25, 0.25, 0.75, 0.75]))
    assert K.calibrate_apply(_t(np.array([0.0, -1e30, 3e38])), x, y).tolist() == [0.5, 0.5, 0.5]


def test_oracle_against_scipy():
    """A second opinion on the oracle: scipy's pool-adjacent-violators on pre-pooled ties."""
    so = pytest.importorskip("scipy.optimize")
    if not hasattr(so, "isotonic_regression"):
        pytest.skip("scipy.optimize.isotonic_regression needs scipy >= 1.12")
    for ties, weighted in ((False, False), (True, False), (True, True)):
        s, y = O.logistic(5000, 20 + ties, ties=ties)
        w = O.general_weights(len(s), 22) if weighted else None
        f = O.fit(s, y, w)
        order, sv = O.sort_order(s)
        w64 = np.ones(len(s)) if w is None else w.astype(np.float64)
        starts = np.flatnonzero(np.r_[True, sv[1:] != sv[:-1]])
        pw = np.add.reduceat(w64[order], starts)
        py = np.add.reduceat((w64 * (y > 0))[order], starts) / pw
        r = so.isotonic_regression(py, weights=pw)
        per_run = f["fitted"][order][starts]
        assert np.abs(r.x - per_run).max() <= 1e-12
        assert len(r.blocks) - 1 >= len(f["v"])  # (scipy keeps neighbouring blocks of equal value apart)
