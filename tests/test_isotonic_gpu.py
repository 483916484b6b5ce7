"""The isotonic fit on the GPU (hip/isotonic.hip through ops/kernels.py ``isotonic_fit`` / ``calibrate_apply``)
against the exact oracle of tests/isotonic_oracle.py and against the CPU twin.

Sizes: one tile of 2048 points of [0, n]; a tile edge on, before and after a point; an odd node at several merge
levels; five levels.  Layouts: one tie run across all tiles, two blocks, a bridge from the first vertex to the
last at every merge, Farey staircases (every vertex survives every merge), a tie run over three tiles.

Criteria as in tests/test_isotonic.py: exact block arrays without weights and with weights that are multiples of
1/64 in (0, 4]; fitted values within 1e-9 with general fp32 weights in [0.5, 2] (fp64 sums of <= 2^17 terms err
by <= n 2^-53 ~ 1.5e-11; a near-tie decided the other way moves the values by no more)."""

import functools

import numpy as np
import pytest
import torch

import isotonic_oracle as O
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 2047, 2048, 2049, 4097, 5 * 2048 + 13, 20 * 2048 + 1]


def _t(a, device="cuda"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def run(s, y, w=None, device="cuda", **kw):
    return K.isotonic_fit(_t(s, device), _t(y, device), _t(w, device), **kw)


def blocks_np(fit):
    return tuple(a.cpu().numpy() for a in fit.blocks())


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("n"):
        n = int(name[1:])
        s, y = O.logistic(n, 100 + n % 97, ties=n % 2 == 0)
    else:
        s, y = O.LAYOUTS[name]()
    return s, y, O.dyadic_weights(len(s), 31), O.general_weights(len(s), 32)


@functools.lru_cache(maxsize=None)
def oracle(name, mode):
    s, y, wd, wg = case(name)
    return O.fit(s, y, {"none": None, "dyadic": wd, "general": wg}[mode])


NAMES = [f"n{n}" for n in SIZES] + sorted(O.LAYOUTS)


@pytest.mark.parametrize("name", NAMES)
def test_unweighted_blocks_are_exact(name):
    s, y, _, _ = case(name)
    f = oracle(name, "none")
    fit = run(s, y, want_fitted=True)
    O.check_exact(blocks_np(fit), f)
    assert fit.totals() == (len(s), int((y > 0).sum()))
    assert np.array_equal(fit.fitted().cpu().numpy(), f["fitted"])
    if name in O.LAYOUT_BLOCKS:
        assert (len(s), fit.count()) == O.LAYOUT_BLOCKS[name]
    cpu = run(s, y, device="cpu")
    assert all(torch.equal(a.cpu(), b) for a, b in zip(fit.blocks(), cpu.blocks()))
    assert torch.equal(fit.rec.cpu(), cpu.rec)


@pytest.mark.parametrize("name", NAMES)
def test_dyadic_weights_blocks_are_exact(name):
    s, y, w, _ = case(name)
    f = oracle(name, "dyadic")
    fit = run(s, y, w, want_fitted=True)
    O.check_exact(blocks_np(fit), f)
    assert np.array_equal(fit.fitted().cpu().numpy(), f["fitted"])
    cpu = run(s, y, w, device="cpu")
    assert all(torch.equal(a.cpu(), b) for a, b in zip(fit.blocks(), cpu.blocks()))


@pytest.mark.parametrize("name", NAMES)
def test_general_weights_fitted_values(name):
    s, y, _, w = case(name)
    fit = run(s, y, w, want_fitted=True)
    O.check_close(fit.fitted().cpu().numpy(), oracle(name, "general"))
    assert (np.diff(fit.blocks()[4].cpu().numpy()) > 0).all()


@pytest.mark.parametrize("mode", ["none", "general"])
def test_repeatable_and_workspace_reuse(mode):
    s, y, _, wg = case("n10253")
    w = wg if mode == "general" else None
    first = run(s, y, w, want_fitted=True)
    b1, f1, r1 = first.blocks(), first.fitted().clone(), first.rec.clone()
    ws = K.isotonic_workspace(len(s), torch.device("cuda"))
    ws.fill_(0xA5)
    for _ in range(2):  # a fresh workspace full of garbage, then the same one again
        again = run(s, y, w, want_fitted=True, ws=ws)
        assert all(torch.equal(a, b) for a, b in zip(again.blocks(), b1))
        assert torch.equal(again.fitted(), f1) and torch.equal(again.rec, r1)
    small, ys = O.logistic(300, 9)  # a smaller fit in the larger workspace
    with pytest.raises(ValueError):
        run(small, ys, ws=ws[:1000])


def test_record_carries_nan_count_and_sort_word():
    s, y, _, _ = case("n4097")
    s = s.copy()
    s[[5, 3000]] = np.nan
    fit = run(s, y, want_fitted=True)
    torch.cuda.synchronize()
    rec = fit.rec.tolist()
    assert rec[3] == 2 and rec[4] == 0 and rec[1] == len(s)
    for reader in (fit.count, fit.blocks, fit.calibrator, fit.fitted):
        with pytest.raises(ValueError, match="NaN"):
            reader()
    K.check_device_errors()


def test_zero_weights_are_dropped_on_the_gpu():
    s, y, w, _ = case("n4097")
    w = w.copy()
    w[::4] = 0
    keep = w > 0
    fit = run(s, y, w)
    ref = run(s[keep], y[keep], w[keep])
    assert all(torch.equal(a, b) for a, b in zip(fit.blocks(), ref.blocks()))


@pytest.mark.parametrize("name", ["one_score", "separated", "farey32_tied", "n5000"])
def test_calibrate_apply(name):
    s, y, _, _ = case(name)
    f = oracle(name, "none")
    ox, oy = O.calibrator(f)
    x, yy = run(s, y).calibrator()
    assert np.array_equal(x.cpu().numpy(), ox) and np.array_equal(yy.cpu().numpy(), oy)
    if name in O.LAYOUT_BLOCKS:
        assert len(ox) == 2 * O.LAYOUT_BLOCKS[name][1]  # m = 1, 2, 325
    grid = O.apply_grid(ox)
    got = K.calibrate_apply(_t(grid), x, yy).cpu()
    O.check_apply(got.numpy(), grid, ox, oy)
    cpu = K.calibrate_apply(_t(grid, "cpu"), x.cpu(), yy.cpu())
    both = torch.stack((got, cpu)).numpy()
    assert np.array_equal(np.isnan(both[0]), np.isnan(both[1]))
    assert np.nanmax(np.abs(both[0] - both[1]), initial=0.0) <= 2.0 ** -21  # (each within 2^-22 of the fp64 rule)
    assert K.calibrate_apply(torch.empty(0, device="cuda"), x, yy).numel() == 0
