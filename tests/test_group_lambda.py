"""The CPU twin of hip/group_lambda.hip against the oracle of tests/group_lambda_oracle.py (its derived bound): the case
list of tests/group_loss_cases.py at K = 1, 3 and 0, the cases placed by the GPU op's geometry (tied scores keep a
gradient; the gradient sums to zero within a group), the exact zeros, the argument checks."""

import numpy as np
import pytest
import torch

import group_lambda_oracle as O
import group_loss_cases as C
from fast_tffm_amd.ops import kernels as K


def _run(g, s, y, k, gs, key_bits=None):
    plan = K.group_plan(torch.from_numpy(g), C.bits_for_ids(g) if key_bits is None else key_bits)
    d, loss = K.group_lambda_loss(plan, torch.from_numpy(s), torch.from_numpy(y), k, gs)
    return d.numpy(), float(loss)


@pytest.mark.parametrize("k", (1, 3, 0))
@pytest.mark.parametrize("n,grouping", C.CASES)
def test_cpu_twin_equals_oracle(n, grouping, k):
    for values in ("wide_scores", "graded_labels"):
        (g, s, y, gs), ref = O.case_ref(n, grouping, values, k)
        d, loss = _run(g, s, y, k, gs)
        O.check(d, loss, g, s, y, k, gs, what=f"{n}/{grouping}/{values}/{k}", ref=ref)
        if grouping in ("all_excluded", "singletons"):
            assert not d.any() and loss == 0.0


@pytest.mark.parametrize("name", O.GEOMETRY_CASES)
def test_cpu_twin_geometry_cases(name):
    g, s, y, k, gs = O.geometry_case(name)
    d, loss = _run(g, s, y, k, gs)
    O.check(d, loss, g, s, y, k, gs, what=name)
    assert loss > 0 and (name != "equal_scores" or np.count_nonzero(d[g == 1]) > 100)
    for grp in np.unique(g):
        dg = d[g == grp].astype(np.float64)
        assert abs(dg.sum()) <= 2.0 ** -22 * np.abs(dg).sum() + 1e-30


def test_exact_zeros_and_argument_checks():
    g, s, y, live = O.exact_zeros_case()
    d, loss = _run(g, s, y, 3, 0.5, key_bits=3)
    rest = np.setdiff1d(np.arange(g.size), live)
    assert (d[rest] == 0.0).all() and np.isfinite(d).all() and (d[live] != 0.0).all()
    O.check(d, loss, g, s, y, 3, 0.5, what="exact zeros")
    plan = K.group_plan(torch.zeros(3, dtype=torch.int32), 4)
    for n, cutoff in ((3, -1), (3, 4097), (4, 10)):
        with pytest.raises(ValueError):
            K.group_lambda_loss(plan, torch.zeros(n), torch.zeros(n), cutoff)
    assert K.RANK_LAMBDA_LOSS == "rank_lambda" and K.GROUP_LOSSES == K.RANK_LOSSES + (K.RANK_LAMBDA_LOSS,)
