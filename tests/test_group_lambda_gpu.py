"""The LambdaRank loss on the GPU (hip/group_lambda.hip through ``ops.kernels.group_lambda_loss``) against the fp64
oracle of tests/group_lambda_oracle.py, within its derived bound: the case list of tests/group_loss_cases.py at K = 1,
3 and 0; the cases placed by the kernel's geometry; the exact zeros; bitwise repeatability -- two calls, a workspace
filled with 0xFF and last used by a larger call, a captured graph replayed on new inputs; one plan feeding all three
group losses."""

import numpy as np
import pytest
import torch

import group_lambda_oracle as O
import group_loss_cases as C
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda")


def run(g, s, y, k, gs, key_bits=None, ws=None, lws=None):
    plan = K.group_plan(_t(g, np.int32), C.bits_for_ids(g) if key_bits is None else key_bits, ws=ws)
    d, loss = K.group_lambda_loss(plan, _t(s), _t(y), k, gs, ws=lws)
    return d.cpu().numpy().tobytes(), loss.cpu().numpy().tobytes()


def checked(g, s, y, k, gs, what, ref=None, **kw):
    d, loss = run(g, s, y, k, gs, **kw)
    d, loss = np.frombuffer(d, np.float32), float(np.frombuffer(loss, np.float32)[0])
    O.check(d, loss, g, s, y, k, gs, what=what, ref=ref)
    return d, loss


@pytest.mark.parametrize("k", (1, 3, 0))
@pytest.mark.parametrize("n,grouping", C.CASES)
def test_gpu_equals_oracle(n, grouping, k):
    for values in ("wide_scores", "graded_labels"):
        (g, s, y, gs), ref = O.case_ref(n, grouping, values, k)
        d, loss = checked(g, s, y, k, gs, f"{n}/{grouping}/{values}/{k}", ref)
        if grouping in ("all_excluded", "singletons"):
            assert not d.any() and loss == 0.0
    K.check_device_errors()


@pytest.mark.parametrize("name", O.GEOMETRY_CASES)
def test_geometry_cases(name):
    assert K.group_lambda_geometry() == (O.ROWS, O.CHUNK, O.SLABS) and O.ROWS == C.TILE
    g, s, y, k, gs = O.geometry_case(name)
    d, loss = checked(g, s, y, k, gs, name)
    assert loss > 0 and (name != "equal_scores" or np.count_nonzero(d[g == 1]) > 100)   # ties keep a gradient
    K.check_device_errors()


def test_exact_zeros():
    g, s, y, live = O.exact_zeros_case()
    d, _ = checked(g, s, y, 3, 0.5, "exact zeros", key_bits=3)
    rest = np.setdiff1d(np.arange(g.size), live)
    assert (d[rest] == 0.0).all() and np.isfinite(d).all() and (d[live] != 0.0).all()
    g, s, y, _, gs = C.case(C.TILE + 1, "no_positive", "graded_labels")
    d, _ = checked(g, s, y, 3, gs, "no positive")
    dead = np.isin(g, [k for k in np.unique(g) if not (y[g == k] > 0).any()])
    assert dead.any() and (d[dead] == 0.0).all()
    K.check_device_errors()


def test_repeatable_and_workspace_reuse():
    gb, sb, yb, _, gsb = C.case(3 * C.TILE + 5, "zipf", "graded_labels")
    g, s, y, _, gs = C.case(C.TILE + 1, "excluded_scattered", "graded_labels")
    first = run(g, s, y, 3, gs)
    assert first == run(g, s, y, 3, gs)
    ws, lws = K.group_loss_workspace(len(gb), "cuda"), K.group_lambda_workspace(len(gb), "cuda")
    ws.fill_(0xFF)
    lws.fill_(0xFF)
    assert first == run(g, s, y, 3, gs, lws=lws)   # the lambda workspace straight after the fill
    run(gb, sb, yb, 0, gsb, ws=ws, lws=lws)
    assert first == run(g, s, y, 3, gs, ws=ws, lws=lws)
    K.check_device_errors()


def test_graph_replays_equal_eager():
    n = 3 * C.TILE + 5
    a = C.case(n, "zipf", "graded_labels")
    g, s, y = _t(a[0], np.int32), _t(a[1]), _t(a[2])
    ws, lws = K.group_loss_workspace(n, "cuda"), K.group_lambda_workspace(n, "cuda")
    dpred = torch.empty(n, dtype=torch.float32, device="cuda")
    K.group_lambda_loss(K.group_plan(g, 10, ws=ws), s, y, 10, a[4], dpred=dpred, ws=lws)   # eager once: lazy loads
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, loss = K.group_lambda_loss(K.group_plan(g, 10, ws=ws), s, y, 10, a[4], dpred=dpred, ws=lws)
    for grouping in ("excluded_scattered", "span_three_tiles", "zipf"):   # several replays, each on new inputs
        b = C.case(n, grouping, "graded_labels")
        for t, src, dt in ((g, b[0], np.int32), (s, b[1], np.float32), (y, b[2], np.float32)):
            t.copy_(_t(src, dt))
        graph.replay()
        torch.cuda.synchronize()
        got = dpred.cpu().numpy().tobytes(), loss.cpu().numpy().tobytes()
        assert got == run(b[0], b[1], b[2], 10, a[4], key_bits=10), grouping
    del graph
    K.check_device_errors()


def test_one_plan_feeds_all_three_losses():
    g, s, y, w, gs = C.case(3 * C.TILE + 5, "zipf", "weights")
    plan = K.group_plan(_t(g, np.int32), C.bits_for_ids(g))
    before = [x.clone() for x in (plan.sidx, plan.first, plan.end)]
    ts, ty, tw = _t(s), _t(y), _t(w)
    alone = [op(plan, ts, ty, tw, gs) for op in (K.group_softmax_loss, K.group_pairwise_loss)]
    dl, ll = K.group_lambda_loss(plan, ts, ty, 10, gs)
    after = [op(plan, ts, ty, tw, gs) for op in (K.group_softmax_loss, K.group_pairwise_loss)]
    torch.cuda.synchronize()
    assert all(torch.equal(x, z) for x, z in zip(before, (plan.sidx, plan.first, plan.end)))
    assert all(torch.equal(d0, d1) and torch.equal(l0, l1) for (d0, l0), (d1, l1) in zip(alone, after))
    O.check(dl.cpu().numpy(), float(ll), g, s, y, 10, gs, what="lambda on a shared plan")
    K.check_device_errors()
