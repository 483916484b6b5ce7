"""Threshold metrics on gfx950 (hip/threshold_metrics.hip) against the numpy / Python-int oracle and the CPU twin:
sizes around the wave, the 2048-position tile and the 8192-key sort tile, tie runs across tile borders, the two
weighted modes, workspace reuse, streams and graph capture."""

import math

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K
from threshold_oracle import (PRECISION_TARGETS, RECALL_TARGETS, SPECIAL_LABELS, SPECIAL_SCORES, Oracle, assert_exact,
                              assert_real, make_case, rel_bound)

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 2047, 2049, 8191, 8192, 8193, 3 * 8192 + 77]
PT, RT = PRECISION_TARGETS, RECALL_TARGETS


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _run(s, y, w=None, device="cuda", pt=PT, rt=RT, **kw):
    return K.threshold_metrics(_t(s, device), _t(y, device), _t(w, device), precision_targets=pt, recall_targets=rt,
                               **kw)


def _bits(ts) -> list:
    return ts.rec.cpu().view(torch.int64).tolist()


def _exact_everywhere(s, y, w=None):
    """GPU == CPU twin in every word but the AP sum (another fixed order), and GPU == oracle."""
    gpu, cpu = _run(s, y, w), _run(s, y, w, "cpu")
    assert_exact(gpu, Oracle(s, y, w), PT, RT)
    assert _bits(gpu)[1:] == _bits(cpu)[1:]
    return gpu


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_unweighted_equal_to_oracle_and_cpu(n, ties):
    s, y, _ = make_case(n, n, ties=ties)
    st = _exact_everywhere(s, y).stats()
    assert all(isinstance(st[k], int) for k in ("P", "N"))


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_integer_weights_exact(n, ties):
    _exact_everywhere(*make_case(n, 3 * n, ties=ties, weights="int"))


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_real_weights_within_bounds_and_reproducible(n, ties):
    s, y, w = make_case(n, 7 * n, ties=ties, weights="real")
    ts, ty, tw = _t(s, "cuda"), _t(y, "cuda"), _t(w, "cuda")
    got = K.threshold_metrics(ts, ty, tw, precision_targets=PT, recall_targets=RT)
    assert_real(got, Oracle(s, y, w), PT, RT)
    again = K.threshold_metrics(ts, ty, tw, precision_targets=PT, recall_targets=RT)
    assert _bits(again) == _bits(got)  # bitwise, run to run


def test_final_block_reduces_several_partials_per_thread():
    n = 1_000_003  # 489 tiles for the 256 threads of the final block
    s, y, _ = make_case(n, 5, ties=True)
    gpu = _run(s, y)
    assert_exact(gpu, Oracle(s, y), PT, RT)
    assert _bits(gpu)[1:] == _bits(_run(s, y, device="cpu"))[1:]


def test_all_equal_scores_across_four_tiles():
    n = 3 * 2048 + 77
    y = make_case(n, 3)[1]
    s = np.full(n, -0.75, np.float32)
    ts = _exact_everywhere(s, y)
    p = int((y > 0).sum())
    assert abs(ts.ap() - p / n) <= 3 * rel_bound(n) * p / n and ts.ks() == (0.0, -0.75)  # (AP = P / W)
    assert ts.best_f1() == (2 * p / (n + p), -0.75, p / n, 1.0)
    assert ts.at_recall(0.25) == (-0.75, p / n, 1.0) and math.isnan(ts.at_precision(0.9)[0])


def test_special_values():
    ts = _exact_everywhere(SPECIAL_SCORES, SPECIAL_LABELS)
    assert ts.stats()["nans"] == 0
    # a +-0 run is one threshold, reported as +0.0
    ts = _run([0.0, -0.0, -1.0], [1, 0, 0], pt=(), rt=(1.0,))
    t, p, r = ts.at_recall(1.0)
    assert (t, p, r) == (0.0, 0.5, 1.0) and math.copysign(1.0, t) == 1.0
    # infinities are ordinary thresholds
    assert _run([np.inf, 1.0, -np.inf], [1, 0, 0], pt=(), rt=()).ks() == (1.0, np.inf)


def test_one_class_nan_scores_and_empty():
    n = 8193
    s, y, _ = make_case(n, 8)
    for labels in (np.zeros(n, np.float32), np.ones(n, np.float32)):
        assert_exact(_run(s, labels), Oracle(s, labels), PT, RT)
    s[[5, 8000]] = np.nan
    ts = _run(s, y)
    assert ts.stats()["nans"] == 2
    assert all(math.isnan(v) for v in (ts.ap(), *ts.ks(), *ts.best_f1(), *ts.at_precision(0.5), *ts.at_recall(0.5)))
    ts = K.threshold_metrics(torch.empty(0, device="cuda"), torch.empty(0, device="cuda"))
    assert math.isnan(ts.ap()) and ts.stats()["P"] == 0


def test_zero_weight_run_at_the_top():
    s = np.array([3.0, 3.0, 2.0, 1.0, 0.5], np.float32)
    y = np.array([1, 0, 1, 0, 1], np.float32)
    w = np.array([0, 0, 2, 1, 1], np.float32)
    ts = _exact_everywhere(s, y, w)
    assert ts.at_precision(1.0) == (2.0, 1.0, 2 / 3)  # (3.0 is no candidate: nothing is predicted there)


def test_reused_workspace_over_shrinking_n():
    n = 3 * 8192 + 77
    ws = K.threshold_workspace(n, torch.device("cuda"))
    for m in (n, 8193, 65):
        s, y, _ = make_case(m, m + 1, ties=True)
        assert_exact(_run(s, y, ws=ws), Oracle(s, y), PT, RT)


def test_non_default_stream():
    s, y, w = make_case(3 * 8192 + 77, 12, ties=True, weights="int")
    ts, ty, tw = _t(s, "cuda"), _t(y, "cuda"), _t(w, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a = K.threshold_metrics(ts, ty, precision_targets=PT, recall_targets=RT)
        b = K.threshold_metrics(ts, ty, tw, precision_targets=PT, recall_targets=RT)
    torch.cuda.current_stream().wait_stream(side)
    assert_exact(a, Oracle(s, y), PT, RT)
    assert_exact(b, Oracle(s, y, w), PT, RT)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_graph_replay_on_new_scores_equals_eager(weighted):
    n = 2 * 2048 + 77  # two full tiles and a partial one
    s, y, w = make_case(n, 21, weights="real" if weighted else None)
    dev = torch.device("cuda")
    ts, ty, tw = _t(np.round(16 * s) / 16, dev), _t(y, dev), _t(w, dev)  # (sixteenths: tie runs cross tile borders)
    ws = K.threshold_workspace(n, dev)
    kw = dict(precision_targets=PT, recall_targets=RT)
    K.threshold_metrics(ts, ty, tw, ws=ws, **kw).stats()  # (warm: the sort's self-check does not run in a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = K.threshold_metrics(ts, ty, tw, ws=ws, **kw)
    s2 = np.round(16 * np.random.default_rng(22).standard_normal(n)).astype(np.float32) / 16
    ts.copy_(_t(s2, dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = K.threshold_metrics(_t(s2, dev), ty, tw, **kw)
    assert _bits(st) == _bits(eager)  # (fp64 words: bit for bit)
    (assert_real if weighted else assert_exact)(st, Oracle(s2, y, w), PT, RT)


def test_workspace_bounds_and_targets():
    h = K.native.hip()
    assert h.threshold_workspace_bytes(0) > 0 and h.threshold_workspace_bytes(8193) > (5 * 4 + 2 * 8) * 8193
    with pytest.raises(ValueError):
        h.threshold_workspace_bytes(2**30)
    s, y, _ = make_case(8193, 2)
    with pytest.raises(ValueError, match="ws"):
        _run(s, y, ws=torch.empty(1024, dtype=torch.uint8, device="cuda"))
    for bad in ((0.0,), (1.5,), (0.1, 0.2, 0.3, 0.4, 0.5), (float("nan"),)):
        with pytest.raises(ValueError):
            _run(s, y, pt=bad, rt=())
        with pytest.raises(ValueError):
            _run(s, y, pt=(), rt=bad)
    rec = torch.empty(35, dtype=torch.int64, device="cuda")
    ws = K.threshold_workspace(8193, torch.device("cuda"))
    with pytest.raises(ValueError):  # the launcher's own check of the targets
        h.threshold_metrics(scores=_t(s, "cuda").data_ptr(), labels=_t(y, "cuda").data_ptr(), weights=0, n=8193,
                            precision_targets=[2.0], recall_targets=[], out=rec.data_ptr(), ws=ws.data_ptr(),
                            ws_bytes=ws.numel(), stream=0)
