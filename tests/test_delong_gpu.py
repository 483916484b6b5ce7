"""``K.auc_delong`` on gfx950 (hip/auc_delong.hip) against the CPU twin and the Python-int oracle, word for word:
sizes around the wave, the 2048-position tile and the 8192-key sort tile, tie runs across tile borders, one and two
models, workspace reuse, streams and graph capture."""

import math

import numpy as np
import pytest
import torch

from fast_tffm_amd.ops import kernels as K
from delong_oracle import Oracle, expected_moments, make_case, moments_case

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 2047, 2049, 8191, 8192, 8193, 3 * 8192 + 77]


def _t(a, device="cuda"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _run(a, y, b=None, device="cuda", **kw):
    return K.auc_delong(_t(a, device), _t(y, device), _t(b, device), **kw)


def _words(st) -> list:
    return st.rec.cpu().tolist()


def _exact_everywhere(a, y, b=None, **kw):
    """GPU record == CPU twin's == oracle's, word for word; so are the floats derived from them."""
    gpu, cpu = _run(a, y, b, **kw), _run(a, y, b, "cpu")
    assert _words(gpu) == _words(cpu) == Oracle(a, y, b).words()
    return gpu


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_record_equal_to_cpu_and_oracle(n, ties, two):
    a, b, y = make_case(n, n + 7, ties=ties, two=two)
    gpu = _exact_everywhere(a, y, b)
    assert gpu.stats()["U2_a"] == K.auc(_t(a), _t(y)).stats()[0]
    if two and n >= 63:
        o = Oracle(a, y, b)
        assert gpu.difference() == o.difference() and gpu.interval() == o.interval(0.95)


def test_all_equal_scores_across_four_tiles():
    n = 3 * 2048 + 77
    y = make_case(n, 3)[2]
    s = np.full(n, -0.75, np.float32)
    b = make_case(n, 4, ties=True)[0]
    gpu = _exact_everywhere(s, y, b)
    o = Oracle(s, y, b)
    assert all(v == (o.N if p else o.P) for v, p in zip(o.pl["a"], o.pos))  # one run: every placement is N or P
    st = gpu.stats()
    assert st["m_pos_aa"] == o.P * o.N * o.N and st["m_neg_aa"] == o.N * o.P * o.P
    assert gpu.auc() == 0.5 and gpu.variance() == 0.0 and gpu.interval() == (0.5, 0.5)


def test_final_block_reduces_several_partials_per_thread():
    n = 1_000_003  # 489 tiles for the 256 threads of the final block; placements above 2^16, squares above 2^32
    a, b, y = make_case(n, 5, ties=True)
    gpu = _exact_everywhere(a, y, b)
    assert gpu.stats()["m_pos_aa"] > 2**32 * n // 4


def test_placement_moments_near_2_31():
    pa, pb, y = moments_case()
    ta, tb = torch.from_numpy(pa.astype(np.int32)).cuda(), torch.from_numpy(pb.astype(np.int32)).cuda()
    want = expected_moments(pa, pb, y)
    assert K.placement_moments(ta, tb, _t(y)).tolist() == want
    assert K.placement_moments(ta, None, _t(y)).tolist() == want[:4] + [0] * 8
    assert K.placement_moments(ta[:1].clone(), tb[:1].clone(), _t(y[:1])).tolist() == \
        expected_moments(pa[:1], pb[:1], y[:1])


def test_reused_workspace_over_shrinking_n():
    n = 3 * 8192 + 77
    ws = K.delong_workspace(n, torch.device("cuda"))
    for m, two in ((n, True), (8193, False), (8193, True), (65, True), (1, False)):
        a, b, y = make_case(m, m + 1, ties=True, two=two)
        _exact_everywhere(a, y, b, ws=ws)


def test_non_default_stream():
    a, b, y = make_case(3 * 8192 + 77, 12, ties=True)
    ta, tb, ty = _t(a), _t(b), _t(y)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        one = K.auc_delong(ta, ty)
        two = K.auc_delong(ta, ty, tb)
    torch.cuda.current_stream().wait_stream(side)
    assert _words(one) == Oracle(a, y).words()
    assert _words(two) == Oracle(a, y, b).words()


@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
def test_graph_replay_on_new_scores_equals_eager(two):
    n = 2 * 2048 + 77  # two full tiles and a partial one
    a, b, y = make_case(n, 21, ties=True, two=two)
    dev = torch.device("cuda")
    ta, tb, ty = _t(a), _t(b), _t(y)
    ws = K.delong_workspace(n, dev, two_models=two)
    K.auc_delong(ta, ty, tb, ws=ws).stats()  # (warm: the sort's self-check does not run in a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = K.auc_delong(ta, ty, tb, ws=ws)
    a2, b2, _ = make_case(n, 22, ties=True, two=two)
    ta.copy_(_t(a2))
    if two:
        tb.copy_(_t(b2))
    graph.replay()
    torch.cuda.synchronize()
    eager = K.auc_delong(_t(a2), ty, _t(b2))
    assert _words(st) == _words(eager) == Oracle(a2, y, b2).words()


def test_workspace_bounds():
    h = K.native.hip()
    one, two = h.delong_workspace_bytes(8193, False), h.delong_workspace_bytes(8193, True)
    assert h.delong_workspace_bytes(0, True) > 0 and two >= one + 4 * 8193 and one > (6 * 4 + 2 * 8) * 8193
    with pytest.raises(ValueError):
        h.delong_workspace_bytes(2**30, False)
    a, b, y = make_case(8193, 2)
    with pytest.raises(ValueError, match="ws"):
        _run(a, y, b, ws=torch.empty(1024, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="ws"):  # a one-model workspace does not serve two
        _run(a, y, b, ws=K.delong_workspace(8193, torch.device("cuda"), two_models=False))
    rec = torch.empty(20, dtype=torch.int64, device="cuda")
    ws = K.delong_workspace(8193, torch.device("cuda"), two_models=False)
    with pytest.raises(RuntimeError, match="-2"):  # the launcher's own check
        h.auc_delong(scores_a=_t(a).data_ptr(), scores_b=_t(b).data_ptr(), labels=_t(y).data_ptr(), n=8193,
                     out=rec.data_ptr(), ws=ws.data_ptr(), ws_bytes=ws.numel(), stream=0)
    with pytest.raises(ValueError):
        K.auc_delong(_t(a), _t(y), _t(b, "cpu"))  # another device


def test_nan_counts_per_model():
    a, b, y = make_case(8193, 8)
    bad = a.copy()
    bad[[5, 8000, 8192]] = np.nan
    for ds, counts in ((_run(bad, y, b), (3, 0)), (_run(a, y, bad), (0, 3)), (_run(bad, y), (3, 0))):
        st = ds.stats()
        assert (st["nans_a"], st["nans_b"]) == counts
        assert all(math.isnan(v) for v in (ds.auc(), ds.variance(), *ds.interval()))
        if st["has_b"]:
            assert all(math.isnan(v) for v in (ds.auc_other(), ds.covariance(), *ds.difference()))
    assert _words(_run(bad, y, b)) == _words(_run(bad, y, b, "cpu"))


def test_one_class_labels_and_empty():
    n = 8193
    a, b, y = make_case(n, 9, ties=True)
    for labels in (np.zeros(n, np.float32), np.ones(n, np.float32)):
        ds = _exact_everywhere(a, labels, b)
        assert all(math.isnan(v) for v in (ds.auc(), ds.auc_other(), ds.variance(), *ds.difference()))
    e = torch.empty(0, device="cuda")
    assert math.isnan(K.auc_delong(e, e, e).auc())
