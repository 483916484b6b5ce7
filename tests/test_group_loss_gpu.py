"""The listwise loss on the GPU (hip/group_loss.hip through ops/kernels.py ``group_plan`` / ``group_softmax_loss``)
against the fp64 oracle on the case list of tests/group_loss_cases.py, within the derived bounds of
tests/group_loss_oracle.py ``check`` (fp64 arithmetic rounded to fp32 once); key widths 1 and 27 with ids at 0 and at
the largest id; bitwise repeatability -- two calls, a workspace last used by a larger call, a captured graph
replayed on new inputs."""

import numpy as np
import pytest
import torch

import group_loss_cases as C
import group_loss_oracle as O
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu


def _t(a, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda")


def run(g, s, y, w, gs, key_bits=None, ws=None):
    plan = K.group_plan(_t(g, np.int32), C.bits_for_ids(g) if key_bits is None else key_bits, ws=ws)
    d, loss = K.group_softmax_loss(plan, _t(s), _t(y), _t(w), gs)
    return d.cpu().numpy(), loss.cpu().numpy()


def test_tile_constant():
    assert K.group_loss_tile() == C.TILE


@pytest.mark.parametrize("n,grouping", C.CASES)
def test_gpu_equals_oracle(n, grouping):
    for values in C.VALUES:
        g, s, y, w, gs = C.case(n, grouping, values)
        d, loss = run(g, s, y, w, gs)
        O.check(d, float(loss), g, s, y, w, gs, what=f"{n}/{grouping}/{values}")
        if grouping == "all_excluded":
            assert not d.any() and float(loss) == 0.0
    K.check_device_errors()


@pytest.mark.parametrize("key_bits", [1, 27])
def test_key_widths(key_bits):
    g, s, y, w, gs = C.key_width_case(key_bits)
    d, loss = run(g, s, y, w, gs, key_bits=key_bits)
    O.check(d, float(loss), g, s, y, w, gs, what=f"key_bits {key_bits}")
    K.check_device_errors()


def test_exact_zeros():
    """Singletons, excluded examples and groups without a positive give exactly 0, whatever the scores."""
    g = np.array([0, 1, -1, 2, 2, 2, 3, -1], dtype=np.int32)
    s = np.array([3.0, -70.0, np.nan, 1.0, 2.0, 3.0, np.inf, np.inf], dtype=np.float32)
    y = np.array([1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 1.0], dtype=np.float32)
    d, loss = run(g, s, y, None, 1.0, key_bits=3)
    assert not d.any() and float(loss) == 0.0


def test_gradient_sums_to_zero_per_group():
    g, s, y, w, gs = C.case(3 * C.TILE + 5, "zipf", "graded_labels")
    d, _ = run(g, s, y, w, 1.0)
    _, _, dscale, _ = O.group_softmax(g, s, y, w, 1.0)
    for k in np.unique(g):
        m = g == k
        assert abs(d[m].astype(np.float64).sum()) <= 2.0 ** -22 * dscale[m].sum() + 1e-30


def test_repeatable_and_workspace_reuse():
    big = C.case(3 * C.TILE + 5, "zipf", "weights")
    small = C.case(C.TILE + 1, "excluded_scattered", "graded_labels")
    first = run(*small)
    again = run(*small)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes()
    ws = K.group_loss_workspace(len(big[0]), torch.device("cuda"))
    ws.fill_(0xFF)
    run(*big, ws=ws)
    reused = run(*small, ws=ws)
    assert first[0].tobytes() == reused[0].tobytes() and first[1].tobytes() == reused[1].tobytes()


def test_graph_replay_equals_eager():
    n = 3 * C.TILE + 5
    a = C.case(n, "zipf", "weights")
    b = C.case(n, "excluded_scattered", "weights")
    dev = torch.device("cuda")
    g, s, y, w = _t(a[0], np.int32), _t(a[1]), _t(a[2]), _t(a[3])
    ws = K.group_loss_workspace(n, dev)
    dpred = torch.empty(n, dtype=torch.float32, device=dev)
    K.group_softmax_loss(K.group_plan(g, 10, ws=ws), s, y, w, a[4], dpred=dpred)  # eager once: the sort's self-check
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _, loss = K.group_softmax_loss(K.group_plan(g, 10, ws=ws), s, y, w, a[4], dpred=dpred)
    for t, src, dt in ((g, b[0], np.int32), (s, b[1], np.float32), (y, b[2], np.float32), (w, b[3], np.float32)):
        t.copy_(_t(src, dt))
    graph.replay()
    torch.cuda.synchronize()
    got = dpred.cpu().numpy(), loss.cpu().numpy()
    del graph
    want = run(*b[:4], a[4], key_bits=10)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
    O.check(got[0], float(got[1]), b[0], b[1], b[2], b[3], a[4], what="graph replay")
