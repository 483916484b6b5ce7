"""Exact weighted ROC AUC on the GPU (hip/auc.hip through ops/kernels.py ``auc``): sizes around the wave,
the AUC tile (2048), the sort tile (8192) and several tiles, against the numpy oracle and the CPU kernel."""

import contextlib
import io
import math
import os

import numpy as np
import pytest
import torch

from auc_oracle import SPECIAL_LABELS, SPECIAL_SCORES, make_case, oracle_stats, rel_bound, value_of
from fast_tffm_amd import cli
from fast_tffm_amd.config import load_config
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.trainer import Trainer

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 2047, 2049, 8191, 8192, 8193, 3 * 8192 + 77, 1_000_003]


def _t(a, device):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(device)


def _both(s, y, w=None):
    """(GPU stats, CPU stats) of one input."""
    return (K.auc(_t(s, "cuda"), _t(y, "cuda"), _t(w, "cuda")).stats(),
            K.auc(_t(s, "cpu"), _t(y, "cpu"), _t(w, "cpu")).stats())


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES)
def test_unweighted_bitwise_equal_to_oracle_and_cpu(n, ties):
    s, y, _ = make_case(n, n, ties=ties)
    gpu, cpu = _both(s, y)
    assert gpu == oracle_stats(s, y) and gpu == cpu
    assert all(isinstance(v, int) for v in gpu)


def test_all_equal_scores_across_four_tiles():
    n = 3 * 8192 + 77
    y = make_case(n, 3)[1]
    s = np.full(n, -0.75, np.float32)
    st = K.auc(_t(s, "cuda"), _t(y, "cuda"))
    assert st.stats() == oracle_stats(s, y) and st.value() == 0.5


def test_special_values_equal_cpu():
    gpu, cpu = _both(SPECIAL_SCORES, SPECIAL_LABELS)
    assert gpu == cpu == oracle_stats(SPECIAL_SCORES, SPECIAL_LABELS)
    for s, y, want in (([0.0, -0.0], [1, 0], 0.5), ([1e-42, 0.0], [1, 0], 1.0), ([-1e-42, -0.0], [1, 0], 0.0),
                       ([1e-42, 3e-42], [1, 0], 0.0), ([np.inf, 3e38, -np.inf], [1, 0, 0], 1.0)):
        assert K.auc(_t(s, "cuda"), _t(y, "cuda")).value() == want, s


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_integer_weights_exact(n, ties):
    s, y, w = make_case(n, 3 * n, ties=ties, weights="int")
    gpu, cpu = _both(s, y, w)
    assert gpu == oracle_stats(s, y, w) and gpu == cpu


@pytest.mark.parametrize("ties", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("n", SIZES[1:])
def test_real_weights_within_summation_bound_and_reproducible(n, ties):
    s, y, w = make_case(n, 7 * n, ties=ties, weights="real")
    ts, ty, tw = _t(s, "cuda"), _t(y, "cuda"), _t(w, "cuda")
    got = K.auc(ts, ty, tw).stats()
    want = oracle_stats(s, y, w)
    print("relative errors", [abs(g - x) / x for g, x in zip(got[:3], want[:3])], "bound", rel_bound(n))
    assert all(abs(g - x) <= rel_bound(n) * x for g, x in zip(got[:3], want[:3])), (got, want)
    assert got[3] == 0
    assert K.auc(ts, ty, tw).stats() == got  # bitwise, run to run


def test_reused_workspace():
    n = 3 * 8192 + 77
    ws = K.auc_workspace(n, torch.device("cuda"))
    for m in (n, 65, 8193):
        s, y, _ = make_case(m, m + 1, ties=True)
        assert K.auc(_t(s, "cuda"), _t(y, "cuda"), ws=ws).stats() == oracle_stats(s, y)


def test_non_default_stream():
    s, y, w = make_case(3 * 8192 + 77, 12, ties=True, weights="int")
    ts, ty, tw = _t(s, "cuda"), _t(y, "cuda"), _t(w, "cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a, b = K.auc(ts, ty), K.auc(ts, ty, tw)
    torch.cuda.current_stream().wait_stream(side)
    assert a.stats() == oracle_stats(s, y) and b.stats() == oracle_stats(s, y, w)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_graph_replay_on_new_scores_equals_eager(weighted):
    n = 2 * 2048 + 77  # two full tiles of the prefix chain and a partial one
    s, y, w = make_case(n, 21, weights="real" if weighted else None)
    dev = torch.device("cuda")
    ts, ty, tw = _t(np.round(16 * s) / 16, dev), _t(y, dev), _t(w, dev)  # (sixteenths: tie runs cross tile borders)
    ws = K.auc_workspace(n, dev)
    K.auc(ts, ty, tw, ws=ws).stats()  # (warm: the sort's one-time self-check does not run in a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = K.auc(ts, ty, tw, ws=ws)
    s2 = np.round(16 * np.random.default_rng(22).standard_normal(n)).astype(np.float32) / 16
    ts.copy_(_t(s2, dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = K.auc(_t(s2, dev), ty, tw)
    assert st.stats() == eager.stats()
    assert torch.equal(st.rec.cpu().view(torch.int64), eager.rec.cpu().view(torch.int64))  # (fp64: bit for bit)
    if not weighted:
        assert st.stats() == K.auc(_t(s2, "cpu"), _t(y, "cpu")).stats() == oracle_stats(s2, y)


def test_one_class_and_nan_scores():
    n = 8193
    s, y, _ = make_case(n, 8)
    for labels in (np.zeros(n, np.float32), np.ones(n, np.float32)):
        st = K.auc(_t(s, "cuda"), _t(labels, "cuda"))
        assert math.isnan(st.value()) and st.stats() == oracle_stats(s, labels)
    s[[5, 8000]] = np.nan
    st = K.auc(_t(s, "cuda"), _t(y, "cuda"))
    assert math.isnan(st.value()) and st.stats()[3] == 2
    st = K.auc(torch.empty(0, device="cuda"), torch.empty(0, device="cuda"))
    assert math.isnan(st.value()) and st.stats() == (0, 0, 0, 0)


def test_workspace_bounds():
    h = K.native.hip()
    assert h.auc_workspace_bytes(0) > 0 and h.auc_workspace_bytes(8193) > 5 * 4 * 8193
    with pytest.raises(ValueError):
        h.auc_workspace_bytes(2**30)
    s, y, _ = make_case(8193, 2)
    with pytest.raises(ValueError, match="ws"):
        K.auc(_t(s, "cuda"), _t(y, "cuda"), ws=torch.empty(1024, dtype=torch.uint8, device="cuda"))


def _copy_head(src, dst, n):
    with open(src, "rb") as f, open(dst, "wb") as g:
        for i, line in enumerate(f):
            if i >= n:
                break
            g.write(line)


def test_trainer_validation_metrics_on_cuda(tmp_path, ref_data_dir):
    d = tmp_path / "data"
    d.mkdir()
    _copy_head(os.path.join(ref_data_dir, "train_0"), d / "train_0", 3000)
    _copy_head(os.path.join(ref_data_dir, "test_0"), d / "test_0", 1500)
    cfg_path = tmp_path / "run.cfg"
    cfg_path.write_text(f"""[General]
vocabulary_size = 200000
vocabulary_block_num = 4
factor_num = 8
hash_feature_id = False
log_dir = {tmp_path / "log"}
device = cuda

[Train]
batch_size = 1000
init_value_range = 0.01
factor_lambda = 0.0001
bias_lambda = 0.0001
epoch_num = 1
learning_rate = 0.05
adagrad.initial_accumulator = 0.1
save_steps = 3
loss_type = logistic
train_files = {d}/train_0
validation_files = {d}/test_0
tolerance = 0.0
validation_auc = true
""")
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        assert cli.main(["train", str(cfg_path)]) == 0
    assert "validation auc at step 3: " in buf.getvalue()
    with Trainer(load_config(str(cfg_path), echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.model.global_step == 3
        vb = tr.load_validation()
        loss, auc = tr.validation_metrics(vb)
        assert loss == tr.validation_loss(vb)
        want = oracle_stats(tr.model.predict(vb).cpu().numpy(), vb.labels.cpu().numpy())
        assert (want[1], want[2]) == (310, 1190)
        assert auc == value_of(want) and ("validation auc at step 3: %.8f" % auc) in buf.getvalue()
