"""The training step with ``loss_type = rank_pairwise`` on the GPU: every executor of the local step -- plain eager
steps, the depth-1 and depth-2 lookahead, ``capture_graph`` replay and the lookahead graph ring -- leaves the table
and the losses bitwise the same after 6 steps over 3 cycling batches; one step agrees with the CPU executor's; and a
``rank_softmax`` and a ``logistic`` model in the same process never touch the pairwise loss (no pair workspace,
none of its ops called)."""

import numpy as np
import pytest
import torch

from fast_tffm_amd.data.batch import Batch
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

V, KF, B, F = 4096, 8, 512, 4
ORDER = [0, 1, 2, 0, 1, 2]


def _model(loss="rank_pairwise", device="cuda"):
    cfg = FMConfig(vocabulary_size=V, factor_num=KF, loss_type=loss, init_value_range=0.05, seed=3,
                   opt=K.OptConfig("adagrad", lr=0.05), batch_size=B, factor_lambda=0.01, bias_lambda=0.01)
    return FactorizationMachine(cfg, device=device)


def _batches(device="cuda"):
    """3 batches of 512 examples with 4 features each: feature 0 is one of 64 users (groups of ~8, scattered through
    the batch), the others repeat over a few hundred rows; weighted, 30% positives."""
    rng = np.random.default_rng(11)
    out = []
    for _ in range(3):
        ids = rng.integers(64, 600, (B, F))
        ids[:, 0] = rng.integers(0, 64, B)
        b = Batch(torch.tensor((rng.random(B) < 0.3).astype(np.float32)),
                  torch.arange(0, B * F + 1, F, dtype=torch.int32), torch.tensor(ids.reshape(-1), dtype=torch.int32),
                  None, torch.tensor(rng.uniform(0.5, 2.0, B).astype(np.float32)), B * F, max_feats=F)
        out.append(b.to(device, non_blocking=False))
    return out


def _state(m):
    t = m.table
    return [x.clone() for x in (t.v, t.w, t.s0v, t.s0w)]


def _fill(dst, src):
    for d, s in ((dst.labels, src.labels), (dst.offsets, src.offsets), (dst.ids, src.ids), (dst.weights, src.weights)):
        d.copy_(s)


def _run(executor, monkeypatch, loss="rank_pairwise"):
    batches = _batches()
    m = _model(loss)
    losses = []
    if executor == "plain":
        losses = [m.train_step(batches[i]).mean_loss() for i in ORDER]
    elif executor in ("lookahead1", "lookahead2"):
        monkeypatch.setenv("FM_LOCAL_DEPTH2", "1" if executor == "lookahead2" else "0")
        seq = [batches[i] for i in ORDER]
        for i, bt in enumerate(seq):
            nb = seq[i + 1] if i + 1 < len(seq) else None
            n2 = seq[i + 2] if i + 2 < len(seq) and executor == "lookahead2" else None
            losses.append(m.train_step(bt, nb, n2).mean_loss())
    elif executor == "graph":
        m.capture_graph(batches[0])
        losses = [m.train_step(batches[i]).mean_loss() for i in ORDER]
    else:
        bufs = m.lookahead_graph_buffers(batches[0], 4)
        _fill(bufs[0], batches[ORDER[0]])
        for s, i in enumerate(ORDER):
            if s + 1 < len(ORDER):
                _fill(bufs[(s + 1) % 4], batches[ORDER[s + 1]])
            losses.append(m.train_step(bufs[s % 4], bufs[(s + 1) % 4]).mean_loss())
    torch.cuda.synchronize()
    K.check_device_errors()
    st = _state(m)
    pair_ws = m.ws.pair_ws
    m.close()
    return st, losses, pair_ws


@pytest.fixture(scope="module")
def plain():
    mp = pytest.MonkeyPatch()
    try:
        return _run("plain", mp)
    finally:
        mp.undo()


def test_plain_steps_train(plain):
    st, losses, pair_ws = plain
    assert all(l == l and l > 0 for l in losses)
    assert losses[3] < losses[0]   # the second visit of batch 0
    # near-zero scores at step 1: every valid group adds W_g ln 2, so the mean is at most the mean weight times ln 2
    assert 0.5 * np.log(2.0) < losses[0] < 1.25 * np.log(2.0) * 1.05
    assert pair_ws is not None and pair_ws.numel() >= K.group_pair_workspace(B, pair_ws.device).numel()
    untouched = _state(_model())
    assert not torch.equal(st[0], untouched[0])


@pytest.mark.parametrize("executor", ["lookahead1", "lookahead2", "graph", "ring"])
def test_executors_agree_bitwise(plain, executor, monkeypatch):
    st, losses, _ = _run(executor, monkeypatch)
    for x, y in zip(plain[0], st):
        assert torch.equal(x, y)
    assert losses == plain[1]


def test_one_step_matches_cpu_executor():
    gb = _batches()[0]
    g, c = _model(), _model(device="cpu")
    assert torch.equal(g.table.reference_rows().cpu(), c.table.reference_rows())
    lg = g.train_step(gb).mean_loss()
    lc = c.train_step(_batches("cpu")[0]).mean_loss()
    torch.cuda.synchronize()
    got, want = g.table.reference_rows().double().cpu(), c.table.reference_rows().double()
    assert not torch.equal(want, _model(device="cpu").table.reference_rows().double())
    torch.testing.assert_close(got, want, rtol=2e-4, atol=5e-6)
    assert abs(lg - lc) <= 1e-5 * abs(lc)
    assert abs(g.eval_loss(gb) - c.eval_loss(_batches("cpu")[0])) <= 1e-5 * abs(lc)


def test_other_models_never_touch_the_pairwise_loss(monkeypatch):
    """A ``rank_softmax`` and a ``logistic`` model train as before -- every executor bitwise equal to the plain one
    -- with the pairwise op and its workspace made to raise."""
    def boom(*a, **k):
        raise AssertionError("a model without the pairwise loss called it")

    for name in ("group_pairwise_loss", "group_pair_workspace"):
        monkeypatch.setattr(K, name, boom)
    for loss in ("rank_softmax", "logistic"):
        ref = None
        for executor in ("plain", "lookahead1", "graph"):
            st, losses, pair_ws = _run(executor, monkeypatch, loss)
            assert pair_ws is None
            assert all(l == l and l > 0 for l in losses)
            if ref is None:
                ref = st, losses
            for x, y in zip(ref[0], st):
                assert torch.equal(x, y)
            assert losses == ref[1]
