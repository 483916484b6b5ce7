"""The training step with ``loss_type = rank_lambda`` on the GPU, on the batches and executors of
tests/test_rank_pair_step_gpu.py: ``forward(b, loss="rank_lambda")`` is the oracle's loss of the model's own scores
under the step's key rule; every executor of the local step -- plain, both lookahead depths, ``capture_graph`` replay,
the lookahead graph ring -- leaves the table and the losses bitwise the same after 6 steps; only a lambda model
allocates the lambda workspace, and it never touches another group loss's op or workspace."""

import pytest
import torch

import group_lambda_oracle as O
import test_rank_pair_step_gpu as S
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

CUT = 3   # below the groups' ~8 examples: the cutoff bites


def _model(loss="rank_lambda", device="cuda"):
    cfg = FMConfig(vocabulary_size=S.V, factor_num=S.KF, loss_type=loss, init_value_range=0.05, seed=3,
                   opt=K.OptConfig("adagrad", lr=0.05), batch_size=S.B, factor_lambda=0.01, bias_lambda=0.01,
                   rank_lambda_cutoff=CUT)
    return FactorizationMachine(cfg, device=device)


def _run(executor, monkeypatch):
    monkeypatch.setattr(S, "_model", _model)
    return S._run(executor, monkeypatch, "rank_lambda")[:2]


@pytest.fixture(scope="module")
def plain():
    with pytest.MonkeyPatch.context() as mp:
        return _run("plain", mp)


def test_forward_matches_oracle(plain):
    m, b = _model(), S._batches()[0]
    fo = m.forward(b, loss="rank_lambda")
    users = b.ids.view(S.B, S.F)[:, 0].cpu().numpy()
    O.check(fo.dpred.cpu().numpy(), float(fo.loss_sum), users, fo.pred.cpu().numpy(), b.labels.cpu().numpy(), CUT,
            what="forward")
    assert float(fo.loss_sum) > 0 and abs(m.eval_loss(b) * S.B - float(fo.loss_sum)) <= 1e-6 * float(fo.loss_sum)
    assert all(l == l and l > 0 for l in plain[1]) and not torch.equal(plain[0][0], m.table.v)
    m.close()


@pytest.mark.parametrize("executor", ["lookahead1", "lookahead2", "graph", "ring"])
def test_executors_agree_bitwise(plain, executor, monkeypatch):
    st, losses = _run(executor, monkeypatch)
    assert all(torch.equal(x, y) for x, y in zip(plain[0], st)) and losses == plain[1]


def test_only_a_lambda_model_allocates_the_lambda_workspace(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a model called another loss's op or workspace")

    b = S._batches()[0]
    need = K.group_lambda_workspace(S.B, b.labels.device).numel()
    for name in ("group_pairwise_loss", "group_pair_workspace", "group_softmax_loss"):
        monkeypatch.setattr(K, name, boom)
    m = _model()
    assert m.train_step(b).mean_loss() > 0 and m.ws.loss_ws.numel() >= need
    m.close()
    for name in ("group_lambda_loss", "group_lambda_workspace"):
        monkeypatch.setattr(K, name, boom)
    m = _model("logistic")
    assert m.train_step(b).mean_loss() > 0 and m.ws.loss_ws is None
    m.close()
