"""The listwise ranking loss on the CPU: the oracle against finite differences of its own loss; the CPU twin of
hip/group_loss.hip against the oracle on the whole case list of tests/group_loss_cases.py (the bounds of
tests/group_loss_oracle.py ``check``); ``group_keys``; the config keys; the refusals; and a planted-teacher run
that the loss has to improve on held-out users."""

import types

import numpy as np
import pytest
import torch

import group_loss_cases as C
import group_loss_oracle as O
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.batch import Batch
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.ops import kernels as K


def _run(g, s, y, w, gs, key_bits=None):
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    plan = K.group_plan(t(g), C.bits_for_ids(g) if key_bits is None else key_bits)
    d, loss = K.group_softmax_loss(plan, t(s), t(y), t(w), gs)
    return d.numpy(), float(loss)


def test_oracle_matches_finite_differences():
    rng = np.random.default_rng(5)
    n = 40
    g = rng.integers(-1, 6, n)
    s = rng.normal(0.0, 2.0, n)
    y = rng.integers(-1, 4, n).astype(np.float64)
    w = rng.uniform(0.0, 2.0, n)
    a = O.gains(y, w)
    d, loss, _, _ = O.group_softmax(g, s, y, w, 1.0)
    assert loss == O.loss_only(g, s, a) and loss > 0
    h = 1e-5
    for i in range(n):
        up, dn = s.copy(), s.copy()
        up[i] += h
        dn[i] -= h
        fd = (O.loss_only(g, up, a) - O.loss_only(g, dn, a)) / (2 * h)
        # central differences: the truncation error is h^2 / 6 |L'''| <= h^2 A_g, the rounding error ~ eps L / h
        assert abs(fd - d[i]) <= 1e-9 * (1.0 + a.sum()) + 1e-16 * loss / h, (i, fd, d[i])
    for k in np.unique(g[g >= 0]):
        assert abs(d[g == k].sum()) <= 1e-12 * (1.0 + a[g == k].sum())


@pytest.mark.parametrize("n,grouping", C.CASES)
def test_cpu_twin_equals_oracle(n, grouping):
    for values in C.VALUES:
        g, s, y, w, gs = C.case(n, grouping, values)
        d, loss = _run(g, s, y, w, gs)
        O.check(d, loss, g, s, y, w, gs, what=f"{n}/{grouping}/{values}")
        if grouping == "all_excluded":
            assert not d.any() and loss == 0.0


@pytest.mark.parametrize("key_bits", [1, 27])
def test_cpu_twin_key_widths(key_bits):
    g, s, y, w, gs = C.key_width_case(key_bits)
    d, loss = _run(g, s, y, w, gs, key_bits=key_bits)
    O.check(d, loss, g, s, y, w, gs, what=f"key_bits {key_bits}")


def test_exact_zeros():
    g = np.array([0, 1, -1, 2, 2, 2, 3, -1], dtype=np.int32)
    s = np.array([3.0, -70.0, np.nan, 1.0, 2.0, 3.0, np.inf, np.inf], dtype=np.float32)
    y = np.array([1.0, 0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 1.0], dtype=np.float32)
    d, loss = _run(g, s, y, None, 1.0, key_bits=3)
    assert not d.any() and loss == 0.0


def test_group_keys():
    num_rows = 1000
    #            ex 0: 3 features   ex 1: none   ex 2: 2   ex 3: 1    ex 4: 4
    sizes = [3, 0, 2, 1, 4]
    rows = torch.tensor([0, 5, 999, 7, 8, 999, 1, 2, 0, 4], dtype=torch.int32)
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32)
    assert K.group_keys(offsets, rows, 0, num_rows).tolist() == [0, -1, 7, 999, 1]
    assert K.group_keys(offsets, rows, 2, num_rows).tolist() == [999, -1, -1, -1, 0]
    assert K.group_keys(offsets, rows, 4, num_rows).tolist() == [-1] * 5
    out = torch.full((8,), 77, dtype=torch.int32)
    assert K.group_keys(offsets, rows, 1, num_rows, out=out).tolist() == [5, -1, 8, -1, 2]
    assert out[5:].tolist() == [77] * 3
    with pytest.raises(ValueError):
        K.group_keys(offsets, rows, -1, num_rows)
    with pytest.raises(ValueError):
        K.group_keys(offsets, rows.long(), 0, num_rows)
    with pytest.raises(ValueError):
        K.group_plan(torch.zeros(3, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        K.group_plan(torch.zeros(3, dtype=torch.int64), 4)
    plan = K.group_plan(torch.zeros(3, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        K.group_softmax_loss(plan, torch.zeros(4), torch.zeros(4), None)
    # the keys of a batch feed the plan: the row num_rows - 1 is a group, the short examples are excluded
    keys = K.group_keys(offsets, rows, 0, num_rows)
    plan = K.group_plan(keys, 10)
    assert plan.sidx.tolist() == [0, 4, 2, 3, 1] and plan.end.tolist() == [1, 2, 3, 4, 0]


CFG = """[General]
vocabulary_size = 1000
vocabulary_block_num = 1
factor_num = 4
hash_feature_id = False
log_dir = {d}/log
device = cpu

[Train]
batch_size = 64
init_value_range = 0.01
factor_lambda = 0
bias_lambda = 0
epoch_num = 1
learning_rate = 0.1
adagrad.initial_accumulator = 0.1
loss_type = {loss}
{extra}
train_files = {d}/train

[Distributed]
{dist}
"""


def _cfg(tmp_path, loss, extra="", dist=""):
    (tmp_path / "train").write_text("1 1:1\n")
    p = tmp_path / "c.cfg"
    p.write_text(CFG.format(d=tmp_path, loss=loss, extra=extra, dist=dist))
    return str(p)


def test_config_accepts_the_loss_and_the_key(tmp_path):
    c = load_config(_cfg(tmp_path, "rank_softmax"), echo=False)
    assert c.loss_type == "rank_softmax" and c.rank_group_feature == 0
    assert c.fm_config().loss_type == "rank_softmax"
    c = load_config(_cfg(tmp_path, "rank_softmax", "rank_group_feature = 2"), echo=False)
    assert c.rank_group_feature == 2 and c.fm_config().rank_group_feature == 2


def test_config_rejections(tmp_path):
    with pytest.raises(ConfigError, match="rank_group_feature"):
        load_config(_cfg(tmp_path, "logistic", "rank_group_feature = 0"), echo=False)
    with pytest.raises(ConfigError, match="rank_group_feature"):
        load_config(_cfg(tmp_path, "rank_softmax", "rank_group_feature = -1"), echo=False)
    with pytest.raises(ConfigError, match="loss_type"):
        load_config(_cfg(tmp_path, "rank_softmax", dist="mode = shard"), echo=False)
    with pytest.raises(ConfigError, match="loss_type"):
        load_config(_cfg(tmp_path, "pairwise"), echo=False)


def test_model_refuses_other_modes_and_ranks():
    cfg = FMConfig(vocabulary_size=100, factor_num=4, loss_type="rank_softmax")
    two = types.SimpleNamespace(world=2, rank=0, group=None)
    with pytest.raises(ValueError, match="loss_type"):
        FactorizationMachine(cfg, "cpu", dist=two)
    for mode in ("shard", "dp", "dp_dense"):
        one = types.SimpleNamespace(world=1, rank=0, group=None)
        with pytest.raises(ValueError, match="loss_type"):
            FactorizationMachine(FMConfig(vocabulary_size=100, factor_num=4, loss_type="rank_softmax", mode=mode),
                                 "cpu", dist=one)
    with pytest.raises(ValueError, match="rank_group_feature"):
        FactorizationMachine(FMConfig(vocabulary_size=100, factor_num=4, loss_type="logistic", rank_group_feature=1),
                             "cpu")


# ---- planted teacher ----------------------------------------------------------------------------------------
USERS, ITEMS, PER_USER, VOCAB = 400, 60, 8, 2000


def _teacher_batches(users, seed, users_per_batch=32):
    """Group-contiguous batches: every user has 8 candidate items; the label is 1 for the two the teacher (an
    item quality plus a little per-pair noise) likes best.  Features: [user, item, a noise feature]."""
    rng = np.random.default_rng(seed)
    quality = np.random.default_rng(99).normal(0.0, 1.0, ITEMS)
    out, gids = [], []
    for u0 in range(0, len(users), users_per_batch):
        us = users[u0: u0 + users_per_batch]
        ids, labels, grp = [], [], []
        for u in us:
            items = rng.choice(ITEMS, PER_USER, replace=False)
            t = quality[items] + 0.3 * rng.normal(size=PER_USER)
            top = set(np.argsort(-t)[:2].tolist())
            for k, it in enumerate(items):
                ids += [int(u), 1000 + int(it), 1500 + int(rng.integers(0, 400))]
                labels.append(1.0 if k in top else 0.0)
                grp.append(int(u))
        B = len(labels)
        out.append(Batch(torch.tensor(labels), torch.arange(0, 3 * B + 1, 3, dtype=torch.int32),
                         torch.tensor(ids, dtype=torch.int32), None, None, 3 * B, max_feats=3))
        gids.append(torch.tensor(grp, dtype=torch.int32))
    return out, gids


def test_planted_teacher_improves_heldout_loss_and_ndcg():
    torch.manual_seed(0)
    cfg = FMConfig(vocabulary_size=VOCAB, factor_num=4, loss_type="rank_softmax", batch_size=256,
                   init_value_range=0.01, seed=3, opt=K.OptConfig("adagrad", lr=0.1))
    model = FactorizationMachine(cfg, "cpu")
    train, _ = _teacher_batches(np.arange(0, 300), seed=1)
    (held,), (hg,) = _teacher_batches(np.arange(300, USERS), seed=2, users_per_batch=USERS)
    hg = hg - 300

    def heldout():
        fo = model.forward(held, loss="rank_softmax")
        assert float(fo.loss_sum) / held.B == model.eval_loss(held)
        return model.eval_loss(held), K.rank_metrics(fo.pred, held.labels, hg, USERS - 300, (5,)).ndcg(5)

    loss0, ndcg0 = heldout()
    first = None
    for _ in range(6):
        for b in train:
            out = model.train_step(b)
            first = out.mean_loss() if first is None else first
    loss1, ndcg1 = heldout()
    # untrained: near-equal scores, so every user's loss is ~ 2 log 8 and the mean per example ~ 2 log 8 / 8
    assert abs(loss0 - 2 * np.log(8) / 8) < 1e-3 and abs(first - loss0) < 1e-3
    print(f"held-out loss {loss0:.6f} -> {loss1:.6f}, ndcg@5 {ndcg0:.4f} -> {ndcg1:.4f}")
    assert loss1 < loss0 and ndcg1 > ndcg0
    model.close()
