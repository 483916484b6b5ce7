"""The pairwise ranking loss on the CPU: the oracle against finite differences of its own loss; the CPU twin of
hip/group_pair.hip against the oracle on the whole case list of tests/group_loss_cases.py (the bound of
tests/group_pair_oracle.py ``check``); the exact zeros; the per-group gradient sums; the GAUC bound; the config
keys; the refusals; ``forward(loss="rank_pairwise")``; and a planted-teacher run that the loss has to improve on
held-out users."""

import math
import types

import numpy as np
import pytest
import torch

import group_loss_cases as C
import group_pair_oracle as O
from fast_tffm_amd.config import ConfigError, load_config
from fast_tffm_amd.data.batch import Batch
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.models.table import bits_for
from fast_tffm_amd.ops import kernels as K


def _run(g, s, y, w, gs, key_bits=None):
    t = lambda a: None if a is None else torch.from_numpy(a)  # noqa: E731
    plan = K.group_plan(t(g), C.bits_for_ids(g) if key_bits is None else key_bits)
    d, loss = K.group_pairwise_loss(plan, t(s), t(y), t(w), gs)
    return d.numpy(), float(loss)


def test_oracle_matches_finite_differences():
    rng = np.random.default_rng(5)
    n = 40
    g = rng.integers(-1, 6, n)
    s = rng.normal(0.0, 2.0, n)
    y = rng.integers(-1, 3, n).astype(np.float64)
    w = rng.uniform(0.0, 2.0, n)
    w[rng.random(n) < 0.15] = 0.0
    p, q = O.class_weights(y, w)
    d, loss, _, per = O.group_pairwise(g, s, y, w, 1.0)
    assert loss == O.loss_only(g, s, p, q) and loss > 0 and len(per) >= 3
    h = 1e-5
    for i in range(n):
        up, dn = s.copy(), s.copy()
        up[i] += h
        dn[i] -= h
        fd = (O.loss_only(g, up, p, q) - O.loss_only(g, dn, p, q)) / (2 * h)
        # central differences: the truncation error is h^2 / 6 |L'''| <= h^2 W_g (|sigma''| < 0.1, c p_i N = W_g
        # p_i / P), the rounding error ~ eps L / h
        assert abs(fd - d[i]) <= 1e-9 * (1.0 + w.sum()) + 1e-16 * loss / h, (i, fd, d[i])
    for k in np.unique(g[g >= 0]):
        assert abs(d[g == k].sum()) <= 1e-12 * (1.0 + np.abs(d[g == k]).sum())


@pytest.mark.parametrize("n,grouping", C.CASES)
def test_cpu_twin_equals_oracle(n, grouping):
    for values in C.VALUES:
        g, s, y, w, gs = C.case(n, grouping, values)
        d, loss = _run(g, s, y, w, gs)
        O.check(d, loss, g, s, y, w, gs, what=f"{n}/{grouping}/{values}")
        if grouping in ("all_excluded", "singletons"):
            assert not d.any() and loss == 0.0


@pytest.mark.parametrize("key_bits", [1, 27])
def test_cpu_twin_key_widths(key_bits):
    g, s, y, w, gs = C.key_width_case(key_bits)
    d, loss = _run(g, s, y, w, gs, key_bits=key_bits)
    O.check(d, loss, g, s, y, w, gs, what=f"key_bits {key_bits}")


def test_exact_zeros():
    g, s, y, w, live = O.exact_zeros_case()
    d, loss = _run(g, s, y, w, 0.5, key_bits=4)
    rest = np.setdiff1d(np.arange(g.size), live)
    assert (d[rest] == 0.0).all() and np.isfinite(d).all() and (d[live] != 0.0).all()
    # the oracle never reads a score outside a pair: the valid group's result is the whole result
    O.check(d, loss, g, s, y, w, 0.5, what="exact zeros")
    ref_d, ref_l, _, per = O.group_pairwise(g, s, y, w, 0.5)
    assert list(per) == [4] and ref_l > 0 and not ref_d[rest].any()
    # without weights the members 12 and 13 count: unspecified scores, but the other groups stay exact zeros
    d2, _ = _run(g, s, y, None, 1.0, key_bits=4)
    assert (d2[g != 4] == 0.0).all()


@pytest.mark.parametrize("values", C.VALUES)
def test_gradient_sums_to_zero_within_every_group(values):
    g, s, y, w, gs = C.case(3 * C.TILE + 5, "zipf", values)
    d, _ = _run(g, s, y, w, gs)
    d = d.astype(np.float64)
    for k in np.unique(g[g >= 0]):
        m = g == k
        assert abs(d[m].sum()) <= 2.0 ** -22 * np.abs(d[m]).sum(), (values, k)


def _auc(s, p, q):
    """Weighted AUC of one group by a direct pair count (a tie counts 1/2)."""
    ip, iq = np.nonzero(p > 0)[0], np.nonzero(q > 0)[0]
    sp, sq = s[ip].astype(np.float64), s[iq].astype(np.float64)
    won = (sp[:, None] > sq[None, :]) + 0.5 * (sp[:, None] == sq[None, :])
    return float((p[ip][:, None] * q[iq][None, :] * won).sum() / (p[ip].sum() * q[iq].sum()))


@pytest.mark.parametrize("values", C.VALUES)
def test_loss_bounds_what_gauc_counts(values):
    g, s, y, w, _ = C.case(C.TILE + 1, "zipf", values)
    p, q = O.class_weights(y, w)
    _, _, _, per = O.group_pairwise(g, s, y, w)
    assert len(per) > 20
    total = 0.0
    for k, (L, W) in per.items():
        m = g == k
        auc = _auc(s[m], p[m], q[m])
        assert L / math.log(2.0) >= W * (1.0 - auc) * (1.0 - 1e-12), (values, k, L, W, auc)
        total += W * (1.0 - auc)
    # and the op's loss, which is the oracle's within the bound, dominates the GAUC deficit of the batch
    _, loss = _run(g, s, y, w, 1.0)
    assert loss / math.log(2.0) >= total * (1.0 - 2.0 ** -20)


def test_equal_scores_give_w_log2():
    g = np.array([0] * 7 + [1] * 4, dtype=np.int32)
    s = np.array([0.75] * 7 + [-3.0] * 4, dtype=np.float32)
    y = np.array([1, 0, 0, 1, 0, 0, 0, 0, 1, 1, 1], dtype=np.float32)
    w = np.array([1.0, 2.0, 0.5, 0.25, 1.0, 0.0, 3.0, 2.0, 1.0, 1.0, 0.5], dtype=np.float32)
    d, loss = _run(g, s, y, w, 1.0, key_bits=2)
    W = float(w.sum())
    assert abs(loss - W * math.log(2.0)) <= 2.0 ** -22 * W * math.log(2.0)
    _, _, _, per = O.group_pairwise(g, s, y, w)
    for k, (L, Wg) in per.items():
        assert abs(L - Wg * math.log(2.0)) <= 1e-14 * Wg
    # sigma(0) = 1/2: a positive gets -c p N / 2 = -p W_g / (2 P)
    P0, W0 = float(w[:7][y[:7] > 0].sum()), float(w[:7].sum())
    assert abs(d[0] + w[0] * W0 / (2 * P0)) <= 2.0 ** -22 * abs(d[0])


def test_argument_checks():
    plan = K.group_plan(torch.zeros(3, dtype=torch.int32), 4)
    with pytest.raises(ValueError):
        K.group_pairwise_loss(plan, torch.zeros(4), torch.zeros(4), None)
    with pytest.raises(ValueError):
        K.group_pairwise_loss(plan, torch.zeros(3, dtype=torch.float64), torch.zeros(3), None)
    with pytest.raises(ValueError):
        K.group_pairwise_loss(plan, torch.zeros(3), torch.zeros(3), None, ws=torch.zeros(8, dtype=torch.uint8))
    empty = K.group_plan(torch.zeros(0, dtype=torch.int32), 4)
    d, loss = K.group_pairwise_loss(empty, torch.zeros(0), torch.zeros(0), None)
    assert d.numel() == 0 and float(loss) == 0.0
    assert K.RANK_PAIR_LOSS == "rank_pairwise" and K.RANK_LOSSES == (K.RANK_LOSS, K.RANK_PAIR_LOSS)


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
    c = load_config(_cfg(tmp_path, "rank_pairwise"), echo=False)
    assert c.loss_type == "rank_pairwise" and c.rank_group_feature == 0
    assert c.fm_config().loss_type == "rank_pairwise"
    c = load_config(_cfg(tmp_path, "rank_pairwise", "rank_group_feature = 2"), echo=False)
    assert c.rank_group_feature == 2 and c.fm_config().rank_group_feature == 2
    c = load_config(_cfg(tmp_path, "rank_pairwise", dist="mode = local"), echo=False)
    assert c.mode == "local"


def test_config_rejections(tmp_path):
    with pytest.raises(ConfigError, match="rank_group_feature"):
        load_config(_cfg(tmp_path, "mse", "rank_group_feature = 1"), echo=False)
    with pytest.raises(ConfigError, match="rank_group_feature"):
        load_config(_cfg(tmp_path, "rank_pairwise", "rank_group_feature = -1"), echo=False)
    for mode in ("shard", "dp", "dp_dense"):
        with pytest.raises(ConfigError, match="loss_type"):
            load_config(_cfg(tmp_path, "rank_pairwise", dist=f"mode = {mode}"), echo=False)
    with pytest.raises(ConfigError, match="loss_type"):
        load_config(_cfg(tmp_path, "rank_pair"), echo=False)


def test_model_refuses_other_modes_and_ranks():
    cfg = FMConfig(vocabulary_size=100, factor_num=4, loss_type="rank_pairwise")
    two = types.SimpleNamespace(world=2, rank=0, group=None)
    with pytest.raises(ValueError, match="loss_type = rank_pairwise"):
        FactorizationMachine(cfg, "cpu", dist=two)
    for mode in ("shard", "dp", "dp_dense"):
        one = types.SimpleNamespace(world=1, rank=0, group=None)
        with pytest.raises(ValueError, match="loss_type = rank_pairwise"):
            FactorizationMachine(FMConfig(vocabulary_size=100, factor_num=4, loss_type="rank_pairwise", mode=mode),
                                 "cpu", dist=one)
    m = FactorizationMachine(FMConfig(vocabulary_size=100, factor_num=4, loss_type="rank_pairwise",
                                      rank_group_feature=1), "cpu")
    assert m.rank_loss and m.pair_loss and m.ws.pair_ws is None
    m.close()


def test_forward_computes_the_op_on_the_batchs_keys():
    rng = np.random.default_rng(11)
    B, F, V = 200, 3, 500
    ids = rng.integers(0, V, (B, F))
    ids[:, 1] = rng.integers(0, 12, B)      # the group feature
    sizes = np.where(rng.random(B) < 0.1, 1, F)   # short examples: excluded with rank_group_feature = 1
    flat = np.concatenate([ids[i, : sizes[i]] for i in range(B)])
    b = Batch(torch.tensor((rng.random(B) < 0.4).astype(np.float32)),
              torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32),
              torch.tensor(flat, dtype=torch.int32), None, torch.tensor(rng.uniform(0.5, 2.0, B).astype(np.float32)),
              int(sizes.sum()), max_feats=F)
    model = FactorizationMachine(FMConfig(vocabulary_size=V, factor_num=4, loss_type="rank_pairwise", seed=4,
                                          init_value_range=0.5, rank_group_feature=1), "cpu")
    fo = model.forward(b, loss="rank_pairwise")
    keys = K.group_keys(b.offsets, b.ids, 1, model.table.rows)
    assert (keys.numpy() == np.where(sizes > 1, ids[:, 1], -1)).all()
    plan = K.group_plan(keys, bits_for(model.table.rows + 1))
    d, loss = K.group_pairwise_loss(plan, model.predict(b), b.labels, b.weights, 1.0)
    assert torch.equal(fo.dpred, d) and float(fo.loss_sum) == float(loss) and float(loss) > 0
    O.check(d.numpy(), float(loss), keys.numpy(), fo.pred.numpy(), b.labels.numpy(), b.weights.numpy(), 1.0)
    model.close()


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


def test_planted_teacher_improves_heldout_loss_and_gauc():
    torch.manual_seed(0)
    cfg = FMConfig(vocabulary_size=VOCAB, factor_num=4, loss_type="rank_pairwise", batch_size=256,
                   init_value_range=0.01, seed=3, opt=K.OptConfig("adagrad", lr=0.1))
    model = FactorizationMachine(cfg, "cpu")
    train, _ = _teacher_batches(np.arange(0, 300), seed=1)
    (held,), (hg,) = _teacher_batches(np.arange(300, USERS), seed=2, users_per_batch=USERS)
    hg = hg - 300

    def heldout():
        fo = model.forward(held, loss="rank_pairwise")
        assert float(fo.loss_sum) / held.B == model.eval_loss(held)
        return model.eval_loss(held), K.gauc(fo.pred, held.labels, hg, USERS - 300).value()

    loss0, gauc0 = heldout()
    first = None
    for _ in range(6):
        for b in train:
            out = model.train_step(b)
            first = out.mean_loss() if first is None else first
    loss1, gauc1 = heldout()
    # untrained: near-equal scores, so every user's loss is ~ W_g ln 2 = 8 ln 2 and the mean per example ~ ln 2
    assert abs(loss0 - np.log(2.0)) < 1e-3 and abs(first - loss0) < 1e-3
    print(f"held-out loss {loss0:.6f} -> {loss1:.6f}, gauc {gauc0:.4f} -> {gauc1:.4f}")
    assert loss1 < loss0 and gauc1 > gauc0
    # the loss dominates the GAUC deficit: mean over examples of W_g (1 - AUC_g) = 1 - GAUC here (all W_g equal)
    assert loss1 / np.log(2.0) >= (1.0 - gauc1) * (1.0 - 1e-6)
    model.close()
