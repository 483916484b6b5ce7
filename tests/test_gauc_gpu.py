"""Grouped AUC on the GPU (hip/gauc.hip through ops/kernels.py ``gauc``) against the exact oracles and the CPU
twin, at the shapes where the segmented chain can go wrong: group boundaries on, one before and one after the
edges of the 2048-position tiles, tie runs that span tiles inside one group, the same score on both sides of a
group boundary, empty groups, one huge group beside thousands of tiny ones.

Tolerances: without weights the per-group records, the valid count and the covered examples are exact and the
scalar is within 1e-10 relative (an fp64 sum of <= 2^17 non-negative terms in another order: n 2^-52 ~ 3e-11);
with weights in [0.5, 2] and n <= 2^17 the records and the scalar are within the same 1e-10 of the exact
(rational) oracle -- no sum of the chain subtracts."""

import functools
import math

import numpy as np
import pytest
import torch

from gauc_oracle import brute_groups, make_groups_case, sorted_groups, summary
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

REL = 1e-10
TILE = 2048


def _t(a, device, dtype=np.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype)).to(device)


def run(s, y, g, G, w=None, device="cuda", ws=None):
    kw = {} if ws is None else {"ws": ws}
    return K.gauc(_t(s, device), _t(y, device), _t(g, device, np.int32), G, _t(w, device), **kw)


def check(st, recs, g, G, weighted):
    got = st.per_group().cpu()
    value, valid, covered = summary(recs, g, G)
    assert got.shape == (G, 3)
    if not weighted:
        assert got.dtype == torch.int64 and got.tolist() == [list(r) for r in recs]
    else:
        want = np.array([[float(x) for x in r] for r in recs], np.float64).reshape(G, 3)
        err = np.abs(got.numpy() - want)
        print("largest relative record error", float((err / np.maximum(want, 1e-300)).max()))
        assert (err <= REL * want).all()
    assert st.valid_groups() == valid
    assert st.coverage() == covered / len(g)
    if valid:
        print("value", st.value(), "oracle", value, "relative error", abs(st.value() - value) / value)
        assert abs(st.value() - value) <= REL * value
    else:
        assert math.isnan(st.value())


def check_cpu(st, s, y, g, G, w):
    """The GPU's records against the CPU twin's: the same integers without weights."""
    cpu = run(s, y, g, G, w, device="cpu")
    a, b = st.per_group().cpu(), cpu.per_group()
    if w is None:
        assert torch.equal(a, b) and st.stats()[1:] == cpu.stats()[1:]
        assert abs(st.stats()[0] - cpu.stats()[0]) <= REL * cpu.stats()[0]
    else:
        assert ((a - b).abs() <= REL * b).all()


def edge_sizes(n):
    """Group sizes whose boundaries lie on, one before and one after every tile edge up to n, and one
    position from either end."""
    cuts = sorted({c for e in range(TILE, n + TILE, TILE) for c in (e - 1, e, e + 1) if 0 < c < n} | {1, n - 1})
    return np.diff([0] + cuts + [n]).tolist()


@functools.lru_cache(maxsize=None)
def case(name, weighted):
    """(s, y, g, w, G, oracle records) of a named layout, computed once."""
    if name.startswith("edges"):
        n = int(name.split("-")[1])
        sizes = edge_sizes(n)
        G = len(sizes)
        s, y, g, w = make_groups_case(n, G, n, distinct=3 if name.endswith("ties") else None, weights=weighted,
                                      sizes=sizes)
    elif name == "one-group-ties":      # runs of ~2050 equal scores: every tie run spans tiles
        n, G = 3 * TILE + 5, 1
        s, y, g, w = make_groups_case(n, G, 1, distinct=3, weights=weighted)
    elif name == "two-groups-ties":     # the same three scores on both sides of a boundary inside a tile
        n, G = 3 * TILE + 5, 2
        s, y, g, w = make_groups_case(n, G, 2, distinct=3, weights=weighted, sizes=[3000, n - 3000])
    elif name == "own-group":
        n = G = 3000
        s, y, g, w = make_groups_case(n, G, 3, distinct=3, weights=weighted, sizes=[1] * n)
    elif name == "empty-groups":        # G > n: no example in groups 0-4, 500-899 and the last 100
        n, G = 700, 1200
        used = np.r_[5:500, 900:1100].astype(np.int32)
        s, y, g, w = make_groups_case(n, G, 4, distinct=5, weights=weighted)
        g = used[np.random.default_rng(4).integers(0, len(used), n)]
    elif name == "skew-50000":          # one group with 90% of 50,000 examples, the rest in groups of 1-3
        r = np.random.default_rng(5)
        small = []
        while sum(small) < 5000:
            small.append(min(int(r.integers(1, 4)), 5000 - sum(small)))
        sizes = small[:len(small) // 2] + [45000] + small[len(small) // 2:]
        n, G = 50000, len(sizes)
        s, y, g, w = make_groups_case(n, G, 5, distinct=None if weighted else 60, weights=weighted, sizes=sizes)
    elif name == "skew-5000-groups":    # 5,000 groups of 1-3 beside one group with 90% of all examples
        small = np.random.default_rng(6).integers(1, 4, 5000).tolist()
        sizes = small[:2500] + [9 * sum(small)] + small[2500:]
        n, G = sum(sizes), len(sizes)
        assert n <= 2 ** 17
        s, y, g, w = make_groups_case(n, G, 6, distinct=200, weights=weighted, sizes=sizes)
    elif name == "packed":              # 20,000 groups of 1-8
        sizes = np.random.default_rng(7).integers(1, 9, 20000).tolist()
        n, G = sum(sizes), len(sizes)
        s, y, g, w = make_groups_case(n, G, 7, distinct=4, weights=weighted, sizes=sizes)
    else:
        raise KeyError(name)
    return s, y, g, w, G, sorted_groups(s, y, g, G, w)


LAYOUTS = [f"edges-{n}{t}" for n in (2047, 2048, 2049, 4097, 3 * TILE + 5) for t in ("", "-ties")] + [
    "one-group-ties", "two-groups-ties", "own-group", "empty-groups", "skew-50000", "skew-5000-groups", "packed"]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name", LAYOUTS)
def test_layouts_against_oracle_and_cpu(name, weighted):
    s, y, g, w, G, recs = case(name, weighted)
    st = run(s, y, g, G, w)
    check(st, recs, g, G, weighted)
    check_cpu(st, s, y, g, G, w)


def test_smallest_inputs():
    one = run([0.3], [1], [0], 1)
    assert math.isnan(one.value()) and one.per_group().tolist() == [[0, 1, 0]] and one.valid_groups() == 0
    s, y = np.array([0.2, 0.7], np.float32), np.array([0, 1], np.float32)
    same = run(s, y, [0, 0], 1)
    assert same.per_group().tolist() == [[2, 1, 1]] and same.value() == 1.0 and same.valid_groups() == 1
    assert same.coverage() == 1.0
    apart = run(s, y, [0, 1], 2)
    assert apart.per_group().tolist() == [[0, 0, 1], [0, 1, 0]]
    assert math.isnan(apart.value()) and apart.valid_groups() == 0 and apart.coverage() == 0.0


def test_one_group_equals_auc_integer_for_integer():
    s, y, g, _ = make_groups_case(5000, 1, 8, distinct=70)
    st = run(s, y, g, 1)
    assert tuple(st.per_group()[0].tolist()) == K.auc(_t(s, "cuda"), _t(y, "cuda")).stats()[:3]
    check(st, sorted_groups(s, y, g, 1), g, 1, False)


def test_special_scores():
    s = np.array([0.0, -0.0, np.inf, -np.inf, 1e-42, -1e-42, 3e-42, 3e38, -3e38, 0.0, -0.0, np.inf, -np.inf, 1e-42],
                 np.float32)
    y = np.array([1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1, 0, 1, 0], np.float32)
    for G, g in ((1, np.zeros(14, np.int32)), (2, np.arange(14, dtype=np.int32) % 2),
                 (3, np.arange(14, dtype=np.int32) % 3)):
        st = run(s, y, g, G)
        check(st, brute_groups(s, y, g, G), g, G, False)
        check_cpu(st, s, y, g, G, None)
    for sc, want in (([0.0, -0.0], 0.5), ([1e-42, 0.0], 1.0), ([-1e-42, -0.0], 0.0), ([np.inf, 3e38], 1.0)):
        assert run(sc, [1, 0], [0, 0], 1).value() == want, sc


def test_one_nan_score():
    s, y, g, _ = make_groups_case(5000, 40, 9)
    s[4321] = np.nan
    st = run(s, y, g, 40)
    assert math.isnan(st.value()) and st.stats()[4] == 1


def test_zero_weights_make_a_group_invalid():
    s, y, g, w = make_groups_case(6000, 50, 10, distinct=9, weights=True)
    w[(g == 7) & (y > 0)] = 0.0     # group 7 keeps positive examples and loses all positive weight
    w[(g == 9) & ~(y > 0)] = 0.0    # group 9: the negatives
    w[::5] = 0.0
    recs = brute_groups(s, y, g, 50, w)
    assert recs[7][1] == 0 and recs[9][2] == 0 and ((g == 7) & (y > 0)).any()
    st = run(s, y, g, 50, w)
    check(st, recs, g, 50, True)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_same_call_twice_is_bitwise_equal(weighted):
    s, y, g, w, G, _ = case("skew-50000", weighted)
    a, b = run(s, y, g, G, w), run(s, y, g, G, w)
    assert torch.equal(a.rec.cpu(), b.rec.cpu())
    assert torch.equal(a.per_group().cpu().view(torch.int64), b.per_group().cpu().view(torch.int64))


def test_graph_replay_on_new_scores_equals_eager():
    s, y, g, w, G, _ = case("packed", True)
    n = len(s)
    dev = torch.device("cuda")
    ts, ty, tg, tw = _t(s, dev), _t(y, dev), _t(g, dev, np.int32), _t(w, dev)
    ws = K.gauc_workspace(n, G, dev)
    K.gauc(ts, ty, tg, G, tw, ws=ws).stats()  # (warm: the sort's one-time self-check does not run in a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = K.gauc(ts, ty, tg, G, tw, ws=ws)
    s2 = np.random.default_rng(12).standard_normal(n).astype(np.float32)
    ts.copy_(_t(s2, dev))
    graph.replay()
    torch.cuda.synchronize()
    eager = K.gauc(_t(s2, dev), ty, tg, G, tw)
    assert torch.equal(st.rec.cpu(), eager.rec.cpu())
    assert torch.equal(st.per_group().cpu(), eager.per_group().cpu())
    check(st, sorted_groups(s2, y, g, G, w), g, G, True)


def test_workspace_bounds_and_reuse():
    h = K.native.hip()
    assert h.gauc_workspace_bytes(0, 1) > 0 and h.gauc_workspace_bytes(8193, 10) > 9 * 4 * 8193
    for n, G in ((2 ** 30, 1), (10, 0), (10, 2 ** 31)):
        with pytest.raises(ValueError):
            h.gauc_workspace_bytes(n, G)
    s, y, g, w, G, recs = case("edges-4097", False)
    with pytest.raises(ValueError, match="ws"):
        run(s, y, g, G, ws=torch.empty(1024, dtype=torch.uint8, device="cuda"))
    ws = K.gauc_workspace(len(s), G, torch.device("cuda"))
    check(run(s, y, g, G, ws=ws), recs, g, G, False)
    s2, y2, g2, _ = make_groups_case(700, 9, 13, distinct=3)
    check(run(s2, y2, g2, 9, ws=ws), brute_groups(s2, y2, g2, 9), g2, 9, False)


def test_train_and_evaluate_on_cuda(tmp_path):
    """The trainer's two users of the chain on the device: the validation line and ``evaluate``."""
    import re

    from test_gauc_cli import GAUC_KEYS, _run, _write_cfg, _write_data
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.data.groups import load_group_files
    from fast_tffm_amd.data.reader import load_file_batch
    from fast_tffm_amd.trainer import Trainer

    _write_data(tmp_path / "train_0", tmp_path / "train_0.grp", 600, 1, 40)
    _write_data(tmp_path / "valid_0", tmp_path / "valid_0.grp", 300, 2, 40)
    _write_data(tmp_path / "valid_1", tmp_path / "valid_1.grp", 120, 3, 25)
    cfg_path = _write_cfg(tmp_path, GAUC_KEYS.format(d=tmp_path) + "validation_auc = true", device="cuda")
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    m = re.search(r"^validation auc at step 3: [0-9.]+\nvalidation gauc at step 3: ([0-9.]+)$", out, re.M)
    assert rc == 0 and m, out
    rc, out = _run(["evaluate", cfg_path])
    assert rc == 0
    with Trainer(load_config(cfg_path, echo=False), None, printer=lambda *a, **k: None) as tr:
        assert tr.restore() and tr.device.type == "cuda"
        for name in ("valid_0", "valid_1"):
            path = str(tmp_path / name)
            b = load_file_batch([path], None, 500, False, 1)
            gi = load_group_files([path + ".grp"], [path])
            scores = tr.model.predict(b.to(tr.device)).cpu().numpy()
            recs = brute_groups(scores, b.labels.numpy(), gi.ids, gi.num_groups)
            value, valid, covered = summary(recs, gi.ids, gi.num_groups)
            e = re.search(r"^evaluate %s: examples %d loss [0-9.]+ auc [0-9.]+ gauc ([0-9.]+) valid_groups %d/%d "
                          r"coverage %.8f$" % (re.escape(path), b.B, valid, gi.num_groups, covered / b.B), out, re.M)
            assert e and e.group(1) == "%.8f" % value, out
            if name == "valid_0":
                assert m.group(1) == e.group(1)  # the validation line reported the same set's GAUC
            lines = open(path + "_gauc").read().splitlines()
            assert len(lines) == gi.num_groups and sum(ln.split()[1] != "nan" for ln in lines) == valid
