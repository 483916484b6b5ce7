"""Ranking metrics on the GPU (hip/rank_metrics.hip through ops/kernels.py ``rank_metrics``) against the
pure-Python oracle, per group and in the means, on the case list of tests/rank_cases.py: one example; one group of
2047 / 2048 / 2049 examples whose top tie run ends the sorted order (with 2049 it straddles the tile boundary); one
run over four tiles; groups of 1 to 5 examples, several per wave, under cutoffs larger than they are; the same
score values on both sides of group boundaries; empty, unranked and all-positive groups; graded and -1/+1 labels;
signed zeros, infinities and denormals; a NaN; 2^17 examples in Zipf-sized groups with 16 score levels.

Tolerance (tests/rank_cases.py ``check``): every per-group value and every mean is a sum of non-negative fp64
terms, each from at most a few correctly rounded operations, so for any summation order the relative error is at
most (m + 8) 2^-52 -- m the case's largest group size for a per-group value, the larger of that and the number of
ranked groups for a mean.  n_g, P_g and the counts are exact."""

import math

import numpy as np
import pytest
import torch

import rank_cases as C
import rank_oracle as R
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu


def _t(a, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).to("cuda")


def run(s, y, g, G, ks, ws=None):
    kw = {} if ws is None else {"ws": ws}
    return K.rank_metrics(_t(s), _t(y), _t(g, np.int32), G, ks, **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_gpu_equals_oracle(name):
    s, y, g, G, ks, recs = C.case(name)
    C.check(run(s, y, g, G, ks), recs, len(s), G, ks)


def test_all_equal_scores_share_the_discount_mass():
    s, y, g, G, ks, _ = C.case("all-equal")
    per = run(s, y, g, G, ks).per_group()[0].tolist()
    n, pos = len(s), int((y > 0).sum())
    assert per[:2] == [n, pos]
    for c, k in enumerate(ks):
        assert per[2 + 3 * c] == pytest.approx(pos * R.D[k] / n, rel=(n + 8) * 2.0 ** -52)
        assert per[4 + 3 * c] == pytest.approx(pos * k / n, rel=(n + 8) * 2.0 ** -52)


def test_nan_score_gives_nan_means_and_is_counted():
    s, y, g, G, ks = C.with_nan()
    st = run(s, y, g, G, ks)
    assert st.stats()[3] == 1
    assert all(math.isnan(f(k)) for k in ks for f in (st.ndcg, st.recall, st.precision))
    assert st.ranked_groups() == R.summary(C.case("special")[5], ks)[1]
    got = st.per_group().cpu().numpy()
    want = np.array([[float(v) for v in r] for r in R.group_records(s, y, g, G, ks)], np.float64)
    assert (np.abs(got - want) <= (C.bound_m(C.case("special")[5])[0] + 8) * 2.0 ** -52 * want).all()


def test_repeated_runs_and_reused_workspace_agree_bitwise():
    s, y, g, G, ks, _ = C.case("zipf")
    args = (_t(s), _t(y), _t(g, np.int32), G, ks)
    a, b = K.rank_metrics(*args), K.rank_metrics(*args)
    ws = K.rank_metrics_workspace(len(s), G, torch.device("cuda"))
    small = C.case("same-scores")  # (leaves other bytes in the workspace than the next call's own)
    run(*small[:5], ws=ws).stats()
    c, d = K.rank_metrics(*args, ws=ws), K.rank_metrics(*args, ws=ws)
    a.stats()
    for other in (b, c, d):
        other.stats()
        assert torch.equal(a.rec, other.rec)
        assert torch.equal(a.groups.view(torch.int64), other.groups.view(torch.int64))


def test_graph_replay_on_new_scores_equals_eager():
    s, y, g, G, ks, _ = C.case("same-scores")
    ts, ty, tg = _t(s), _t(y), _t(g, np.int32)
    ws = K.rank_metrics_workspace(len(s), G, torch.device("cuda"))
    K.rank_metrics(ts, ty, tg, G, ks, ws=ws).stats()  # (warm: the sort's self-check and the table's upload)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st = K.rank_metrics(ts, ty, tg, G, ks, ws=ws)
    s2 = np.random.default_rng(12).integers(0, 3, len(s)).astype(np.float32)
    ts.copy_(_t(s2))
    graph.replay()
    torch.cuda.synchronize()
    eager = K.rank_metrics(_t(s2), ty, tg, G, ks)
    assert torch.equal(st.rec.cpu(), eager.rec.cpu())
    assert torch.equal(st.per_group().cpu(), eager.per_group().cpu())
    C.check(st, R.group_records(s2, y, g, G, ks), len(s), G, ks)


def test_workspace_bounds():
    h = K.native.hip()
    assert h.rank_metrics_workspace_bytes(0, 1) > 0 and h.rank_metrics_workspace_bytes(8193, 10) > 8 * 4 * 8193
    for n, G in ((2 ** 30, 1), (10, 0), (10, 2 ** 31)):
        with pytest.raises(ValueError):
            h.rank_metrics_workspace_bytes(n, G)
    s, y, g, G, ks, _ = C.case("tile-2049")
    with pytest.raises(ValueError, match="ws"):
        run(s, y, g, G, ks, ws=torch.empty(1024, dtype=torch.uint8, device="cuda"))


def test_train_and_evaluate_on_cuda(tmp_path):
    """The trainer's two users of the chain on the device: the validation line and ``evaluate``."""
    import re

    from test_gauc_cli import _run, _write_cfg, _write_data
    from fast_tffm_amd.config import load_config
    from fast_tffm_amd.data.groups import load_group_files
    from fast_tffm_amd.data.reader import load_file_batch
    from fast_tffm_amd.trainer import Trainer

    _write_data(tmp_path / "train_0", tmp_path / "train_0.grp", 600, 1, 40)
    _write_data(tmp_path / "valid_0", tmp_path / "valid_0.grp", 300, 2, 40)
    _write_data(tmp_path / "valid_1", tmp_path / "valid_1.grp", 120, 3, 25)
    cfg_path = _write_cfg(tmp_path, f"validation_group_files = {tmp_path}/valid_0.grp\nvalidation_ndcg = 3",
                          device="cuda")
    with open(cfg_path, "a") as f:
        f.write("rank_cutoffs = 3, 10\n")  # (the [Predict] section is the file's last)
    rc, out = _run(["train", cfg_path, "--max-steps", "3"])
    m = re.search(r"^validation loss at step 3: [0-9.]+\nvalidation ndcg@3 at step 3: ([0-9.]+)$", out, re.M)
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
            means, ranked, _ = R.summary(R.group_records(scores, b.labels.numpy(), gi.ids, gi.num_groups, (3, 10)),
                                         (3, 10))
            e = re.search(r"^evaluate %s: .* ndcg@3 ([0-9.]+) recall@3 ([0-9.]+) precision@3 ([0-9.]+) ndcg@10 "
                          r"([0-9.]+) recall@10 ([0-9.]+) precision@10 ([0-9.]+) ranked_groups %d/%d$"
                          % (re.escape(path), ranked, gi.num_groups), out, re.M)
            assert e, out
            want = [v for t in means for v in t]
            assert all(abs(float(a) - w) <= 0.5e-8 + 1e-12 * w for a, w in zip(e.groups(), want)), (e.groups(), want)
            if name == "valid_0":
                assert m.group(1) == e.group(1)  # the validation line reported the same set's NDCG@3
            lines = open(path + "_rank").read().splitlines()
            assert len(lines) == gi.num_groups and sum(ln.split()[3] != "nan" for ln in lines) == ranked


def test_gpu_matches_cpu_twin_counts():
    s, y, g, G, ks, _ = C.case("empty-unranked")
    a = run(s, y, g, G, ks)
    b = K.rank_metrics(*(t.cpu() for t in (_t(s), _t(y), _t(g, np.int32))), G, ks)
    assert a.stats()[1:] == b.stats()[1:]
    assert torch.equal(a.per_group().cpu()[:, :2], b.per_group()[:, :2])


def test_bad_cutoffs_launch_nothing():
    with pytest.raises(ValueError):
        run([0.0, 1.0], [1.0, 0.0], [0, 0], 1, (3, 2))
    e = torch.empty(0, device="cuda")
    st = K.rank_metrics(e, e, e.to(torch.int32), 2, (1,))
    assert math.isnan(st.ndcg(1)) and not st.rec.is_cuda
