"""``K.fm_pairs`` (CPU twin) and ``run.py explain --pairs`` against an fp64 oracle.  Bound: the fp64 ``q_jl`` and
the fp32 ``p_jl`` differ by at most ``t_jl = (Kp + 3) 2^-24 |x_j x_l| sum_k |v_jk v_lk|`` (a Kp-term fma chain plus
two products), evaluated in fp64 on the stored (widened) rows."""

import contextlib
import io
import os

import numpy as np
import pytest
import torch

from explain_oracle import ROWS, example_sums, explain_oracle, make_table, table_f64
from fast_tffm_amd import cli
from fast_tffm_amd.ops import kernels as K

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
LENS = [100, 0, 17, 1, 33, 16, 2, 15, 0, 15, 2, 16, 33, 1, 17, 100]  # n in {0, 1, 2, 15, 16, 17, 33, 100}, mixed
# (Kf, dtype, values, top): one sweep per axis around the base case
GRID = ([(20, "fp32", True, 8)] + [(Kf, "fp32", True, 8) for Kf in (1, 10, 16, 64, 256)] + [(20, "bf16", True, 8)]
        + [(20, "fp32", False, 8), (20, "fp32", True, 1), (20, "fp32", True, 64)])


def batch_of(lens, seed, with_vals=True):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    ids = rng.integers(0, ROWS, int(off[-1])).astype(np.int32)
    vals = rng.choice(np.array([1.0, -2.5, 0.0, 0.3], dtype=np.float32), ids.size) if with_vals else None
    return off, ids, vals


def oracle(rows, x, V, Kp):
    """(q [n, n], t [n, n]) of one example in fp64: every pair term and its bound."""
    Vr = V[rows]
    xx = np.outer(x, x)
    return xx * (Vr @ Vr.T), (Kp + 3) * 2.0 ** -24 * np.abs(xx) * (np.abs(Vr) @ np.abs(Vr).T)


def run(off, ids, vals, v, Kp, top, device="cpu", **kw):
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)  # noqa: E731
    return K.fm_pairs(t(off), t(ids), t(vals), v, Kp, top, **kw)


def check_lists(off, ids, vals, v, Kp, top, out):
    """The acceptance of the returned lists; returns per example (sum of p, sum of t) over the returned pairs."""
    V = v[:, :Kp].float().double().cpu().numpy()
    first, second, value, count = [a.cpu().numpy() for a in out]
    assert first.shape == second.shape == value.shape == (off.size - 1, top) and count.shape == (off.size - 1,)
    sums = np.zeros((off.size - 1, 2))
    for i in range(off.size - 1):
        s, n = off[i], off[i + 1] - off[i]
        c = count[i]
        assert c == (-1 if n > K.PAIRS_MAX_N else min(top, n * (n - 1) // 2)), i
        c = max(c, 0)
        assert (first[i, c:] == -1).all() and (second[i, c:] == -1).all() and (value[i, c:] == 0).all(), i
        if c == 0:
            continue
        x = np.ones(n) if vals is None else vals[s:s + n].astype(np.float64)
        q, t = oracle(ids[s:s + n], x, V, Kp)
        j, l, p = first[i, :c], second[i, :c], value[i, :c].astype(np.float64)
        assert (0 <= j).all() and (j < l).all() and (l < n).all() and len(set(zip(j, l))) == c, i
        assert (np.abs(p - q[j, l]) <= t[j, l]).all(), i
        a = np.abs(p)
        assert (a[1:] <= a[:-1]).all(), i
        tie = a[1:] == a[:-1]
        assert ((j[1:] > j[:-1]) | ((j[1:] == j[:-1]) & (l[1:] > l[:-1])))[tie].all(), i
        rest = np.triu(np.ones((n, n), dtype=bool), 1)
        rest[j, l] = False
        assert (np.abs(q[rest]) <= abs(q[j[-1], l[-1]]) + t[j[-1], l[-1]] + t[rest]).all(), i
        sums[i] = p.sum(), t[j, l].sum()
    return sums


@pytest.mark.parametrize("Kf,dtype,with_vals,top", GRID)
def test_cpu_grid_against_oracle(Kf, dtype, with_vals, top):
    off, ids, vals = batch_of(LENS, Kf + top, with_vals)
    v, _, Kp = make_table(DTYPES[dtype], Kf)
    check_lists(off, ids, vals, v, Kp, top, run(off, ids, vals, v, Kp, top, threads=2))


def constructed(kind, n=100):
    """Rows a_j e_0 (exact products): (off, ids, v, Kp) of one example of n occurrences, row j = occurrence j."""
    a = {"ascending": np.arange(1, n + 1), "descending": np.arange(n, 0, -1), "constant": np.ones(n)}[kind]
    v = torch.zeros((n, 4))
    v[:, 0] = torch.from_numpy(a.astype(np.float32))
    return np.array([0, n], dtype=np.int32), np.arange(n, dtype=np.int32), v, a.astype(np.float64)


def check_constructed(kind, out, top=8, n=100):
    """ascending: the buffer overflows and re-sorts; descending: nothing late wins; constant: all tie.  Exact."""
    a = constructed(kind, n)[3]
    jj, ll = np.triu_indices(n, 1)
    best = np.lexsort((ll, jj, -(a[jj] * a[ll])))[:top]
    got = [t.cpu().numpy()[0].tolist() for t in out]
    assert got == [jj[best].tolist(), ll[best].tolist(), (a[jj] * a[ll])[best].tolist(), top]


@pytest.mark.parametrize("kind", ["ascending", "descending", "constant"])
def test_cpu_constructed_examples(kind):
    off, ids, v, _ = constructed(kind)
    check_constructed(kind, run(off, ids, None, v, 4, 8))


def check_long_example(device, v, Kp):
    """4097 occurrences between two ordinary examples: count -1, no pairs, the neighbours as without it."""
    off, ids, vals = batch_of([5, K.PAIRS_MAX_N + 1, 7], 3)
    out = run(off, ids, vals, v, Kp, 8, device)
    check_lists(off, ids, vals, v, Kp, 8, out)
    assert out[3].tolist() == [8, -1, 8]
    keep = np.r_[0:5, off[2]:off[3]]
    ref = run(np.array([0, 5, 12], dtype=np.int32), ids[keep], vals[keep], v, Kp, 8, device)
    assert all(torch.equal(a[[0, 2]], b) for a, b in zip(out, ref))


def test_cpu_long_example():
    check_long_example("cpu", *make_table(torch.float32, 20)[::2])


def test_cpu_sum_identity():
    """top = 64, n <= 11: every pair is back; sum x w + sum p is fm_forward's score within the t's + its own bound."""
    off, ids, vals = batch_of(list(range(12)) * 2, 9)
    v, w, Kp = make_table(torch.float32, 20)
    sums = check_lists(off, ids, vals, v, Kp, 64, run(off, ids, vals, v, Kp, 64))
    V, wv, _ = table_f64(v, w, Kp)
    _, tol = explain_oracle(off, ids, vals, V, wv)
    lin = example_sums(off, vals.astype(np.float64) * wv[ids])
    fo = K.fm_forward(torch.from_numpy(off), torch.from_numpy(ids), torch.from_numpy(vals), v, w, Kp, want_r1=False)
    gap = np.abs(fo.pred.double().numpy() - (lin + sums[:, 0]))
    assert (gap <= sums[:, 1] + example_sums(off, tol)).all(), float(gap.max())


def test_argument_errors():
    off, ids, vals = batch_of([3, 4], 1)
    v, _, Kp = make_table(torch.float32, 8)
    for what, ids_, v_, top in (("top", ids, v, 0), ("top", ids, v, 65), ("fp8", ids, v.to(K.FP8), 8),
                                ("rows", ids.astype(np.int64), v, 8)):
        with pytest.raises(ValueError, match=what):
            run(off, ids_, vals, v_, Kp, top)


def test_cli_explain_pairs(tmp_path):
    rng = np.random.default_rng(4)
    os.makedirs(tmp_path / "data")
    for name, lens in (("train", rng.integers(2, 9, 60)), ("test", [1, 2, 3] + list(rng.integers(4, 9, 9)))):
        with open(tmp_path / "data" / name, "w") as f:
            for n in lens:
                feats = [f"{int(rng.integers(0, 50))}:{rng.choice([1, 0.5, -2])}" for _ in range(n)]
                f.write(" ".join([str(int(rng.integers(0, 2)))] + feats) + "\n")
    cfg, test = str(tmp_path / "run.cfg"), str(tmp_path / "data" / "test")
    with open(cfg, "w") as f:
        f.write(f"[General]\nvocabulary_size = 50\nvocabulary_block_num = 1\nfactor_num = 6\nhash_feature_id = False\n"
                f"log_dir = {tmp_path}/log\ndevice = cpu\n"
                f"[Train]\nbatch_size = 20\ninit_value_range = 0.3\nfactor_lambda = 0\nbias_lambda = 0\nepoch_num = 1\n"
                f"learning_rate = 0.1\nadagrad.initial_accumulator = 0.1\nloss_type = logistic\n"
                f"train_files = {tmp_path}/data/train\n[Predict]\npredict_files = {test}\n")
    read = lambda *sfx: [open(test + x, "rb").read() for x in sfx]  # noqa: E731
    with contextlib.redirect_stdout(io.StringIO()):
        assert cli.main(["train", cfg]) == 0 and cli.main(["predict", cfg]) == 0 and cli.main(["explain", cfg]) == 0
        plain = read("_contrib", "_importance")
        assert not os.path.exists(test + "_pairs") and cli.main(["explain", cfg, "--pairs", "3"]) == 0
    assert read("_contrib", "_importance") == plain
    lines = [ln.split() for ln in open(test + "_pairs")]
    feats = [[int(tok.split(":")[0]) for tok in ln.split()[1:]] for ln in open(test)]
    assert [ln[0] for ln in lines] == open(test + "_score").read().split()
    assert [len(ln) - 1 for ln in lines] == [min(3, len(f) * (len(f) - 1) // 2) for f in feats]
    acc = {}
    for ln, f in zip(lines, feats):
        for a, b, x in (tok.split(":") for tok in ln[1:]):
            assert int(a) in f and int(b) in f
            acc.setdefault((min(int(a), int(b)), max(int(a), int(b))), []).append(np.float64(np.float32(x)))
    imp = [ln.split() for ln in open(test + "_pair_importance")]
    assert [(int(r[0]), int(r[1])) for r in imp] == sorted(acc, key=lambda k: (-sum(abs(x) for x in acc[k]), k))
    for r in imp:
        xs = np.array(acc[(int(r[0]), int(r[1]))])
        assert r[2:] == [str(xs.size)] + [str(np.float32(sum(y) / xs.size)) for y in (np.abs(xs), xs)]
