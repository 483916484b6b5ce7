"""fp64 oracle of the exact per-occurrence attributions (numpy), its error bound, and the shared test cases.

For example i with occurrences j = (row r_j, value x_j) and S_f = sum_j x_j v_{r_j,f}:

    c_j = x_j w_j + 1/2 sum_f x_j v_jf (S_f - x_j v_jf)                    (fp32 / bf16 rows)
    c_j = x_j w_j + 1/2 (x_j <v_j, S> - x_j^2 n2_j)                        (fp8 rows: stored norm n2_j)

on the table *as stored* (bf16 / fp8 values converted exactly; fp8: scale x e4m3).  The bound of every
comparison with a kernel is

    |c - c_oracle| <= 2 (n_i + Kp + 8) 2^-24 M_j,   M_j = |x_j w_j| + 1/2 sum_f |x_j v_jf| (A_f + |x_j v_jf|),
    A_f = sum_j |x_j v_jf|

(the first-order forward error of an n-term sum followed by a Kp-term dot product, doubled), and the sum
identity |pred - bias - sum_j c_oracle| <= the sum of the example's per-occurrence bounds.
"""

import math

import numpy as np
import torch

FP8 = torch.float8_e4m3fn
LENGTHS = [0, 1, 2, 39, 63, 64, 65, 130]
VALUES = [1.0, -2.5, 0.0, 0.3]
ROWS = 1000


def table_f64(v: torch.Tensor, w: torch.Tensor, Kp: int):
    """(V [rows, Kp], w [rows], n2 [rows] or None) in fp64 of a table or wire source as stored; ``w`` is the
    (strided) weight view, for fp8 rows the first word of the [w, scale, |v|^2, .] tails."""
    rows = v.shape[0]
    V = v[:, :Kp].float().double().cpu().numpy()  # (bf16 / e4m3 -> fp32 -> fp64: exact)
    if v.dtype == FP8:
        tails = torch.as_strided(w, (rows, 3), (w.stride(0), 1), w.storage_offset()).double().cpu().numpy()
        return V * tails[:, 1:2], tails[:, 0].copy(), tails[:, 2].copy()
    return V, w[:rows].double().cpu().numpy(), None


def explain_oracle(offsets, rows, vals, V, w, n2=None):
    """(c [nnz], tol [nnz]) in fp64; arguments are numpy arrays (``vals`` may be None: all 1)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    nnz = rows.size
    x = np.ones(nnz) if vals is None else np.asarray(vals, dtype=np.float64)
    Kp = V.shape[1]
    c = np.zeros(nnz)
    tol = np.zeros(nnz)
    for i in range(offsets.size - 1):
        s, e = offsets[i], offsets[i + 1]
        if e == s:
            continue
        xv = x[s:e, None] * V[rows[s:e]]          # [n, Kp]
        S = xv.sum(0)
        A = np.abs(xv).sum(0)
        lin = x[s:e] * w[rows[s:e]]
        if n2 is None:
            pair = (xv * (S[None, :] - xv)).sum(1)
        else:
            pair = xv @ S - x[s:e] ** 2 * n2[rows[s:e]]
        c[s:e] = lin + 0.5 * pair
        M = np.abs(lin) + 0.5 * (np.abs(xv) * (A[None, :] + np.abs(xv))).sum(1)
        tol[s:e] = 2.0 * ((e - s) + Kp + 8) * 2.0 ** -24 * M
    return c, tol


def example_sums(offsets, a):
    offsets = np.asarray(offsets, dtype=np.int64)
    cs = np.concatenate([[0.0], np.cumsum(a)])
    return cs[offsets[1:]] - cs[offsets[:-1]]


def make_batch(seed: int = 0, with_vals: bool = True):
    """(offsets int32, rows int32, vals fp32 or None) -- numpy: every length of LENGTHS five times in a
    shuffled order between an empty first and an empty last example (B = 42), one example repeating one id
    three times, values from VALUES."""
    rng = np.random.default_rng(seed)
    mid = [n for n in LENGTHS for _ in range(5)]
    rng.shuffle(mid)
    lens = [0] + mid + [0]
    offsets = np.zeros(len(lens) + 1, dtype=np.int32)
    np.cumsum(lens, out=offsets[1:])
    nnz = int(offsets[-1])
    rows = rng.integers(0, ROWS, nnz).astype(np.int32)
    i = lens.index(39)
    rows[offsets[i] + np.array([3, 4, 20])] = 7  # the same id three times in one example
    vals = rng.choice(np.array(VALUES, dtype=np.float32), nnz) if with_vals else None
    if vals is not None:
        vals[offsets[i] + np.array([3, 4, 20])] = [1.0, -2.5, 0.3]
    return offsets, rows, vals


def make_table(dtype, K: int, device="cpu", seed: int = 1, rows: int = ROWS, row_stride: int | None = None):
    """(v [rows, Kp] view, w strided view, Kp): rows random at two magnitudes (even rows 0.01, odd rows 1) so
    that pairwise terms matter; columns K .. Kp are zero.  fp8: per-row power-of-two scales and the tails
    [w, scale, |v|^2, 0] of a table (``w`` = column 0, stride 4).  ``row_stride``: a v view of wider rows."""
    from fast_tffm_amd.ops import kernels as Kn

    Kp = Kn.padded_k(K)
    g = torch.Generator().manual_seed(seed)
    mag = torch.where(torch.arange(rows) % 2 == 0, 0.01, 1.0)[:, None]
    dense = torch.zeros(rows, Kp)
    dense[:, :K] = (torch.rand(rows, K, generator=g) * 2 - 1) * mag
    wv = (torch.rand(rows, generator=g) * 2 - 1) * 0.5
    stride = row_stride or Kp
    if dtype == FP8:
        q, s = Kn.quantize_fp8_rows(dense.to(device))
        store = torch.zeros((rows, stride), dtype=torch.uint8, device=device).view(FP8)
        store[:, :Kp] = q
        tails = torch.zeros((rows, 4), dtype=torch.float32, device=device)
        tails[:, 0] = wv.to(device)
        tails[:, 1] = s
        tails[:, 2] = (q.float() ** 2).sum(1) * s * s
        return store[:, :Kp], tails[:, 0], Kp
    store = torch.zeros((rows, stride), dtype=dtype, device=device)
    store[:, :Kp] = dense.to(dtype).to(device)
    return store[:, :Kp], wv.to(device), Kp


def check_case(off, rows, vals, v, w, Kp, contrib, pred, factor=1.0, what=""):
    """A run without bias: contributions within ``factor`` x the bound of the oracle, the sum identity for
    ``pred``, and pred == 0 for empty examples.  Returns (c_oracle, tol)."""
    V, wv, n2 = table_f64(v, w, Kp)
    c, tol = explain_oracle(off, rows, vals, V, wv, n2)
    got = contrib.double().cpu().numpy()
    err = np.abs(got - c)
    worst = float((err / np.maximum(tol, 1e-300)).max()) if c.size else 0.0
    print(f"{what}: max |c - oracle| / bound = {worst:.4f}")
    assert (err <= factor * tol).all(), (what, worst)
    check_sum_identity(off, c, tol, pred, what)
    return c, tol


def check_sum_identity(off, c, tol, pred, what=""):
    """|pred - sum_j c_oracle| <= sum_j tol for scores computed without a bias; empty examples score 0."""
    p = pred.double().cpu().numpy()
    gap = np.abs(p - example_sums(off, c))
    lim = example_sums(off, tol)
    print(f"{what}: max sum-identity gap / bound = {float((gap / np.maximum(lim, 1e-300)).max()):.4f}")
    assert (gap <= lim).all(), (what, "sum identity", float(gap.max()))
    assert (p[np.diff(np.asarray(off)) == 0] == 0.0).all(), (what, "empty examples")


def check_bias(off, pred_bias, pred, bias, what=""):
    """Scores with a bias are the bias-free scores plus the bias, one fp32 addition (so the sum identity holds
    for ``pred - bias`` up to that addition's rounding, which the bound above does not model); empty examples
    score exactly the bias."""
    pb, p0 = pred_bias.cpu().numpy(), pred.cpu().numpy()
    assert pb.dtype == np.float32 and np.array_equal(pb, p0 + np.float32(bias)), (what, "bias")
    assert (pb[np.diff(np.asarray(off)) == 0] == np.float32(bias)).all(), (what, "empty examples")


def group_by(ids, c):
    """(uniq, count, sum |c|, sum c) per distinct id; the sums are exact (math.fsum), rounded once to fp64."""
    ids = np.asarray(ids)
    order = np.argsort(ids, kind="stable")
    uniq, start, cnt = np.unique(ids[order], return_index=True, return_counts=True)
    cs = np.asarray(c, dtype=np.float64)[order]
    sa = np.array([math.fsum(np.abs(cs[s:s + n])) for s, n in zip(start, cnt)])
    sm = np.array([math.fsum(cs[s:s + n]) for s, n in zip(start, cnt)])
    return uniq, cnt, sa, sm


def check_importance(ids, contrib, got):
    """``feature_importance``'s (uniq, count, sum_abs, sum): counts equal the group-by's, sums within
    n 2^-53 sum |c| of it."""
    uniq, cnt, sa, sm = group_by(ids, contrib)
    g_u, g_n, g_a, g_s = [t.cpu().numpy() for t in got]
    assert np.array_equal(g_u.astype(np.int64), uniq.astype(np.int64)) and np.array_equal(g_n.astype(np.int64), cnt)
    assert g_a.dtype == np.float64 and g_s.dtype == np.float64
    lim = cnt * 2.0 ** -53 * sa
    assert (np.abs(g_a - sa) <= lim).all() and (np.abs(g_s - sm) <= lim).all()
    return cnt
