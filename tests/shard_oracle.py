"""Plain numpy / torch references of the row-sharded exchange's owner-side kernels
(csrc/hip/shard.hip), written the obvious way and with no project code in them: the request
lists are small, so memberships are ``np.isin`` over slices and run lookups are loops or
``np.searchsorted`` over the run boundaries.  tests/test_shard_oracle.py checks each helper on
hand-written cases; tests/test_shard_kernels_gpu.py compares the kernels with them.

Vocabulary: a request list ``req`` [R] is W ascending, distinct runs laid end to end, one per
source rank; ``run_off`` [W+1] is the prefix of the run lengths (``splits``).
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import adagrad_step, ftrl_step

# Run shapes of the tests: W runs, the listed ones empty, the others of lo..hi rows.
SHAPES = {
    "A": dict(W=1, empty=(), lo=300, hi=600),
    "B": dict(W=2, empty=(0,), lo=300, hi=600),
    "C": dict(W=5, empty=(1, 4), lo=300, hi=600),
    "D": dict(W=8, empty=(), lo=300, hi=600),
    "E": dict(W=64, empty=tuple(range(1, 64, 2)), lo=1, hi=40),
}


def make_runs(rng, W, rows, lo, hi, empty=()):
    """(req int32 [R], splits, run_off int32 [W+1]): W ascending runs of distinct rows of
    [0, rows), lo..hi rows each, the runs in ``empty`` of length 0.  All runs draw from one
    random pool of rows half as large as the request list, so they overlap: with two or more
    non-empty runs at least a third of the distinct rows occur in two or more runs (asserted)."""
    splits = [0 if q in empty else int(rng.integers(lo, hi + 1)) for q in range(W)]
    total = sum(splits)
    span = min(rows, max(max(splits), total // 2, 1))
    pool = np.sort(rng.choice(rows, size=span, replace=False))
    runs = [np.sort(rng.choice(pool, size=n, replace=False)) for n in splits]
    req = np.concatenate(runs).astype(np.int32) if total else np.zeros(0, np.int32)
    run_off = np.concatenate([[0], np.cumsum(splits)]).astype(np.int32)
    for r in runs:
        assert np.all(np.diff(r) > 0)
    if sum(n > 0 for n in splits) >= 2:
        _, cnt = np.unique(req, return_counts=True)
        assert 3 * int((cnt >= 2).sum()) >= cnt.size, (int((cnt >= 2).sum()), cnt.size)
    return req, splits, run_off


def shape_runs(name, seed, rows):
    """The runs of shape ``name`` (SHAPES) over a table of ``rows`` rows."""
    s = SHAPES[name]
    return make_runs(np.random.default_rng(seed), s["W"], rows, s["lo"], s["hi"], s["empty"])


def member(req, prev, prev_off):
    """flag[i] = 1 when req[i] is in one of the runs of ``prev`` (``prev_off`` [Wp+1])."""
    flag = np.zeros(len(req), np.int32)
    for q in range(len(prev_off) - 1):
        flag |= np.isin(req, prev[prev_off[q]:prev_off[q + 1]]).astype(np.int32)
    return flag


def dirty(req, run_off, prev, prev_off, skip):
    """(flag, dcount [W]): membership of ``req`` in ``prev`` with the requests of ``skip`` =
    (s0, s1) (or None) never flagged, and the number of flagged requests per run of ``req``."""
    flag = member(req, prev, prev_off)
    if skip is not None:
        flag[skip[0]:skip[1]] = 0
    W = len(run_off) - 1
    dcount = np.array([flag[run_off[q]:run_off[q + 1]].sum() for q in range(W)], np.int32)
    return flag, dcount


def excl(req, run_off, me):
    """flag per row of run ``me``: 1 when no other run holds the row."""
    mine = req[run_off[me]:run_off[me + 1]]
    others = np.concatenate([req[:run_off[me]], req[run_off[me + 1]:run_off[-1]]])
    return (~np.isin(mine, others)).astype(np.int32)


def tags(idx, run_off):
    """idx[p] - run_off[run of idx[p]]: the position of request idx[p] inside its run."""
    out = np.zeros(len(idx), np.int32)
    for p, i in enumerate(idx):
        run = [q for q in range(len(run_off) - 1) if run_off[q] <= i < run_off[q + 1]]
        assert len(run) == 1
        out[p] = i - run_off[run[0]]
    return out


def wire_rows(table, fmt, rows, tag=None):
    """Expected wire rows of table rows ``rows``: (v section uint8 [R, Kp * esz], tail int32
    [R, 4]).  The v section is the stored bits of ``table.v[rows]`` (an fp32 table on a bf16
    wire: of ``table.v[rows].to(torch.bfloat16)``); the tail the bits of [w, scale | 0,
    |v|^2 | 0] (scale and norm from an fp8 table's [w, scale, |v|^2, .] row tails) and the
    integer ``tag`` (None: 0)."""
    rows = np.asarray(rows, np.int64)
    R = len(rows)
    v = table.v.detach().cpu()
    if fmt.dtype != v.dtype:
        assert v.dtype == torch.float32 and fmt.dtype == torch.bfloat16
        v = v.to(torch.bfloat16)
    esz = v.element_size()
    vbytes = v.contiguous().view(torch.uint8).numpy().reshape(v.shape[0], -1)[rows][:, : fmt.Kp * esz]
    tail = np.zeros((R, 4), np.float32)
    if getattr(table, "wx", None) is not None:
        tail[:, :3] = table.wx.detach().cpu().numpy()[rows][:, :3]
    else:
        tail[:, 0] = table.w.detach().cpu().numpy()[rows]
    tail = tail.view(np.int32)
    if tag is not None:
        tail[:, 3] = np.asarray(tag, np.int32)
    return np.ascontiguousarray(vbytes), tail


def opt_reference(name, p, s0, s1, g, lr, l1=0.0, l2=0.0, beta=0.0):
    """One optimizer step in fp64 on 2-D [n, c] tensors (every row touched): (p, s0, s1).
    adagrad / ftrl: tests/oracle.py's formulas; sgd: p - lr * g."""
    p, g = p.double(), g.double()
    if name == "adagrad":
        assert bool((g != 0).any(dim=1).all())
        p1, a1 = adagrad_step(p, s0.double(), g, lr)
        return p1, a1, None
    if name == "ftrl":
        touched = torch.ones(p.shape[0], dtype=torch.bool)
        p1, n1, z1 = ftrl_step(p, s0.double(), s1.double(), g, touched, lr, l1, l2, beta)
        return p1, n1, z1
    assert name == "sgd"
    return p - lr * g, None, None


def fp8_e4m3_values():
    """The 256 values of the OCP e4m3 (fn) byte codes as fp32 (0x7f / 0xff: NaN)."""
    out = np.zeros(256, np.float32)
    for b in range(256):
        e, m = (b >> 3) & 15, b & 7
        mag = m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7)
        if e == 15 and m == 7:
            mag = float("nan")
        out[b] = -mag if b & 0x80 else mag
    return out


def apply_reference(name, state, req, grad, Kp, lr, l1=0.0, l2=0.0, beta=0.0, keep_rows=()):
    """The owner apply in fp64.  ``state``: dict of CPU tensors v [rows, >= Kp], w, s0v, s0w,
    s1v, s1w (None where the optimizer has none); ``req`` [R] the table row of every gradient
    row of ``grad`` [R, >= Kp + 1] ([g_v | g_w]).  Every distinct requested row outside
    ``keep_rows`` gets the sum of all its gradient rows and one step.  Returns (rows [U], p, s0,
    s1, near): [U, Kp + 1] fp64 results with w in column Kp (s0 / s1 None without that state) and
    ``near``, the FTRL elements whose |z| is within 1e-4 of l1 (p is discontinuous there)."""
    req = np.asarray(req, np.int64)
    rows = np.setdiff1d(np.unique(req), np.asarray(keep_rows, np.int64))
    g = torch.zeros((len(rows), Kp + 1), dtype=torch.float64)
    sel = np.flatnonzero(np.isin(req, rows))  # gradient rows of the applied table rows
    slot = np.searchsorted(rows, req[sel])    # rows is sorted and holds every req[sel]
    g.index_add_(0, torch.from_numpy(slot), grad[torch.from_numpy(sel), : Kp + 1].double())
    idx = torch.from_numpy(rows)

    def cat(v, w):
        if v is None:
            return None
        return torch.cat([v[idx][:, :Kp].double(), w[idx].double()[:, None]], dim=1)

    p0 = cat(state["v"], state["w"])
    s0 = cat(state["s0v"], state["s0w"]) if name != "sgd" else None
    s1 = cat(state["s1v"], state["s1w"]) if name == "ftrl" else None
    p1, n1, z1 = opt_reference(name, p0, s0, s1, g, lr, l1, l2, beta)
    near = (z1.abs() - l1).abs() < 1e-4 if name == "ftrl" else torch.zeros_like(p1, dtype=torch.bool)
    return rows, p1, n1, z1, near
