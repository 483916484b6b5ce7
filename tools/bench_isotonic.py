"""Cost of the isotonic fit on the GPU: ``K.isotonic_fit`` (hip/isotonic.hip) beside ``K.auc`` on the same inputs
(the two share the key, the sort and the scans) and, where it imports, scipy's pool-adjacent-violators on the host
(sort and tie pooling included, one call).

Inputs per size: random logistic data; the Farey staircase of order 48 (a run of q examples with p positives per
reduced fraction p/q, positives first, increasing scores: 713 blocks in 22964 examples) repeated to the size with
shifted scores -- every leaf hull keeps its staircase, the merges pool the repeats --; the Farey staircase of the
order that fills the size -- every vertex survives every merge, so every level copies the whole list: the input
that shows what the merge levels cost --; one score for all examples.  Unweighted and weighted (weights in
[0.5, 2]); a reused workspace; warm-up calls, then every repeat timed with device events around the call (no host
read in it but, with weights, the wrapper's check that drops zero weights), median over the repeats.  A record,
not a gate: writes the table to ``--out``.

    python tools/bench_isotonic.py [--sizes 131072,1048576,16777216] [--repeats 30] [--out FILE]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fast_tffm_amd.ops import kernels as K  # noqa: E402


def farey(order: int) -> np.ndarray:
    """[terms, 2] numerators and denominators of the Farey sequence, ascending (the next-term recurrence)."""
    a, b, c, d = 0, 1, 1, order
    out = [(a, b)]
    while c <= order:
        k = (order + b) // d
        a, b, c, d = c, d, k * c - a, k * d - b
        out.append((a, b))
    return np.array(out, np.int64)


def staircase_labels(order: int) -> np.ndarray:
    f = farey(order)
    starts = np.concatenate([[0], np.cumsum(f[:, 1])])
    within = np.arange(starts[-1]) - np.repeat(starts[:-1], f[:, 1])
    return (within < np.repeat(f[:, 0], f[:, 1])).astype(np.float32)


def order_filling(n: int) -> int:
    """The largest Farey order whose staircase (1 + sum over q of q phi(q) examples) has at most n examples."""
    cap = 1024
    phi = np.arange(cap + 1)
    for p in range(2, cap + 1):
        if phi[p] == p:
            phi[p::p] -= phi[p::p] // p
    sizes = 1 + np.cumsum(np.arange(1, cap + 1) * phi[1:])
    return int(np.searchsorted(sizes, n, side="right"))


def inputs(n: int):
    g = np.random.default_rng(n)
    s = g.normal(0, 2, n).astype(np.float32)
    yield "logistic", s, (g.random(n) < 1 / (1 + np.exp(-(0.7 * s + 0.3)))).astype(np.float32)
    unit = staircase_labels(48)
    yield "farey48 x%d" % (n // len(unit) + 1), np.arange(n, dtype=np.float32), np.tile(unit, n // len(unit) + 1)[:n]
    order = order_filling(n)
    lab = staircase_labels(order)
    lab = np.concatenate([lab, np.ones(n - len(lab), np.float32)])  # (the last step, 1/1, made longer)
    yield "farey%d" % order, np.arange(n, dtype=np.float32), lab
    yield "one score", np.full(n, 0.25, np.float32), (g.random(n) < 0.3).astype(np.float32)


def timed(fn, warmup: int, repeats: int) -> float:
    """Median milliseconds of fn() between two device events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def scipy_ms(s: np.ndarray, y: np.ndarray, w: np.ndarray | None) -> float | None:
    try:
        from scipy.optimize import isotonic_regression
    except ImportError:
        return None
    t0 = time.perf_counter()
    order = np.argsort(s, kind="stable")
    ss = s[order]
    w64 = np.ones(len(s)) if w is None else w[order].astype(np.float64)
    starts = np.flatnonzero(np.r_[True, ss[1:] != ss[:-1]])
    pw = np.add.reduceat(w64, starts)
    isotonic_regression(np.add.reduceat(w64 * (y[order] > 0), starts) / pw, weights=pw)
    return (time.perf_counter() - t0) * 1e3


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{2**17},{2**20},{2**24}")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calibration", "isotonic.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_isotonic: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    lines = [f"K.isotonic_fit beside K.auc, {torch.cuda.get_device_name(dev)}; median of {a.repeats} event-timed "
             f"calls after {a.warmup} warm-up calls, reused workspace; ms per call; scipy: one host call "
             "(sort + tie pooling + isotonic_regression)",
             f"{'n':>9} {'input':>14} {'mode':>10} {'blocks':>8} {'isotonic':>9} {'auc':>8} {'iso/auc':>8} "
             f"{'scipy':>9}"]
    for n in (int(x) for x in a.sizes.split(",")):
        wr = np.random.default_rng(n + 1).uniform(0.5, 2, n).astype(np.float32)
        ws, aws = K.isotonic_workspace(n, dev), K.auc_workspace(n, dev)
        for name, s_h, y_h in inputs(n):
            s, y = torch.from_numpy(s_h).to(dev), torch.from_numpy(y_h).to(dev)
            for mode, w_h in (("unweighted", None), ("weighted", wr)):
                w = None if w_h is None else torch.from_numpy(w_h).to(dev)
                blocks = K.isotonic_fit(s, y, w, ws=ws).count()
                t_i = timed(lambda: K.isotonic_fit(s, y, w, ws=ws), a.warmup, a.repeats)
                t_a = timed(lambda: K.auc(s, y, w, ws=aws), a.warmup, a.repeats)
                t_s = scipy_ms(s_h, y_h, w_h) if name == "logistic" else None
                lines.append(f"{n:>9} {name:>14} {mode:>10} {blocks:>8} {t_i:>9.3f} {t_a:>8.3f} {t_i / t_a:>8.2f} "
                             f"{'-' if t_s is None else '%.1f' % t_s:>9}")
                print(lines[-1], flush=True)
    K.check_device_errors()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
