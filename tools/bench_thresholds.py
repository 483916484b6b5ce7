"""Cost of the threshold metrics on the GPU: ``K.threshold_metrics`` (hip/threshold_metrics.hip) without targets
and with 4 precision + 4 recall targets, beside ``K.auc`` (the same key, sort and tile scans) and
``K.isotonic_fit`` (the same two prefixes, then the hull merges) on the same input in the same process.

Inputs per size: continuous scores (logistic data, ~30% positives) and the same scores rounded to one decimal
(about a hundred tie runs, each across many tiles: every positive's run end is a binary search); unweighted and
weighted (weights in [0.5, 2]); reused workspaces; warm-up calls, then every repeat timed with device events around
the call (no host read in it), the four ops alternating per input; median over the repeats.  A record, not a gate:
writes the table to ``--out``.

    python tools/bench_thresholds.py [--sizes 131072,1048576,16777216] [--repeats 30] [--out FILE]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from fast_tffm_amd.ops import kernels as K  # noqa: E402

PT = (0.5, 0.8, 0.9, 0.99)
RT = (0.5, 0.8, 0.9, 0.99)


def inputs(n: int):
    g = np.random.default_rng(n)
    s = g.normal(0, 2, n).astype(np.float32)
    y = (g.random(n) < 1 / (1 + np.exp(-(0.7 * s - 1.2)))).astype(np.float32)
    yield "continuous", s, y
    yield "one decimal", np.round(s, 1), y


def timed(fns: list, warmup: int, repeats: int) -> list:
    """Median milliseconds of every fn() between two device events, the fns alternating within a repeat."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    return [statistics.median(m) for m in ms]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{2**17},{2**20},{2**24}")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "thresholds", "thresholds.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_thresholds: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    lines = [f"K.threshold_metrics beside K.auc and K.isotonic_fit, {torch.cuda.get_device_name(dev)}; median of "
             f"{a.repeats} event-timed calls after {a.warmup} warm-up calls, the ops alternating, reused workspaces; "
             "ms per call; thr: no targets, thr 4+4: 4 precision and 4 recall targets",
             f"{'n':>9} {'scores':>12} {'mode':>10} {'thr':>8} {'thr 4+4':>8} {'auc':>8} {'isotonic':>9} "
             f"{'thr/auc':>8} {'4+4/auc':>8} {'iso/auc':>8} {'ap':>11}"]
    for n in (int(x) for x in a.sizes.split(",")):
        wr = np.random.default_rng(n + 1).uniform(0.5, 2, n).astype(np.float32)
        tws, aws, iws = K.threshold_workspace(n, dev), K.auc_workspace(n, dev), K.isotonic_workspace(n, dev)
        for name, s_h, y_h in inputs(n):
            s, y = torch.from_numpy(s_h).to(dev), torch.from_numpy(y_h).to(dev)
            for mode, w_h in (("unweighted", None), ("weighted", wr)):
                w = None if w_h is None else torch.from_numpy(w_h).to(dev)
                v = K.threshold_metrics(s, y, w, ws=tws).ap()
                t0, t8, ta, ti = timed([
                    lambda: K.threshold_metrics(s, y, w, ws=tws),
                    lambda: K.threshold_metrics(s, y, w, precision_targets=PT, recall_targets=RT, ws=tws),
                    lambda: K.auc(s, y, w, ws=aws),
                    lambda: K.isotonic_fit(s, y, w, ws=iws)], a.warmup, a.repeats)
                lines.append(f"{n:>9} {name:>12} {mode:>10} {t0:>8.3f} {t8:>8.3f} {ta:>8.3f} {ti:>9.3f} "
                             f"{t0 / ta:>8.2f} {t8 / ta:>8.2f} {ti / ta:>8.2f} {v:>11.8f}")
                print(lines[-1], flush=True)
    K.check_device_errors()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
