"""Cost of the DeLong statistics on the GPU: ``K.auc_delong`` (hip/auc_delong.hip) with one model and with two,
beside ``K.auc`` (the same key, sort and tile scans) on the same input in the same process.

Inputs per size: continuous scores (logistic data, ~30% positives) and the same scores rounded to one decimal
(about a hundred tie runs, each across many tiles: every position's run is two binary searches); the second model
is correlated with the first; reused workspaces; warm-up calls, then every repeat timed with device events around
the call (no host read in it), the three ops alternating per input; median over the repeats.  A record, not a
gate: writes the table to ``--out``.

    python tools/bench_delong.py [--sizes 131072,1048576,16777216] [--repeats 30] [--out FILE]
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


def inputs(n: int):
    g = np.random.default_rng(n)
    s = g.normal(0, 2, n).astype(np.float32)
    y = (g.random(n) < 1 / (1 + np.exp(-(0.7 * s - 1.2)))).astype(np.float32)
    o = (0.8 * s + 1.2 * g.normal(0, 1, n)).astype(np.float32)
    yield "continuous", s, o, y
    yield "one decimal", np.round(s, 1), np.round(o, 1), y


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "delong", "delong.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_delong: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    lines = [f"K.auc_delong beside K.auc, {torch.cuda.get_device_name(dev)}; median of {a.repeats} event-timed calls "
             f"after {a.warmup} warm-up calls, the ops alternating, reused workspaces; ms per call; delong 1 / 2: one "
             "model / two models",
             f"{'n':>9} {'scores':>12} {'delong 1':>9} {'delong 2':>9} {'auc':>8} {'1/auc':>7} {'2/auc':>7} "
             f"{'auc value':>11} {'se':>11} {'z':>9}"]
    for n in (int(x) for x in a.sizes.split(",")):
        dws, aws = K.delong_workspace(n, dev), K.auc_workspace(n, dev)
        for name, s_h, o_h, y_h in inputs(n):
            s, o, y = (torch.from_numpy(v).to(dev) for v in (s_h, o_h, y_h))
            ds = K.auc_delong(s, y, o, ws=dws)
            v, se, z = ds.auc(), ds.std_error(), ds.difference()[2]
            assert v == K.auc(s, y, ws=aws).value()
            t1, t2, ta = timed([lambda: K.auc_delong(s, y, ws=dws), lambda: K.auc_delong(s, y, o, ws=dws),
                                lambda: K.auc(s, y, ws=aws)], a.warmup, a.repeats)
            lines.append(f"{n:>9} {name:>12} {t1:>9.3f} {t2:>9.3f} {ta:>8.3f} {t1 / ta:>7.2f} {t2 / ta:>7.2f} "
                         f"{v:>11.8f} {se:>11.3e} {z:>9.3f}")
            print(lines[-1], flush=True)
    K.check_device_errors()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
