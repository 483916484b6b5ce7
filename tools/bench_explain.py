"""Cost of explaining a batch on the GPU: ``K.fm_explain`` and ``K.feature_importance`` (hip/fm_explain.hip)
next to ``K.fm_forward(want_r1=False)``, the scorer the attributions decompose.

One bench-shaped batch (131072 examples x 39 features, Zipf(1.1) ids over 125M slots), two tables -- k=64
fp32 and k=128 fp8 -- in one process.  After warm-up calls, every repeat times each kernel of each table in
turn (the two tables alternating) with device events; medians and minima over the repeats, and the
explain / forward ratio.  A record, not a gate: writes the table to ``--out``.

    python tools/bench_explain.py [--batch 131072] [--slots 125000000] [--repeats 50] [--registers FILE]
                                  [--out profiles/explain/explain.txt]

``--registers FILE``: lines to append (the new kernels' registers and occupancy from the build's
``-Rpass-analysis=kernel-resource-usage`` report).
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fast_tffm_amd.data.synthetic import CriteoSynth  # noqa: E402
from fast_tffm_amd.models.table import FMTable, bits_for  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--slots", type=int, default=125_000_000)
    ap.add_argument("--alpha", type=float, default=1.1)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--registers", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain", "explain.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_explain: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    b = CriteoSynth(a.slots, alpha=a.alpha, seed=1000, device=dev).batch(a.batch)
    rows = b.ids.to(torch.int32)
    dd = K.dedup(rows, key_bits=bits_for(a.slots), want_perm=True)
    U = dd.sync()
    seg = dd.seg_start[: U + 1]
    longest = int((seg[1:] - seg[:-1]).max())
    cases = []
    for name, k, dtype in (("k64 fp32", 64, torch.float32), ("k128 fp8", 128, K.FP8)):
        t = FMTable(a.slots, k, dtype=dtype, opt=K.OptConfig("sgd"), init_range=0.01, seed=7, device=dev)
        t.s0v = t.s0w = None  # (only the parameters are read)
        contrib = torch.empty(b.nnz, dtype=torch.float32, device=dev)
        pred = torch.empty(b.B, dtype=torch.float32, device=dev)
        fns = {
            "explain": lambda t=t, c=contrib, p=pred: K.fm_explain(b.offsets, rows, b.vals, t.v, t.w, t.Kp,
                                                                   contrib=c, pred=p),
            "forward": lambda t=t, p=pred: K.fm_forward(b.offsets, rows, b.vals, t.v, t.w, t.Kp, want_r1=False,
                                                        pred=p, max_feats=b.max_feats),
            "importance": lambda c=contrib: K.feature_importance(c, dd),
        }
        cases.append((name, fns, {n: [] for n in fns}))
    for _ in range(a.warmup):
        for _, fns, _ in cases:
            for fn in fns.values():
                fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, fns, ms in cases:  # the two tables alternate; each kernel timed on its own
            for n, fn in fns.items():
                ms[n].append(event_ms(fn))
    lines = [f"fm_explain / feature_importance vs fm_forward(want_r1=False), {torch.cuda.get_device_name(dev)}",
             f"batch {b.B} x {b.nnz // max(b.B, 1)} features ({b.nnz} occurrences, {U} distinct ids, longest "
             f"segment {longest}), Zipf({a.alpha}) over {a.slots} slots; {a.repeats} event-timed calls per kernel "
             f"after {a.warmup} warm-up calls, the two tables alternating in one process; ms, median (min)",
             f"{'table':>10} {'explain':>16} {'forward':>16} {'importance':>16} {'explain/forward':>16}"]
    for name, _, ms in cases:
        med = {n: statistics.median(v) for n, v in ms.items()}
        cell = {n: f"{med[n]:.3f} ({min(v):.3f})" for n, v in ms.items()}
        ratio = med["explain"] / med["forward"]
        lines.append(f"{name:>10} {cell['explain']:>16} {cell['forward']:>16} {cell['importance']:>16} {ratio:>16.2f}")
        if ratio > 2.0:
            lines.append(f"  ({name}: above the 2x of the forward expected from two gathers -- the second mostly from "
                         "L2 -- plus the contributions' store; not tuned)")
    if a.registers and os.path.exists(a.registers):
        with open(a.registers) as f:
            lines += ["", f.read().rstrip("\n")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
