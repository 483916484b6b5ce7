"""Cost of ranking every example's feature pairs on the GPU: ``K.fm_pairs`` at ``top = 10`` (hip/fm_pairs.hip)
next to ``K.fm_explain`` on the same batch, and next to the torch alternative (gather the rows to ``[B, n, Kp]``,
``bmm``, mask the lower triangle, ``topk``).

The bench-shaped batch of tools/bench_explain.py (131072 examples x 39 features, Zipf(1.1) ids over 125M slots),
two k = 64 tables -- fp32 and bf16 -- in one process.  After warm-up calls, every repeat times each kernel of
each table in turn with device events; medians and minima over the repeats.  Two floors beside them: the
batch's row gathers at the random-row rate of profiles/r3/roofline.txt (6.4 TB/s), and 2 * n (n - 1) / 2 * Kp
flops per example at the fp32 matrix-core peak.  A record, not a gate: writes the table to ``--out``.

    python tools/bench_pairs.py [--batch 131072] [--slots 125000000] [--repeats 30] [--note FILE]
                                [--out profiles/explain/pairs.txt]

``--note FILE``: lines to append (what was expected, what was not tried, the headline before and after).
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
from fast_tffm_amd.models.table import FMTable  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402
from tools.bench_explain import event_ms  # noqa: E402

GATHER_BYTES_PER_S = 6.4e12   # profiles/r3/roofline.txt: random 256-B rows, read-only
MATRIX_FP32_FLOPS = 157.3e12  # MI355X fp32 matrix peak


def torch_pairs(b, rows, v, n, top):
    """The alternative without the kernel: needs examples of one length n; materialises [B, n, n]."""
    g = v[rows.long()].float().view(b.B, n, -1)
    x = torch.ones(b.B, n, device=g.device) if b.vals is None else b.vals.view(b.B, n)
    p = torch.bmm(g, g.transpose(1, 2)) * (x[:, :, None] * x[:, None, :])
    p = p.masked_fill(~torch.ones(n, n, dtype=torch.bool, device=g.device).triu(1), 0.0)
    return p.abs().view(b.B, n * n).topk(top, dim=1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=131072)
    ap.add_argument("--slots", type=int, default=125_000_000)
    ap.add_argument("--alpha", type=float, default=1.1)
    ap.add_argument("--top", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--note", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "explain", "pairs.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_pairs: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    b = CriteoSynth(a.slots, alpha=a.alpha, seed=1000, device=dev).batch(a.batch)
    rows = b.ids.to(torch.int32)
    n = b.nnz // b.B
    assert n * b.B == b.nnz, "the torch line needs examples of one length"
    cases = []
    for name, dtype in (("k64 fp32", torch.float32), ("k64 bf16", torch.bfloat16)):
        t = FMTable(a.slots, 64, dtype=dtype, opt=K.OptConfig("sgd"), init_range=0.01, seed=7, device=dev)
        t.s0v = t.s0w = None  # (only the parameters are read)
        out = dict(first=torch.empty((b.B, a.top), dtype=torch.int32, device=dev),
                   second=torch.empty((b.B, a.top), dtype=torch.int32, device=dev),
                   value=torch.empty((b.B, a.top), dtype=torch.float32, device=dev),
                   count=torch.empty(b.B, dtype=torch.int32, device=dev))
        contrib = torch.empty(b.nnz, dtype=torch.float32, device=dev)
        pred = torch.empty(b.B, dtype=torch.float32, device=dev)
        fns = {
            "pairs": lambda t=t, o=out: K.fm_pairs(b.offsets, rows, b.vals, t.v, t.Kp, a.top, **o),
            "explain": lambda t=t, c=contrib, p=pred: K.fm_explain(b.offsets, rows, b.vals, t.v, t.w, t.Kp,
                                                                   contrib=c, pred=p),
            "torch": lambda t=t: torch_pairs(b, rows, t.v, n, a.top),
        }
        floors = (b.nnz * t.Kp * t.v.element_size() / GATHER_BYTES_PER_S * 1e3,
                  b.B * 2 * (n * (n - 1) // 2) * t.Kp / MATRIX_FP32_FLOPS * 1e3)
        cases.append((name, fns, {k: [] for k in fns}, floors))
    for _ in range(a.warmup):
        for _, fns, _, _ in cases:
            for fn in fns.values():
                fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, fns, ms, _ in cases:  # the two tables alternate; each kernel timed on its own
            for k, fn in fns.items():
                ms[k].append(event_ms(fn))
    lines = [f"fm_pairs (top {a.top}) vs fm_explain vs torch (gather, bmm, mask, topk), "
             f"{torch.cuda.get_device_name(dev)}",
             f"batch {b.B} x {n} features ({b.nnz} occurrences, {n * (n - 1) // 2} pairs per example), Zipf({a.alpha}) "
             f"over {a.slots} slots; {a.repeats} event-timed calls per kernel after {a.warmup} warm-up calls, the two "
             "tables alternating in one process; ms, median (min); floors: the row gathers at 6.4 TB/s, the pair "
             "flops at 157.3 TFLOP/s",
             f"{'table':>10} {'pairs':>16} {'explain':>16} {'torch':>16} {'pairs/explain':>14} {'torch/pairs':>12} "
             f"{'gather floor':>13} {'flop floor':>11}"]
    for name, _, ms, floors in cases:
        med = {k: statistics.median(v) for k, v in ms.items()}
        cell = {k: f"{med[k]:.3f} ({min(v):.3f})" for k, v in ms.items()}
        lines.append(f"{name:>10} {cell['pairs']:>16} {cell['explain']:>16} {cell['torch']:>16} "
                     f"{med['pairs'] / med['explain']:>14.2f} {med['torch'] / med['pairs']:>12.2f} "
                     f"{floors[0]:>13.3f} {floors[1]:>11.3f}")
    if a.note and os.path.exists(a.note):
        with open(a.note) as f:
            lines += ["", f.read().rstrip("\n")]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
