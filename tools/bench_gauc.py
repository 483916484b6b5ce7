"""Cost of the grouped AUC on the GPU: ``K.gauc`` (hip/gauc.hip) against ``K.auc`` (hip/auc.hip) on the same
scores -- the yardstick: most of either chain is the radix sort, and the grouped chain adds a second, shorter
sort pass by group id and the segmented steps.

Per size (2^20 and 2^24 scores by default), group layout and mode (unweighted, weighted): warm-up calls, then
``--repeats`` rounds that time one ``K.auc`` call and one ``K.gauc`` call each, alternating, with device events
around the call; medians.  Layouts: ``uniform8`` (n / 8 groups of exactly 8, dealt to random positions),
``zipf`` (n / 8 groups, sizes ~ 1 / rank), ``one90`` (one group with 90% of the examples beside groups of
~8).  The unweighted per-group records at the smallest size must equal the CPU twin's.  After the timings the
largest size is profiled once per layout (torch.profiler, device activity only, outside the timed rounds) to
say where the time goes: the share of the sort kernels, of the chain's own kernels and of the memsets.
A record, not a gate: writes the table to ``--out``.

    python tools/bench_gauc.py [--sizes 1048576,16777216] [--repeats 20] [--out profiles/gauc/gauc.txt]
"""

from __future__ import annotations

import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fast_tffm_amd.ops import kernels as K  # noqa: E402

LAYOUTS = ("uniform8", "zipf", "one90")


def make_groups(layout: str, n: int, g: torch.Generator) -> tuple[torch.Tensor, int]:
    """(int32 ids, number of groups) of a layout, on the host."""
    if layout == "uniform8":
        G = (n + 7) // 8
        return (torch.randperm(n, generator=g) // 8).to(torch.int32), G
    if layout == "zipf":  # log-uniform ranks: P(group k) ~ 1 / (k + 1)
        G = max(n // 8, 1)
        ids = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * math.log(G + 1)).floor() - 1
        return ids.clamp_(0, G - 1).to(torch.int32), G
    G = max(n // 80, 1) + 1  # one90: group 0 holds 9 of 10, the others ~8 each
    ids = torch.randint(1, G, (n,), generator=g)
    ids[torch.rand(n, generator=g) < 0.9] = 0
    return ids.to(torch.int32), G


def timed_pair(fa, fb, warmup: int, repeats: int) -> tuple[float, float]:
    """Median milliseconds of fa() and of fb(), one call of each per round, between device events."""
    for _ in range(warmup):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(repeats):
        for k, fn in enumerate((fa, fb)):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            ms[k].append(t0.elapsed_time(t1))
    return statistics.median(ms[0]), statistics.median(ms[1])


def kernel_shares(fn, calls: int = 5) -> str:
    """Where the device time of fn() goes: sort kernels / the chain's own kernels / memsets and the rest."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    buckets: dict[str, float] = {}
    for ev in prof.key_averages():
        t = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0))
        if t <= 0:
            continue
        name = ev.key
        kind = ("sort" if "os_" in name or "rs_" in name else
                name.split("<")[0].split("(")[0].split("::")[-1] if "auc_" in name or "prefix_" in name else "other")
        buckets[kind] = buckets.get(kind, 0.0) + t
    total = sum(buckets.values()) or 1.0
    per_call = total / calls / 1000.0
    parts = ", ".join(f"{k} {100 * v / total:.0f}%" for k, v in sorted(buckets.items(), key=lambda kv: -kv[1]))
    return f"{per_call:.3f} ms of kernels per call: {parts}"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{2**20},{2**24}")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gauc", "gauc.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_gauc: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    sizes = [int(x) for x in a.sizes.split(",")]
    lines = [f"K.gauc vs K.auc on the same scores, {torch.cuda.get_device_name(dev)}; medians of {a.repeats} "
             f"alternating event-timed calls after {a.warmup} warm-up calls; ms per call",
             f"{'n':>10} {'layout':>9} {'groups':>9} {'mode':>10} {'K.auc':>9} {'K.gauc':>9} {'gauc/auc':>9}"]
    shares = []
    for n in sizes:
        g = torch.Generator(device="cpu").manual_seed(n)
        s = torch.randn(n, generator=g).to(dev)   # logit-like continuous scores
        y = (torch.rand(n, generator=g) < 0.25).float().to(dev)
        wr = (torch.rand(n, generator=g) + 0.01).to(dev)
        aws = K.auc_workspace(n, dev)
        for layout in LAYOUTS:
            ids_h, G = make_groups(layout, n, g)
            ids = ids_h.to(dev)
            gws = K.gauc_workspace(n, G, dev)
            if n == min(sizes):  # the timed code computes what the CPU twin computes
                got = K.gauc(s, y, ids, G, ws=gws)
                ref = K.gauc(s.cpu(), y.cpu(), ids_h, G)
                assert torch.equal(got.per_group().cpu(), ref.per_group()), layout
                assert got.stats()[1:] == ref.stats()[1:], layout
            for mode, w in (("unweighted", None), ("weighted", wr)):
                t_a, t_g = timed_pair(lambda: K.auc(s, y, w, ws=aws), lambda: K.gauc(s, y, ids, G, w, ws=gws),
                                      a.warmup, a.repeats)
                lines.append(f"{n:>10} {layout:>9} {G:>9} {mode:>10} {t_a:>9.3f} {t_g:>9.3f} {t_g / t_a:>9.2f}")
            if n == max(sizes):
                shares.append(f"{layout:>9} n={n} weighted, K.gauc: "
                              + kernel_shares(lambda: K.gauc(s, y, ids, G, wr, ws=gws)))
        if n == max(sizes):
            shares.append(f"{'':>9} n={n} weighted, K.auc:  " + kernel_shares(lambda: K.auc(s, y, wr, ws=aws)))
    text = "\n".join(lines + ["", "where the time goes (device time by kernel, one profiled run of 5 calls):"]
                     + shares) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
