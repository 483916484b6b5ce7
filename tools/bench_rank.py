"""Cost of the ranking metrics on the GPU: ``K.rank_metrics`` (hip/rank_metrics.hip) against ``K.gauc``
(hip/gauc.hip) on the same scores, labels and group ids -- the yardstick: the ranking chain runs the grouped
chain's two sorts twice (once on the scores, once on the gains for the ideal order), so roughly twice its cost is
what to expect.

Per size (2^17, 2^20 and 2^24 scores by default) with a Zipf group-size mix (n / 8 groups, sizes ~ 1 / rank: one
group of a large share of the examples beside a long tail of tiny ones) and cutoffs 1, 5, 10, 100: warm-up calls,
then ``--repeats`` rounds that time one ``K.gauc`` call and one ``K.rank_metrics`` call each, alternating, with
device events around the call and a reused workspace; medians.  The counts at the smallest size must equal the
CPU twin's and the values agree with it to 1e-10.  After the timings the largest size is profiled once
(torch.profiler, device activity only, outside the timed rounds) to say where the time goes.
A record, not a gate: writes the table to ``--out``.

    python tools/bench_rank.py [--sizes 131072,1048576,16777216] [--repeats 20] [--out profiles/rank/rank.txt]
"""

from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_gauc import make_groups, timed_pair  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402

CUTOFFS = (1, 5, 10, 100)


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
        own = "rank_" in name or "auc_" in name
        kind = ("sort" if "os_" in name or "rs_" in name else
                name.split("<")[0].split("(")[0].split("::")[-1] if own else "other")
        buckets[kind] = buckets.get(kind, 0.0) + t
    total = sum(buckets.values()) or 1.0
    parts = ", ".join(f"{k} {100 * v / total:.0f}%" for k, v in sorted(buckets.items(), key=lambda kv: -kv[1]))
    return f"{total / calls / 1000.0:.3f} ms of kernels per call: {parts}"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{2**17},{2**20},{2**24}")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank", "rank.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_rank: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    sizes = [int(x) for x in a.sizes.split(",")]
    lines = [f"K.rank_metrics (cutoffs {','.join(map(str, CUTOFFS))}) vs K.gauc (unweighted) on the same inputs, "
             f"{torch.cuda.get_device_name(dev)}; zipf group sizes; medians of {a.repeats} alternating event-timed "
             f"calls with a reused workspace after {a.warmup} warm-up calls; ms per call",
             f"{'n':>10} {'groups':>9} {'largest':>9} {'K.gauc':>9} {'K.rank':>9} {'rank/gauc':>10}"]
    shares = []
    for n in sizes:
        g = torch.Generator(device="cpu").manual_seed(n)
        s = torch.randn(n, generator=g).to(dev)   # logit-like continuous scores
        y = (torch.rand(n, generator=g) < 0.25).float().to(dev)
        ids_h, G = make_groups("zipf", n, g)
        ids = ids_h.to(dev)
        gws, rws = K.gauc_workspace(n, G, dev), K.rank_metrics_workspace(n, G, dev)
        if n == min(sizes):  # the timed code computes what the CPU twin computes
            got = K.rank_metrics(s, y, ids, G, CUTOFFS, ws=rws)
            ref = K.rank_metrics(s.cpu(), y.cpu(), ids_h, G, CUTOFFS)
            assert got.stats()[1:] == ref.stats()[1:]
            assert torch.allclose(got.per_group().cpu(), ref.per_group(), rtol=1e-10, atol=0)
        t_g, t_r = timed_pair(lambda: K.gauc(s, y, ids, G, ws=gws),
                              lambda: K.rank_metrics(s, y, ids, G, CUTOFFS, ws=rws), a.warmup, a.repeats)
        largest = int(torch.bincount(ids_h.long()).max())
        lines.append(f"{n:>10} {G:>9} {largest:>9} {t_g:>9.3f} {t_r:>9.3f} {t_r / t_g:>10.2f}")
        if n == max(sizes):
            shares.append(f"n={n}, K.rank_metrics: "
                          + kernel_shares(lambda: K.rank_metrics(s, y, ids, G, CUTOFFS, ws=rws)))
            shares.append(f"n={n}, K.gauc:         " + kernel_shares(lambda: K.gauc(s, y, ids, G, ws=gws)))
    notes = ["",
             "not tried: one sort of (group, score) pairs shared by both orders; an ideal order from a counting sort",
             "of the gains when the labels take few values; cutting the binary searches for runs below every cutoff;",
             "fusing the tile and run kernels; one cutoff instead of four."]
    text = "\n".join(lines + ["", "where the time goes (device time by kernel, one profiled run of 5 calls):"]
                     + shares + notes) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
