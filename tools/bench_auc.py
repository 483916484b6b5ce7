"""Validation AUC on the GPU: ``K.auc`` (hip/auc.hip) against the same statistics from torch ops on the same
device -- ``torch.sort`` + ``cumsum`` + ``searchsorted``, what a user had to write before ``K.auc``.

Per size (2^20 and 2^23 scores by default) and mode (unweighted, weighted): warm-up calls, then every repeat
timed with device events around the whole call (the torch version's host syncs included: both times are
"until the statistics are on the device"), median over the repeats.  The unweighted statistics of the two
must be equal.  A record, not a gate: writes the table to ``--out``.

    python tools/bench_auc.py [--sizes 1048576,8388608] [--repeats 20] [--out profiles/auc/bench_auc.txt]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fast_tffm_amd.ops import kernels as K  # noqa: E402


def torch_stats(s: torch.Tensor, y: torch.Tensor, w: torch.Tensor | None) -> torch.Tensor:
    """[U2, P, N] with torch ops (torch.sort orders -0.0 == +0.0 and keeps denormals, like K.auc)."""
    ss, order = torch.sort(s, stable=True)
    pos = y[order] > 0
    wo = torch.ones_like(order) if w is None else w[order].double()
    wneg = torch.where(pos, torch.zeros_like(wo), wo)
    nex = torch.cat([wneg.new_zeros(1), torch.cumsum(wneg, 0)])
    sp = ss[pos]
    lb, ub = torch.searchsorted(ss, sp, right=False), torch.searchsorted(ss, sp, right=True)
    return torch.stack([(wo[pos] * (nex[lb] + nex[ub])).sum(), wo[pos].sum(), wneg.sum()])


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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=f"{2**20},{2**23}")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "auc", "bench_auc.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_auc: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    lines = [f"K.auc vs torch.sort + cumsum + searchsorted, {torch.cuda.get_device_name(dev)}; median of "
             f"{a.repeats} event-timed calls after {a.warmup} warm-up calls; ms per call",
             f"{'n':>10} {'mode':>10} {'K.auc':>10} {'torch':>10} {'torch/K.auc':>12}"]
    for n in (int(x) for x in a.sizes.split(",")):
        g = torch.Generator(device="cpu").manual_seed(n)
        s = torch.randn(n, generator=g).to(dev)   # logit-like continuous scores
        y = (torch.rand(n, generator=g) < 0.25).float().to(dev)
        wr = (torch.rand(n, generator=g) + 0.01).to(dev)
        ws = K.auc_workspace(n, dev)
        for mode, w in (("unweighted", None), ("weighted", wr)):
            got = K.auc(s, y, w, ws=ws).stats()[:3]
            ref = torch_stats(s, y, w).tolist()
            if w is None:
                assert list(got) == ref, (got, ref)
            else:
                assert all(abs(g_ - r) <= 4 * n * 2.0 ** -53 * r for g_, r in zip(got, ref)), (got, ref)
            t_k = timed(lambda: K.auc(s, y, w, ws=ws), a.warmup, a.repeats)
            t_t = timed(lambda: torch_stats(s, y, w), a.warmup, a.repeats)
            lines.append(f"{n:>10} {mode:>10} {t_k:>10.3f} {t_t:>10.3f} {t_t / t_k:>12.2f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
