"""Cost of leaving out every context's already-seen candidates on the GPU (hip/fm_seen.hip): ``K.fm_topk(k = 10)``
and ``K.fm_place`` without lists -- the plain kernels, the numbers to hold against the parent commit's -- next to
the same calls with 100 seen candidates per context spread over the catalogue, with the context's own top 100 seen
(every one of them beats the thresholds and pays a membership search), and with 90% of the catalogue seen (the
degenerate case: the thresholds stay low, so most candidates pay a search; place scores every listed candidate).

nq in {1, 64, 1024} contexts against nc = 2^20 candidates, Kp = 64, fp32 normal profiles, reused workspaces.  After
warm-up calls every repeat times all methods of every nq in turn (alternating) with device events; medians and
minima.  The 90% rows take ``--slow-repeats`` calls.  A record, not a gate: writes the table to ``--out``.

    python tools/bench_seen.py [--nc 1048576] [--kp 64] [--repeats 30] [--out profiles/topk/seen.txt]
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

TOPK_K = 10
LISTS = ("none", "100 uniform", "own top 100", "90%")


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def csr(rows: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """The seen pair of ``rows`` [nq, n]: every context's n ascending candidates."""
    nq, n = rows.shape
    off = torch.arange(nq + 1, device=rows.device, dtype=torch.int64) * n
    return off.to(torch.int32), rows.to(torch.int32).reshape(-1).contiguous()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--slow-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "seen.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_seen: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(a.nc, a.kp, generator=g, device=dev)
    cb = torch.randn(a.nc, generator=g, device=dev)
    cand = torch.arange(a.nc, device=dev)
    most = cand[cand % 10 != 9]
    cases = []
    for nq in a.nq:
        Q = torch.randn(nq, a.kp, generator=g, device=dev)
        qb = torch.randn(nq, generator=g, device=dev)
        t = torch.randint(0, a.nc, (nq,), generator=g, device=dev, dtype=torch.int32)
        step = a.nc // 100
        seen = {
            "none": None,
            "100 uniform": csr(torch.randint(0, step, (nq, 1), generator=g, device=dev) + cand[:100] * step),
            "own top 100": csr(K.fm_topk(Q, qb, C, cb, 100)[0].long().sort(1).values),
            "90%": csr(most.expand(nq, -1)),
        }
        wp, wt = K.place_workspace(nq, a.nc, 1, dev), K.topk_workspace(nq, a.nc, TOPK_K, dev)
        counts = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        idx = torch.empty((nq, TOPK_K), dtype=torch.int32, device=dev)
        score = torch.empty((nq, TOPK_K), dtype=torch.float32, device=dev)
        fns = {}
        for name, s in seen.items():
            fns["fm_topk", name] = lambda Q=Q, qb=qb, s=s, wt=wt, idx=idx, score=score: K.fm_topk(
                Q, qb, C, cb, TOPK_K, idx=idx, score=score, ws=wt, seen=s)
            fns["fm_place", name] = lambda Q=Q, qb=qb, t=t, s=s, wp=wp, counts=counts: K.fm_place(
                Q, qb, C, cb, t, (TOPK_K,), counts=counts, ws=wp, seen=s)
        cases.append((nq, fns, {n: [] for n in fns}))
    for _, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
    torch.cuda.synchronize()
    for rep in range(a.repeats):
        for _, fns, ms in cases:
            for n, fn in fns.items():
                if n[1] != "90%" or rep < a.slow_repeats:
                    ms[n].append(event_ms(fn))
    lines = [f"fm_topk(k = {TOPK_K}) and fm_place with per-context seen lists (hip/fm_seen.hip), "
             f"{torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, one cutoff, fp32 normal profiles, reused workspaces; {a.repeats} "
             f"event-timed calls per method ({a.slow_repeats} for the 90% lists) after {a.warmup} warm-up calls, "
             "methods and sizes alternating in one process; ms, median (min); `none` launches the plain kernels",
             f"{'op':>9} {'nq':>6} " + " ".join(f"{n:>20}" for n in LISTS) + f" {'100 uniform / none':>19} "
             f"{'own top 100 / none':>19}"]
    for nq, _, ms in cases:
        for op in ("fm_topk", "fm_place"):
            med = {n: statistics.median(ms[op, n]) for n in LISTS}
            cells = " ".join(f"{f'{med[n]:.3f} ({min(ms[op, n]):.3f})':>20}" for n in LISTS)
            lines.append(f"{op:>9} {nq:>6} {cells} {med['100 uniform'] / med['none']:>19.3f} "
                         f"{med['own top 100'] / med['none']:>19.3f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
