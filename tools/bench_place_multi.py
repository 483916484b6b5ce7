"""Cost of placing several held-out targets per context among a whole catalogue on the GPU: ``K.fm_place`` with a
target pair (hip/fm_place_multi.hip: every score once, placed among the context's sorted target scores) next to the
only other way to the same counts -- ``K.fm_place`` on the contexts repeated once per target -- and next to the two
floors of tools/bench_place.py: the candidate profiles read once from HBM (nc Kp 4 bytes at 6.29 TB/s measured
streaming) and one product per (context, candidate) on the fp32 matrix cores (2 nq nc Kp flops at 157.3 TF).

nq in {1, 64, 1024} contexts x {1, 10, 100} targets each against nc = 2^20 candidates, Kp = 64, fp32 normal profiles,
uniformly drawn targets, reused workspaces.  After warm-up calls every repeat times both methods of every case in turn
(alternating) with device events; medians, minima and spreads (max - min).  The counts of the two methods are compared
at every case.  The share of scores that took the slow path (reached their row's smallest threshold) is read from the
counts: per row, greater + equal of its lowest-scoring entry.  Uniform targets are the pessimistic input -- the lowest
of T uniform places lies near the bottom of the catalogue -- so one more line times 1024 x 10 with every context's
targets drawn from its own 128 best candidates, as a trained model's would mostly be.  A record, not a gate: writes the
table to ``--out``.

    python tools/bench_place_multi.py [--nc 1048576] [--kp 64] [--repeats 30] [--out profiles/topk/place_multi.txt]
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

HBM_BYTES_PER_S = 6.29e12     # measured float4 copy
MATRIX_FP32_FLOPS = 157.3e12  # fp32-input MFMA peak


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def slow_share(counts: torch.Tensor, nq: int, T: int, nc: int) -> float:
    """Scores that reached their row's smallest threshold, over all scores of all rows."""
    seg = K.PLACE_SEGMENT
    reach = counts.long().sum(1).view(nq, T)
    rows = [reach[:, s:s + seg].max(1).values for s in range(0, T, seg)]
    return float(torch.stack(rows).double().mean()) / nc


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--targets", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "place_multi.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_place_multi: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(a.nc, a.kp, generator=g, device=dev)
    cb = torch.randn(a.nc, generator=g, device=dev)
    cases = []

    def add_case(name, nq, T, Q, qb, idx):
        """idx [nq, T]: every context's distinct targets, ascending."""
        off = torch.arange(0, nq * T + 1, T, dtype=torch.int32, device=dev)
        flat = idx.reshape(-1).to(torch.int32).contiguous()
        Qx, qbx = Q.repeat_interleave(T, 0).contiguous(), qb.repeat_interleave(T).contiguous()
        wm = K.place_workspace(nq, a.nc, 1, dev, entries=nq * T)
        wx = K.place_workspace(nq * T, a.nc, 1, dev)
        cm = torch.empty((nq * T, 2), dtype=torch.int32, device=dev)
        cx = torch.empty((nq * T, 2), dtype=torch.int32, device=dev)
        fns = {"multi": lambda: K.fm_place(Q, qb, C, cb, (off, flat), (10,), counts=cm, ws=wm),
               "expanded": lambda: K.fm_place(Qx, qbx, C, cb, flat, (10,), counts=cx, ws=wx)}
        cases.append((name, nq, T, fns, {n: [] for n in fns}))

    for nq in a.nq:
        Q = torch.randn(nq, a.kp, generator=g, device=dev)
        qb = torch.randn(nq, generator=g, device=dev)
        for T in a.targets:
            idx = torch.rand(nq, a.nc, generator=g, device=dev).topk(T, dim=1).indices.sort(1).values \
                if nq * a.nc <= 1 << 26 else \
                torch.stack([torch.randperm(a.nc, generator=g, device=dev)[:T].sort().values for _ in range(nq)])
            add_case("uniform", nq, T, Q, qb, idx)
    nq, T = a.nq[-1], 10
    best = K.fm_topk(Q, qb, C, cb, 128)[0].long()   # (Q, qb: the last nq's)
    pick = torch.rand(nq, 128, generator=g, device=dev).topk(T, dim=1).indices
    add_case("own top 128", nq, T, Q, qb, best.gather(1, pick).sort(1).values)

    info = []
    for _, nq, T, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        cm, cx = fns["multi"]().counts(), fns["expanded"]().counts()
        info.append((int((cm == cx).all(1).sum()), slow_share(cm, nq, T, a.nc)))
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for *_, fns, ms in cases:
            for n, fn in fns.items():
                ms[n].append(event_ms(fn))
    floor_hbm = a.nc * a.kp * 4 / HBM_BYTES_PER_S * 1e3
    lines = [f"fm_place with a target pair (multi) vs fm_place on the contexts repeated once per target (expanded), "
             f"{torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, one cutoff, fp32 normal profiles, reused workspaces; {a.repeats} "
             f"event-timed calls per method after {a.warmup} warm-up calls, methods and cases alternating in one "
             "process; ms, median (min) [max - min]",
             f"floors: HBM = nc Kp 4 B at {HBM_BYTES_PER_S / 1e12:.2f} TB/s = {floor_hbm:.4f} ms; matrix = 2 nq nc Kp "
             f"flops at {MATRIX_FP32_FLOPS / 1e12:.1f} TF (one product per context and candidate)",
             f"{'targets':>12} {'nq':>6} {'T':>4} {'rows':>6} {'multi':>26} {'expanded':>28} {'exp/multi':>10} "
             f"{'gap > spreads':>14} {'matrix floor':>13} {'multi/HBM':>10} {'multi/matrix':>13} {'same counts':>14} "
             f"{'slow path':>10}"]
    for (name, nq, T, _, ms), (same, share) in zip(cases, info):
        med = {n: statistics.median(v) for n, v in ms.items()}
        spread = {n: max(v) - min(v) for n, v in ms.items()}
        cell = {n: f"{med[n]:.3f} ({min(v):.3f}) [{spread[n]:.3f}]" for n, v in ms.items()}
        floor_mx = 2.0 * nq * a.nc * a.kp / MATRIX_FP32_FLOPS * 1e3
        faster = med["expanded"] - med["multi"] > spread["multi"] + spread["expanded"]
        lines.append(f"{name:>12} {nq:>6} {T:>4} {nq * -(-T // K.PLACE_SEGMENT):>6} {cell['multi']:>26} "
                     f"{cell['expanded']:>28} {med['expanded'] / med['multi']:>10.2f} {str(faster):>14} "
                     f"{floor_mx:>13.4f} {med['multi'] / floor_hbm:>10.1f} {med['multi'] / floor_mx:>13.1f} "
                     f"{same:>8}/{nq * T:<5} {share:>10.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
