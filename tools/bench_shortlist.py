"""Cost of ranking and placing every context among its own shortlist on the GPU (hip/fm_shortlist.hip):
``K.fm_topk(k = 10, shortlist=)`` and ``K.fm_place(shortlist=)`` on equal-length lists spread over the catalogue, next
to

  * the torch line on the same lists, ``torch.topk(qb[:, None] + cb[idx] + (C[idx] @ Q[:, :, None]).squeeze(-1), k)``;
  * plain ``K.fm_topk`` / ``K.fm_place`` over the whole catalogue (per nq: the list length at which a full ranking
    becomes the cheaper call);
  * the gather floor: ``nnz x (4 Kp + 8)`` bytes at the random 256-byte-row rate of profiles/r3/roofline.txt.

Contexts {1, 64, 1024, 16384} x list lengths {100, 1000, 10000} (combinations above 2^24 entries are skipped), nc = 2^20
candidates, Kp = 64, fp32 normal profiles, reused workspaces.  After warm-up calls every repeat times all methods of
every size in turn (alternating) with device events; medians, minima and maxima.  The plain calls of 16384 contexts
take ``--slow-repeats`` calls.  The record also states whether the new op and the torch line picked the same
candidates (rows that differ are near-ties of two differently rounded sums and are listed).

A record, except for one line: at 1024 contexts x 1000 entries the new ``fm_topk`` median must lie below the torch
line's by more than the two spreads (max - min of each side's calls) together; the tool exits 1 if it does not.

    python tools/bench_shortlist.py [--nc 1048576] [--kp 64] [--repeats 30] [--out profiles/topk/shortlist.txt]
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
ROW_RATE = 6.4e12   # bytes / s, uniformly random 256-byte rows (profiles/r3/roofline.txt)
GATE = (1024, 1000)


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def cell(ms: list) -> str:
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024, 16384])
    ap.add_argument("--len", type=int, nargs="+", default=[100, 1000, 10000])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--slow-repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "shortlist.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_shortlist: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(a.nc, a.kp, generator=g, device=dev)
    cb = torch.randn(a.nc, generator=g, device=dev)
    cases, same = [], []
    for nq in a.nq:
        Q = torch.randn(nq, a.kp, generator=g, device=dev)
        qb = torch.randn(nq, generator=g, device=dev)
        t = torch.randint(0, a.nc, (nq,), generator=g, device=dev, dtype=torch.int32)
        idx = torch.empty((nq, TOPK_K), dtype=torch.int32, device=dev)
        score = torch.empty((nq, TOPK_K), dtype=torch.float32, device=dev)
        counts = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        wt, wp = K.topk_workspace(nq, a.nc, TOPK_K, dev), K.place_workspace(nq, a.nc, 1, dev)
        fns = {
            ("plain", "fm_topk"): lambda Q=Q, qb=qb, wt=wt, idx=idx, score=score: K.fm_topk(
                Q, qb, C, cb, TOPK_K, idx=idx, score=score, ws=wt),
            ("plain", "fm_place"): lambda Q=Q, qb=qb, t=t, wp=wp, counts=counts: K.fm_place(
                Q, qb, C, cb, t, (TOPK_K,), counts=counts, ws=wp),
        }
        for n in a.len:
            if nq * n > 1 << 24:
                continue
            # one random candidate out of each of n equal strata of the catalogue: ascending, distinct, spread out
            step = a.nc // n
            rows = torch.randint(0, step, (nq, n), generator=g, device=dev) + torch.arange(n, device=dev) * step
            sl = ((torch.arange(nq + 1, device=dev) * n).to(torch.int32), rows.to(torch.int32).reshape(-1))
            ws = K.shortlist_workspace(nq, nq * n, a.nc, TOPK_K, dev)
            line = lambda Q=Q, qb=qb, rows=rows: torch.topk(
                qb[:, None] + cb[rows] + (C[rows] @ Q[:, :, None]).squeeze(-1), TOPK_K)
            fns[n, "fm_topk"] = lambda Q=Q, qb=qb, sl=sl, ws=ws, idx=idx, score=score: K.fm_topk(
                Q, qb, C, cb, TOPK_K, idx=idx, score=score, ws=ws, shortlist=sl)
            fns[n, "torch"] = line
            fns[n, "fm_place"] = lambda Q=Q, qb=qb, t=t, sl=sl, ws=ws, counts=counts: K.fm_place(
                Q, qb, C, cb, t, (TOPK_K,), counts=counts, ws=ws, shortlist=sl)
            # the same candidates?  (the torch line's places are positions in the list)
            got = fns[n, "fm_topk"]()[0].long().sort(1).values
            want = rows.gather(1, line().indices).sort(1).values
            bad = (got != want).any(1).nonzero().flatten().tolist()
            same.append((nq, n, bad))
        cases.append((nq, fns, {m: [] for m in fns}))
    for _, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
    torch.cuda.synchronize()
    for rep in range(a.repeats):
        for nq, fns, ms in cases:
            for m, fn in fns.items():
                if m[0] != "plain" or nq < 16384 or rep < a.slow_repeats:
                    ms[m].append(event_ms(fn))
    lines = [f"fm_topk(k = {TOPK_K}) and fm_place with per-context shortlists (hip/fm_shortlist.hip), "
             f"{torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, one cutoff, fp32 normal profiles, equal-length lists (one random "
             f"candidate per stratum of the catalogue), reused workspaces; {a.repeats} event-timed calls per method "
             f"({a.slow_repeats} for the plain calls of 16384 contexts) after {a.warmup} warm-up calls, methods and "
             "sizes alternating in one process; ms, median (min .. max); parts: shortlist_plan; floor: nnz x (4 Kp + 8)"
             f" bytes at {ROW_RATE / 1e12:.1f} TB/s (random 256-byte rows, profiles/r3/roofline.txt)",
             f"{'nq':>6} {'len':>6} {'parts':>5} {'fm_topk(shortlist=)':>26} {'torch line':>26} "
             f"{'fm_place(shortlist=)':>26} {'floor':>7} {'torch / fm_topk':>15}"]
    verdict = None
    for nq, _, ms in cases:
        for n in a.len:
            if (n, "fm_topk") not in ms:
                continue
            ours, line = ms[n, "fm_topk"], ms[n, "torch"]
            floor = nq * n * (4 * a.kp + 8) / ROW_RATE * 1e3
            lines.append(f"{nq:>6} {n:>6} {K.shortlist_plan(nq, nq * n, a.nc):>5} {cell(ours):>26} {cell(line):>26} "
                         f"{cell(ms[n, 'fm_place']):>26} {floor:>7.3f} "
                         f"{statistics.median(line) / statistics.median(ours):>15.2f}")
            if (nq, n) == GATE:
                gap = statistics.median(line) - statistics.median(ours)
                spread = (max(ours) - min(ours)) + (max(line) - min(line))
                verdict = (gap > spread, f"condition at {nq} x {n}: torch median - fm_topk median = {gap:.3f} ms, the "
                           f"two spreads together {spread:.3f} ms: {'met' if gap > spread else 'NOT MET'}")
        lines.append(f"{nq:>6} {'all':>6} {'':>5} {cell(ms['plain', 'fm_topk']):>26} {'':>26} "
                     f"{cell(ms['plain', 'fm_place']):>26}   (plain fm_topk / fm_place over the catalogue)")
    lines.append("same candidates as the torch line (sets of the k places per context): " + "; ".join(
        f"{nq} x {n}: " + ("all" if not bad else f"rows {bad[:8]} of {len(bad)} differ") for nq, n, bad in same))
    if verdict:
        lines.append(verdict[1])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if verdict is None or verdict[0] else 1


if __name__ == "__main__":
    sys.exit(main())
