"""Cost of diversified recommendations on the GPU (hip/fm_diversify.hip): ``K.fm_diversify(n = 10, lam = 0.5)`` on
pools ``K.fm_topk`` retrieved, next to

  * the torch alternative on the same pools: gather ``C[idx]``, scale the rows, ``bmm`` for the pool's similarity
    matrix, then a Python loop of ``n`` masked arg-max steps (no host read);
  * the serving path ``fm_topk(k = M)`` + ``fm_diversify`` against plain ``fm_topk(k = n)``.

Contexts {1, 64, 1024} x pools M {32, 128}, nc = 2^20 candidates, Kp = 64, fp32 normal profiles, cosine scale, reused
outputs and workspaces.  After warm-up calls every repeat times all methods of every size in turn (alternating) with
device events; medians, minima and maxima.  The record also states whether the op and the torch alternative picked the
same candidates (they round differently, so near-ties may differ; such rows are counted).

A record, except for one line: at 1024 contexts x M = 128 the ``fm_diversify`` median must lie below the torch
alternative's by more than the two spreads (max - min of each side's calls) together; the tool exits 1 if it does not.

    python tools/bench_diversify.py [--nc 1048576] [--kp 64] [--repeats 30] [--out profiles/topk/diversify.txt]
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

PICKS, LAM = 10, 0.5
GATE = (1024, 128)


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def cell(ms: list) -> str:
    return f"{statistics.median(ms):.3f} ({min(ms):.3f} .. {max(ms):.3f})"


def torch_mmr(C, inv, pidx, pscore, n, lam):
    """The alternative: one gather, one bmm, n steps of masked arg-max (pools without -1 entries)."""
    rows = pidx.long()
    P = C[rows] * inv[rows][:, :, None]
    sim = torch.bmm(P, P.transpose(1, 2))
    rel, pen = lam * pscore, torch.zeros_like(pscore)
    taken = torch.zeros_like(pscore, dtype=torch.bool)
    picks = []
    for t in range(n):
        m = (rel - (1.0 - lam) * pen).masked_fill(taken, float("-inf"))
        s = m.argmax(dim=1, keepdim=True)
        picks.append(s)
        taken.scatter_(1, s, True)
        col = sim.gather(2, s[:, :, None].expand(-1, sim.shape[1], 1)).squeeze(2)
        pen = col if t == 0 else torch.maximum(pen, col)
    return rows.gather(1, torch.cat(picks, dim=1))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--pool", type=int, nargs="+", default=[32, 128])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "diversify.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_diversify: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(a.nc, a.kp, generator=g, device=dev)
    cb = torch.randn(a.nc, generator=g, device=dev)
    inv = K.diversify_scale(C)
    cases, same = [], []
    for nq in a.nq:
        Q = torch.randn(nq, a.kp, generator=g, device=dev)
        qb = torch.randn(nq, generator=g, device=dev)
        wk = K.topk_workspace(nq, a.nc, PICKS, dev)
        fns = {("plain", "fm_topk"): lambda Q=Q, qb=qb, wk=wk: K.fm_topk(Q, qb, C, cb, PICKS, ws=wk)}
        for M in a.pool:
            wm = K.topk_workspace(nq, a.nc, M, dev)
            pidx, pscore = K.fm_topk(Q, qb, C, cb, M, ws=wm)
            out = K.fm_diversify(C, inv, pidx, pscore, PICKS, LAM)
            fns[M, "fm_diversify"] = lambda pidx=pidx, pscore=pscore, out=out: K.fm_diversify(
                C, inv, pidx, pscore, PICKS, LAM, out=out)
            fns[M, "torch"] = lambda pidx=pidx, pscore=pscore: torch_mmr(C, inv, pidx, pscore, PICKS, LAM)
            fns[M, "both"] = lambda Q=Q, qb=qb, M=M, wm=wm, pidx=pidx, pscore=pscore, out=out: K.fm_diversify(
                C, inv, *K.fm_topk(Q, qb, C, cb, M, ws=wm, idx=pidx, score=pscore), PICKS, LAM, out=out)
            bad = int((out[0].long() != fns[M, "torch"]()).any(1).sum())
            same.append((nq, M, bad))
        cases.append((nq, fns, {m: [] for m in fns}))
    for _, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, fns, ms in cases:
            for m, fn in fns.items():
                ms[m].append(event_ms(fn))
    lines = [f"fm_diversify(n = {PICKS}, lam = {LAM}) on fm_topk's pools (hip/fm_diversify.hip), "
             f"{torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, fp32 normal profiles, cosine scale, reused outputs and workspaces; "
             f"{a.repeats} event-timed calls per method after {a.warmup} warm-up calls, methods and sizes alternating "
             "in one process; ms, median (min .. max); torch: gather, bmm and a Python loop of n masked arg-max steps",
             f"{'nq':>6} {'M':>4} {'fm_diversify':>26} {'torch alternative':>26} {'fm_topk(M) + fm_diversify':>26} "
             f"{'torch / op':>10}"]
    verdict = None
    for nq, _, ms in cases:
        for M in a.pool:
            ours, alt = ms[M, "fm_diversify"], ms[M, "torch"]
            lines.append(f"{nq:>6} {M:>4} {cell(ours):>26} {cell(alt):>26} {cell(ms[M, 'both']):>26} "
                         f"{statistics.median(alt) / statistics.median(ours):>10.2f}")
            if (nq, M) == GATE:
                gap = statistics.median(alt) - statistics.median(ours)
                spread = (max(ours) - min(ours)) + (max(alt) - min(alt))
                verdict = (gap > spread, f"condition at {nq} x {M}: torch median - fm_diversify median = {gap:.3f} ms, "
                           f"the two spreads together {spread:.3f} ms: {'met' if gap > spread else 'NOT MET'}")
        lines.append(f"{nq:>6} {'-':>4} {'':>26} {'':>26} {cell(ms['plain', 'fm_topk']):>26}   (plain fm_topk(k = "
                     f"{PICKS}) over the catalogue)")
    lines.append("contexts whose picks differ from the torch alternative's (differently rounded sums): " + "; ".join(
        f"{nq} x {M}: {bad}" for nq, M, bad in same))
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
