"""Cost of placing a held-out candidate among a whole catalogue on the GPU: ``K.fm_place`` (hip/fm_place.hip) next
to ``K.fm_topk(k = 10)`` of the same tree -- the same exact-fp32 product followed by a selection instead of two
counters -- next to the torch line ``((qb[:, None] + cb[None, :] + Q @ C.T) > s_t).sum(1)``, which writes the
[nq, nc] score matrix, and next to the two floors of tools/bench_topk.py: the candidate profiles read once from HBM
(nc Kp 4 bytes at 6.29 TB/s measured streaming) and the products on the fp32 matrix cores (2 nq nc Kp flops at
157.3 TF).

nq in {1, 64, 1024} queries against nc = 2^20 candidates, Kp = 64, fp32 normal profiles, reused workspaces.  After
warm-up calls every repeat times the three methods of every nq in turn (alternating) with device events; medians
and minima.  ``greater`` is compared with the torch line at every size (equal unless the matrix product's rounding
moves a near-tie across s_t; the rows that differ are counted).  A record, not a gate: writes the table to ``--out``.

    python tools/bench_place.py [--nc 1048576] [--kp 64] [--repeats 30] [--out profiles/topk/place.txt]
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
TOPK_K = 10


def event_ms(fn) -> float:
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "place.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_place: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(a.nc, a.kp, generator=g, device=dev)
    cb = torch.randn(a.nc, generator=g, device=dev)
    cases = []
    for nq in a.nq:
        Q = torch.randn(nq, a.kp, generator=g, device=dev)
        qb = torch.randn(nq, generator=g, device=dev)
        t = torch.randint(0, a.nc, (nq,), generator=g, device=dev, dtype=torch.int32)
        tl = t.long()
        wp, wt = K.place_workspace(nq, a.nc, 1, dev), K.topk_workspace(nq, a.nc, TOPK_K, dev)
        counts = torch.empty((nq, 2), dtype=torch.int32, device=dev)
        idx = torch.empty((nq, TOPK_K), dtype=torch.int32, device=dev)
        score = torch.empty((nq, TOPK_K), dtype=torch.float32, device=dev)

        def torch_line(Q=Q, qb=qb, tl=tl):
            s = qb[:, None] + cb[None, :] + Q @ C.T
            return (s > s.gather(1, tl[:, None])).sum(1)

        fns = {
            "fm_place": lambda Q=Q, qb=qb, t=t, wp=wp, counts=counts: K.fm_place(Q, qb, C, cb, t, (TOPK_K,),
                                                                                 counts=counts, ws=wp),
            "fm_topk": lambda Q=Q, qb=qb, wt=wt, idx=idx, score=score: K.fm_topk(Q, qb, C, cb, TOPK_K, idx=idx,
                                                                                  score=score, ws=wt),
            "torch": torch_line,
        }
        cases.append((nq, fns, {n: [] for n in fns}))
    agree = {}
    for nq, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        mine, ref = fns["fm_place"]().counts(), fns["torch"]()
        agree[nq] = (int((mine[:, 0].long() == ref).sum()), int((mine[:, 1] < 1).sum()))
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, fns, ms in cases:
            for n, fn in fns.items():
                ms[n].append(event_ms(fn))
    floor_hbm = a.nc * a.kp * 4 / HBM_BYTES_PER_S * 1e3
    lines = [f"fm_place vs fm_topk(k = {TOPK_K}) vs the torch comparison over the materialised score matrix, "
             f"{torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, one cutoff, fp32 normal profiles, reused workspaces; {a.repeats} "
             f"event-timed calls per method after {a.warmup} warm-up calls, methods and sizes alternating in one "
             "process; ms, median (min)",
             f"floors: HBM = nc Kp 4 B at {HBM_BYTES_PER_S / 1e12:.2f} TB/s = {floor_hbm:.4f} ms; matrix = 2 nq nc Kp "
             f"flops at {MATRIX_FP32_FLOPS / 1e12:.1f} TF",
             f"{'nq':>6} {'slab':>8} {'parts':>6} {'fm_place':>18} {'fm_topk':>18} {'torch':>18} {'topk/place':>11} "
             f"{'torch/place':>12} {'matrix floor':>13} {'place/HBM':>10} {'place/matrix':>13} {'same greater':>13} "
             f"{'equal < 1':>10}"]
    for nq, _, ms in cases:
        med = {n: statistics.median(v) for n, v in ms.items()}
        cell = {n: f"{med[n]:.3f} ({min(v):.3f})" for n, v in ms.items()}
        floor_mx = 2.0 * nq * a.nc * a.kp / MATRIX_FP32_FLOPS * 1e3
        slab, parts = K.place_plan(nq, a.nc)
        lines.append(f"{nq:>6} {slab:>8} {parts:>6} {cell['fm_place']:>18} {cell['fm_topk']:>18} {cell['torch']:>18} "
                     f"{med['fm_topk'] / med['fm_place']:>11.2f} {med['torch'] / med['fm_place']:>12.2f} "
                     f"{floor_mx:>13.4f} {med['fm_place'] / floor_hbm:>10.1f} {med['fm_place'] / floor_mx:>13.1f} "
                     f"{agree[nq][0]:>8}/{nq:<4} {agree[nq][1]:>10}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
