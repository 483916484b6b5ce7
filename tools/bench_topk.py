"""Cost of ranking a catalogue on the GPU: ``K.fm_topk`` (hip/fm_topk.hip) next to the only alternative there
was before it, ``torch.topk(qb[:, None] + cb[None, :] + Q @ C.T, k)``, which writes the [nq, nc] score matrix,
and next to two floors from the hardware's documented rates: reading the candidate profiles once from HBM
(nc Kp 4 bytes at 6.29 TB/s measured streaming) and the products on the fp32 matrix cores (2 nq nc Kp flops at
157.3 TF).

nq in {1, 64, 1024} queries against nc = 2^20 candidates, Kp = 64, k = 10, fp32 normal profiles.  After warm-up
calls every repeat times the two methods of every nq in turn (alternating) with device events; medians and
minima.  The two results are compared at every size: candidates bit for bit unless the matrix product's
rounding reorders near-ties (counted).  A record, not a gate: writes the table to ``--out``.

    python tools/bench_topk.py [--nc 1048576] [--kp 64] [--k 10] [--repeats 30] [--out profiles/topk/topk.txt]
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


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--nc", type=int, default=1 << 20)
    ap.add_argument("--kp", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "topk", "topk.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_topk: needs a GPU", file=sys.stderr)
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
        ws = K.topk_workspace(nq, a.nc, a.k, dev)
        idx = torch.empty((nq, a.k), dtype=torch.int32, device=dev)
        score = torch.empty((nq, a.k), dtype=torch.float32, device=dev)
        fns = {
            "fm_topk": lambda Q=Q, qb=qb, ws=ws, idx=idx, score=score: K.fm_topk(Q, qb, C, cb, a.k, idx=idx,
                                                                                  score=score, ws=ws),
            "torch": lambda Q=Q, qb=qb: torch.topk(qb[:, None] + cb[None, :] + Q @ C.T, a.k),
        }
        cases.append((nq, fns, {n: [] for n in fns}))
    agree = {}
    for nq, fns, _ in cases:
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        mine, ref = fns["fm_topk"](), fns["torch"]()
        same = (mine[0].long() == ref[1]).all(dim=1)
        agree[nq] = (int(same.sum()), float((mine[1] - ref[0]).abs().max()))
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for _, fns, ms in cases:
            for n, fn in fns.items():
                ms[n].append(event_ms(fn))
    floor_hbm = a.nc * a.kp * 4 / HBM_BYTES_PER_S * 1e3
    lines = [f"fm_topk vs torch.topk over the materialised score matrix, {torch.cuda.get_device_name(dev)}",
             f"nc = {a.nc} candidates, Kp = {a.kp}, k = {a.k}, fp32 normal profiles; {a.repeats} event-timed calls "
             f"per method after {a.warmup} warm-up calls, methods and sizes alternating in one process; ms, median "
             "(min)",
             f"floors: HBM = nc Kp 4 B at {HBM_BYTES_PER_S / 1e12:.2f} TB/s = {floor_hbm:.4f} ms; matrix = 2 nq nc Kp "
             f"flops at {MATRIX_FP32_FLOPS / 1e12:.1f} TF",
             f"{'nq':>6} {'slab':>8} {'parts':>6} {'fm_topk':>18} {'torch':>18} {'torch/fm_topk':>14} "
             f"{'matrix floor':>13} {'fm_topk/HBM':>12} {'fm_topk/matrix':>15} {'same rows':>10} {'max |ds|':>10}"]
    for nq, _, ms in cases:
        med = {n: statistics.median(v) for n, v in ms.items()}
        cell = {n: f"{med[n]:.3f} ({min(v):.3f})" for n, v in ms.items()}
        floor_mx = 2.0 * nq * a.nc * a.kp / MATRIX_FP32_FLOPS * 1e3
        slab, parts = K.topk_plan(nq, a.nc, a.k)
        lines.append(f"{nq:>6} {slab:>8} {parts:>6} {cell['fm_topk']:>18} {cell['torch']:>18} "
                     f"{med['torch'] / med['fm_topk']:>14.2f} {floor_mx:>13.4f} {med['fm_topk'] / floor_hbm:>12.1f} "
                     f"{med['fm_topk'] / floor_mx:>15.1f} {agree[nq][0]:>6}/{nq:<4}{agree[nq][1]:>10.2e}")
        if med["fm_topk"] > med["torch"]:
            bound = "the matrix floor" if floor_mx > floor_hbm else "the HBM floor"
            lines.append(f"  (nq = {nq}: fm_topk is SLOWER than the torch line; the larger floor here is {bound}. "
                         "One wave per 16 queries reads its slab of C on its own, so C is fetched once per 16 queries "
                         "from L2 / Infinity Cache, and 4-byte operands feed one 16x16x4 instruction per 16 B loaded "
                         "per lane; sharing candidate tiles between the waves of a workgroup through LDS is the "
                         "untried lever)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
