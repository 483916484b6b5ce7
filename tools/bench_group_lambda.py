"""Cost of the LambdaRank loss on the GPU (hip/group_lambda.hip): the op alone beside the pairwise op on the same
plan, and the training step with it.

Op, at B = 131072 examples, 30% positives, for five groupings -- all singletons, Zipf-1.1 ids over 1M keys, groups of
8, one group of B/10 among Zipf groups, one group of the whole batch -- at K = 10 and K = 0: ``K.group_lambda_loss``
and ``K.group_pairwise_loss`` on one plan, each call timed alone with device events, reused workspaces, the two ops
alternating call by call; medians of ``--repeats`` calls after warm-up calls (a call slower than 200 ms is timed
once more only).  ``walked``: the columns the rows walk, ``sum_g n_g h + (n_g - h) h`` with ``h = min(K, n_g)``
(``n_g^2`` at K = 0); a walked column of equal gain is skipped, the others are one pair evaluation each.  The
singletons row has no pair to walk: it is what the inverse, the four stable sorts (two over 32 bits, two over
``bits_for(n + 1)``) and the ideal / head / grad passes cost, the floor every other row stands on.  The smallest check
first: the timed code computes what the CPU twin computes (inputs that walk fewer than 2^24 columns).

Step: the eager lookahead local step of ``bench.py``'s k64 fp32 preset (same synthetic batches, depth-2 lookahead)
with ``loss_type = logistic`` and ``rank_lambda`` (K = 10, group key: feature 0), wall time per step over ``--steps``
steps after warm-up, two rounds each, models alternating, twice; medians.
A record, not a gate: writes the table to ``--out``.

    python tools/bench_group_lambda.py [--repeats 30] [--steps 40] [--out profiles/group_loss/group_lambda.txt]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_group_loss import B, KEYS, step_ms  # noqa: E402
from bench_group_pair import alternating, ids_for  # noqa: E402
from fast_tffm_amd.data.synthetic import CriteoSynth  # noqa: E402
from fast_tffm_amd.models.table import bits_for  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402

NOT_TRIED = """Not tried: a cooperative walk for the head rows (the workgroup's threads taking the staged columns of
one head row and a fixed-order block reduction, instead of one thread per row), which is what the K > 0 rows of big
groups wait for; hoisting the ideal order (labels and plan only) beside the batch's dedup, which would take two of
the four sorts off the step's critical path; one 64-bit-key sort in place of each pair of 32-bit-key sorts; a
separate span for the head columns a tail row needs (a tile that holds the tail of one big group and the start of the
next stages every chunk between that group's head and itself, though no row walks them); computing each pair once and
reducing its transpose (every pair is evaluated from both of its rows); fp32 pair arithmetic (the definition is
fp64 throughout)."""


def walked(ids_h: torch.Tensor, cutoff: int) -> int:
    n_g = torch.bincount(ids_h.long())
    n_g = n_g[n_g >= 2]
    h = n_g if cutoff == 0 else n_g.clamp(max=cutoff)
    return int((n_g * h + (n_g - h) * h).sum())


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=125_000_000)
    ap.add_argument("--no-step", action="store_true", help="the op table only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_loss", "group_lambda.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_group_lambda: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    s_h = torch.randn(B, generator=g)
    y_h = (torch.rand(B, generator=g) < 0.30).float()
    s, y = s_h.to(dev), y_h.to(dev)
    ws = K.group_loss_workspace(B, dev)
    pws = K.group_pair_workspace(B, dev)
    lws = K.group_lambda_workspace(B, dev)
    dpred = torch.empty(B, dtype=torch.float32, device=dev)
    kb = bits_for(KEYS + 1)
    rows, chunk, slabs = K.group_lambda_geometry()
    lines = [f"K.group_lambda_loss beside K.group_pairwise_loss on one plan at B = {B}, 30% positives, "
             f"{torch.cuda.get_device_name(dev)}; key_bits {kb}; row tile {rows}, column chunk {chunk}, {slabs} slabs; "
             f"lambda workspace {lws.numel() / 2**20:.1f} MiB; medians of {a.repeats} event-timed calls (one more call "
             f"only when a call takes above 200 ms), the two ops alternating, reused workspaces, {a.warmup} warm-up "
             f"calls; ms per call",
             f"{'grouping':>12} {'K':>3} {'groups':>8} {'largest':>8} {'walked':>14} {'/ n':>9} {'pairwise':>9} "
             f"{'lambda':>9} {'- floor':>9} {'ns/walked':>10}"]
    floor = {}
    for kind in ("singletons", "zipf-1.1", "groups of 8", "B/10 + zipf", "whole batch"):
        ids_h = ids_for(kind, g)
        ids = ids_h.to(dev)
        cnt = torch.bincount(ids_h.long())
        plan = K.group_plan(ids, kb, ws=ws)
        for cutoff in (10, 0):
            w = walked(ids_h, cutoff)
            d, loss = K.group_lambda_loss(plan, s, y, cutoff, 1.0 / B, dpred=dpred, ws=lws)
            torch.cuda.synchronize()
            if w < 2**24:
                dc, lc = K.group_lambda_loss(K.group_plan(ids_h, kb), s_h, y_h, cutoff, 1.0 / B)
                assert torch.allclose(d.cpu(), dc, rtol=1e-5, atol=1e-12), (kind, cutoff)
                assert abs(float(loss) - float(lc)) <= 1e-6 * abs(float(lc)), (kind, cutoff)
            fns = [lambda: K.group_pairwise_loss(plan, s, y, None, 1.0 / B, dpred=dpred, ws=pws),
                   lambda: K.group_lambda_loss(plan, s, y, cutoff, 1.0 / B, dpred=dpred, ws=lws)]
            probe = alternating(fns, 1, 1)
            slow = max(probe) > 200.0
            t_p, t_l = alternating(fns, 0 if slow else a.warmup, 1 if slow else a.repeats)
            if kind == "singletons":
                floor[cutoff] = t_l
            over = t_l - floor[cutoff]
            per = f"{1e6 * over / w:10.3f}" if w else f"{'-':>10}"
            lines.append(f"{kind:>12} {cutoff:>3} {int((cnt > 0).sum()):>8} {int(cnt.max()):>8} {w:>14} {w / B:>9.1f} "
                         f"{t_p:>9.3f} {t_l:>9.3f} {over:>9.3f} {per}")
    K.check_device_errors(dev)
    lines += ["",
              "The singletons rows are the cost of the four sorts and the per-position passes; '- floor' is what the "
              "pair pass (and the wider grad pass) adds to it, 'ns/walked' that per walked column.  At K = 0 a group "
              "costs n_g^2 fp64 transcendental evaluations, as the pairwise op's P N: do not point rank_group_feature "
              "at a low-cardinality feature without a cutoff.  At K > 0 the time of a big group is not its walked "
              "columns but its longest walk: the K head rows sit on K / 4 threads of one row tile, and each walks "
              "n_g / slabs columns per slab, one dependent fp64 exp / log1p / division chain after the other, while "
              "the tail rows (K columns each) finish at once -- hence the high ns/walked of those rows."]
    del ws, pws, lws, dpred

    if not a.no_step:
        gen = CriteoSynth(a.vocab, alpha=1.1, seed=1000, device=dev)
        pool = [gen.batch(B) for _ in range(16)]
        torch.cuda.synchronize()
        losses = ("logistic", K.RANK_LAMBDA_LOSS)
        t = {k: [] for k in losses}
        for _ in range(2):  # alternating, so that drift hits both
            for k in losses:
                t[k] += step_ms(k, pool, a.vocab, 10, a.steps, 2)
        keys = K.group_keys(pool[0].offsets, pool[0].ids.to(torch.int32), 0, a.vocab).cpu()
        cnt = torch.bincount(keys[keys >= 0].long())
        med = {k: statistics.median(v) for k, v in t.items()}
        lines += ["",
                  f"eager lookahead (depth 2) k64 fp32 local step, vocab {a.vocab}, B = {B}, bench.py's synthetic "
                  f"batches (group key: feature 0 -> {int((cnt > 0).sum())} groups in batch 0, the largest "
                  f"{int(cnt.max())}, walked at K = 10: {walked(keys[keys >= 0], 10)}); wall ms per step over "
                  f"{a.steps} steps, 4 rounds each, alternating models"]
        for k in losses:
            lines.append(f"    {k:<13} median {med[k]:.4f}   rounds {' '.join(f'{x:.4f}' for x in t[k])}"
                         + ("" if k == "logistic" else f"   ({med[k] - med['logistic']:+.4f} ms, "
                                                       f"{100 * (med[k] / med['logistic'] - 1):+.1f}% on logistic)"))
    else:
        lines += ["", "The k64 training step with logistic / rank_lambda: not taken in this run."]
    lines += ["", NOT_TRIED]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
