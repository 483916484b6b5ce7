"""Cost of the pairwise ranking loss on the GPU (hip/group_pair.hip): the op alone beside the listwise score half on
the same plan, and the training step with each loss.

Op, at B = 131072 examples, 3% and 30% positives, for five groupings -- Zipf-1.1 ids over 1M keys, all singletons,
groups of 8, one group of B/10 among Zipf groups, one group of the whole batch: ``K.group_pairwise_loss`` and
``K.group_softmax_loss`` (its score half) on one plan, each call timed alone with device events, reused workspaces,
the two ops alternating call by call; medians of ``--repeats`` calls after warm-up calls (a call slower than 200 ms
is repeated 5 times only).  ``sum P_g N_g``: the (positive, negative) pairs of the input, every one evaluated from
both of its rows.  The smallest check first: the timed code computes what the CPU twin computes (inputs with fewer
than 2^24 pairs).  The one expectation to check: on inputs with ``sum P_g N_g`` below about 64 n the op stays within
a small multiple of the softmax half.

Step: the eager lookahead local step of ``bench.py``'s k64 fp32 preset (same synthetic batches, depth-2 lookahead)
with ``loss_type = logistic``, ``rank_softmax`` and ``rank_pairwise`` (group key: feature 0), wall time per step
over ``--steps`` steps after warm-up, two rounds each, models alternating, twice; medians.
A record, not a gate: writes the table to ``--out``.

    python tools/bench_group_pair.py [--repeats 30] [--steps 40] [--out profiles/group_loss/group_pair.txt]
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

from bench_group_loss import B, KEYS, make_ids, step_ms  # noqa: E402
from fast_tffm_amd.data.synthetic import CriteoSynth  # noqa: E402
from fast_tffm_amd.models.table import bits_for  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402

NOT_TRIED = """Not tried: fp32 pair arithmetic (the definition is fp64 throughout); computing each pair once and
reducing its transpose (every pair is evaluated twice, once from each of its rows); a plan sorted by (group, class),
so that a row meets only columns of the opposite class (a row walks its whole group and skips its own class)."""


def ids_for(kind: str, g: torch.Generator) -> torch.Tensor:
    if kind == "groups of 8":
        return (torch.randperm(B, generator=g) // 8).to(torch.int32)
    if kind == "B/10 + zipf":
        ids = make_ids("zipf-1.1", g)
        ids[torch.randperm(B, generator=g)[: B // 10]] = KEYS - 7
        return ids
    if kind == "whole batch":
        return make_ids("one group", g)
    return make_ids(kind, g)


def pair_count(ids_h: torch.Tensor, y_h: torch.Tensor) -> int:
    n_g = torch.bincount(ids_h.long())
    p_g = torch.bincount(ids_h.long(), weights=y_h.double(), minlength=n_g.numel()).long()
    return int((p_g * (n_g - p_g)).sum())


def alternating(fns, warmup: int, repeats: int) -> list:
    """Median ms of every fn, each call timed alone, the fns taking turns."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return [statistics.median(m) for m in ms]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=125_000_000)
    ap.add_argument("--no-step", action="store_true", help="the op table only")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_loss", "group_pair.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_group_pair: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    s_h = torch.randn(B, generator=g)
    s = s_h.to(dev)
    ws = K.group_loss_workspace(B, dev)
    sws = K.group_loss_workspace(B, dev)
    pws = K.group_pair_workspace(B, dev)
    dpred = torch.empty(B, dtype=torch.float32, device=dev)
    kb = bits_for(KEYS + 1)
    rows, chunk, slabs = K.group_pair_geometry()
    lines = [f"K.group_pairwise_loss beside K.group_softmax_loss's score half on one plan at B = {B}, "
             f"{torch.cuda.get_device_name(dev)}; key_bits {kb}; row tile {rows}, column chunk {chunk}, {slabs} slabs; "
             f"pair workspace {pws.numel() / 2**20:.1f} MiB; medians of {a.repeats} event-timed calls (5 for a call "
             f"above 200 ms), the two ops alternating, reused workspaces, {a.warmup} warm-up calls; ms per call",
             f"{'grouping':>12} {'pos':>4} {'groups':>8} {'largest':>8} {'sum P_g N_g':>14} {'/ n':>9} "
             f"{'softmax':>8} {'pairwise':>9} {'ratio':>7} {'ns/pair':>8}"]
    small_ok = True
    for kind in ("zipf-1.1", "singletons", "groups of 8", "B/10 + zipf", "whole batch"):
        ids_h = ids_for(kind, g)
        ids = ids_h.to(dev)
        cnt = torch.bincount(ids_h.long())
        for share in (0.03, 0.30):
            y_h = (torch.rand(B, generator=g) < share).float()
            y = y_h.to(dev)
            pairs = pair_count(ids_h, y_h)
            plan = K.group_plan(ids, kb, ws=ws)
            d, loss = K.group_pairwise_loss(plan, s, y, None, 1.0 / B, dpred=dpred, ws=pws)
            torch.cuda.synchronize()
            if pairs < 2**24:
                dc, lc = K.group_pairwise_loss(K.group_plan(ids_h, kb), s_h, y_h, None, 1.0 / B)
                assert torch.allclose(d.cpu(), dc, rtol=1e-6, atol=1e-30), kind
                assert abs(float(loss) - float(lc)) <= 1e-6 * abs(float(lc)), kind
            fns = [lambda: K.group_softmax_loss(plan, s, y, None, 1.0 / B, dpred=dpred, ws=sws),
                   lambda: K.group_pairwise_loss(plan, s, y, None, 1.0 / B, dpred=dpred, ws=pws)]
            probe = alternating(fns, 1, 1)
            slow = probe[1] > 200.0
            t_s, t_p = alternating(fns, 0 if slow else a.warmup, 5 if slow else a.repeats)
            if pairs < 64 * B:
                small_ok = small_ok and t_p <= 4.0 * t_s
            per = f"{1e6 * t_p / pairs:8.3f}" if pairs else f"{'-':>8}"
            lines.append(f"{kind:>12} {int(100 * share):>3}% {int((cnt > 0).sum()):>8} {int(cnt.max()):>8} "
                         f"{pairs:>14} {pairs / B:>9.1f} {t_s:>8.3f} {t_p:>9.3f} {t_p / t_s:>7.2f} {per}")
    K.check_device_errors(dev)
    lines += ["",
              "Expectation (inputs with sum P_g N_g below 64 n: the pairwise op within a small multiple -- taken as 4x "
              f"-- of the softmax half): {'holds' if small_ok else 'DOES NOT HOLD'} on the rows above.",
              "The whole-batch group costs time proportional to P N fp64 transcendental evaluations (an exp, a "
              "division and, from the positive's side, a log1p per pair and side): the ns/pair column times P N.  Do "
              "not point rank_group_feature at a low-cardinality feature."]
    del ws, sws, pws, dpred

    if not a.no_step:
        gen = CriteoSynth(a.vocab, alpha=1.1, seed=1000, device=dev)
        pool = [gen.batch(B) for _ in range(16)]
        torch.cuda.synchronize()
        losses = ("logistic", K.RANK_LOSS, K.RANK_PAIR_LOSS)
        t = {k: [] for k in losses}
        for _ in range(2):  # alternating, so that drift hits all
            for k in losses:
                t[k] += step_ms(k, pool, a.vocab, 10, a.steps, 2)
        keys = K.group_keys(pool[0].offsets, pool[0].ids.to(torch.int32), 0, a.vocab).cpu()
        cnt = torch.bincount(keys[keys >= 0].long())
        pairs = pair_count(keys[keys >= 0], (pool[0].labels.cpu() > 0).float()[keys >= 0])
        med = {k: statistics.median(v) for k, v in t.items()}
        lines += ["",
                  f"eager lookahead (depth 2) k64 fp32 local step, vocab {a.vocab}, B = {B}, bench.py's synthetic "
                  f"batches (group key: feature 0 -> {int((cnt > 0).sum())} groups in batch 0, the largest "
                  f"{int(cnt.max())}, sum P_g N_g {pairs}); wall ms per step over {a.steps} steps, 4 rounds each, "
                  f"alternating models"]
        for k in losses:
            lines.append(f"    {k:<13} median {med[k]:.4f}   rounds {' '.join(f'{x:.4f}' for x in t[k])}"
                         + ("" if k == "logistic" else f"   ({med[k] - med['logistic']:+.4f} ms, "
                                                       f"{100 * (med[k] / med['logistic'] - 1):+.1f}% on logistic)"))
    else:
        lines += ["", "The k64 training step with logistic / rank_softmax / rank_pairwise: not taken in this run."]
    lines += ["", NOT_TRIED]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
