"""Cost of the listwise ranking loss on the GPU (hip/group_loss.hip): each half of the op alone, and the training
step with and without it.

Halves, at B = 131072 examples, for three groupings -- Zipf-1.1 ids over 1M keys (one user owns a large share of
the batch beside a long tail of tiny groups), all singletons, one group: ``K.group_plan`` (keys -> sort -> ranges)
and ``K.group_softmax_loss`` (the score half), each timed alone with device events around the call and a reused
workspace; medians of ``--repeats`` calls after warm-up calls.  The smallest check first: the timed code computes
what the CPU twin computes.

Step: the eager lookahead local step of ``bench.py``'s k64 fp32 preset (same synthetic batches, depth-2 lookahead)
with ``loss_type = logistic`` and with ``rank_softmax`` (group key: feature 0), wall time per step over
``--steps`` steps after warm-up, three rounds each, alternating; medians.  The expectation to confirm or refute:
the step grows by about the score half alone, the plan half hidden beside the dedup on the side stream.
A record, not a gate: writes the table to ``--out``.

    python tools/bench_group_loss.py [--repeats 30] [--steps 40] [--out profiles/group_loss/group_loss.txt]
"""

from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fast_tffm_amd.data.synthetic import CriteoSynth  # noqa: E402
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig  # noqa: E402
from fast_tffm_amd.models.table import bits_for  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402

B = 131072
KEYS = 1_000_000


def make_ids(kind: str, g: torch.Generator) -> torch.Tensor:
    if kind == "singletons":
        return torch.randperm(B, generator=g).to(torch.int32)
    if kind == "one group":
        return torch.full((B,), 12345, dtype=torch.int32)
    # Zipf-1.1 over KEYS ids by inverse-CDF sampling
    w = torch.arange(1, KEYS + 1, dtype=torch.float64).pow(-1.1)
    cdf = torch.cumsum(w / w.sum(), 0)
    u = torch.rand(B, generator=g, dtype=torch.float64)
    return torch.searchsorted(cdf, u).clamp_(max=KEYS - 1).to(torch.int32)


def timed(fn, warmup: int, repeats: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def step_ms(loss: str, pool, vocab: int, warmup: int, steps: int, rounds: int) -> list:
    cfg = FMConfig(vocabulary_size=vocab, factor_num=64, loss_type=loss, batch_size=B, init_value_range=0.01, seed=42,
                   opt=K.OptConfig("adagrad", lr=0.01, initial_accumulator=0.1), mode="local")
    model = FactorizationMachine(cfg, device=pool[0].device)
    n = len(pool)
    out = []
    i = 0
    for r in range(rounds + 1):  # round 0: warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(warmup if r == 0 else steps):
            model.train_step(pool[i % n], pool[(i + 1) % n], pool[(i + 2) % n])
            i += 1
        torch.cuda.synchronize()
        if r:
            out.append(1000.0 * (time.perf_counter() - t0) / steps)
    K.check_device_errors(pool[0].device)
    model.close()
    del model
    torch.cuda.empty_cache()
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--vocab", type=int, default=125_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_loss", "group_loss.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_group_loss: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(7)
    s_h = torch.randn(B, generator=g)
    y_h = (torch.rand(B, generator=g) < 0.25).float()
    s, y = s_h.to(dev), y_h.to(dev)
    ws = K.group_loss_workspace(B, dev)
    dpred = torch.empty(B, dtype=torch.float32, device=dev)
    kb = bits_for(KEYS + 1)
    lines = [f"K.group_plan / K.group_softmax_loss at B = {B}, {torch.cuda.get_device_name(dev)}; key_bits {kb}; "
             f"medians of {a.repeats} event-timed calls with a reused workspace after {a.warmup} warm-up calls; "
             f"ms per call",
             f"{'grouping':>12} {'groups':>8} {'largest':>8} {'plan':>8} {'softmax':>8}"]
    for kind in ("zipf-1.1", "singletons", "one group"):
        ids_h = make_ids(kind, g)
        ids = ids_h.to(dev)
        plan = K.group_plan(ids, kb, ws=ws)
        d, loss = K.group_softmax_loss(plan, s, y, None, 1.0 / B, dpred=dpred)
        dc, lc = K.group_softmax_loss(K.group_plan(ids_h, kb), s_h, y_h, None, 1.0 / B)
        assert torch.allclose(d.cpu(), dc, rtol=1e-6, atol=1e-12) and abs(float(loss) - float(lc)) <= 1e-6 * float(lc)
        t_p = timed(lambda: K.group_plan(ids, kb, ws=ws), a.warmup, a.repeats)
        t_s = timed(lambda: K.group_softmax_loss(plan, s, y, None, 1.0 / B, dpred=dpred), a.warmup, a.repeats)
        cnt = torch.bincount(ids_h.long())
        lines.append(f"{kind:>12} {int((cnt > 0).sum()):>8} {int(cnt.max()):>8} {t_p:>8.3f} {t_s:>8.3f}")
    K.check_device_errors(dev)
    del ws, dpred

    gen = CriteoSynth(a.vocab, alpha=1.1, seed=1000, device=dev)
    pool = [gen.batch(B) for _ in range(16)]
    torch.cuda.synchronize()
    t_log, t_rank = [], []
    for _ in range(2):  # alternating, so that drift hits both
        t_log += step_ms("logistic", pool, a.vocab, 10, a.steps, 2)
        t_rank += step_ms(K.RANK_LOSS, pool, a.vocab, 10, a.steps, 2)
    m_log, m_rank = statistics.median(t_log), statistics.median(t_rank)
    keys = K.group_keys(pool[0].offsets, pool[0].ids.to(torch.int32), 0, a.vocab).cpu()
    cnt = torch.bincount(keys[keys >= 0].long())
    lines += ["",
              f"eager lookahead (depth 2) k64 fp32 local step, vocab {a.vocab}, B = {B}, bench.py's synthetic batches "
              f"(group key: feature 0 -> {int((cnt > 0).sum())} groups in batch 0, the largest {int(cnt.max())}); "
              f"wall ms per step over {a.steps} steps, 4 rounds each, alternating models",
              f"    logistic     median {m_log:.4f}   rounds {' '.join(f'{t:.4f}' for t in t_log)}",
              f"    rank_softmax median {m_rank:.4f}   rounds {' '.join(f'{t:.4f}' for t in t_rank)}",
              f"    difference   {m_rank - m_log:+.4f} ms per step ({100 * (m_rank / m_log - 1):+.1f}%)"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
