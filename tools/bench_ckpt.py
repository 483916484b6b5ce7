"""Sparse against dense checkpoints of a partly trained table (utils/checkpoint.py, hip/ckpt.hip).

A k64 fp32 Adagrad table of ``--vocab`` rows (8M by default) is trained for ``--steps`` steps on synthetic
Criteo-shaped batches -- once per batch size of ``--batches``: the batch size sets the share of the table a run
of that many steps touches --, then timed: the changed-row scan alone (device events around the whole call, its one
host read included; median) with the table bytes it reads per second, a sparse and a dense save, both
restores (wall clock, device synchronised; the files go to a temporary directory, through the page cache like any
training run's), the file sizes and the share of rows changed.  The dense path is the one every checkpoint
took before the sparse format existed: the yardstick.  The restored tables are compared bitwise.  A record,
not a gate: writes the table to ``--out``.

    python tools/bench_ckpt.py [--vocab 8388608] [--steps 300] [--batches 131072,16384,2048]
                               [--out profiles/ckpt/sparse_ckpt.txt]
"""

from __future__ import annotations

import argparse
import glob
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from fast_tffm_amd.data.synthetic import CriteoSynth  # noqa: E402
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig  # noqa: E402
from fast_tffm_amd.ops import kernels as K  # noqa: E402
from fast_tffm_amd.utils import checkpoint as ckpt  # noqa: E402


def wall(fn) -> tuple[float, object]:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, r


def same_tables(a, b) -> bool:
    names = ("v", "w", "s0v", "s0w")
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in names)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--vocab", type=int, default=1 << 23)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--batches", default="131072,16384,2048")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ckpt", "sparse_ckpt.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        print("bench_ckpt: needs a GPU", file=sys.stderr)
        return 1
    K.set_debug_checks(False)
    dev = torch.device("cuda:0")
    text, ok = "", True
    for batch in (int(x) for x in a.batches.split(",")):
        t, good = run(a, dev, batch)
        text += t
        ok = ok and good
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)
    return 0 if ok else 2


def run(a, dev, batch: int) -> tuple[str, bool]:
    V, Kf = a.vocab, 64

    def model(seed):
        cfg = FMConfig(vocabulary_size=V, factor_num=Kf, loss_type="logistic", batch_size=batch, seed=seed,
                       dtype=torch.float32, opt=K.OptConfig("adagrad", lr=0.05))
        return FactorizationMachine(cfg, device=dev)

    m = model(1)
    t = m.table
    gen = CriteoSynth(V, device=dev, seed=3)
    for _ in range(a.steps):
        m.train_step(gen.batch(batch))
    torch.cuda.synchronize()

    rows = t.changed_rows()
    n = int(rows.numel())
    ms = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t.changed_rows()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    scan_ms = statistics.median(ms)
    scanned = t.real_rows * (2 * t.Kp * 4 + 8)  # v, s0v rows and w, s0w words: every byte once

    tmp = tempfile.mkdtemp(prefix="bench_ckpt_")
    res = {}
    try:
        for fmt in ("sparse", "dense"):
            log = os.path.join(tmp, fmt)
            shutil.rmtree(log, ignore_errors=True)
            save_s, path = wall(lambda: ckpt.save_checkpoint(m, log, m.global_step, table_format=fmt))
            size = sum(os.path.getsize(f) for f in glob.glob(os.path.join(path, "*.safetensors")))
            m2 = model(2)  # (another seed: a sparse restore must bring the checkpoint's)
            restore_s, _ = wall(lambda: ckpt.restore_checkpoint(m2, path))
            ok = same_tables(t, m2.table)
            m2.close()
            del m2
            shutil.rmtree(log, ignore_errors=True)
            res[fmt] = (save_s, restore_s, size, ok)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    gb = 1e9
    lines = [f"sparse vs dense checkpoints, {torch.cuda.get_device_name(dev)}; k{Kf} fp32 Adagrad table of {V} rows "
             f"({t.nbytes() / gb:.2f} GB), {a.steps} steps of {batch} Criteo-shaped examples",
             f"rows changed: {n} of {t.real_rows} ({100.0 * n / max(t.real_rows, 1):.2f}%)",
             f"changed-row scan (one call, host read of the count included; median of {a.repeats}): "
             f"{scan_ms:.3f} ms, {scanned / gb:.2f} GB read = {scanned / gb / (scan_ms / 1e3):.0f} GB/s",
             f"{'format':>8} {'save s':>9} {'restore s':>10} {'file GB':>9} {'restored == saved':>18}"]
    for fmt in ("sparse", "dense"):
        s, r, size, ok = res[fmt]
        lines.append(f"{fmt:>8} {s:>9.3f} {r:>10.3f} {size / gb:>9.3f} {str(ok):>18}")
    ds, ss = res["dense"], res["sparse"]
    lines.append(f"dense / sparse: save {ds[0] / ss[0]:.1f}x, restore {ds[1] / ss[1]:.1f}x, file {ds[2] / ss[2]:.1f}x")
    m.close()
    return "\n".join(lines) + "\n\n", bool(ds[3] and ss[3])


if __name__ == "__main__":
    sys.exit(main())
