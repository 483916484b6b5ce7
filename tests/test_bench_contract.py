"""bench.py output contract (one JSON line with the driver's keys), exercised on CPU with a
tiny configuration; the real measurement runs on the GPU (see profiles/)."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config"}


def _run(args):
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.parametrize("args", [["--steps", "2", "--warmup", "1", "--batch", "256", "--slots-per-gpu", "20000"],
                                  ["--preset", "a1a_cpu", "--steps", "2", "--warmup", "1"]])
def test_bench_prints_one_json_line(args):
    d = _run(args)
    assert KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["scaling"] == "weak"
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(d["config"])


def test_bench_dump_outputs_and_full(tmp_path):
    """``--dump-outputs DIR``: the last timed step's loss and a seeded sample of the rows and optimizer
    slots it left, float32 / float64 .npy well under 64 MB, for the same rows and with the same values
    from run to run; the timed steps still number ``--steps``.  ``--full`` adds the batch statistics (on
    stderr) that a plain run no longer computes; stdout stays the one JSON line either way."""
    import numpy as np

    args = ["--steps", "3", "--warmup", "1", "--batch", "256", "--slots-per-gpu", "20000"]
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    runs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(out)]
                           + extra, capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout
        d = json.loads(lines[0])
        assert KEYS <= set(d) and d["steps"] == 3 and d["ms_per_step"] > 0
        assert ("batch stats:" in r.stderr) == bool(extra)
        arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
        assert set(arrays) == {"loss_sum", "row_ids", "rows", "slot0"}
        assert all(x.dtype in (np.float32, np.float64) for x in arrays.values())
        assert sum(x.nbytes for x in arrays.values()) <= 64 * 2**20
        runs.append(arrays)
    a, b = runs
    n = a["row_ids"].shape[0]
    assert n == 2 * 8192 and a["rows"].shape == (n, 65) and a["slot0"].shape == (n, 65)
    assert a["loss_sum"].shape == (1,) and np.isfinite(a["loss_sum"]).all() and np.isfinite(a["rows"]).all()
    assert (a["slot0"] > 0.1).any()  # (sampled rows of the last batch: their accumulators moved)
    assert np.array_equal(a["row_ids"], b["row_ids"])
    for k in ("loss_sum", "rows", "slot0"):  # (CPU kernels: OpenMP may reorder fp32 sums between runs)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-8)


def test_bench_two_ranks_one_json_line():
    """The driver's N>1 launch (torch.distributed.run, one process per device, 127.0.0.1):
    stdout holds exactly rank 0's JSON line (the gloo side-group's connection messages and
    every other rank's output go to stderr), n_gpus / global_batch / parallelism follow the
    world size.  CPU + gloo here; the same path runs RCCL on MI355X."""
    import socket

    from ports import free_port

    port = free_port()
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "256", "--slots-per-gpu", "20000",
                        "--preset", "k64"],  # (bf16 storage wires of the default preset are a GPU path)
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert KEYS <= set(d) and d["n_gpus"] == 2 and d["config"]["global_batch"] == 512
    assert d["config"]["parallelism"] == "rowshard2" and d["config"]["early_rows"] and d["config"]["split_grads"]
    assert d["config"]["rccl_world"] == 2 and d["config"]["comm_backend"] == "gloo"
    assert d["config"]["per_rank_ms"]["max"] >= d["config"]["per_rank_ms"]["min"] > 0
    assert d["config"]["comm_bytes_per_rank"] > 0


def test_bench_self_launches_ranks():
    """``bench.py --gpus 2`` with no launcher environment starts the 2 ranks itself (through
    torch.distributed.run, before any device call) instead of measuring one process."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                          "MASTER_PORT")}
    env.update(CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup",
                        "1", "--batch", "256", "--slots-per-gpu", "20000"],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rccl_world"] == 2 and d["config"]["global_batch"] == 512


def test_bench_world_mismatch_exits_nonzero():
    """An existing WORLD_SIZE that disagrees with --gpus is refused (exit 2, no JSON line)."""
    env = dict(os.environ, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="", WORLD_SIZE="1", RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup",
                        "0", "--batch", "64", "--slots-per-gpu", "2000"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])
    assert not r.stdout.strip()
    assert "WORLD_SIZE" in r.stderr
