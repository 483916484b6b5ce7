#!/usr/bin/env python3
"""Call order of the step executors: every native entry point and collective they issue, in order.

A refactor of ``models/fm.py`` / ``parallel/exchange.py`` must leave this log unchanged.  The probe wraps
the callables of the native module (``native.hip()``, or ``native.cpu()`` with ``--cpu``), the collectives of
``torch.distributed`` and the roctx ranges in Python and logs, per call: the entry's name, the stream it was
given (collectives: the group and the current stream) and the calling thread, each numbered by first
appearance so that two processes give the same text.  Per executor it runs 8 training steps with two
batches of lookahead, then one ``forward`` and one ``explain`` (B = 256, 8 features per example, k = 16,
4096 rows: the order does not depend on the size).

    python tools/probe/call_order.py --out after.txt          # GPU, RCCL at world 1
    python tools/probe/call_order.py --cpu --out after.txt    # CPU module, gloo at world 2

Every executor (and every rank) runs in a fresh process under its own time limit, one executor at a time;
the first failure ends the run.  Run it on both trees and ``diff`` the two files.
"""
import argparse
import os
import socket
import subprocess
import sys
import tempfile
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS, B, FEATS, KF, V = 8, 256, 8, 16, 4096

# name -> (mode, lookahead, FMConfig extras, environment)
GPU_EXECUTORS = {
    "local": ("local", False, {}, {}),
    "local_lookahead": ("local", True, {}, {}),
    "shard_emit": ("shard", True, {}, {"FM_SHARD_W1_LOCAL": "0"}),
    "shard_emit_no_self_rows": ("shard", True, {}, {"FM_SHARD_W1_LOCAL": "0", "FM_SELF_ROWS": "0"}),
    "shard_stale": ("shard", True, {"staleness": 1}, {}),
    "dp_dense": ("dp_dense", True, {}, {"FM_DP_W1_LOCAL": "0"}),
}
CPU_EXECUTORS = {
    "local": ("local", False, {}, {}),
    "shard": ("shard", True, {"overlap_grads": "on"}, {}),
    "shard_prefetch_on": ("shard", True, {"prefetch_rows": "on"}, {}),
    "shard_microbatches": ("shard", True, {"microbatches": 2}, {}),
    "shard_stale": ("shard", True, {"staleness": 1}, {}),
    "dp": ("dp", False, {}, {}),
    "dp_dense": ("dp_dense", True, {}, {}),
}


class _Names:
    """Handles (streams, groups, threads) numbered by first appearance."""

    def __init__(self):
        self.seen = {}

    def __call__(self, kind, key):
        if key is None:
            return "-"
        return self.seen.setdefault((kind, key), f"{kind}{sum(1 for k in self.seen if k[0] == kind)}")


def run_one(name: str, cpu: bool, out_path: str) -> None:
    mode, lookahead, extra, env = (CPU_EXECUTORS if cpu else GPU_EXECUTORS)[name]
    os.environ.update(env)
    sys.path.insert(0, ROOT)
    import torch
    import torch.distributed as tdist

    from fast_tffm_amd.data.synthetic import random_batch
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
    from fast_tffm_amd.ops import kernels as K
    from fast_tffm_amd.ops import native
    from fast_tffm_amd.parallel import dist as fmdist
    from fast_tffm_amd.utils import trace

    log, names = [], _Names()

    def note(what, where):
        log.append(f"{what} {where} {names('t', threading.get_ident())}")

    def cur_stream():
        return None if cpu else torch.cuda.current_stream().cuda_stream

    class Logged:
        def __init__(self, mod):
            self._mod = mod

        def __getattr__(self, attr):
            f = getattr(self._mod, attr)
            if not callable(f):
                return f

            def call(*a, **kw):
                note(attr, names("s", kw.get("stream")))
                return f(*a, **kw)

            return call

    which = "cpu" if cpu else "hip"
    proxy = Logged(getattr(native, which)())
    setattr(native, which, lambda: proxy)
    for coll in ("all_to_all_single", "all_to_all", "all_gather", "all_gather_into_tensor", "reduce_scatter_tensor",
                 "all_reduce"):
        def wrap(f=getattr(tdist, coll), coll=coll):
            def call(*a, **kw):
                g = kw.get("group")
                note(coll + (" async" if kw.get("async_op") else ""),
                     f"{names('g', id(g) if g is not None else None)} {names('s', cur_stream())}")
                return f(*a, **kw)
            return call
        setattr(tdist, coll, wrap())
    trace._ROCTX_ON = True
    trace._roctx = (lambda s: note("range", f"push {s}"), lambda: note("range", "pop"))

    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if mode == "local":
        ctx, dev = None, torch.device("cpu" if cpu else "cuda:0")
    elif cpu:
        ctx = fmdist.init_distributed(backend="gloo", rank=rank, world=world, device="cpu")
        dev = ctx.device
    else:
        ctx = fmdist.init_distributed(force_pg=True)
        dev = ctx.device
    cfg = FMConfig(vocabulary_size=V, factor_num=KF, loss_type="logistic", batch_size=B, seed=1, threads=1,
                   opt=K.OptConfig("adagrad", lr=0.05), mode=mode, **extra)
    m = FactorizationMachine(cfg, device=dev, dist=ctx)
    bs = [random_batch(B, V, max_feats=FEATS, min_feats=FEATS, seed=100 * s + rank, device=dev)
          for s in range(STEPS + 2)]
    if not cpu:
        torch.cuda.synchronize()
    for s in range(STEPS):
        log.append(f"# train_step {s}")
        out = m.train_step(bs[s], *((bs[s + 1], bs[s + 2]) if lookahead else ()))
    log.append("# forward")
    m.forward(bs[STEPS], loss="logistic")
    log.append("# explain")
    m.explain(bs[STEPS])
    if not cpu:
        torch.cuda.synchronize()
    loss = out.mean_loss()
    assert loss == loss, "the last step's loss is NaN"
    log.append("# close")
    m.close()
    if ctx is not None:
        fmdist.shutdown()
    with open(out_path, "w") as f:
        f.write(f"== {name}, rank {rank} of {world}\n" + "\n".join(log) + "\n")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="CPU module and gloo at world 2 (default: GPU, RCCL at world 1)")
    ap.add_argument("--out", default="call_order.txt")
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per executor")
    ap.add_argument("--executor", help=argparse.SUPPRESS)  # (child process: run this one)
    a = ap.parse_args()
    if a.executor:
        run_one(a.executor, a.cpu, a.out)
        return 0
    chunks = []
    for name, (mode, *_) in (CPU_EXECUTORS if a.cpu else GPU_EXECUTORS).items():
        world = 2 if a.cpu and mode != "local" else 1
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        with tempfile.TemporaryDirectory() as tmp:
            procs = []
            for r in range(world):
                env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK=str(r),
                           MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
                cmd = [sys.executable, os.path.abspath(__file__), "--executor", name, "--out",
                       os.path.join(tmp, f"rank{r}.txt")] + (["--cpu"] if a.cpu else [])
                procs.append(subprocess.Popen(cmd, env=env))
            try:
                codes = [p.wait(timeout=a.timeout) for p in procs]
            except subprocess.TimeoutExpired:
                codes = [124]
            finally:
                for p in procs:
                    if p.poll() is None:
                        p.kill()
                        p.wait()
            if any(codes):
                print(f"{name}: exit codes {codes}; stopping", file=sys.stderr)
                return 1
            for r in range(world):
                with open(os.path.join(tmp, f"rank{r}.txt")) as f:
                    chunks.append(f.read())
        print(f"{name}: {sum(c.count(chr(10)) for c in chunks[-world:])} lines", flush=True)
    with open(a.out, "w") as f:
        f.write("".join(chunks))
    return 0


if __name__ == "__main__":
    sys.exit(main())
