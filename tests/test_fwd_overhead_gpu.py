"""The forward's per-example overhead work (hip/fm_fwd.hip): DPP / permlane reductions, the loss and
dpred computed lane-parallel once per 64 examples of a wave, and the all-ones-x instantiations.

All three leave the forward's results bit for bit what they were, so the checks are exact:

* the new butterfly sums against the ``__shfl_xor`` ones on hostile floats (``fwd_reduce_probe``);
* ``vals=None`` against ``vals=ones``;
* every output against the ones the kernels gave before the change, recorded once on an MI355X
  under ``tests/golden/fwd_overhead/`` (``PYTHONPATH=. python tests/test_fwd_overhead_gpu.py --record``
  on the commit before the change wrote them; the inputs are regenerated from seeds);
* and, loosely, against the fp64 formula.

The kernels are launched through the binding with a grid of one workgroup as well as the default
one: at B = 300 a wave of the single workgroup sees 75 examples, so the 64-example flush of the
parked predictions runs mid-loop and at the end.
"""

import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

from fast_tffm_amd.models.table import FMTable
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.ops import native

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fwd_overhead", "parent_outputs.npz")
V = 1000
BS = (1, 5, 67, 300)
FEATS = (39, 0, 1, 64, 65, 130)          # per example, cycled: 64-wide pieces and wrapped slots
KPS = (16, 64, 128)
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": K.FP8}
# (loss, weights, want_reg): each of logistic / MSE, weights on / off, want_reg on / off
COMBOS = (("logistic", False, False), ("logistic", True, True), ("mse", True, False), ("mse", False, True))
OUTS = ("pred", "r1", "dpred", "loss_partial", "reg_partial")
FULL_B = 67  # one-workgroup cases up to this B keep their arrays in the golden file, the others a digest only


@functools.lru_cache(maxsize=None)
def _table(dname: str, Kp: int) -> FMTable:
    return FMTable(V, Kp, dtype=DTYPES[dname], init_range=0.05, seed=7 + Kp, device="cuda")


@functools.lru_cache(maxsize=None)
def _batch(B: int):
    rs = np.random.RandomState(1234 + B)
    counts = np.array([FEATS[i % len(FEATS)] for i in range(B)], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    nnz = int(offsets[-1])
    rows = rs.randint(0, V, size=nnz).astype(np.int32)
    rows[rs.rand(nnz) < 0.2] = 3          # a hot row
    vals = rs.uniform(0.5, 1.5, size=nnz).astype(np.float32)
    labels = rs.randint(0, 2, size=B).astype(np.float32)
    weights = rs.uniform(0.5, 2.0, size=B).astype(np.float32)
    dev = "cuda"
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    return dict(B=B, offsets=t(offsets), rows=t(rows), vals=t(vals), ones=torch.ones(nnz, device=dev),
                labels=t(labels), weights=t(weights))


@functools.lru_cache(maxsize=None)
def _shard_plan(dname: str, Kp: int, B: int):
    """A self-rows plan: rows become segment ids over the batch's sorted unique keys; the middle half of
    the segments are this rank's own table rows, the others come from gathered wire rows."""
    tb, b = _table(dname, Kp), _batch(B)
    keys, seg = torch.unique(b["rows"].long(), return_inverse=True)
    U = keys.numel()
    wire_v = tb.v[keys].contiguous()
    wire_w = (tb.wx[keys].contiguous()[:, 0] if tb.fp8 else tb.w[keys].contiguous())
    return dict(keys=keys.int().contiguous(), seg=seg.int().contiguous(), u0=U // 4, u1=U - U // 4, wire_v=wire_v,
                wire_w=wire_w)


def _grids(B: int):
    g = native.hip().fwd_grid(max(B, 1))
    return (1,) if g == 1 else (1, g)


def _forward(dname, Kp, B, *, x, loss, weighted, want_reg, grid, shard):
    """One launch of the forward through the binding; every output as a tensor."""
    tb, b = _table(dname, Kp), _batch(B)
    h = native.hip()
    dev = "cuda"
    vals = {"vals": b["vals"], "ones": b["ones"], "none": None}[x]
    pred = torch.zeros(B, device=dev)
    dpred = torch.zeros(B, device=dev)
    r1 = torch.zeros((B, Kp), dtype=K.r1_dtype(tb.dtype), device=dev)
    lp = torch.zeros(grid, device=dev)
    rp = torch.zeros(2 * grid, device=dev)
    lt = K.LOSS_TYPES[loss]
    p = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
    kw = {}
    if shard:
        sp = _shard_plan(dname, Kp, B)
        rows, v, w = sp["seg"], sp["wire_v"], sp["wire_w"]
        kw["self_rows"] = [sp["u0"], sp["u1"], 0, p(sp["keys"]), 0, p(tb.v), tb.v.stride(0), p(tb.w), tb.w.stride(0)]
    else:
        rows, v, w = b["rows"], tb.v, tb.w
    h.fwd(B=B, offsets=p(b["offsets"]), rows=p(rows), vals=p(vals), v=p(v), v_stride=v.stride(0), w=p(w),
          w_stride=w.stride(0), Kp=Kp, dtype=K.dtype_code(tb.dtype), labels=p(b["labels"]),
          weights=p(b["weights"]) if weighted else 0, loss_type=lt, grad_scale=1.0 / B, pred=p(pred), r1=p(r1),
          dpred=p(dpred) if lt else 0, loss_partial=p(lp) if lt else 0, reg_partial=p(rp) if want_reg else 0,
          grid=grid, stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    return dict(pred=pred, r1=r1, dpred=dpred, loss_partial=lp, reg_partial=rp)


def _bits(t: torch.Tensor) -> np.ndarray:
    t = t.contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16).cpu().numpy()


def _golden_cases(dname, Kp, shard):
    for B in BS:
        for ci, (loss, weighted, want_reg) in enumerate(COMBOS):
            for x in ("vals", "none"):
                if x == "none" and ci >= 2:
                    continue
                for grid in _grids(B):
                    key = f"B{B}/{loss}-w{int(weighted)}-r{int(want_reg)}/{x}/g{grid}"
                    yield key, dict(x=x, loss=loss, weighted=weighted, want_reg=want_reg, grid=grid, shard=shard), B


def _digest(out) -> str:
    hsh = hashlib.sha256()
    for name in OUTS:
        hsh.update(_bits(out[name]).tobytes())
    return hsh.hexdigest()


PATHS = [(d, k, s) for d in DTYPES for k in KPS for s in (False, True)]
_ids = [f"{d}-k{k}-{'shard' if s else 'local'}" for d, k, s in PATHS]


def _path_id(dname, Kp, shard) -> str:
    return f"{dname}-k{Kp}-{'shard' if shard else 'local'}"


def _path_record(dname, Kp, shard):
    """(words, digests) of one (dtype, Kp, path): the int32 bits of pred, dpred and the loss / reg partials of
    the small cases on one workgroup, concatenated in case order, and every case's digest over all outputs."""
    words, digests = [], []
    for _key, kw, B in _golden_cases(dname, Kp, shard):
        out = _forward(dname, Kp, B, **kw)
        if B <= FULL_B and kw["grid"] == 1:
            words += [_bits(out[name]).ravel() for name in OUTS if name != "r1"]
        digests.append(_digest(out))
    return np.concatenate(words).astype(np.int32), np.array(digests)


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLD)


@pytest.mark.parametrize("dname,Kp,shard", PATHS, ids=_ids)
def test_forward_bits_are_the_parent_commits(golden, dname, Kp, shard):
    pid = _path_id(dname, Kp, shard)
    words, digests = _path_record(dname, Kp, shard)
    want_words, want_digests = golden[pid + "/words"], golden[pid + "/sha256"]
    assert words.shape == want_words.shape and digests.shape == want_digests.shape
    assert np.array_equal(words, want_words), np.nonzero(words != want_words)[0][:8]
    keys = [k for k, _, _ in _golden_cases(dname, Kp, shard)]
    bad = [k for k, a, b in zip(keys, digests, want_digests) if a != b]
    assert not bad, bad[:8]


@pytest.mark.parametrize("dname,Kp,shard", PATHS, ids=_ids)
def test_all_ones_x_forward_equals_ones_values(dname, Kp, shard):
    for B in BS:
        for loss, weighted, want_reg in COMBOS:
            for grid in _grids(B):
                kw = dict(loss=loss, weighted=weighted, want_reg=want_reg, grid=grid, shard=shard)
                a = _forward(dname, Kp, B, x="none", **kw)
                o = _forward(dname, Kp, B, x="ones", **kw)
                for name in OUTS:
                    assert np.array_equal(_bits(a[name]), _bits(o[name])), (B, loss, weighted, want_reg, grid, name)


@pytest.mark.parametrize("dname,Kp,shard", PATHS, ids=_ids)
def test_forward_matches_fp64_formula(dname, Kp, shard):
    """pred, dpred and the summed loss against the fp64 formula on the stored (dequantised) rows, with the
    tolerances of tests/test_headline_oracle_gpu.py (values rtol 2e-5 / atol 2e-7, loss 1e-5 relative)."""
    tb = _table(dname, Kp)
    vd, wd = tb.dense_v().double(), tb.w.double()
    for B in BS:
        b = _batch(B)
        ex = torch.repeat_interleave(torch.arange(B, device="cuda"), (b["offsets"][1:] - b["offsets"][:-1]).long())
        rows = b["rows"].long()
        for x in ("vals", "none"):
            xs = (b["vals"] if x == "vals" else b["ones"]).double()
            xv = vd[rows] * xs[:, None]
            lin = torch.zeros(B, dtype=torch.float64, device="cuda").index_add(0, ex, wd[rows] * xs)
            s1 = torch.zeros((B, Kp), dtype=torch.float64, device="cuda").index_add(0, ex, xv)
            s2 = torch.zeros((B, Kp), dtype=torch.float64, device="cuda").index_add(0, ex, xv * xv)
            pred = lin + 0.5 * (s1 * s1 - s2).sum(1)
            y = b["labels"].double()
            for loss, weighted, want_reg in COMBOS[:3]:
                wt = b["weights"].double() if weighted else torch.ones_like(y)
                if loss == "mse":
                    l, d = wt * (pred - y) ** 2, 2 * wt * (pred - y)
                else:
                    l = wt * torch.nn.functional.binary_cross_entropy_with_logits(pred, y, reduction="none")
                    d = wt * (torch.sigmoid(pred) - y)
                out = _forward(dname, Kp, B, x=x, loss=loss, weighted=weighted, want_reg=want_reg, grid=1, shard=shard)
                torch.testing.assert_close(out["pred"].double(), pred, rtol=2e-5, atol=2e-7)
                torch.testing.assert_close(out["dpred"].double(), d / B, rtol=2e-5, atol=2e-7)
                got, want = float(out["loss_partial"].double().sum()), float(l.sum())
                assert abs(got - want) <= 1e-5 * abs(want), (B, x, loss, got, want)


def _hostile_floats(n: int) -> torch.Tensor:
    rs = np.random.RandomState(99)
    mag = 10.0 ** rs.uniform(-20, 20, size=n)
    x = (mag * rs.choice([-1.0, 1.0], size=n)).astype(np.float32)
    den = rs.randint(1, 1 << 23, size=n).astype(np.uint32) | (rs.randint(0, 2, size=n).astype(np.uint32) << 31)
    pick = rs.rand(n)
    x = np.where(pick < 0.15, den.view(np.float32), x)                       # denormals, both signs
    x = np.where((pick >= 0.15) & (pick < 0.2), 0.0, x).astype(np.float32)   # zeros
    x[: n // 4] = rs.uniform(-1, 1, size=n // 4).astype(np.float32)          # waves of ordinary values
    x[n // 4: n // 4 + 64] = den[:64].view(np.float32)                       # a wave of denormals only
    return torch.from_numpy(x).cuda()


def test_dpp_and_permlane_sums_equal_the_shuffle_sums():
    """group_sum widths 2..64 and across-groups sums of group widths 1..32: the DPP / permlane-swap
    butterflies against the ``__shfl_xor`` ones, bit for bit."""
    h = native.hip()
    waves = 96
    x = _hostile_floats(waves * 64)
    out = torch.zeros((4, 6, waves * 64), device="cuda")
    h.fwd_reduce_probe(x=x.data_ptr(), waves=waves, out=out.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o = out.view(torch.int32).cpu().numpy()
    for i, width in enumerate((2, 4, 8, 16, 32, 64)):
        assert np.array_equal(o[0, i], o[1, i]), f"group_sum<{width}>"
    for i, lpr in enumerate((1, 2, 4, 8, 16, 32)):
        assert np.array_equal(o[2, i], o[3, i]), f"across_groups_sum<{lpr}>"
    # and the shuffle sums are sums: a wave of ones
    ones = torch.ones(64, device="cuda")
    out1 = torch.zeros((4, 6, 64), device="cuda")
    h.fwd_reduce_probe(x=ones.data_ptr(), waves=1, out=out1.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for i, width in enumerate((2, 4, 8, 16, 32, 64)):
        assert bool((out1[1, i] == width).all())
        assert bool((out1[3, i] == 64 // (width // 2)).all())


def _record(path: str) -> None:
    """Write the golden file from the kernels of the package on the path."""
    import fast_tffm_amd

    rec = {}
    for dname, Kp, shard in PATHS:
        pid = _path_id(dname, Kp, shard)
        rec[pid + "/words"], rec[pid + "/sha256"] = _path_record(dname, Kp, shard)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **rec)
    print(f"recorded {len(rec)} arrays, {os.path.getsize(path)} bytes -> {path}")
    print("from", os.path.dirname(fast_tffm_amd.__file__), native.build_hashes())


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "--record":
        _record(sys.argv[2] if len(sys.argv) > 2 else GOLD)
