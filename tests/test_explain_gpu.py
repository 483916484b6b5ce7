"""Exact per-feature attributions on the GPU (hip/fm_explain.hip): every dtype and lanes-per-row value against
the fp64 oracle within its bound, the sum identity against the GPU forward, the launch's grid stride, strided
and wire-style sources, bitwise determinism, the importance kernel, and the executors."""

import os

import numpy as np
import pytest
import torch

from explain_oracle import (FP8, ROWS, check_bias, check_case, check_importance, check_sum_identity, explain_oracle,
                            make_batch, make_table, table_f64)
from fast_tffm_amd.ops import kernels as K

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp8": FP8}
# lanes per row 1, 1, 2, 4, 4, 8, 16, 32, 32, 64; padded columns / masked lanes at 10 and 100
KS = [1, 4, 8, 10, 16, 32, 64, 100, 128, 256]


def _g(a):
    return None if a is None else torch.from_numpy(a).cuda()


def _grid_case(dtype, Kf, with_vals):
    off, rows, vals = make_batch(seed=Kf, with_vals=with_vals)
    v, w, Kp = make_table(DTYPES[dtype], Kf, device="cuda")
    what = f"gpu {dtype} k{Kf}{'' if with_vals else ' novals'}"
    contrib, pred = K.fm_explain(_g(off), _g(rows), _g(vals), v, w, Kp)
    c, tol = check_case(off, rows, vals, v, w, Kp, contrib, pred, what=what)
    fo = K.fm_forward(_g(off), _g(rows), _g(vals), v, w, Kp, want_r1=False)
    check_sum_identity(off, c, tol, fo.pred, what + " fm_forward")
    bias = torch.tensor([0.375], device="cuda")
    contrib_b, pred_b = K.fm_explain(_g(off), _g(rows), _g(vals), v, w, Kp, bias=bias)
    assert torch.equal(contrib_b, contrib)
    check_bias(off, pred_b, pred, 0.375, what)
    fo_b = K.fm_forward(_g(off), _g(rows), _g(vals), v, w, Kp, want_r1=False, bias=bias)
    check_bias(off, fo_b.pred, fo.pred, 0.375, what + " fm_forward")
    if dtype != "fp8":  # the CPU twin: each side is within the bound of the oracle
        cc, cp = K.fm_explain(torch.from_numpy(off), torch.from_numpy(rows),
                              None if vals is None else torch.from_numpy(vals), v.cpu(), w.cpu(), Kp, threads=2)
        assert (np.abs(cc.double().numpy() - contrib.double().cpu().numpy()) <= 2 * tol).all(), what


@pytest.mark.parametrize("Kf", KS)
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_grid_against_oracle(dtype, Kf):
    _grid_case(dtype, Kf, True)


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_grid_without_values(dtype):
    _grid_case(dtype, 10, False)


def test_more_examples_than_waves():
    """B = 20011 > the launch's 16384 waves (the forward's cap and this launcher's): waves stride."""
    rng = np.random.default_rng(11)
    B = 20011
    lens = rng.integers(0, 9, B)
    off = np.zeros(B + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    rows = rng.integers(0, ROWS, int(off[-1])).astype(np.int32)
    vals = rng.choice(np.array([1.0, -2.5, 0.0, 0.3], dtype=np.float32), rows.size)
    v, w, Kp = make_table(torch.float32, 64, device="cuda")
    assert K.native.hip().fwd_grid(B) * 4 == 16384 < B
    contrib, pred = K.fm_explain(_g(off), _g(rows), _g(vals), v, w, Kp)
    c, tol = check_case(off, rows, vals, v, w, Kp, contrib, pred, what="gpu fp32 k64 B=20011")
    fo = K.fm_forward(_g(off), _g(rows), _g(vals), v, w, Kp, want_r1=False)
    check_sum_identity(off, c, tol, fo.pred, "B=20011 fm_forward")


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_strided_factor_rows(dtype):
    """A v view whose row stride is larger than Kp."""
    off, rows, vals = make_batch(seed=5)
    v, w, Kp = make_table(DTYPES[dtype], 10, device="cuda", row_stride=32)
    assert v.stride(0) == 32 > Kp
    contrib, pred = K.fm_explain(_g(off), _g(rows), _g(vals), v, w, Kp)
    check_case(off, rows, vals, v, w, Kp, contrib, pred, what=f"gpu {dtype} k10 stride 32")


@pytest.mark.parametrize("layout", ["wire", "offset"])
def test_fp8_wire_style_tails(layout):
    """fp8 rows whose [w, scale, |v|^2, .] tails are not a table's: wire rows (factor bytes, then the tail, the
    weight view starting behind the factors) and tails at a column offset of a wider fp32 buffer."""
    off, rows, vals = make_batch(seed=6)
    tv, tw, Kp = make_table(FP8, 100, device="cuda")
    tails = torch.as_strided(tw, (ROWS, 4), (4, 1), tw.storage_offset())
    if layout == "wire":
        fmt = K.WireFormat.make(FP8, Kp)
        buf = fmt.empty(ROWS, "cuda")
        buf[:, :Kp] = tv.view(torch.uint8)
        buf.view(torch.float32)[:, fmt.vb // 4:] = tails
        v, w = fmt.views(buf)
        assert w.stride(0) == fmt.rb // 4 != 4 and w.storage_offset() == fmt.vb // 4
    else:
        wide = torch.zeros((ROWS, 8), dtype=torch.float32, device="cuda")
        wide[:, 4:] = tails
        v, w = tv, wide[:, 4]
        assert w.stride(0) == 8 and w.storage_offset() == 4
    contrib, pred = K.fm_explain(_g(off), _g(rows), _g(vals), v, w, Kp)
    check_case(off, rows, vals, v, w, Kp, contrib, pred, what=f"gpu fp8 k100 {layout} tails")
    ref, ref_pred = K.fm_explain(_g(off), _g(rows), _g(vals), tv, tw, Kp)
    assert torch.equal(contrib, ref) and torch.equal(pred, ref_pred)  # the same bits from either layout


@pytest.fixture(scope="module")
def zipf_batch():
    """A bench-like small batch: B = 4096 examples of 39 features, Zipf(1.1) ids over 100000 rows."""
    rng = np.random.default_rng(17)
    B, F, V = 4096, 39, 100000
    p = np.arange(1, V + 1, dtype=np.float64) ** -1.1
    ids = rng.choice(V, size=B * F, p=p / p.sum()).astype(np.int32)
    off = (np.arange(B + 1) * F).astype(np.int32)
    v, w, Kp = make_table(torch.float32, 64, device="cuda", rows=V, seed=9)
    return off, ids, v, w, Kp


def test_bitwise_repeatable(zipf_batch):
    off, ids, v, w, Kp = zipf_batch
    a, pa = K.fm_explain(_g(off), _g(ids), None, v, w, Kp)
    b, pb = K.fm_explain(_g(off), _g(ids), None, v, w, Kp)
    assert torch.equal(a, b) and torch.equal(pa, pb)


def test_importance_kernel(zipf_batch):
    off, ids, v, w, Kp = zipf_batch
    contrib, _ = K.fm_explain(_g(off), _g(ids), None, v, w, Kp)
    dd = K.dedup(_g(ids), want_perm=True, key_bits=17)
    got = K.feature_importance(contrib, dd)
    cnt = check_importance(ids, contrib.cpu().numpy(), got)
    # one occurrence, packed segments of several rounds, long segments, and one of more than 10000
    assert cnt.min() == 1 and cnt.max() > 10000
    assert ((cnt > 8) & (cnt <= 64)).any() and ((cnt > 64) & (cnt < 1000)).any()
    again = K.feature_importance(contrib, dd)
    assert all(torch.equal(x, y) for x, y in zip(got, again))
    empty = K.feature_importance(torch.empty(0, device="cuda"),
                                 K.dedup(torch.empty(0, dtype=torch.int32, device="cuda"), want_perm=True))
    assert [t.numel() for t in empty] == [0, 0, 0, 0] and empty[2].dtype == torch.float64


# ---- executors ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rccl_ctx():
    from fast_tffm_amd.parallel import dist as fmdist
    from ports import free_port

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(free_port())
    ctx = fmdist.init_distributed(backend="nccl", rank=0, world=1, device="cuda:0", force_pg=True)
    yield ctx
    fmdist.shutdown()


@pytest.mark.parametrize("w1_local", [True, False], ids=["default", "emit"])
@pytest.mark.parametrize("dtype", list(DTYPES))
def test_sharded_explain_equals_local(rccl_ctx, dtype, w1_local, monkeypatch):
    from fast_tffm_amd.data.synthetic import CriteoSynth
    from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig

    if not w1_local:
        monkeypatch.setenv("FM_SHARD_W1_LOCAL", "0")
    V, Kf = 20000, 16
    gen = CriteoSynth(V, device="cuda", seed=23)
    batches = [gen.batch(512) for _ in range(3)]

    def cfg(mode):
        return FMConfig(vocabulary_size=V, factor_num=Kf, loss_type="logistic", init_value_range=0.3, seed=3,
                        opt=K.OptConfig("adagrad", lr=0.05), batch_size=512, factor_lambda=0.01, bias_lambda=0.01,
                        mode=mode, dtype=DTYPES[dtype], global_bias=True)

    loc = FactorizationMachine(cfg("local"), device="cuda")
    dm = FactorizationMachine(cfg("shard"), device="cuda", dist=rccl_ctx)
    try:
        assert torch.equal(dm.table.v.view(torch.uint8), loc.table.v.view(torch.uint8))  # (the same seeded init)
        b = batches[1]
        c_loc, p_loc = loc.explain(b)
        c_sh, p_sh = dm.explain(b)
        if dtype == "fp32":  # default wire dtype: the table's bits
            assert torch.equal(c_sh, c_loc) and torch.equal(p_sh, p_loc)
        off, ids = b.offsets.cpu().numpy(), b.ids.cpu().numpy()
        vals = None if b.vals is None else b.vals.cpu().numpy()
        for m, c_m, what in ((loc, c_loc, "local"), (dm, c_sh, "shard")):
            t = m.table
            V64, w64, n2 = table_f64(t.v[:V], t.w[:V], t.Kp)
            c, tol = explain_oracle(off, ids, vals, V64, w64, n2)
            assert (np.abs(c_m.double().cpu().numpy() - c) <= tol).all(), (dtype, what)
        # the plan slots were left in order: the next steps still equal the local ones
        for i in (0, 1, 2):
            l1 = loc.train_step(batches[i]).mean_loss()
            l2 = dm.train_step(batches[i], batches[i + 1] if i + 1 < len(batches) else None).mean_loss()
            assert abs(l1 - l2) <= 1e-5 * max(1.0, abs(l1))
        torch.cuda.synchronize()
        torch.testing.assert_close(dm.table.reference_rows(), loc.table.reference_rows(), rtol=1e-5, atol=1e-6)
    finally:
        dm.close()
        loc.close()
