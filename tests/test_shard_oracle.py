"""The references of tests/shard_oracle.py on hand-written cases whose answers are written out,
make_runs' overlap guarantee for every run shape, and the size of the FTRL exclusion set of the
owner-apply cases of tests/test_shard_kernels_gpu.py: the references are right, and within their
own conditions, before a kernel is compared with them."""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import shard_oracle as O
import test_shard_kernels_gpu as T

# W = 3 with an empty middle run, 7 requests; a previous step of 5 requests, its middle run empty too
REQ = np.array([2, 5, 9, 1, 5, 7, 9], np.int32)
OFF = np.array([0, 3, 3, 7], np.int32)
PREV = np.array([5, 8, 0, 1, 9], np.int32)
POFF = np.array([0, 2, 2, 5], np.int32)


def test_member():
    assert O.member(REQ, PREV, POFF).tolist() == [0, 1, 1, 1, 1, 0, 1]
    assert O.member(REQ, PREV, np.array([0, 2], np.int32)).tolist() == [0, 1, 0, 0, 1, 0, 0]  # run 0 alone
    assert O.member(REQ[:0], PREV, POFF).tolist() == []


def test_dirty():
    flag, cnt = O.dirty(REQ, OFF, PREV, POFF, None)
    assert flag.tolist() == [0, 1, 1, 1, 1, 0, 1] and cnt.tolist() == [2, 0, 3]
    flag, cnt = O.dirty(REQ, OFF, PREV, POFF, (0, 3))  # the first run skipped
    assert flag.tolist() == [0, 0, 0, 1, 1, 0, 1] and cnt.tolist() == [0, 0, 3]
    flag, cnt = O.dirty(REQ, OFF, PREV, POFF, (3, 7))  # the last run skipped
    assert flag.tolist() == [0, 1, 1, 0, 0, 0, 0] and cnt.tolist() == [2, 0, 0]
    flag, cnt = O.dirty(REQ, OFF, PREV, POFF, (3, 3))  # an empty range
    assert flag.tolist() == [0, 1, 1, 1, 1, 0, 1] and cnt.tolist() == [2, 0, 3]


def test_excl():
    assert O.excl(REQ, OFF, 0).tolist() == [1, 0, 0]
    assert O.excl(REQ, OFF, 1).tolist() == []
    assert O.excl(REQ, OFF, 2).tolist() == [1, 0, 1, 0]


def test_tags():
    assert O.tags(np.array([0, 2, 3, 6]), OFF).tolist() == [0, 2, 0, 3]
    assert O.tags(np.array([0, 2]), np.array([0, 0, 3, 3])).tolist() == [0, 2]  # empty runs at both ends
    assert O.tags(np.array([], np.int64), OFF).tolist() == []


def _f32_bits(x: float) -> int:
    b = int(np.array([x], np.float32).view(np.int32)[0])
    return b


def test_wire_rows_fp32_table_on_a_bf16_wire():
    # 1 + 2^-8 is a tie and goes to the even 1; 1 + 3 * 2^-8 is a tie and goes up to the even 1 + 2^-6
    v = torch.tensor([[0.0, 0.0, 0.0, 0.0], [1.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -2.0]])
    tab = SimpleNamespace(v=v, w=torch.tensor([0.25, 0.5]), wx=None)
    fmt = SimpleNamespace(dtype=torch.bfloat16, Kp=4)
    vb, tail = O.wire_rows(tab, fmt, [1, 0, 1], tag=[7, 8, 9])
    row1 = [0x80, 0x3F, 0x80, 0x3F, 0x82, 0x3F, 0x00, 0xC0]
    assert vb.dtype == np.uint8 and vb.tolist() == [row1, [0] * 8, row1]
    assert tail.tolist() == [[0x3F000000, 0, 0, 7], [0x3E800000, 0, 0, 8], [0x3F000000, 0, 0, 9]]
    assert O.wire_rows(tab, fmt, [0])[1].tolist() == [[0x3E800000, 0, 0, 0]]  # no tag: 0


def test_wire_rows_storage_bits():
    bf = SimpleNamespace(v=torch.tensor([[1.0, -2.0, 0.5, 3.0]], dtype=torch.bfloat16), w=torch.tensor([2.0]), wx=None)
    vb, tail = O.wire_rows(bf, SimpleNamespace(dtype=torch.bfloat16, Kp=2), [0])
    assert vb.tolist() == [[0x80, 0x3F, 0x00, 0xC0]] and tail.tolist() == [[0x40000000, 0, 0, 0]]
    raw = torch.tensor([[0x38, 0xB8, 0x00, 0x7E], [1, 2, 3, 4]], dtype=torch.uint8)
    wx = torch.tensor([[0.25, 0.5, 3.0, 99.0], [1.0, 2.0, 4.0, 98.0]])
    f8 = SimpleNamespace(v=raw.view(torch.float8_e4m3fn), w=wx[:, 0], wx=wx)
    vb, tail = O.wire_rows(f8, SimpleNamespace(dtype=torch.float8_e4m3fn, Kp=4), [1, 0], tag=[5, 6])
    assert vb.tolist() == [[1, 2, 3, 4], [0x38, 0xB8, 0x00, 0x7E]]
    assert tail.tolist() == [[_f32_bits(1.0), _f32_bits(2.0), _f32_bits(4.0), 5],
                             [_f32_bits(0.25), _f32_bits(0.5), _f32_bits(3.0), 6]]


def test_fp8_values():
    lut = O.fp8_e4m3_values()
    assert lut[0x38] == 1.0 and lut[0xB8] == -1.0 and lut[0x7E] == 448.0 and lut[0x01] == 2.0 ** -9
    assert lut[0x08] == 2.0 ** -6 and lut[0x00] == 0.0 and math.isnan(lut[0x7F]) and math.isnan(lut[0xFF])
    ok = ~np.isnan(lut)
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float().numpy()
    assert np.array_equal(lut[ok], ref[ok])


def test_opt_reference():
    one = lambda x: torch.tensor([[x]], dtype=torch.float64)  # noqa: E731
    p, s0, s1 = O.opt_reference("sgd", one(1.0), None, None, one(2.0), 0.05)
    assert float(p) == pytest.approx(0.9, abs=1e-15) and s0 is None and s1 is None
    p, s0, s1 = O.opt_reference("adagrad", one(1.0), one(0.1), None, one(2.0), 0.05)
    assert float(s0) == pytest.approx(4.1, abs=1e-15) and s1 is None
    assert float(p) == pytest.approx(1.0 - 0.05 * 2.0 / math.sqrt(4.1), abs=1e-15)
    p, n, z = O.opt_reference("ftrl", one(0.5), one(0.1), one(0.0), one(2.0), 0.1, 0.01, 0.02, 1.0)
    z_want = 2.0 - (math.sqrt(4.1) - math.sqrt(0.1)) / 0.1 * 0.5
    assert float(n) == pytest.approx(4.1, abs=1e-15) and float(z) == pytest.approx(z_want, abs=1e-14)
    assert z_want < -0.01
    assert float(p) == pytest.approx((-0.01 - z_want) / ((1.0 + math.sqrt(4.1)) / 0.1 + 0.04), abs=1e-15)
    p, n, z = O.opt_reference("ftrl", one(0.0), one(0.1), one(0.0), one(0.001), 0.1, 0.01, 0.02, 1.0)
    assert float(z) == pytest.approx(0.001, abs=1e-15) and float(p) == 0.0  # |z| <= l1


def test_apply_reference_sums_every_run_and_keeps_rows():
    # rows 5 and 9 come twice (both runs), row 2 is kept back
    st = dict(v=torch.zeros(10, 4), w=torch.zeros(10), s0v=None, s0w=None, s1v=None, s1w=None)
    grad = torch.arange(7 * 6, dtype=torch.float32).reshape(7, 6)
    rows, p, n, z, near = O.apply_reference("sgd", st, REQ, grad, 4, 1.0, keep_rows=[2])
    assert rows.tolist() == [1, 5, 7, 9] and n is None and z is None and not bool(near.any())
    want = -torch.stack([grad[3], grad[1] + grad[4], grad[5], grad[2] + grad[6]])[:, :5].double()
    assert torch.equal(p, want)


@pytest.mark.parametrize("shape", list(O.SHAPES))
def test_make_runs_shapes_and_overlap(shape):
    s = O.SHAPES[shape]
    for seed in range(5):
        for rows in (1000, 1200, 2000, 5000):
            req, splits, off = O.shape_runs(shape, seed, rows)
            assert req.dtype == np.int32 and off.dtype == np.int32 and len(splits) == s["W"] == len(off) - 1
            assert off[0] == 0 and np.array_equal(np.diff(off), splits) and off[-1] == len(req)
            assert req.min() >= 0 and req.max() < rows
            uniq, cnt = np.unique(req, return_counts=True)
            for q, n in enumerate(splits):
                run = req[off[q]:off[q + 1]]
                assert (n == 0) == (q in s["empty"]) and (n == 0 or s["lo"] <= n <= s["hi"])
                assert np.all(np.diff(run) > 0)
            if s["W"] - len(s["empty"]) >= 2:
                assert 3 * int((cnt >= 2).sum()) >= len(uniq)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [4, 64, 100])
@pytest.mark.parametrize("shape", list("ACDE"))
def test_ftrl_exclusion_stays_under_one_percent(shape, k, dtype):
    """The owner-apply cases' seeds: fewer than 1 % of the reference's elements lie within 1e-4 of
    FTRL's |z| = l1 discontinuity (they are left out of the comparison of p)."""
    req, splits, off, opt, tab, grad = T.apply_case(shape, "ftrl", k, dtype, "cpu")
    rows, p, n, z, near = T._reference(opt, T._snap(tab), req, grad, tab.Kp)
    assert near.shape == (len(np.unique(req)), tab.Kp + 1)
    assert float(near.double().mean()) < 0.01
    assert bool(((z.abs() > opt.l1) == (p != 0)).all())
