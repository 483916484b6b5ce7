"""The owner-side kernels of the row-sharded exchange (csrc/hip/shard.hip) against the plain
references of tests/shard_oracle.py, called through the ``ops.kernels`` wrappers at the shapes
the end-to-end tests never produce: empty runs in front of and behind non-empty ones, 64 runs,
wire rows whose v section is no multiple of 16 bytes, skip ranges at both ends, a device count
above its cap, a non-zero ``row0``.  Integer outputs and copied bits are compared exactly, the
owner apply with an fp64 optimizer step.  Wrappers with a CPU path run on the CPU too.
"""

import zlib

import numpy as np
import pytest
import torch

from fast_tffm_amd.models.table import FMTable
from fast_tffm_amd.ops import kernels as K

import shard_oracle as O

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
gpu = pytest.mark.gpu

KS = [4, 10, 16, 64, 100, 128]
SENT = -7777          # int sentinel of prefilled outputs
SENT_BYTE = 0xA5      # byte sentinel of prefilled row buffers
OPTS = {
    "adagrad": K.OptConfig("adagrad", lr=0.05),
    "ftrl": K.OptConfig("ftrl", lr=0.1, l1=0.01, l2=0.02, beta=1.0),
    "sgd": K.OptConfig("sgd", lr=0.05),
}
FIELDS = ("v", "w", "s0v", "s0w", "s1v", "s1w")


def _seed(*parts) -> int:
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def _t(a, device, dtype=np.int32) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.detach().cpu().numpy()


def _bytes(t: torch.Tensor) -> np.ndarray:
    """The stored bytes of a tensor's rows: uint8 [rows, bytes per row]."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.uint8).numpy().reshape(t.shape[0] if t.dim() else 1, -1)


def _table(rows, k, dtype, opt, seed, device):
    return FMTable(rows, k, dtype=dtype, opt=opt, init_range=0.05, seed=seed, device=device)


def _sync(device):
    if device == "cuda":
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# searches and compaction: integers, exact
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("shape", list("ABCDE"))
def test_run_member(device, shape):
    """3000 requests, about half of them rows of ``prev`` (runs of every shape), against np.isin."""
    rows = 5000
    prev, psplits, poff = O.shape_runs(shape, _seed("member", shape), rows)
    rng = np.random.default_rng(_seed("member-req", shape))
    req = np.concatenate([rng.choice(prev, 1500), rng.integers(0, rows, 1500)]).astype(np.int32)
    rng.shuffle(req)
    want = O.member(req, prev, poff)
    assert 1400 <= int(want.sum()) < 3000
    got = K.run_member(_t(req, device), _t(prev, device), _t(poff, device), psplits)
    assert got.dtype == torch.int32 and np.array_equal(_np(got), want)


@pytest.mark.parametrize("device", DEVICES)
def test_run_member_no_requests(device):
    prev, psplits, poff = O.shape_runs("C", 1, 5000)
    got = K.run_member(torch.empty(0, dtype=torch.int32, device=device), _t(prev, device), _t(poff, device), psplits)
    assert got.numel() == 0 and got.dtype == torch.int32


def _me_list(splits):
    """First, middle and last run, and an empty run where the shape has one."""
    W = len(splits)
    mes = {0, W // 2, W - 1}
    empty = [q for q, n in enumerate(splits) if n == 0]
    if empty:
        mes.add(empty[0])
    return sorted(mes)


@gpu
@pytest.mark.parametrize("shape", list("BCDE"))
def test_self_excl(shape):
    """Rows of run ``me`` that no other run holds; entries of ``out`` past the run stay untouched."""
    req, splits, off = O.shape_runs(shape, _seed("excl", shape), 5000)
    W = len(splits)
    req_t, off_t = _t(req, "cuda"), _t(off, "cuda")
    seen_empty = False
    for me in _me_list(splits):
        n = splits[me]
        seen_empty |= n == 0
        out = torch.full((n + 7,), SENT, dtype=torch.int32, device="cuda")
        K.self_excl(req_t, W, off_t, me, n, out)
        got = _np(out)
        want = O.excl(req, off, me)
        assert np.array_equal(got[:n], want), (shape, me)
        assert np.all(got[n:] == SENT), (shape, me)
        if n >= 100 and sum(s > 0 for s in splits) >= 2:
            assert 0 < int(want.sum()) < n  # the runs overlap: both answers occur
    assert seen_empty or shape == "D"


def _skips(splits, off):
    """None, each of the first / middle / last run as the skip range, and an empty range."""
    W = len(splits)
    R = int(off[-1])
    out = [None] + [(int(off[q]), int(off[q + 1])) for q in sorted({0, W // 2, W - 1})]
    return out + [(R // 2, R // 2)]


@gpu
@pytest.mark.parametrize("nxt,prv", [("A", "A"), ("C", "D"), ("D", "C"), ("E", "E"), ("B", "E")])
def test_dirty_scan(nxt, prv):
    """Dirty flags and per-run counts of the next step's requests, for every skip range.  All
    calls share one ``dcount`` buffer, and every call is made twice: the launch clears the counts
    itself, and the word behind them is not its to write."""
    rows = 1200  # (a small range: the two steps share many rows)
    req, splits, off = O.shape_runs(nxt, _seed("dirty-next", nxt, prv), rows)
    prev, psplits, poff = O.shape_runs(prv, _seed("dirty-prev", nxt, prv), rows)
    W, Wp, R = len(splits), len(psplits), len(req)
    dev = "cuda"
    req_t, off_t, prev_t, poff_t = _t(req, dev), _t(off, dev), _t(prev, dev), _t(poff, dev)
    dcount = torch.full((W + 1,), SENT, dtype=torch.int32, device=dev)
    for skip in _skips(splits, off):
        want_flag, want_cnt = O.dirty(req, off, prev, poff, skip)
        if skip is None:
            assert 0 < int(want_flag.sum()) < R
        for _ in range(2):
            flag = torch.full((R,), SENT, dtype=torch.int32, device=dev)
            K.dirty_scan(req_t, off_t, W, prev_t, poff_t, Wp, flag, dcount, skip=skip)
            assert np.array_equal(_np(flag), want_flag), (skip,)
            assert np.array_equal(_np(dcount)[:W], want_cnt), (skip, _np(dcount)[:W], want_cnt)
            assert int(dcount[W]) == SENT


@gpu
def test_dirty_scan_rejects_65_runs():
    """More runs than the kernel's shared counters (kMaxRuns = 64): refused before any launch."""
    W = 65
    req = torch.arange(W, dtype=torch.int32, device="cuda")
    off = torch.arange(W + 1, dtype=torch.int32, device="cuda")
    flag = torch.full((W,), SENT, dtype=torch.int32, device="cuda")
    dcount = torch.full((W,), SENT, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError):
        K.dirty_scan(req, off, W, req, off, W, flag, dcount)
    torch.cuda.synchronize()
    assert bool((flag == SENT).all()) and bool((dcount == SENT).all())


@gpu
@pytest.mark.parametrize("pattern", ["zero", "set", "random", "values"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 20000])
def test_select_flagged(n, pattern):
    """out[:count] = the ascending positions of the non-zero flags (any non-zero value counts)."""
    rng = np.random.default_rng(_seed("select", n, pattern))
    if pattern == "zero":
        flag = np.zeros(n, np.int32)
    elif pattern == "set":
        flag = np.ones(n, np.int32)
    else:
        flag = (rng.random(n) < 0.4).astype(np.int32)
        if pattern == "values":
            flag *= rng.choice(np.array([-1, 2, 1 << 30], np.int32), n)
    want = np.flatnonzero(flag)
    out = torch.full((max(n, 1),), SENT, dtype=torch.int32, device="cuda")
    count = torch.full((1,), SENT, dtype=torch.int32, device="cuda")
    K.select_flagged(_t(flag, "cuda"), out, count, K.select_workspace(n, "cuda"))
    c = int(count)
    assert c == len(want)
    got = _np(out)
    assert np.array_equal(got[:c], want)
    assert np.all(got[c:] == SENT)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("W", [1, 2, 3, 8])
def test_shard_keys(device, W):
    Rps = 613
    rng = np.random.default_rng(W)
    ids = rng.integers(0, W * Rps, 3000).astype(np.int32)
    ids[5], ids[-1] = 0, W * Rps - 1
    out = torch.full((3000,), SENT, dtype=torch.int32, device=device)
    got = K.shard_keys(_t(ids, device), W, Rps, out)
    assert np.array_equal(_np(got), (ids % W) * Rps + ids // W)


@gpu
@pytest.mark.parametrize("width", [8, 20, 132])
@pytest.mark.parametrize("count", [0, 1, 37, 100, 250])
def test_zero_listed_rows(width, count):
    """Exactly the first min(count, max_n) listed rows are cleared; a device count above the cap
    clears the 100 listed rows and nothing else."""
    g = torch.Generator().manual_seed(width * 1000 + count)
    buf = torch.randn((300, width), generator=g).cuda()
    before = _bytes(buf).copy()
    rows = torch.randperm(300, generator=g)[:100].to(torch.int32)
    K.zero_listed_rows(buf, rows.cuda(), torch.tensor([count], dtype=torch.int32, device="cuda"), 100)
    after = _bytes(buf)
    cleared = np.zeros(300, bool)
    cleared[rows.numpy()[: min(count, 100)]] = True
    assert np.all(after[cleared] == 0)
    assert np.array_equal(after[~cleared], before[~cleared])


# ---------------------------------------------------------------------------
# gathers: bitwise
# ---------------------------------------------------------------------------
T_ROWS = 1000  # rows of the gathers' tables


def _skip_ranges(R):
    n, a, b = R // 5, R // 3, R // 3 + R // 4
    return [None, (0, n), (R - n, R), (a, b), (0, R)]


def _dense_rows(tab) -> np.ndarray:
    """fp32 [rows, Kp + 4] = [v dequantised | w | 0 0 0] of a table, from its stored bytes."""
    v = tab.v.detach().cpu()
    if tab.fp8:
        scale = _np(tab.wx)[:, 1]
        mant, _ = np.frexp(scale)
        assert np.all(mant == 0.5)  # powers of two: byte value * scale is exact in fp32
        vals = O.fp8_e4m3_values()[v.view(torch.uint8).numpy()] * scale[:, None]
    else:
        vals = v.float().numpy()
    out = np.zeros((tab.rows, tab.Kp + 4), np.float32)
    out[:, : tab.Kp] = vals
    out[:, tab.Kp] = _np(tab.w)
    return out


GATHER_TABLES = [pytest.param(dev, dt, id=f"{did}-{n}", marks=[pytest.mark.gpu] if dev == "cuda" else [])
                 for dev, did in (("cpu", "cpu"), ("cuda", "gpu"))
                 for dt, n in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"), (K.FP8, "fp8"))
                 if not (dev == "cpu" and dt == K.FP8)]  # (fp8 tables are a GPU path)


@pytest.mark.parametrize("device,dtype", GATHER_TABLES)
@pytest.mark.parametrize("k", KS)
def test_gather_rows(device, dtype, k):
    """Every row once, one row 500 times and random rows, with every skip range (GPU): the gathered
    rows are the table's values bit for bit, skipped rows are not written."""
    tab = _table(T_ROWS, k, dtype, OPTS["adagrad"], _seed("gather", k) % 997, device)
    Kp = tab.Kp
    dense = _dense_rows(tab)
    assert np.count_nonzero(dense[:, :k]) > 0.9 * dense[:, :k].size
    rng = np.random.default_rng(_seed("gather-req", k, str(dtype)))
    reqs = [np.arange(T_ROWS), np.full(500, int(rng.integers(0, T_ROWS))), rng.integers(0, T_ROWS, 777)]
    for req in reqs:
        R = len(req)
        for skip in _skip_ranges(R) if device == "cuda" else [None]:
            out = torch.empty((R, Kp + 4), dtype=torch.float32, device=device)
            out.view(torch.int32).fill_(SENT)
            K.gather_rows(_t(req, device), tab.state, Kp, out, skip=skip)
            got = _np(out).view(np.int32)
            want = dense[req].view(np.int32).copy()
            if skip is not None:
                want[skip[0]:skip[1]] = SENT
            assert np.array_equal(got, want), (R, skip)


WIRES = [pytest.param(torch.float32, "bf16", id="fp32-bf16"), pytest.param(torch.bfloat16, "storage", id="bf16"),
         pytest.param(K.FP8, "storage", id="fp8"), pytest.param(torch.float32, "fp32", id="fp32-fp32")]


def _wire_check(out, fmt, n, want_v, want_tail, written):
    """Value bytes and tail words of the written rows; unwritten rows keep the sentinel."""
    got = _bytes(out)[:n]
    assert got.shape[1] == fmt.rb
    nv = want_v.shape[1]
    assert nv <= fmt.vb
    assert np.array_equal(got[written, :nv], want_v[written])
    tail = np.ascontiguousarray(got[:, fmt.vb:fmt.vb + 16]).view(np.int32)
    assert np.array_equal(tail[written], want_tail[written])
    assert np.all(got[~written] == SENT_BYTE)


@gpu
@pytest.mark.parametrize("dtype,comm", WIRES[:3])
@pytest.mark.parametrize("k", KS)
def test_gather_wire_plain(dtype, comm, k):
    """Wire rows of random requests with every skip range: stored bits (fp32 on a bf16 wire: torch's
    rounding; an fp32 table whose Kp is no multiple of 8 stays on an fp32 wire), tail [w, scale, norm]
    and a zero tag."""
    tab = _table(T_ROWS, k, dtype, OPTS["adagrad"], _seed("wire", k) % 997, "cuda")
    fmt = K.WireFormat.make(dtype, tab.Kp, comm)
    rng = np.random.default_rng(_seed("wire-req", k, comm))
    req = rng.integers(0, T_ROWS, 777).astype(np.int32)
    R = len(req)
    want_v, want_tail = O.wire_rows(tab, fmt, req)
    assert np.count_nonzero(want_v) > want_v.size // 2
    for skip in _skip_ranges(R):
        out = fmt.empty(R, "cuda")
        out.view(torch.uint8).fill_(SENT_BYTE)
        K.gather_wire(_t(req, "cuda"), tab.state, fmt, out, skip=skip)
        written = np.ones(R, bool)
        if skip is not None:
            written[skip[0]:skip[1]] = False
        _wire_check(out, fmt, R, want_v, want_tail, written)


def _subsets(rng, R):
    """idx lists of a patch gather: a random ascending subset, none, and every request."""
    return [np.sort(rng.choice(R, R // 3, replace=False)), np.zeros(0, np.int64), np.arange(R)]


@gpu
@pytest.mark.parametrize("dtype,comm", WIRES)
@pytest.mark.parametrize("k", KS)
def test_gather_wire_tagged(dtype, comm, k):
    """Patch gathers: row p is req[idx[p]], tagged with its position in its source's run, for runs
    with empty ones in front, between and behind and for 64 runs."""
    tab = _table(T_ROWS, k, dtype, OPTS["adagrad"], _seed("wire", k) % 997, "cuda")
    fmt = K.WireFormat.make(dtype, tab.Kp, comm)
    for shape in "BCDE":
        req, splits, off = O.shape_runs(shape, _seed("tagged", shape, k), T_ROWS)
        W, R = len(splits), len(req)
        rng = np.random.default_rng(_seed("tagged-idx", shape, k, comm))
        for idx in _subsets(rng, R):
            D = len(idx)
            out = fmt.empty(D + 3, "cuda")
            out.view(torch.uint8).fill_(SENT_BYTE)
            K.gather_wire(_t(req, "cuda"), tab.state, fmt, out, idx=_t(idx, "cuda"), run_off=_t(off, "cuda"), W=W)
            tag = O.tags(idx, off)
            want_v, want_tail = O.wire_rows(tab, fmt, req[idx], tag=tag)
            written = np.arange(D + 3) < D
            pad = D + 3 - len(want_v)
            _wire_check(out, fmt, D + 3, np.pad(want_v, ((0, pad), (0, 0))), np.pad(want_tail, ((0, pad), (0, 0))),
                        written)
            if D == R and shape != "B":
                assert len(np.unique(tag)) > 1 and int(tag.max()) == max(splits) - 1


def _bf16_edge_values() -> torch.Tensor:
    """fp32 [8, 16]: exact ties, overflow to inf, zeros, infs, denormals and values around the
    smallest bf16 normal and subnormal; element [7, 15] is a NaN."""
    t = 2.0 ** -126  # the smallest normal of fp32 and of bf16
    edge = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -23,
            1 + 2.0 ** -8 - 2.0 ** -23, 3.4028234663852886e38, -3.4028234663852886e38, 3.3895313892515355e38,
            0.0, -0.0, float("inf"), float("-inf"), 2.0 ** -149, -(2.0 ** -149), t - 2.0 ** -149, t * (1 - 2.0 ** -9),
            t * (1 - 2.0 ** -8), -t * (1 - 2.0 ** -10), t, 2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134, 2.0 ** -135,
            -(2.0 ** -134), 65280.0, 65408.0, 1.0, -1.0, 0.1, 1e-40, -1e-40]
    g = torch.Generator().manual_seed(5)
    v = torch.randn(128, generator=g) * torch.logspace(-30, 30, 128)
    v[: len(edge)] = torch.tensor(edge, dtype=torch.float64).float()
    v[127] = float("nan")
    return v.view(8, 16)


@gpu
def test_gather_wire_bf16_rounding_edges():
    """f32_to_bf16_bits (round to nearest even, overflow to inf, denormals kept) against torch's
    conversion bit for bit, and against the literal bits of the ties; the NaN stays a NaN."""
    tab = _table(8, 16, torch.float32, OPTS["adagrad"], 1, "cuda")
    vals = _bf16_edge_values()
    tab.v.copy_(vals)
    fmt = K.WireFormat.make(torch.float32, 16, "bf16")
    assert fmt.dtype == torch.bfloat16
    req = np.arange(8, dtype=np.int32)
    out = fmt.empty(8, "cuda")
    out.view(torch.uint8).fill_(SENT_BYTE)
    K.gather_wire(_t(req, "cuda"), tab.state, fmt, out)
    got = np.ascontiguousarray(_bytes(out)[:, :32]).view(np.uint16).reshape(-1)
    want = vals.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16).reshape(-1)
    assert np.array_equal(got[:127], want[:127]), [(i, hex(a), hex(b)) for i, (a, b) in
                                                   enumerate(zip(got[:127], want[:127])) if a != b]
    assert (got[127] & 0x7F80) == 0x7F80 and (got[127] & 0x7F) != 0  # NaN
    assert [hex(x) for x in got[:4]] == ["0x3f80", "0x3f82", "0xbf80", "0xbf82"]
    assert got[6] == 0x7F80 and got[7] == 0xFF80 and got[9] == 0 and got[10] == 0x8000
    assert got[13] == 0 and got[21] == 0 and got[22] == 2 and got[19] == 0x0080
    want_v, want_tail = O.wire_rows(tab, fmt, req)
    assert np.array_equal(_bytes(out)[:, :32][:, :30], want_v[:, :30])  # (all but the NaN's two bytes)
    assert np.array_equal(np.ascontiguousarray(_bytes(out)[:, 32:48]).view(np.int32), want_tail)


@gpu
@pytest.mark.parametrize("shape", ["C", "E"])
@pytest.mark.parametrize("dtype,k,rb", [(torch.bfloat16, 16, 48), (K.FP8, 128, 144)], ids=["bf16-k16", "fp8-k128"])
def test_patch_scatter_closes_the_loop(shape, dtype, k, rb):
    """Requester side of the early exchange: the tagged patch rows of every owner land on that
    owner's block of ``gathered`` at their tags, over the stale copies; no other row changes.
    Owners with no requests and owners with requests but no patch are both present; the blocks
    of ``gathered`` are spaced apart, so ``sc_start`` differs from the run offsets."""
    dev = "cuda"
    fresh = _table(T_ROWS, k, dtype, OPTS["adagrad"], 11, dev)
    stale = _table(T_ROWS, k, dtype, OPTS["adagrad"], 12, dev)
    fmt = K.WireFormat.make(dtype, fresh.Kp, "storage")
    assert fmt.rb == rb
    req, splits, off = O.shape_runs(shape, _seed("patch", shape), T_ROWS)
    W, R = len(splits), len(req)
    rng = np.random.default_rng(_seed("patch-idx", shape, k))
    idx = np.sort(rng.choice(R, R // 3, replace=False))
    clean = [q for q in range(W) if splits[q]][1]  # an owner with requests and no dirty row
    idx = idx[(idx < off[clean]) | (idx >= off[clean + 1])]
    D = len(idx)
    recv = fmt.empty(D, dev)
    K.gather_wire(_t(req, dev), fresh.state, fmt, recv, idx=_t(idx, dev), run_off=_t(off, dev), W=W)
    owner = np.searchsorted(off, idx, side="right") - 1
    counts = np.bincount(owner, minlength=W)
    assert counts[clean] == 0 and np.all(counts[np.array(splits) == 0] == 0) and counts.sum() == D
    recv_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    sc_start = (off[:W] + 3 * np.arange(W)).astype(np.int32)
    run_of = np.searchsorted(off, np.arange(R), side="right") - 1
    pos = sc_start[run_of] + np.arange(R) - off[run_of]  # row of ``gathered`` of every request

    gathered = fmt.empty(R + 3 * W, dev)
    gathered.view(torch.uint8).fill_(SENT_BYTE)
    tmp = fmt.empty(R, dev)
    K.gather_wire(_t(req, dev), stale.state, fmt, tmp)
    gathered[_t(pos, dev, np.int64)] = tmp
    before = _bytes(gathered).copy()

    K.patch_scatter(recv, 0, W, _t(recv_off, dev), _t(sc_start, dev), gathered)  # D == 0: nothing moves
    assert np.array_equal(_bytes(gathered), before)
    K.patch_scatter(recv, D, W, _t(recv_off, dev), _t(sc_start, dev), gathered)
    after = _bytes(gathered)
    patched = np.zeros(R + 3 * W, bool)
    patched[pos[idx]] = True
    assert patched.sum() == D
    assert np.array_equal(after[pos[idx]], _bytes(recv))
    want_v, want_tail = O.wire_rows(fresh, fmt, req[idx], tag=O.tags(idx, off))
    assert np.array_equal(after[pos[idx]][:, : want_v.shape[1]], want_v)
    assert np.array_equal(np.ascontiguousarray(after[pos[idx]][:, fmt.vb:]).view(np.int32), want_tail)
    assert np.array_equal(after[~patched], before[~patched])
    assert not np.array_equal(after[patched], before[patched])


# ---------------------------------------------------------------------------
# owner apply against an fp64 optimizer step
# ---------------------------------------------------------------------------
A_ROWS = 2000


def _snap(tab) -> dict:
    s = {f: None if getattr(tab, f) is None else getattr(tab, f).detach().cpu().clone() for f in FIELDS}
    s["wx"] = None if tab.wx is None else tab.wx.detach().cpu().clone()
    return s


def _assert_rows_unchanged(s0, s1, rows_mask):
    """Every tensor of the table (fp8: the whole [w, scale, norm, pad] tails) keeps its bits in the masked rows."""
    for f in FIELDS + ("wx",):
        if s0[f] is None:
            assert s1[f] is None
            continue
        a, b = _bytes(s0[f].reshape(len(rows_mask), -1)), _bytes(s1[f].reshape(len(rows_mask), -1))
        assert np.array_equal(a[rows_mask], b[rows_mask]), f


def _assert_close(got, ref, bf16, skip=None, what=""):
    """fp32: |got - ref| <= 2e-6 + 1e-4 |ref| (test_kernels.py's step tolerance); bf16 storage (round
    to nearest): within one bf16 step of the rounded reference, |got - bf16(ref)| <= 2^-7 |ref| + 2e-6."""
    got = got.double()
    if bf16:
        err, tol = (got - ref.to(torch.bfloat16).double()).abs(), 2.0 ** -7 * ref.abs() + 2e-6
    else:
        err, tol = (got - ref).abs(), 2e-6 + 1e-4 * ref.abs()
    bad = ~(err <= tol)
    if skip is not None:
        bad &= ~skip
    assert not bool(bad.any()), (what, int(bad.sum()), float((err - tol).max()))


def _assert_applied(s0, s1, ref, Kp, opt, dtype):
    """The table after an apply (snapshots before / after) against ``apply_reference``'s result."""
    rows, p, n, z, near = ref
    assert near.float().mean() < 0.01  # FTRL elements left out at the p = 0 discontinuity
    idx = torch.from_numpy(rows)
    bf16 = dtype == torch.bfloat16
    _assert_close(s1["v"][idx][:, :Kp], p[:, :Kp], bf16, near[:, :Kp], "v")
    _assert_close(s1["w"][idx], p[:, Kp], False, near[:, Kp], "w")
    if opt.name == "sgd":
        for f in ("s0v", "s0w"):
            assert torch.equal(s0[f], s1[f])
    else:
        _assert_close(s1["s0v"][idx][:, :Kp], n[:, :Kp], False, None, "s0v")
        _assert_close(s1["s0w"][idx], n[:, Kp], False, None, "s0w")
    if opt.name == "ftrl":
        _assert_close(s1["s1v"][idx][:, :Kp], z[:, :Kp], False, None, "s1v")
        _assert_close(s1["s1w"][idx], z[:, Kp], False, None, "s1w")
    else:
        assert s1["s1v"] is None and s1["s1w"] is None
    untouched = np.ones(len(s0["w"]), bool)
    untouched[rows] = False
    assert untouched.any()
    _assert_rows_unchanged(s0, s1, untouched)


def _assert_fp8_rows_moved(s0, s1, applied, state=True):
    """fp8 tables: every row outside ``applied`` keeps all its bits; every applied row moved (its
    factors or, with a stateful optimizer, its factor accumulators: >= 16 randn gradients, one of
    which would have to be too small to register), and no accumulator shrank."""
    untouched = np.ones(len(s0["w"]), bool)
    untouched[applied] = False
    assert untouched.any() and not untouched.all()
    _assert_rows_unchanged(s0, s1, untouched)
    f = "s0v" if state else "v"
    moved = (_bytes(s0[f]) != _bytes(s1[f])).any(axis=1)
    assert np.array_equal(moved, ~untouched)
    if state:
        assert bool((s1["s0w"] >= s0["s0w"]).all()) and bool((s1["s0v"].float() >= s0["s0v"].float()).all())


def apply_case(shape, opt_name, k, dtype, device):
    """Runs of ``shape`` over a 2000-row table, randn gradient rows, and the fp64 result."""
    seed = _seed("apply", shape, opt_name, k, str(dtype))
    req, splits, off = O.shape_runs(shape, seed, A_ROWS)
    opt = OPTS[opt_name]
    tab = _table(A_ROWS, k, dtype, opt, seed % 997, device)
    grad = torch.randn((len(req), tab.Kp + 4), generator=torch.Generator().manual_seed(seed))
    return req, splits, off, opt, tab, grad


def _reference(opt, snap, req, grad, Kp, keep_rows=()):
    return O.apply_reference(opt.name, snap, req, grad, Kp, opt.lr, opt.l1, opt.l2, opt.beta, keep_rows=keep_rows)


def _apply_runs(req, off, splits, grad, tab, opt, device, **kw):
    R, W = len(req), len(splits)
    match = torch.full((R * W,), SENT, dtype=torch.int32, device=device) if W > 1 else None
    K.apply_runs(_t(req, device), _t(off, device), splits, grad.to(device), tab.state, opt, tab.Kp, match=match, **kw)
    _sync(device)


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("k", [4, 64, 100])
@pytest.mark.parametrize("opt_name", list(OPTS))
@pytest.mark.parametrize("shape", list("ACDE"))
def test_owner_apply_matches_fp64(device, shape, opt_name, k, dtype):
    """apply_rows (sorted grouping) and apply_runs (cross-run match) each against the fp64 sum of
    every row's gradient rows and one fp64 optimizer step; unrequested rows keep their bits."""
    req, splits, off, opt, tab, grad = apply_case(shape, opt_name, k, dtype, device)
    Kp = tab.Kp
    s0 = _snap(tab)
    ref = _reference(opt, s0, req, grad, Kp)
    assert len(ref[0]) == len(np.unique(req))

    dd = K.dedup(_t(req, device), key_bits=32, want_perm=True)
    K.apply_rows(dd, grad.to(device), tab.state, opt, Kp)
    _sync(device)
    _assert_applied(s0, _snap(tab), ref, Kp, opt, dtype)

    tab2 = _table(A_ROWS, k, dtype, opt, tab.seed, device)
    _assert_rows_unchanged(s0, _snap(tab2), np.ones(A_ROWS, bool))  # the same initial table
    _apply_runs(req, off, splits, grad, tab2, opt, device)
    _assert_applied(s0, _snap(tab2), ref, Kp, opt, dtype)


@gpu
@pytest.mark.parametrize("k", [16, 128])
@pytest.mark.parametrize("shape", list("ACDE"))
def test_owner_apply_fp8_untouched_rows(shape, k):
    """fp8 tables (approximate hardware epilogue: no numeric bound here): rows nobody requested keep
    every bit, scales and norms included; every requested row's accumulator moves."""
    req, splits, off, opt, tab, grad = apply_case(shape, "adagrad", k, K.FP8, "cuda")
    s0 = _snap(tab)
    tab2 = _table(A_ROWS, k, K.FP8, opt, tab.seed, "cuda")
    K.apply_rows(K.dedup(_t(req, "cuda"), key_bits=32, want_perm=True), grad.cuda(), tab.state, opt, tab.Kp)
    _apply_runs(req, off, splits, grad, tab2, opt, "cuda")
    for t in (tab, tab2):
        _assert_fp8_rows_moved(s0, _snap(t), np.unique(req))


SELF_TABLES = [pytest.param(torch.float32, 64, id="fp32-k64"), pytest.param(torch.bfloat16, 100, id="bf16-k100"),
               pytest.param(K.FP8, 16, id="fp8-k16"), pytest.param(K.FP8, 128, id="fp8-k128")]


@gpu
@pytest.mark.parametrize("dtype,k", SELF_TABLES)
@pytest.mark.parametrize("flags", ["none", "excl"])
@pytest.mark.parametrize("which", ["first", "middle", "last"])
@pytest.mark.parametrize("shape", ["C", "D"])
def test_apply_runs_self_run(shape, which, flags, dtype, k):
    """apply_runs with a self run: its exclusive rows (``self_excl`` flags from the oracle) were
    applied in place by the backward and keep their bits; its other rows get the full sum over all
    runs, the self run's own gradient row included.

    ``self_excl=None`` declares the whole run exclusive, which the exchange only does at world 1;
    with rows shared between the self run and another run that is outside the wrapper's contract.
    That case therefore removes the self run's rows from the other runs (which still overlap each
    other) and asserts the documented behaviour: the whole self run keeps its bits."""
    req, splits, off, opt, tab, grad = apply_case(shape, "adagrad", k, dtype, "cuda")
    W = len(splits)
    me = {"first": 0, "middle": W // 2, "last": W - 1}[which]
    mine = req[off[me]:off[me + 1]]
    if flags == "none":
        keep = (np.repeat(np.arange(W), splits) == me) | ~np.isin(req, mine)
        req, grad = req[keep], grad[torch.from_numpy(keep)]
        splits = [int(np.sum(keep[off[q]:off[q + 1]])) for q in range(W)]
        off = np.concatenate([[0], np.cumsum(splits)]).astype(np.int32)
        assert splits[me] == len(mine)
        kept_rows, self_excl = mine, None
    else:
        ex = O.excl(req, off, me)
        assert len(mine) == 0 or 0 < int(ex.sum()) < len(mine)
        kept_rows, self_excl = mine[ex != 0], _t(ex, "cuda")
    s0 = _snap(tab)
    applied = np.setdiff1d(np.unique(req), kept_rows)
    assert len(applied) == len(np.unique(req)) - len(kept_rows)
    _apply_runs(req, off, splits, grad, tab, opt, "cuda", self_run=me, self_excl=self_excl)
    s1 = _snap(tab)
    if dtype == K.FP8:
        _assert_fp8_rows_moved(s0, s1, applied)  # (the kept self rows among the unchanged ones)
    else:
        ref = _reference(opt, s0, req, grad, tab.Kp, keep_rows=kept_rows)
        assert np.array_equal(ref[0], applied)
        _assert_applied(s0, s1, ref, tab.Kp, opt, dtype)


DENSE_TABLES = [pytest.param(dt, k, id=f"{n}-k{k}") for dt, n in ((torch.float32, "fp32"), (torch.bfloat16, "bf16"))
                for k in (4, 64, 100)] + [pytest.param(K.FP8, 128, id="fp8-k128")]


@gpu
@pytest.mark.parametrize("dtype,k", DENSE_TABLES)
@pytest.mark.parametrize("opt_name", list(OPTS))
def test_dense_apply(opt_name, dtype, k):
    """dense_apply over a [600, Kp + 4] buffer at row0 0 and 700, all rows and the first 300, with and
    without clearing: touched rows (the first and the last among them) get one fp64-checked step on
    table row row0 + i and are cleared over their full width (``zero``); untouched rows, whose
    gradient columns hold garbage, neither move the table nor get cleared; rows past ``rows`` are
    left alone.  fp8 tables: which rows change, not their values."""
    opt = OPTS[opt_name]
    for row0 in (0, 700):
        for nrows in (None, 300):
            for zero in (True, False):
                seed = _seed("dense", opt_name, k, str(dtype), row0, nrows)
                tab = _table(A_ROWS, k, dtype, opt, seed % 997, "cuda")
                Kp = tab.Kp
                n = 600 if nrows is None else nrows
                g = torch.Generator().manual_seed(seed)
                buf = torch.randn((600, Kp + 4), generator=g)
                touch = torch.rand(600, generator=g) < 1 / 3
                touch[0] = touch[n - 1] = True
                mark = torch.tensor([1.0, 2.0, 0.5])[torch.randint(0, 3, (600,), generator=g)]
                buf[:, Kp + 1] = torch.where(touch, mark, torch.zeros(600))
                live = touch.clone()
                live[n:] = False
                rows_i = torch.nonzero(live).flatten()
                s0 = _snap(tab)
                dbuf = buf.cuda()
                K.dense_apply(dbuf, tab.state, opt, Kp, row0=row0, rows=nrows, zero=zero)
                torch.cuda.synchronize()
                s1 = _snap(tab)
                if dtype == K.FP8:
                    _assert_fp8_rows_moved(s0, s1, (rows_i + row0).numpy(), state=opt_name != "sgd")
                else:
                    ref = _reference(opt, s0, (rows_i + row0).numpy(), buf[rows_i], Kp)
                    _assert_applied(s0, s1, ref, Kp, opt, dtype)
                want = buf.clone()
                if zero:
                    want[live] = 0.0
                assert np.array_equal(_bytes(dbuf), _bytes(want)), (row0, nrows, zero)
