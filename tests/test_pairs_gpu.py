"""The pair-interaction kernel on the GPU (hip/fm_pairs.hip) against the fp64 oracle of test_pairs.py and, bit
for bit, against the CPU twin."""

import numpy as np
import pytest
import torch

from explain_oracle import make_batch, make_table
from fast_tffm_amd.ops import kernels as K
from test_pairs import (DTYPES, GRID, LENS, batch_of, check_constructed, check_lists, check_long_example, constructed,
                        run)

pytestmark = pytest.mark.gpu


def same(a, b):  # all four outputs equal, the values by their bits
    return all(torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)) for x, y in zip(a, b))


@pytest.mark.parametrize("Kf,dtype,with_vals,top", GRID)
def test_grid_against_oracle_and_cpu_twin(Kf, dtype, with_vals, top):
    off, ids, vals = batch_of(LENS, Kf + top, with_vals)
    v, _, Kp = make_table(DTYPES[dtype], Kf, device="cuda")
    out = run(off, ids, vals, v, Kp, top, "cuda")
    check_lists(off, ids, vals, v, Kp, top, out)
    assert same(out, run(off, ids, vals, v.cpu(), Kp, top, threads=2))


@pytest.mark.parametrize("kind", ["ascending", "descending", "constant"])
def test_constructed_examples(kind):
    off, ids, v, _ = constructed(kind)
    check_constructed(kind, run(off, ids, None, v.cuda(), 4, 8, "cuda"))


def test_long_example():
    check_long_example("cuda", *make_table(torch.float32, 20, device="cuda")[::2])


def test_more_examples_than_waves():
    """B = 20011 > the launch's 16384 waves: workgroups stride."""
    off, ids, vals = batch_of(np.random.default_rng(11).integers(0, 9, 20011), 12)
    v, _, Kp = make_table(torch.float32, 64, device="cuda")
    out = run(off, ids, vals, v, Kp, 4, "cuda")
    assert same(out, run(off, ids, vals, v.cpu(), Kp, 4))
    check_lists(off[:2001], ids[:off[2000]], vals[:off[2000]], v, Kp, 4, [t[:2000] for t in out])


@pytest.mark.parametrize("dtype", list(DTYPES))
def test_wire_style_rows_repeatable_and_captured(dtype):
    """Wider rows (the wire buffer's shape); a second call and replays of a captured one give the same bits."""
    off, ids, vals = make_batch(seed=5)
    v, _, Kp = make_table(DTYPES[dtype], 10, device="cuda", row_stride=32)
    assert v.stride(0) == 32 > Kp
    out = run(off, ids, vals, v, Kp, 10, "cuda")
    check_lists(off, ids, vals, v, Kp, 10, out)
    assert same(out, run(off, ids, vals, v.cpu(), Kp, 10)) and same(out, run(off, ids, vals, v, Kp, 10, "cuda"))
    bufs = {k: torch.full_like(t, 7) for k, t in zip(("first", "second", "value", "count"), out)}
    args = [torch.from_numpy(a).cuda() for a in (off, ids, vals)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        K.fm_pairs(*args, v, Kp, 10, **bufs)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        K.fm_pairs(*args, v, Kp, 10, **bufs)
    for _ in range(3):
        for t in bufs.values():
            t.fill_(7)
        g.replay()
        torch.cuda.synchronize()
        assert same(out, list(bufs.values()))
