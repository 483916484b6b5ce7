"""Torch reference for ``FMTable.changed_rows`` (shared by test_sparse_ckpt*.py).

The expected set never comes from the code under test: a second table with the same seed, range,
dtype, optimizer, world and rank is compared, as integer views over ``[:real_rows, :K]``, against the
table under test -- the six state tensors and the fp8 scale."""

import torch

from fast_tffm_amd.models.table import FMTable

T = 1024  # rows per compaction tile (hip/ckpt.hip kCkTile)

_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(_INT[t.element_size()])


def fresh_like(table: FMTable) -> FMTable:
    return FMTable(table.vocab_size, table.K, world=table.world, rank=table.rank, dtype=table.dtype, opt=table.opt,
                   init_range=table.init_range, seed=table.init_seed, device=table.device)


STATE = ("v", "w", "s0v", "s0w", "s1v", "s1w")


def torch_changed_rows(table: FMTable) -> torch.Tensor:
    ref = fresh_like(table)
    n, K = table.real_rows, table.K
    diff = torch.zeros(n, dtype=torch.bool, device=table.device)
    for name in STATE:
        a, b = getattr(table, name), getattr(ref, name)
        if a is None:
            continue
        if a.dim() == 2:
            diff |= (bits(a)[:n, :K] != bits(b)[:n, :K]).any(dim=1)
        else:
            diff |= bits(a)[:n] != bits(b)[:n]
    if table.fp8:
        diff |= bits(table.scale)[:n] != bits(ref.scale)[:n]
    return torch.nonzero(diff).flatten()


def assert_same_state(a: FMTable, b: FMTable, norm: bool = True) -> None:
    """Every state tensor bitwise equal over the real rows and columns 0 .. K-1 (fp8: scale and norm too)."""
    n, K = a.real_rows, a.K
    assert b.real_rows == n
    for name in STATE:
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is None:
            continue
        if x.dim() == 2:
            assert torch.equal(bits(x)[:n, :K], bits(y)[:n, :K]), name
        else:
            assert torch.equal(bits(x)[:n], bits(y)[:n]), name
    if a.fp8:
        assert torch.equal(bits(a.scale)[:n], bits(b.scale)[:n]), "scale"
        if norm:
            assert torch.equal(bits(a.norm2)[:n], bits(b.norm2)[:n]), "norm"


def flip(t: torch.Tensor, *idx) -> None:
    """Flip the lowest bit of one element."""
    b = bits(t)
    b[idx] = b[idx] ^ 1
