"""Sparse checkpoints on the GPU: ``changed_rows`` (hip/ckpt.hip) against a torch comparison with a second,
freshly initialised table -- which also proves that the kernel regenerates the init kernels' values bit
for bit (a fresh table reports nothing) --, against the CPU twin, and through sparse save / restore for
fp32, bf16 and fp8 tables.  Every comparison is bitwise."""

import pytest
import torch

from fast_tffm_amd.data.synthetic import CriteoSynth
from fast_tffm_amd.models.fm import FactorizationMachine, FMConfig
from fast_tffm_amd.models.table import FMTable
from fast_tffm_amd.ops import kernels as K
from fast_tffm_amd.ops import native
from fast_tffm_amd.utils import checkpoint as ckpt

from sparse_ckpt_oracle import STATE, T, assert_same_state, bits, flip, torch_changed_rows

pytestmark = pytest.mark.gpu
FP8 = torch.float8_e4m3fn
DTYPES = [torch.float32, torch.bfloat16, FP8]
OPTS = ["adagrad", "ftrl", "sgd"]


def _table(rows=200, Kf=16, dtype=torch.float32, opt="ftrl", world=1, rank=0, seed=3, vocab=None, device="cuda"):
    return FMTable(rows * world if vocab is None else vocab, Kf, world=world, rank=rank, dtype=dtype,
                   opt=K.OptConfig(opt, lr=0.1), seed=seed, init_range=0.05, device=device)


def _check(table, want=None):
    got = table.changed_rows()
    assert got.dtype == torch.int64 and got.device.type == table.device.type
    assert torch.equal(got, torch_changed_rows(table))
    if want is not None:
        assert got.tolist() == sorted(want)


def test_tile_constant():
    assert native.hip().CKPT_TILE == T


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", OPTS)
def test_fresh_table_reports_nothing(dtype, opt):
    """Bitwise identity with init_rows_kernel / init_rows_fp8_kernel and torch.full's slot patterns."""
    for Kf in (4, 16, 64, 100, 128):
        for rows in (1, 65, 2 * T + 37):
            t = _table(rows, Kf, dtype, opt)
            assert t.changed_rows().numel() == 0, (Kf, rows)
    t.reinit(seed=77)
    assert t.init_seed == 77
    _check(t, [])
    assert K.changed_rows(t, seed=3).numel() == t.real_rows  # (another seed: every row differs)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("Kf", [6, 100])
def test_targeted_edits(dtype, Kf):
    rows = T + 300
    edits = [("v", (17, 0)), ("v", (18, Kf - 1)), ("w", (3,)), ("s0v", (150, Kf - 1)), ("s0w", (64,)),
             ("s1v", (63, 0)), ("s1w", (rows - 1,)), ("v", (T, 1)), ("s0w", (T - 1,))]
    for name, idx in edits:
        t = _table(rows, Kf, dtype)
        flip(getattr(t, name), *idx)
        _check(t, [idx[0]])
    t = _table(rows, Kf, dtype)
    for name, idx in edits:
        flip(getattr(t, name), *idx)
    _check(t, [i[0] for _, i in edits])
    if K.padded_k(Kf, dtype) > Kf:  # pad columns are not looked at
        t = _table(rows, Kf, dtype)
        flip(t.v, 40, Kf)
        flip(t.s0v, 41, t.Kp - 1)
        flip(t.s1v, 42, Kf)
        _check(t, [])


def test_fp8_scale_and_norm():
    t = _table(300, 16, FP8)
    flip(t.norm2, 7)       # derived data: not reported
    t.wx[9, 3] = 5.0       # the pad word of the w row
    _check(t, [])
    flip(t.scale, 11)
    _check(t, [11])
    flip(t.v, 250, 5)      # one stored byte
    _check(t, [11, 250])


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 2 * T + 37])
def test_row_counts(rows):
    for case in ("all", "first", "last"):
        t = _table(rows, 4, torch.float32, "adagrad")
        if case == "all":
            t.w += 1.0
            want = list(range(rows))
        else:
            want = [0 if case == "first" else rows - 1]
            flip(t.s0w, want[0])
        _check(t, want)


def test_shard_offsets():
    V = 3 * 100 + 2
    for rank in range(3):
        t = _table(Kf=16, dtype=FP8, world=3, rank=rank, vocab=V)
        _check(t, [])
        flip(t.v, t.real_rows - 1, 1)
        flip(t.w, 0)
        _check(t, [0, t.real_rows - 1])
    t = FMTable(10, 4, seed=1, rows_multiple=8, device="cuda")
    assert t.rows == 16 and t.real_rows == 10
    _check(t, [])
    t = _table(Kf=4, world=3, rank=2, vocab=2)
    assert t.real_rows == 0
    t.w += 1.0
    assert t.changed_rows().numel() == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gpu_and_cpu_agree(dtype):
    g = _table(2 * T + 37, 6, dtype)
    gen = torch.Generator().manual_seed(1)
    pick = torch.randperm(g.real_rows, generator=gen)[:300]  # (distinct rows: no element is flipped twice)
    for i, r in enumerate(pick.tolist()):
        name = STATE[i % len(STATE)]
        t = getattr(g, name)
        flip(t, r, i % g.K) if t.dim() == 2 else flip(t, r)
    c = _table(2 * T + 37, 6, dtype, device="cpu")
    for name in STATE:
        getattr(c, name).copy_(getattr(g, name))
    got = g.changed_rows()
    assert torch.equal(got.cpu(), c.changed_rows())
    assert torch.equal(got, torch.unique(pick).to("cuda"))


CONFIGS = [(torch.float32, "adagrad", 64), (torch.bfloat16, "adagrad", 16), (FP8, "ftrl", 128)]


def _model(V, Kf, dtype, opt, seed=5):
    o = (K.OptConfig("ftrl", lr=0.05, l1=0.001, l2=0.001, beta=1.0) if opt == "ftrl" else K.OptConfig(opt, lr=0.05))
    cfg = FMConfig(vocabulary_size=V, factor_num=Kf, loss_type="logistic", init_value_range=0.05, seed=seed, opt=o,
                   batch_size=4096, factor_lambda=0.01, bias_lambda=0.01, dtype=dtype)
    return FactorizationMachine(cfg, device="cuda")


@pytest.mark.parametrize("dtype,opt,Kf", CONFIGS)
def test_after_training_steps(dtype, opt, Kf):
    V = 200_000
    m = _model(V, Kf, dtype, opt)
    gen = CriteoSynth(V, device="cuda", seed=9)
    seen = []
    for _ in range(3):
        b = gen.batch(4096)
        seen.append(b.ids)
        m.train_step(b)
    got = m.table.changed_rows()
    assert torch.equal(got, torch_changed_rows(m.table))
    assert 0 < got.numel() < V // 2
    assert bool(torch.isin(got, torch.unique(torch.cat(seen).long())).all())


@pytest.mark.parametrize("dtype,opt,Kf", CONFIGS)
def test_round_trip(tmp_path, monkeypatch, dtype, opt, Kf):
    monkeypatch.setattr(ckpt, "CHUNK_BYTES", 1 << 20)  # (several chunks)
    V = 50_003
    m = _model(V, Kf, dtype, opt)
    gen = CriteoSynth(V, device="cuda", seed=11)
    for _ in range(2):
        m.train_step(gen.batch(4096))
    want = torch_changed_rows(m.table)
    path = ckpt.save_checkpoint(m, str(tmp_path / "log"), m.global_step, table_format="sparse")
    from safetensors import safe_open

    with safe_open(f"{path}/shard-00000-of-00001.safetensors", framework="pt") as f:
        assert torch.equal(f.get_tensor("rows"), want.cpu())
        assert ("v_fp8" in f.keys()) == (dtype == FP8)
    m2 = _model(V, Kf, dtype, opt)
    m2.table.reinit(seed=999)  # (the checkpoint's seed is used, not the table's)
    m2.table.s0v.fill_(3.0)
    ckpt.restore_checkpoint(m2, path)
    assert m2.table.init_seed == 5 and m2.global_step == m.global_step
    assert_same_state(m.table, m2.table)
    if dtype == FP8:
        n = m.table.real_rows
        assert torch.equal(m.table.wx[:n, :3], m2.table.wx[:n, :3])
    assert torch.equal(m2.table.changed_rows(), want)
    # one further step from the restored model == one from the original
    b = gen.batch(4096)
    m.train_step(b)
    m2.train_step(b)
    assert_same_state(m.table, m2.table)
    # a sparse checkpoint restores into one process of two (re-shard)
    half = FMTable(V, Kf, world=2, rank=1, dtype=dtype, opt=m.table.opt, seed=1, init_range=0.05, device="cuda")

    class Shard:
        table, mode, cfg, global_step = half, "shard", m.cfg, 0

    path2 = ckpt.save_checkpoint(m, str(tmp_path / "log"), m.global_step, table_format="sparse")
    ckpt.restore_checkpoint(Shard, path2)
    mine = torch.arange(1, V, 2, device="cuda")
    for name in STATE:
        a = getattr(m.table, name)
        if a is not None:
            b_ = getattr(half, name)[: mine.numel()]
            a_ = a[mine]
            if a.dim() == 2:
                a_, b_ = a_[:, :Kf], b_[:, :Kf]
            assert torch.equal(bits(a_), bits(b_)), name
    if dtype == FP8:
        assert torch.equal(m.table.wx[mine, :3], half.wx[: mine.numel(), :3])


def test_fp8_offline_readers_refuse(tmp_path):
    m = _model(3000, 32, FP8, "adagrad")
    m.train_step(CriteoSynth(3000, device="cuda", seed=1).batch(512))
    path = ckpt.save_checkpoint(m, str(tmp_path / "log"), 1, table_format="sparse")
    with pytest.raises(ValueError, match="checkpoint_format = dense"):
        ckpt.export_reference_blocks(path, str(tmp_path / "ref"), 2)
