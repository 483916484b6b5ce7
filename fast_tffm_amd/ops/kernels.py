"""Typed, validated wrappers over the native step kernels.

Every wrapper dispatches on the device of its tensors: CUDA (HIP) tensors go to
the gfx950 kernels of ``_fm_hip``, CPU tensors to ``_fm_cpu``.  Launches are
asynchronous on the current torch stream; nothing here synchronises the host
unless ``FM_DEBUG_CHECKS=1`` asks for index range checks.

Row layout contract (see csrc/hip/fm_common.h): a factor table ``v`` is
``[rows, Kp]`` (fp32 or bf16, Kp padded so that a lane moves 16 bytes), the
linear weights ``w`` are a separate fp32 vector (or column ``Kp`` of a packed
``[rows, Kp+4]`` exchange buffer, passed as a strided view).
"""

from __future__ import annotations

import math
import os
import statistics
import struct
from dataclasses import dataclass
from fractions import Fraction

import torch

from . import native

LOSS_TYPES = {"none": 0, "mse": 1, "logistic": 2}
OPT_TYPES = {"adagrad": 0, "ftrl": 1, "sgd": 2}
BWD_LOCAL, BWD_EMIT = 0, 1
BWD_EMIT_TABLE = 2   # params from table rows uniq[u]; gradient scattered to grad_out[uniq[u]] + touch mark

_DEBUG = os.environ.get("FM_DEBUG_CHECKS", "0") == "1"


def debug_checks() -> bool:
    """FM_DEBUG_CHECKS=1: index range checks in the kernel wrappers and exchange split checks."""
    return _DEBUG


def set_debug_checks(on: bool) -> None:
    global _DEBUG
    _DEBUG = bool(on)


def set_fwd_mfma(on: bool) -> bool:
    """Route fp8 k=128 binary-feature forwards to the matrix-core kernel (hip/fm_fwd_mfma.hip: the "mfma"
    build variant only, where it is the default; the default module has no such kernel and stays on the
    VALU kernel) or the VALU kernel; returns the previous setting."""
    h = native.hip()
    was = bool(h.fwd_mfma_enabled())
    h.set_fwd_mfma(bool(on))
    return was


FP8 = torch.float8_e4m3fn   # OCP e4m3 table storage (+ fp32 scale per row), GPU only
FP8_MAX = 448.0


def dtype_code(t: torch.dtype) -> int:
    if t == torch.float32:
        return 0
    if t == torch.bfloat16:
        return 1
    if t == FP8:
        return 2
    raise TypeError(f"unsupported table dtype {t}; use float32, bfloat16 or float8_e4m3fn")


def elems_per_lane(dtype: torch.dtype) -> int:
    """Table elements one lane moves per row access: 4 (16 B fp32, 8 B bf16, 4 B fp8)."""
    return 4


def padded_k(K: int, dtype: torch.dtype = torch.float32) -> int:
    """Factor columns stored per row: K rounded up to whole lanes (multiples of 4)."""
    e = elems_per_lane(dtype)
    return ((K + e - 1) // e) * e


def r1_dtype(table_dtype: torch.dtype) -> torch.dtype:
    """Storage dtype of the forward's r1 cache [B, Kp] for a table dtype: fp32, or bf16 for fp8
    tables (3-bit factor mantissas; bf16 r1 halves the backward's per-occurrence gather --
    hip/fm_common.h R1Bf16)."""
    return torch.bfloat16 if table_dtype == FP8 else torch.float32


def fp8_row_scale(m: torch.Tensor) -> torch.Tensor:
    """Row scales of fp8 rows with largest |value| m (hip/fm_common.h fp8_row_scale): the power of
    two s with m / s in (224, 448]; 1 for empty rows."""
    m = m.float()
    t = torch.clamp(m / FP8_MAX, min=2.0 ** -126)
    mant, e = torch.frexp(t)  # t = mant * 2^e, mant in [0.5, 1)
    s = torch.where(mant == 0.5, t, torch.ldexp(torch.ones_like(t), e))
    return torch.where(m > 0, s, torch.ones_like(m))


def quantize_fp8_rows(vals: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-row fp8 quantisation (the kernels' store_row): scale = fp8_row_scale(max|v|) (a power of
    two), q = rne(v / scale)."""
    v = vals.float()
    m = v.abs().amax(dim=1) if v.shape[1] else torch.zeros(v.shape[0], device=v.device)
    s = fp8_row_scale(m)
    q = (v * (1.0 / s)[:, None]).clamp(-FP8_MAX, FP8_MAX).to(FP8)
    return q, s


@dataclass
class OptConfig:
    name: str = "adagrad"
    lr: float = 0.01
    l1: float = 0.0
    l2: float = 0.0
    beta: float = 0.0
    initial_accumulator: float = 0.1

    @property
    def code(self) -> int:
        return OPT_TYPES[self.name]

    @property
    def n_state(self) -> int:
        return 2 if self.name == "ftrl" else (1 if self.name == "adagrad" else 0)


def _p(t: torch.Tensor | None) -> int:
    return 0 if t is None else t.data_ptr()


def _is_gpu(t: torch.Tensor) -> bool:
    return t.device.type == "cuda"


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor) -> int:
    """The current HIP stream's handle on ``t``'s device (the raw accessor: the Stream-object path costs
    several Python calls per kernel launch, ~16 launches per sharded step)."""
    idx = t.device.index
    if _raw_stream is not None and idx is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(t.device).cuda_stream


def _check(cond: bool, msg: str) -> None:
    if not cond:
        raise ValueError(msg)


def _chk_vec(t: torch.Tensor | None, dtype: torch.dtype, n: int | None, name: str, dev: torch.device) -> None:
    if t is None:
        return
    _check(t.dtype == dtype, f"{name}: expected {dtype}, got {t.dtype}")
    _check(t.device == dev, f"{name}: expected device {dev}, got {t.device}")
    _check(t.is_contiguous(), f"{name}: must be contiguous")
    if n is not None:
        _check(t.numel() >= n, f"{name}: needs >= {n} elements, has {t.numel()}")


def _chk_rows(v: torch.Tensor, Kp: int, name: str) -> int:
    """Validate a row-major factor source and return its row stride in elements."""
    _check(v.dim() == 2, f"{name}: expected 2-D rows")
    _check(v.stride(1) == 1, f"{name}: rows must be contiguous")
    epl = elems_per_lane(v.dtype)
    _check(Kp % epl == 0, f"{name}: Kp={Kp} must be a multiple of {epl} for {v.dtype}")
    _check(v.shape[1] >= Kp, f"{name}: has {v.shape[1]} columns < Kp={Kp}")
    _check(v.stride(0) % epl == 0, f"{name}: row stride {v.stride(0)} must be a multiple of {epl}")
    _check(v.data_ptr() % 16 == 0, f"{name}: base must be 16-byte aligned")
    return v.stride(0)


def _range_check(idx: torch.Tensor, hi: int, name: str) -> None:
    if _DEBUG and idx.numel() > 0 and not (idx.is_cuda and torch.cuda.is_current_stream_capturing()):
        lo_v, hi_v = int(idx.min()), int(idx.max())
        _check(lo_v >= 0 and hi_v < hi, f"{name}: index range [{lo_v}, {hi_v}] outside [0, {hi})")


# ---------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------
class FwdOut:
    """Outputs of fm_forward. ``loss_sum``/``regv``/``regw`` are 0-d tensors on the op's device."""

    __slots__ = ("pred", "r1", "dpred", "loss_sum", "regv", "regw", "loss_partial")

    def __init__(self, pred, r1, dpred, loss_sum, regv, regw, loss_partial=None):
        self.pred, self.r1, self.dpred = pred, r1, dpred
        self.loss_sum, self.regv, self.regw = loss_sum, regv, regw
        self.loss_partial = loss_partial  # per-workgroup loss sums when the reduction was deferred

    def finish_loss(self) -> torch.Tensor | None:
        """The summed loss; a deferred reduction (``fm_forward(defer_loss=True)``) is enqueued now,
        on the current stream."""
        if self.loss_sum is None and self.loss_partial is not None:
            self.loss_sum = self.loss_partial.sum(dtype=torch.float32)
        return self.loss_sum


def fm_forward(offsets: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor | None, v: torch.Tensor,
               w: torch.Tensor, Kp: int, *, labels: torch.Tensor | None = None,
               weights: torch.Tensor | None = None, loss: str = "none", grad_scale: float = 1.0,
               want_r1: bool = True, want_reg: bool = False, pred: torch.Tensor | None = None,
               r1: torch.Tensor | None = None, dpred: torch.Tensor | None = None,
               partial: torch.Tensor | None = None, threads: int = 0,
               bias: torch.Tensor | None = None, self_rows: SelfRows | None = None,
               seg_lookup: "SegIndex | None" = None, defer_loss: bool = False, max_feats: int = -1) -> FwdOut:
    """FM score of a CSR batch (reference FmScorer, cc/fm_scorer_op.h:101-140), fused with the loss.

    pred_i = sum_j x_j w_j + 1/2 sum_k [(sum_j x_j v_jk)^2 - sum_j x_j^2 v_jk^2]  (+ bias[0], optional
    global bias; the reference has none, fm_scorer_op.h:134-136)
    With ``loss`` in {mse, logistic} also returns the summed weighted loss and
    ``dpred = grad_scale * dL_i/dpred_i``.

    ``self_rows`` (GPU, ``rows`` = segment ids): segments in its range read this rank's table.
    ``seg_lookup`` (GPU): ``rows`` are the dedup's keys and every occurrence's segment (its
    row of ``v``) is found through the bucket index (``seg_index``) instead of an inverse map.
    (``defer_loss``, GPU: the per-workgroup loss partials are left for ``FwdOut.finish_loss``, so the
    reduction can be enqueued after the backward instead of between forward and backward.)
    ``max_feats`` (host-known maximum occurrences per example, -1 unknown): lets fp8 k=128 batches of
    binary features run on the matrix cores (hip/fm_fwd_mfma.hip).
    """
    dev = rows.device
    B = offsets.numel() - 1
    _chk_vec(offsets, torch.int32, B + 1, "offsets", dev)
    nnz = rows.numel()
    _chk_vec(rows, torch.int32, nnz, "rows", dev)
    _chk_vec(vals, torch.float32, nnz, "vals", dev)
    v_stride = _chk_rows(v, Kp, "v")
    _check(w.dim() == 1 or (w.dim() == 2 and w.shape[1] == 1), "w: expected a vector (possibly strided)")
    _check(w.dtype == torch.float32 and w.device == dev, "w: expected float32 on the rows' device")
    w_stride = w.stride(0)
    _check(w.shape[0] >= v.shape[0], "w: fewer rows than v")
    # fp8 rows: w is the row tails [w, scale, |v|^2, .] (Table rows / wire rows): the forward reads all three
    _check(v.dtype != FP8 or w_stride >= 3, "fp8 rows: w must be a strided view of [w, scale, |v|^2, .] row tails")
    lt = LOSS_TYPES[loss]
    if bias is not None:
        _chk_vec(bias, torch.float32, 1, "bias", dev)
    if lt:
        _chk_vec(labels, torch.float32, B, "labels", dev)
        _chk_vec(weights, torch.float32, B, "weights", dev)
    if seg_lookup is None:
        _range_check(rows, v.shape[0], "rows")
    else:
        _check(_is_gpu(rows), "segment lookup is a GPU path")
    if pred is None:
        pred = torch.empty(B, dtype=torch.float32, device=dev)
    if want_r1 and r1 is None:
        r1 = torch.empty((B, Kp), dtype=r1_dtype(v.dtype), device=dev)
    if want_r1:
        _check(r1.dtype == r1_dtype(v.dtype) and r1.is_contiguous() and r1.shape[1] == Kp and r1.shape[0] >= B,
               f"r1: contiguous [B, Kp] {r1_dtype(v.dtype)} for a {v.dtype} table")
    if not want_r1:
        r1 = None
    if lt and dpred is None:
        dpred = torch.empty(B, dtype=torch.float32, device=dev)
    dt = dtype_code(v.dtype)
    host_checks = _DEBUG and not (offsets.is_cuda and torch.cuda.is_current_stream_capturing())
    if host_checks and max_feats is not None and max_feats >= 0 and B > 0:
        _check(int((offsets[1:] - offsets[:-1]).max()) <= max_feats, "max_feats: an example has more features")
    if host_checks and v.dtype == FP8 and w_stride == 4 and v.shape[0] > 0:
        # table rows [w, scale, |v|^2, .]: the kernels apply only the scale's exponent, so every host
        # write of v / scale must keep scales powers of two (FMTable.set_v / adopt_fp8_rows do)
        sc = torch.as_strided(w, (v.shape[0],), (4,), w.storage_offset() + 1)
        _check(bool((torch.frexp(sc)[0] == 0.5).all()), "fp8 table: a row scale is not a power of two")
    if _is_gpu(rows):
        h = native.hip()
        grid = h.fwd_grid(max(B, 1))
        if partial is None or partial.numel() < 3 * grid:
            partial = torch.zeros(3 * grid, dtype=torch.float32, device=dev)
        lp = partial[:grid]
        rp = partial[grid:3 * grid]
        dkw = {}
        if self_rows is not None and self_rows.u1 > self_rows.u0:
            _self_check(self_rows, v, None)
            dkw["self_rows"] = self_rows.packed()
        h.fwd(B=B, offsets=_p(offsets), rows=_p(rows), vals=_p(vals), v=_p(v), v_stride=v_stride, w=_p(w),
              w_stride=w_stride, Kp=Kp, dtype=dt, labels=_p(labels), weights=_p(weights), loss_type=lt,
              grad_scale=float(grad_scale), pred=_p(pred), r1=_p(r1), dpred=_p(dpred) if lt else 0,
              loss_partial=_p(lp) if lt else 0, reg_partial=_p(rp) if want_reg else 0, grid=grid,
              stream=_stream(rows), bias=_p(bias),
              seg_idx=_p(seg_lookup.idx) if seg_lookup is not None else 0,
              seg_keys=_p(seg_lookup.keys) if seg_lookup is not None else 0,
              seg_shift=seg_lookup.shift if seg_lookup is not None else 0,
              max_feats=int(max_feats) if max_feats is not None else -1, **dkw)
        # (an in-kernel last-block reduction was measured slower: the per-block agent-scope
        # release fence writes back L2 -- fwd 211 -> 412 us; a separate reduce is ~10 us; the same
        # reduce on a second stream beside the backward measured slower too: 0.668-0.671 -> 0.676 ms,
        # profiles/r3/loss_stream_ab.txt)
        # A sum by the chunk backward's first workgroup (no reduce kernel between forward and
        # backward) made the chunk kernel itself ~30% slower even when not taken -- a workgroup
        # barrier in the chunk kernel changes its code (k64 0.668 -> 0.88 ms, same box;
        # profiles/r3/fused_loss_ab.txt)
        # (the local step defers this reduction past the backward: nothing reads the loss before it)
        loss_sum = lp.sum(dtype=torch.float32) if lt and not defer_loss else None
        regv = rp.view(grid, 2)[:, 0].sum() if want_reg else None
        regw = rp.view(grid, 2)[:, 1].sum() if want_reg else None
        if lt and defer_loss:
            return FwdOut(pred, r1, dpred, None, regv, regw, loss_partial=lp)
    else:
        _check(self_rows is None, "self rows are a GPU path")
        c = native.cpu()
        ls, rv, rw = c.fwd(B=B, offsets=_p(offsets), rows=_p(rows), vals=_p(vals), v=_p(v), v_stride=v_stride,
                           w=_p(w), w_stride=w_stride, Kp=Kp, dtype=dt, labels=_p(labels), weights=_p(weights),
                           loss_type=lt, grad_scale=float(grad_scale), pred=_p(pred), r1=_p(r1),
                           dpred=_p(dpred) if lt else 0, threads=threads, bias=_p(bias))
        loss_sum = torch.tensor(ls, dtype=torch.float32) if lt else None
        regv = torch.tensor(rv, dtype=torch.float32) if want_reg else None
        regw = torch.tensor(rw, dtype=torch.float32) if want_reg else None
    return FwdOut(pred, r1, dpred if lt else None, loss_sum, regv, regw)


def fm_explain(offsets: torch.Tensor, rows: torch.Tensor, vals: torch.Tensor | None, v: torch.Tensor,
               w: torch.Tensor, Kp: int, *, bias: torch.Tensor | None = None, contrib: torch.Tensor | None = None,
               pred: torch.Tensor | None = None, threads: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """Exact attribution of every occurrence of a CSR batch (hip/fm_explain.hip; the reference has none).

    c_j = x_j w_j + 1/2 sum_f x_j v_jf (S_f - x_j v_jf) with S_f = sum_j x_j v_jf over the example: each
    pair's term split equally between its two occurrences, the Shapley value of the occurrence against the
    empty example.  Returns ``(contrib [nnz], pred [B])`` with ``pred_i = sum_j c_j + bias`` -- ``fm_forward``'s
    score up to rounding.  fp8 rows (GPU only): the dot product on the dequantised row, the self term from
    the row's stored |v|^2, as the forward.  ``rows`` are plain row indices into ``v`` / ``w`` (table rows
    or gathered wire rows)."""
    dev = rows.device
    B = offsets.numel() - 1
    _chk_vec(offsets, torch.int32, B + 1, "offsets", dev)
    nnz = rows.numel()
    _chk_vec(rows, torch.int32, nnz, "rows", dev)
    _chk_vec(vals, torch.float32, nnz, "vals", dev)
    v_stride = _chk_rows(v, Kp, "v")
    _check(v.device == dev, "v: expected the rows' device")
    _check(w.dim() == 1 or (w.dim() == 2 and w.shape[1] == 1), "w: expected a vector (possibly strided)")
    _check(w.dtype == torch.float32 and w.device == dev, "w: expected float32 on the rows' device")
    w_stride = w.stride(0)
    _check(w.shape[0] >= v.shape[0], "w: fewer rows than v")
    _check(v.dtype != FP8 or w_stride >= 3, "fp8 rows: w must be a strided view of [w, scale, |v|^2, .] row tails")
    _check(v.dtype != FP8 or (w_stride % 4 == 0 and w.data_ptr() % 16 == 0),
           "fp8 rows: the [w, scale, |v|^2, .] tails must be 16-byte aligned")
    _check(v_stride * v.element_size() < 2**32, "v: row stride must be below 4 GiB")
    _check(nnz == 0 or v.shape[0] > 0, "rows index an empty table")
    if bias is not None:
        _chk_vec(bias, torch.float32, 1, "bias", dev)
    _range_check(rows, v.shape[0], "rows")
    if contrib is None:
        contrib = torch.empty(nnz, dtype=torch.float32, device=dev)
    if pred is None:
        pred = torch.empty(B, dtype=torch.float32, device=dev)
    _chk_vec(contrib, torch.float32, nnz, "contrib", dev)
    _chk_vec(pred, torch.float32, B, "pred", dev)
    dt = dtype_code(v.dtype)
    kw = dict(B=B, offsets=_p(offsets), rows=_p(rows), vals=_p(vals), v=_p(v), v_stride=v_stride, w=_p(w),
              w_stride=w_stride, Kp=Kp, dtype=dt, bias=_p(bias), contrib=_p(contrib), pred=_p(pred))
    if _is_gpu(rows):
        native.hip().explain(stream=_stream(rows), **kw)
    else:
        _check(v.dtype != FP8, "fp8 tables are a GPU path")
        native.cpu().explain(threads=threads, **kw)
    return contrib[:nnz], pred[:B]


# ---------------------------------------------------------------------------
# dedup
# ---------------------------------------------------------------------------
class DedupOut:
    """Grouping of a batch's occurrences by key (sorted unique keys = segments).

    ``counts`` is a 2-element int32 device tensor (U, #chunks) -- no host sync;
    ``num_unique`` is a view of counts[0]; ``U_host`` is set on CPU and after
    ``.sync()``.  ``perm`` is the sorted payload: the occurrence index, unless
    the dedup ran with the example index as payload (then ``sorted_ex is perm``).
    """

    __slots__ = ("n", "skeys", "perm", "uniq", "seg_start", "seg_chunk", "chunk_start", "chunk_seg", "chunk_key",
                 "counts", "num_unique", "inv", "sorted_ex", "sorted_x", "U_host", "CH", "big_list", "big_count",
                 "multi", "ex_shift", "bwd_fresh")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def sync(self) -> int:
        if self.U_host is None:
            # counts[7]: the in-tree sort's look-back verdict (nonzero: this grouping is invalid)
            u, err = self.counts[0:8:7].tolist() if self.counts.numel() >= 8 else (int(self.num_unique.item()), 0)
            if err:
                raise RuntimeError(f"dedup: the radix sort's look-back spin bound was hit (error word {err}); "
                                   "this batch's grouping is invalid")
            self.U_host = int(u)
        return self.U_host

    def unique_keys(self) -> torch.Tensor:
        return self.uniq[: self.sync()]


class DedupWorkspace:
    """Reusable device buffers for dedup + chunk plan of up to ``cap`` occurrences."""

    def __init__(self, cap: int, device: torch.device, CH: int = 32):
        self.cap, self.device, self.CH = cap, device, CH
        n1 = max(cap, 1)
        i32 = dict(dtype=torch.int32, device=device)
        self.iota = torch.arange(n1, **i32)
        self.skeys = torch.empty(n1, **i32)
        self.perm = torch.empty(n1, **i32)
        self.uniq = torch.empty(n1, **i32)
        self.seg_start = torch.empty(n1 + 1, **i32)
        self.seg_chunk = torch.empty(n1 + 1, **i32)
        self.chunk_start = torch.empty(n1 + 1, **i32)
        self.chunk_seg = torch.empty(n1, **i32)   # segment id | first (bit 30) | single (bit 31)
        self.chunk_key = torch.empty(n1, **i32)
        self.counts = torch.zeros(8, **i32)   # U, #chunks, #multi-chunk rows, -, bwd big rows, -
        self.multi = torch.empty(n1, **i32)
        self.inv = torch.empty(n1, **i32)
        self.sorted_ex = torch.empty(n1, **i32)
        self.sorted_x = torch.empty(n1, dtype=torch.float32, device=device)
        self.ex_of_occ = torch.empty(n1, **i32)
        self.big_list = torch.empty(n1, **i32)
        self.big_count = self.counts[4:5]     # zeroed with the counts by every GPU dedup
        if device.type == "cuda":
            nbytes = native.hip().dedup_workspace_bytes(n1)
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        else:
            self.ws = None


DEV_ERR_SORT = 1  # hip/fm_common.h kDevErrSort


def check_device_errors(device: torch.device | None = None, clear: bool = True) -> None:
    """Raise if a kernel on ``device`` (default: the current GPU) flagged an invalid result in the
    module's sticky error word since the last check (synchronises the device).  Kernels that cannot
    fail loudly without a host sync set it -- the in-tree radix sort when a look-back spin bound is
    hit -- and the bench / trainer check it at their reporting points.  No-op without a GPU."""
    if device is not None and device.type != "cuda":
        return
    if not torch.cuda.is_available() or not torch.cuda.is_initialized():
        return
    with torch.cuda.device(device if device is not None else torch.cuda.current_device()):
        err = int(native.hip().device_errors(clear))
    if err:
        what = ["radix sort look-back spin bound hit (a dedup plan or AUC was invalid)"] if err & DEV_ERR_SORT else []
        raise RuntimeError(f"device error word {err:#x}: {'; '.join(what) or 'unknown'}")


_SORT_CHECKED: set = set()


def _sort_selfcheck(dev: torch.device) -> None:
    """Once per device and process, before the in-tree sort first groups a batch: its passes are
    stable only if the LDS returns ds_add_rtn ranks in ascending lane order for lanes of one
    instruction that hit the same counter (radix_sort.hip rs_rank_wave) -- measured on gfx950, not
    documented.  Sort a digit-colliding pattern against torch's stable sort; on a mismatch switch the
    dedup to rocPRIM's sort (bitwise the same order) and warn."""
    if dev.index in _SORT_CHECKED or torch.cuda.is_current_stream_capturing():
        return
    _SORT_CHECKED.add(dev.index)
    h = native.hip()
    if not h.sort_algo():
        return
    g = torch.Generator(device="cpu").manual_seed(7)
    n = 3 * 8192 + 77  # several tiles, a partial last one
    keys = (torch.randint(0, 6, (n,), generator=g) * 0x01010101 + torch.randint(0, 2, (n,), generator=g)).to(
        torch.int32).to(dev)  # every digit of every pass collides heavily
    vals = torch.arange(n, dtype=torch.int32, device=dev)
    ko, vo = radix_sort(keys, vals, key_bits=32)
    ref_k, ref_v = torch.sort(keys.long(), stable=True)
    if not (torch.equal(ko.long(), ref_k) and torch.equal(vo, ref_v.to(torch.int32))):
        import warnings

        h.set_sort_algo(0)
        _SORT_UNSTABLE.add(dev.index)
        warnings.warn("in-tree radix sort failed its stability self-check on this device: the dedup uses "
                      "rocPRIM's sort (FM_SORT=rocprim)")


def set_sort_algo(algo: str) -> str:
    """The dedup's sort backend: "fm" (in-tree onesweep radix sort, hip/radix_sort.hip, default) or
    "rocprim" (rocPRIM's onesweep; same stable order); returns the previous one.  FM_SORT=rocprim at
    start-up too."""
    _check(algo in ("rocprim", "fm"), f"sort backend {algo!r}: rocprim or fm")
    h = native.hip()
    was = "fm" if h.sort_algo() else "rocprim"
    h.set_sort_algo(1 if algo == "fm" else 0)
    return was


def radix_sort(keys: torch.Tensor, vals: torch.Tensor, key_bits: int = 32) -> tuple[torch.Tensor, torch.Tensor]:
    """Stable sort of int32 (key, value) pairs by the keys' low ``key_bits`` bits on the in-tree
    radix sort (GPU): returns (sorted keys, values in the same order)."""
    n = keys.numel()
    _chk_vec(keys, torch.int32, n, "keys", keys.device)
    _chk_vec(vals, torch.int32, n, "vals", keys.device)
    _check(_is_gpu(keys), "radix_sort is a GPU kernel")
    h = native.hip()
    ko, vo = torch.empty_like(keys), torch.empty_like(vals)
    ws = torch.empty(max(1, int(h.radix_sort_ws_bytes(n))), dtype=torch.uint8, device=keys.device)
    h.radix_sort(keys=_p(keys), vals=_p(vals), kout=_p(ko), vout=_p(vo), n=n, end_bit=int(key_bits), ws=_p(ws),
                 ws_bytes=ws.numel(), stream=_stream(keys))
    return ko, vo


def slot_bits_for(B: int, max_feats: int) -> int:
    """Bits of the in-example slot of a packed occurrence code, or 0 when codes do not fit int32."""
    if max_feats is None or max_feats < 1:
        return 0
    sb = max(1, (max_feats - 1).bit_length())
    return sb if (B << sb) < 2**31 else 0


def csr_rows(offsets: torch.Tensor, out: torch.Tensor | None = None, nnz: int | None = None,
             slot_bits: int = 0) -> torch.Tensor:
    """Example index of every CSR occurrence (the reference gets it implicitly from feature_poses).

    With ``slot_bits > 0`` (GPU) the packed code ``example << slot_bits | slot`` instead:
    the dedup sort carries it and decodes example and occurrence index from it.
    """
    B = offsets.numel() - 1
    if nnz is None:
        nnz = int(offsets[-1])
    if out is None:
        out = torch.empty(nnz, dtype=torch.int32, device=offsets.device)
    if _is_gpu(offsets):
        native.hip().csr_rows(B=B, offsets=_p(offsets), ex_of_occ=_p(out), slot_bits=int(slot_bits),
                              stream=_stream(offsets))
    else:
        _check(slot_bits == 0, "packed occurrence codes are a GPU path")
        native.cpu().csr_rows(B=B, offsets=_p(offsets), ex_of_occ=_p(out))
    return out


# FM_DEDUP_FUSE=0: the dedup's producers (shard_keys, csr_rows) as separate kernels (A/B switch)
_FUSE_PRODUCERS = os.environ.get("FM_DEDUP_FUSE", "1") != "0"


def dedup(keys: torch.Tensor, *, ws: DedupWorkspace | None = None, key_bits: int = 32,
          ex_of_occ: torch.Tensor | None = None, vals: torch.Tensor | None = None, want_inv: bool = False,
          CH: int | None = None, want_perm: bool = False, num_examples: int | None = None,
          Kp: int | None = None, ex_shift: int = 0, offsets: torch.Tensor | None = None,
          gen_codes: bool = False, shard_ids: torch.Tensor | None = None,
          shard: tuple[int, int] | None = None) -> DedupOut:
    """Sort-based unique over non-negative int32 keys (reference tf.unique, fm_model.py:72).

    Unique keys come out in ascending order (the reference's first-occurrence
    order is an implementation detail no result depends on).  On the GPU the
    result also carries the backward's chunk plan.  When neither the inverse
    map, per-occurrence values nor the occurrence permutation are needed, the
    sort carries the example index directly (one gather pass less).
    (``num_examples`` / ``Kp`` are accepted for interface stability; the plan does not use them.)

    Fused producers (GPU; folded into the in-tree sort's histogram / first pass, the separate kernels
    first under FM_SORT=rocprim): ``gen_codes`` -- the occurrence codes ``csr_rows(offsets,
    slot_bits=ex_shift)`` (``ex_of_occ`` not given); ``shard_ids`` + ``shard = (world, rows_per_shard)``
    -- ``keys`` is the OUTPUT buffer of ``shard_keys(shard_ids, ...)``.
    """
    dev = keys.device
    n = keys.numel()
    _chk_vec(keys, torch.int32, n, "keys", dev)
    if ws is None or ws.cap < n:
        ws = DedupWorkspace(max(n, 1), dev, CH or 32)
    CH = CH or ws.CH
    fuse_ids = 0
    if shard_ids is not None:
        _check(shard is not None and shard_ids.numel() == n, "shard_ids needs shard=(world, rows_per_shard)")
        if _FUSE_PRODUCERS and _is_gpu(keys) and shard_ids.dtype == torch.int32 and shard_ids.is_contiguous():
            _check(shard[0] * shard[1] < 2**31, "sharded keys must fit int32")
            fuse_ids = _p(shard_ids)
        else:
            shard_keys(shard_ids, shard[0], shard[1], keys)
    fuse_codes = False
    if gen_codes:
        _check(ex_of_occ is None and offsets is not None, "gen_codes: offsets, no ex_of_occ")
        in_payload = _is_gpu(keys) and not want_perm and (ex_shift > 0 or (vals is None and not want_inv))
        ex_of_occ = ws.ex_of_occ[:n]
        if _FUSE_PRODUCERS and in_payload and offsets.numel() > 1:
            fuse_codes = True     # written into ex_of_occ only by the rocPRIM backend's csr_rows
        else:
            csr_rows(offsets, out=ex_of_occ, nnz=n, slot_bits=ex_shift)
    if ex_of_occ is not None:
        _chk_vec(ex_of_occ, torch.int32, n, "ex_of_occ", dev)
    if vals is not None:
        _chk_vec(vals, torch.float32, n, "vals", dev)
    key_bits = max(1, min(32, int(key_bits)))
    packed = ex_shift > 0
    if packed:  # ex_of_occ holds packed codes (csr_rows slot_bits): the payload decodes to example + occurrence
        _check(_is_gpu(keys) and ex_of_occ is not None and offsets is not None and not want_perm,
               "packed occurrence codes need the GPU, codes and offsets")
    ex_payload = ex_of_occ is not None and _is_gpu(keys) and not want_perm and (
        packed or (vals is None and not want_inv))
    out = DedupOut(n=n, skeys=ws.skeys, perm=ws.perm, uniq=ws.uniq, seg_start=ws.seg_start,
                   seg_chunk=ws.seg_chunk, chunk_start=ws.chunk_start, chunk_seg=ws.chunk_seg,
                   chunk_key=ws.chunk_key, counts=ws.counts,
                   num_unique=ws.counts[:1], inv=ws.inv if want_inv else None,
                   sorted_ex=(ws.perm if ex_payload else ws.sorted_ex) if ex_of_occ is not None else None,
                   sorted_x=ws.sorted_x if vals is not None else None, CH=CH, big_list=ws.big_list,
                   big_count=ws.big_count, multi=ws.multi, ex_shift=int(ex_shift))
    if _is_gpu(keys):
        h = native.hip()
        _check(1 <= CH <= h.MAX_CH, f"CH must be in [1, {h.MAX_CH}]")
        _sort_selfcheck(dev)
        h.dedup(n=n, end_bit=key_bits, CH=CH, keys=_p(keys), payload=_p(ex_of_occ if ex_payload else ws.iota),
                skeys=_p(ws.skeys), spay=_p(ws.perm), uniq=_p(ws.uniq), seg_start=_p(ws.seg_start),
                seg_chunk=_p(ws.seg_chunk), chunk_start=_p(ws.chunk_start), chunk_seg=_p(ws.chunk_seg),
                chunk_key=_p(ws.chunk_key),
                counts=_p(ws.counts), inv=_p(out.inv),
                ex_of_occ=0 if ex_payload else _p(ex_of_occ),
                sorted_ex=0 if ex_payload else _p(out.sorted_ex), vals=_p(vals), sorted_x=_p(out.sorted_x),
                payload_is_ex=int(ex_payload), ex_shift=int(ex_shift), offsets=_p(offsets),
                ws=_p(ws.ws), ws_bytes=ws.ws.numel(), stream=_stream(keys), ids=fuse_ids,
                kW=int(shard[0]) if fuse_ids else 1, kRps=int(shard[1]) if fuse_ids else 0,
                gen_codes=int(fuse_codes), B=offsets.numel() - 1 if fuse_codes else 0)
        out.bwd_fresh = True  # the backward counters were zeroed on this stream
    else:
        U = native.cpu().dedup(n=n, keys=_p(keys), skeys=_p(ws.skeys), perm=_p(ws.perm), uniq=_p(ws.uniq),
                               seg_start=_p(ws.seg_start), inv=_p(out.inv), ex_of_occ=_p(ex_of_occ),
                               sorted_ex=_p(out.sorted_ex), vals=_p(vals), sorted_x=_p(out.sorted_x))
        ws.counts[0] = U
        out.U_host = U
    return out


def feature_importance(contrib: torch.Tensor, dd: DedupOut) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor,
                                                                     torch.Tensor]:
    """Per-feature sums of ``fm_explain``'s contributions over a batch: ``(uniq, count, sum_abs, sum)`` for the
    U distinct ids of ``dd``, a dedup of the batch's ids that kept the occurrence permutation
    (``dedup(ids, want_perm=True)``).  Sums are fp64 in a fixed order (hip/fm_explain.hip: lane-strided
    partial sums over the segment in sorted order, then a butterfly): bitwise repeatable.  Synchronises
    for U."""
    dev = contrib.device
    _chk_vec(contrib, torch.float32, dd.n, "contrib", dev)
    _check(dd.perm is not None and dd.sorted_ex is not dd.perm and dd.ex_shift == 0,
           "feature_importance: the dedup must carry the occurrence permutation (want_perm=True)")
    _check(dd.perm.device == dev, "contrib: expected the dedup's device")
    U = dd.sync()
    uniq = dd.uniq[:U]
    count = torch.empty(U, dtype=torch.int32, device=dev)
    sum_abs = torch.empty(U, dtype=torch.float64, device=dev)
    total = torch.empty(U, dtype=torch.float64, device=dev)
    if U == 0:
        return uniq, count, sum_abs, total
    if _is_gpu(contrib):
        native.hip().importance(U=U, contrib=_p(contrib), perm=_p(dd.perm), seg_start=_p(dd.seg_start),
                                count=_p(count), sum_abs=_p(sum_abs), sum=_p(total), stream=_stream(contrib))
    else:
        seg = dd.seg_start[: U + 1].long()
        count.copy_(seg[1:] - seg[:-1])
        c = contrib[dd.perm[: dd.n].long()].double()
        which = torch.repeat_interleave(torch.arange(U), count.long())
        sum_abs.zero_().index_add_(0, which, c.abs())
        total.zero_().index_add_(0, which, c)
    return uniq, count, sum_abs, total


# ---------------------------------------------------------------------------
# backward (+ optimizer)
# ---------------------------------------------------------------------------
@dataclass
class TableState:
    """Parameters and optimizer slots of one (local) table shard."""

    v: torch.Tensor                 # [rows, Kp] fp32 / bf16 / fp8
    w: torch.Tensor                 # [rows] fp32
    s0v: torch.Tensor | None = None  # adagrad accumulator / ftrl n   [rows, Kp] state_dtype(v.dtype)
    s1v: torch.Tensor | None = None  # ftrl z                          [rows, Kp] state_dtype(v.dtype)
    s0w: torch.Tensor | None = None  # [rows] fp32
    s1w: torch.Tensor | None = None  # [rows] fp32

    def __post_init__(self):
        want = state_dtype(self.v.dtype)
        for name in ("s0v", "s1v"):
            t = getattr(self, name)
            _check(t is None or t.dtype == want, f"{name}: {want} optimizer state for a {self.v.dtype} table")


def state_dtype(table_dtype: torch.dtype) -> torch.dtype:
    """Storage of the per-factor optimizer state: fp32, bf16 for fp8 tables (hip/fm_common.h
    StateBf16: 8 mantissa bits with stochastic rounding next to factors carrying 3; halves the
    state bytes of the row read-modify-write)."""
    return torch.bfloat16 if table_dtype == FP8 else torch.float32


@dataclass
class SelfRows:
    """Row-sharded step (GPU): segments ``[u0, u1)`` of a batch's sorted unique keys ``keys``
    are this rank's own table rows (row = key - ``base``).  ``fm_forward`` / ``fm_backward``
    read them from ``table`` instead of the gathered wire rows, and the backward applies the
    optimizer in place to the exclusive ones (``excl`` int32 [u1 - u0], 1 = no other rank
    requested the row this step; None = all, world 1) -- hip/fm_common.h SelfRows."""

    u0: int
    u1: int
    base: int
    keys: torch.Tensor
    table: TableState
    excl: torch.Tensor | None = None

    def packed(self) -> list[int]:
        """The binding's form: [u0, u1, base, keys, excl, v, v_stride, w, w_stride]."""
        t = self.table
        return [self.u0, self.u1, self.base, _p(self.keys), _p(self.excl), _p(t.v), t.v.stride(0), _p(t.w),
                t.w.stride(0)]


def _self_check(sr: SelfRows, v: torch.Tensor, keys: torch.Tensor | None) -> None:
    _check(sr.table.v.dtype == v.dtype, "self rows: the table and the wire rows must share the dtype")
    _check(keys is None or sr.keys.data_ptr() == keys.data_ptr(), "self rows: keys must be the dedup's uniq")
    _check(0 <= sr.u0 <= sr.u1, "self rows: bad segment range")
    if sr.excl is not None:
        _chk_vec(sr.excl, torch.int32, None, "self excl", v.device)
        _check(sr.excl.numel() >= sr.u1 - sr.u0, "self excl too short")


@dataclass
class SegIndex:
    """Bucket index over a dedup's sorted unique keys (``seg_index``): key -> segment."""

    idx: torch.Tensor     # int32 [nb + 1]
    keys: torch.Tensor    # the dedup's uniq (sorted keys)
    shift: int


def seg_lookup_enabled() -> bool:
    """Row-sharded step: segment lookup through a bucket index instead of the dedup's inverse
    map (FM_SEG_LOOKUP, default on; profiles/r2/inv_cost.txt)."""
    return os.environ.get("FM_SEG_LOOKUP", "1") != "0"


def seg_index_bits(nnz: int, key_bits: int) -> tuple[int, int]:
    """(shift, nb) of the key-bucket index: nb ~ nnz / 4 buckets (a power of two in [16, 2^20],
    at most 2^key_bits), bucket = key >> shift over ``key_bits``-bit keys.  A Criteo-shaped
    batch (5.1M occurrences, ~378k unique keys) gets 2^20 buckets: ~0.4 keys per bucket."""
    bb = max(4, min(20, max(1, nnz).bit_length() - 2, key_bits))
    shift = max(0, key_bits - bb)
    return shift, 1 << (key_bits - shift)


def seg_index(dd: DedupOut, key_bits: int, out: torch.Tensor | None = None) -> SegIndex:
    """Build the bucket index of ``dd``'s unique keys on the current stream (GPU, no host sync)."""
    _check(_is_gpu(dd.uniq), "seg_index is a GPU path")
    shift, nb = seg_index_bits(dd.n, key_bits)
    if out is None or out.numel() < nb + 1:
        out = torch.empty(nb + 1, dtype=torch.int32, device=dd.uniq.device)
    native.hip().seg_index(n_max=int(dd.n), uniq=_p(dd.uniq), counts=_p(dd.counts), shift=int(shift), nb=int(nb),
                           idx=_p(out), stream=_stream(dd.uniq))
    return SegIndex(out, dd.uniq, shift)


def partial_rows(n: int, CH: int) -> int:
    """Upper bound on backward chunks (= partial rows) for n occurrences: U + n / CH."""
    return max(n, 1) + max(n, 1) // max(CH, 1) + 1


def fm_backward(dd: DedupOut, dpred: torch.Tensor, r1: torch.Tensor, Kp: int, *, mode: int,
                table: TableState | None = None, opt: OptConfig | None = None,
                src_v: torch.Tensor | None = None, src_w: torch.Tensor | None = None,
                grad_out: torch.Tensor | None = None, reg_v: float = 0.0, reg_w: float = 0.0,
                partial: torch.Tensor | None = None, threads: int = 0, grad_bf16: bool = False,
                sr_counter: torch.Tensor | None = None,
                seg_bounds: torch.Tensor | None = None, piece: int = -1,
                self_rows: SelfRows | None = None) -> torch.Tensor | None:
    """Segmented FM backward over the dedup grouping (reference FmGrad, cc/fm_grad_op.h:59-163).

    Per unique row u with occurrences (i, x):
      g_v = sum x*dpred_i*(r1_i - x*v) + reg_v * n_u * v
      g_w = sum x*dpred_i            + reg_w * n_u * w
    mode=BWD_LOCAL applies ``opt`` in place on ``table`` rows ``uniq[u]``;
    mode=BWD_EMIT writes [g_v, g_w] rows into ``grad_out[u]`` (``src_v``/``src_w``
    hold the gathered parameter rows in unique order).  ``piece`` 0 / 1 with
    ``seg_bounds`` (GPU, int32 [2W+1]) reduces only the segments of every owner's first /
    second part (split backward of the row-sharded exchange); piece 1 must follow piece 0.
    ``self_rows`` (GPU, EMIT): segments in its range are read from its table; the exclusive ones
    get ``opt`` applied in place (with ``sr_counter``) and no gradient row.
    """
    dev = dpred.device
    _check(dd.sorted_ex is not None, "dedup must be run with ex_of_occ")
    _chk_vec(dpred, torch.float32, None, "dpred", dev)
    _check(r1.is_contiguous() and r1.shape[1] == Kp, "r1: [B, Kp] contiguous")
    if mode == BWD_EMIT_TABLE:
        _check(_is_gpu(dpred) and table is not None and grad_out is not None,
               "EMIT_TABLE mode: GPU, table (parameter rows) + dense grad_out")
        v, w = table.v, table.w
        dt = dtype_code(v.dtype)
        s0v = s1v = s0w = s1w = None
        s_stride = 0
        _check(grad_out.dtype == torch.float32 and grad_out.stride(1) == 1 and grad_out.shape[0] >= v.shape[0],
               "grad_out: dense fp32 rows covering the table")
        gstride, gptr = grad_out.stride(0), grad_out.data_ptr()
        g_wcol = Kp
        _check(gstride >= Kp + 2 and gstride % 4 == 0, "grad_out rows: [g_v | g_w | touch | ...], stride % 4 == 0")
    elif mode == BWD_LOCAL:
        _check(table is not None and opt is not None, "LOCAL mode needs table + opt")
        v, w = table.v, table.w
        dt = dtype_code(v.dtype)
        _check(opt.name == "sgd" or table.s0v is not None, "optimizer state missing")
        s_stride = table.s0v.stride(0) if table.s0v is not None else 0
        s0v, s1v, s0w, s1w = table.s0v, table.s1v, table.s0w, table.s1w
        if opt.name == "sgd":  # kernels always touch s0: give them scratch
            s0v, s0w, s_stride = (table.s0v, table.s0w, s_stride)
        gstride, gptr = 0, 0
    else:
        _check(src_v is not None and src_w is not None and grad_out is not None, "EMIT mode needs src + grad_out")
        v, w = src_v, src_w
        dt = dtype_code(v.dtype)  # gathered wire rows: fp32, bf16 or fp8 (+ scale at w + 1)
        s0v = s1v = s0w = s1w = None
        s_stride = 0
        _check(grad_out.dtype == torch.float32 and grad_out.stride(1) == 1, "grad_out: fp32 rows")
        gstride, gptr = grad_out.stride(0), grad_out.data_ptr()
        g_wcol = (Kp * 2 + 15) // 16 * 4 if grad_bf16 else Kp
        _check(gstride >= g_wcol + 1 and gstride % 4 == 0,
               "grad_out row stride must hold the w column and be a multiple of 4")
        _check(not grad_bf16 or _is_gpu(dpred), "bf16 gradient rows are a GPU path")
        if self_rows is not None and self_rows.u1 > self_rows.u0:
            _check(_is_gpu(dpred) and opt is not None, "self rows: GPU path with the optimizer")
            _self_check(self_rows, v, dd.uniq)
            t = self_rows.table
            s0v, s1v, s0w, s1w = t.s0v, t.s1v, t.s0w, t.s1w
            _check(s0v is not None and s0w is not None, "self rows: the table's optimizer state")
            s_stride = s0v.stride(0)
    v_stride = _chk_rows(v, Kp, "v")
    _check(r1.dtype == r1_dtype(v.dtype), f"r1: {r1_dtype(v.dtype)} for {v.dtype} rows (the forward's r1)")
    o = opt or OptConfig()
    if piece >= 0:
        _check(_is_gpu(dpred) and seg_bounds is not None and mode in (BWD_EMIT, BWD_EMIT_TABLE),
               "split backward pieces: GPU, EMIT / EMIT_TABLE, seg_bounds")
        _chk_vec(seg_bounds, torch.int32, 3, "seg_bounds", dev)
    if _is_gpu(dpred):
        h = native.hip()
        if partial is None:
            partial = torch.empty((partial_rows(dd.n, dd.CH), Kp + 4), dtype=torch.float32, device=dev)
        _check(partial.numel() >= partial_rows(dd.n, dd.CH) * (Kp + 4), "partial scratch too small")
        skw = {}
        if mode == BWD_EMIT and self_rows is not None and self_rows.u1 > self_rows.u0:
            skw = dict(self_rows=self_rows.packed())
        h.bwd(mode=mode, counts=_p(dd.counts), chunk_start=_p(dd.chunk_start), chunk_seg=_p(dd.chunk_seg),
              chunk_key=_p(dd.chunk_key),
              seg_start=_p(dd.seg_start), seg_chunk=_p(dd.seg_chunk), uniq=_p(dd.uniq),
              sorted_ex=_p(dd.sorted_ex), ex_shift=int(dd.ex_shift or 0), sorted_x=_p(dd.sorted_x),
              dpred=_p(dpred), r1=_p(r1), Kp=Kp,
              v=_p(v), v_stride=v_stride, w=_p(w), w_stride=w.stride(0), s0v=_p(s0v), s1v=_p(s1v),
              s_stride=s_stride, s0w=_p(s0w), s1w=_p(s1w), reg_v=float(reg_v), reg_w=float(reg_w),
              opt_type=o.code, lr=float(o.lr), l1=float(o.l1), l2=float(o.l2), beta=float(o.beta),
              grad_out=gptr, g_stride=gstride, partial=_p(partial), big_list=_p(dd.big_list),
              big_count=_p(dd.big_count), multi=_p(dd.multi), nex=int(dpred.numel()), dtype=dt, max_chunks=dd.n,
              max_unique=dd.n,
              stream=_stream(dpred), g_wcol=g_wcol if mode != BWD_LOCAL else -1, g_bf16=int(bool(grad_bf16)),
              sr_counter=_p(sr_counter), counters_ready=int(bool(dd.bwd_fresh)),
              seg_bounds=_p(seg_bounds), piece=int(piece),
              n_owners=(seg_bounds.numel() - 1) // 2 if seg_bounds is not None else 0, **skw)
        dd.bwd_fresh = False  # a second backward over this grouping zeroes its counters itself
    else:
        _check(self_rows is None, "self rows are a GPU path")
        U = dd.sync()
        native.cpu().bwd(mode=mode, U=U, seg_start=_p(dd.seg_start), uniq=_p(dd.uniq), sorted_ex=_p(dd.sorted_ex),
                         sorted_x=_p(dd.sorted_x), dpred=_p(dpred), r1=_p(r1), Kp=Kp, v=_p(v), v_stride=v_stride,
                         w=_p(w), w_stride=w.stride(0), s0v=_p(s0v), s1v=_p(s1v), s_stride=s_stride, s0w=_p(s0w),
                         s1w=_p(s1w), reg_v=float(reg_v), reg_w=float(reg_w), opt_type=o.code, lr=float(o.lr),
                         l1=float(o.l1), l2=float(o.l2), beta=float(o.beta), grad_out=gptr, g_stride=gstride,
                         dtype=dt, threads=threads)
    return grad_out


# ---------------------------------------------------------------------------
# validation metric: exact weighted ROC AUC
# ---------------------------------------------------------------------------
class _SortedScoreRecord:
    """What the records of ``auc`` / ``gauc`` / ``isotonic_fit`` share: ``rec``, 64-bit words on the op's device
    whose last one is the sort error word, and ``done``, the event behind the GPU launch chain on its stream
    (None on the CPU, and for a chain captured into a graph: an event recorded into a graph cannot be waited
    for, the reader synchronises with the replay)."""

    __slots__ = ("rec", "weighted", "n", "done")
    _op, _result = "", ""  # for the error message: the op's name, what there is none of

    def __init__(self, rec: torch.Tensor, weighted: bool, n: int, done: "torch.cuda.Event | None" = None):
        self.rec, self.weighted, self.n, self.done = rec, weighted, n, done

    def _host_rec(self) -> torch.Tensor:
        """The record on the host, once the chain has finished; raises on a nonzero sort error word."""
        if self.done is not None:  # (the reader's current stream need not be the chain's)
            self.done.synchronize()
        r = self.rec.cpu()
        err = int(r[-1])
        if err:
            raise RuntimeError(f"{self._op}: the radix sort's look-back spin bound was hit (error word {err}); "
                               f"no {self._result} for this input")
        return r


class AucStats(_SortedScoreRecord):
    """The record of one ``auc`` call, on the op's device: ``[U2, P, N, NaN scores, sort error word]`` --
    int64 (unweighted: exact) or float64 (weighted).  ``stats()`` / ``value()`` read it (a host sync on
    the GPU) and raise when the GPU sort reported a failed look-back: never a number then."""

    __slots__ = ()
    _op, _result = "auc", "AUC"

    def stats(self) -> tuple:
        """(U2, P, N, nans) on the host: Python ints (unweighted) or floats and the int NaN count."""
        u2, p, n, nans, _ = self._host_rec().tolist()
        return u2, p, n, int(nans)

    def value(self) -> float:
        """U2 / (2 P N); NaN when a score is NaN or a class has no weight (undefined, not an error)."""
        u2, p, n, nans = self.stats()
        if nans or not p > 0 or not n > 0:
            return float("nan")
        return u2 / (2 * p * n)


_SORT_UNSTABLE: set = set()  # devices whose in-tree sort failed _sort_selfcheck


def _sorted_score_inputs(op: str, scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None,
                         groups: torch.Tensor | None = None) -> tuple:
    """The input checks of ``auc`` / ``gauc`` / ``isotonic_fit``: fp32 vectors (int32 ``groups``) on one device,
    one entry per score, fewer than 2^30 scores.  Returns (device, n, weighted, record dtype)."""
    dev = scores.device
    n = scores.numel()
    _chk_vec(scores, torch.float32, n, "scores", dev)
    _chk_vec(labels, torch.float32, n, "labels", dev)
    _chk_vec(groups, torch.int32, n, "groups", dev)
    _chk_vec(weights, torch.float32, n, "weights", dev)
    _check(labels.numel() == n and (groups is None or groups.numel() == n)
           and (weights is None or weights.numel() == n),
           f"{op}: one label / {'' if groups is None else 'group / '}weight per score")
    _check(n < 2**30, f"{op}: n must be < 2^30 (the radix sort's bound)")
    weighted = weights is not None
    return dev, n, weighted, torch.float64 if weighted else torch.int64


def _sorted_score_launch(op: str, dev: torch.device, need: int, ws: torch.Tensor | None, launch) -> tuple:
    """The GPU launch of those ops: the sort's self-check, the workspace (``need`` bytes; allocated when ``ws`` is
    None), ``launch(ws)`` on the current stream.  Returns (ws, the event behind the chain on that stream -- None
    while the stream is capturing: an event recorded into a graph cannot be waited for, the reader synchronises
    with the replay)."""
    _sort_selfcheck(dev)
    if dev.index in _SORT_UNSTABLE:
        raise RuntimeError(f"{op}: the in-tree radix sort failed its stability self-check on this device")
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk_vec(ws, torch.uint8, need, "ws", dev)
    launch(ws)
    if torch.cuda.is_current_stream_capturing():
        return ws, None
    done = torch.cuda.Event()
    done.record(torch.cuda.current_stream(dev))
    return ws, done


def auc_workspace(n: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``auc`` for up to ``n`` scores (GPU)."""
    return torch.empty(int(native.hip().auc_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def auc(scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None = None, *,
        ws: torch.Tensor | None = None) -> AucStats:
    """Exact weighted ROC AUC statistics of raw scores (logits: the sigmoid is monotone).

    An example is positive iff ``label > 0`` (0/1 and -1/+1 labels alike); ``weights`` None = all ones.
    With P / N the weight of the positives / negatives, U2 = sum over positives of w_i (Nlt(s_i) +
    Nle(s_i)) (Nlt / Nle: weight of the negatives with a score below / not above s_i) and AUC = U2 /
    (2 P N): a positive-negative tie counts one half.  Scores compare as IEEE fp32 values (-0.0 == +0.0,
    infinities and denormals ordered as usual); NaN scores are counted and make the AUC NaN.
    Unweighted statistics are integers (exact, the same on GPU and CPU); weighted ones are fp64 sums in a
    fixed order (bitwise the same run to run).  GPU: hip/auc.hip on the current stream (``ws``: reusable
    ``auc_workspace``); CPU: a sort and one pass.  ``n == 0`` launches nothing (NaN).  With a caller's ``ws`` the
    GPU chain can be captured into a graph (after one eager call on the device: the sort's self-check does not
    run in a capture); the record of a captured call carries no event, so read it after synchronising with the
    replay.
    """
    dev, n, weighted, rdt = _sorted_score_inputs("auc", scores, labels, weights)
    if _DEBUG and weighted and n > 0 and not (scores.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check(bool(weights.min() >= 0), "weights: must be >= 0")
    if n == 0:
        return AucStats(torch.zeros(5, dtype=rdt), weighted, 0)  # (a host record: nothing is launched)
    rec = torch.empty(5, dtype=rdt, device=dev)
    if _is_gpu(scores):
        h = native.hip()
        _, done = _sorted_score_launch("auc", dev, int(h.auc_workspace_bytes(n)), ws, lambda w: h.auc(
            scores=_p(scores), labels=_p(labels), weights=_p(weights), n=n, out=_p(rec), ws=_p(w),
            ws_bytes=w.numel(), stream=_stream(scores)))
        return AucStats(rec, weighted, n, done)
    _check(ws is None, "auc: the workspace is a GPU argument")
    native.cpu().auc(n=n, scores=_p(scores), labels=_p(labels), weights=_p(weights), out=_p(rec))
    return AucStats(rec, weighted, n)


# ---------------------------------------------------------------------------
# AUC confidence intervals and paired model comparison (DeLong)
# ---------------------------------------------------------------------------
_DELONG_WORDS = 20    # csrc/hip/auc_delong.hip: kDelongRecWords
_DELONG_MOMENTS = ("m_pos_aa", "m_neg_aa", "m_pos_bb", "m_neg_bb", "m_pos_ab", "m_neg_ab")  # words 4.., (hi, lo) each


class DelongStats(_SortedScoreRecord):
    """The record of one ``auc_delong`` call, on the op's device: 20 int64 words ``[U2_a, U2_b, P, N, (hi, lo) of
    M_pos(a,a), M_neg(a,a), M_pos(b,b), M_neg(b,b), M_pos(a,b), M_neg(a,b), NaN scores of a, of b, has_b, sort error
    word]``; a second moment is ``(hi << 32) + lo``.  The readers synchronise with the launch chain on the GPU,
    raise when the GPU sort reported a failed look-back, finish the arithmetic in Python integers and fractions
    and convert to float once at the end: a GPU record and a CPU record give identical floats.  Values that are
    undefined (a NaN score in either model, an empty class; for the variances a class of one) are NaN."""

    __slots__ = ()
    _op, _result = "auc_delong", "DeLong statistics"

    def stats(self) -> dict:
        """The exact Python ints: ``U2_a``, ``U2_b``, ``P``, ``N``, the six second moments ``m_pos_aa`` ...
        ``m_neg_ab``, ``nans_a``, ``nans_b`` and ``has_b``."""
        w = [int(x) for x in self._host_rec().tolist()]
        st = {"U2_a": w[0], "U2_b": w[1], "P": w[2], "N": w[3], "nans_a": w[16], "nans_b": w[17], "has_b": w[18]}
        for i, name in enumerate(_DELONG_MOMENTS):
            st[name] = (w[4 + 2 * i] << 32) + w[5 + 2 * i]
        return st

    def _stats_for(self, other: bool) -> dict:
        st = self.stats()
        if other and not st["has_b"]:
            raise ValueError("auc_delong: the call had no other model")
        return st

    @staticmethod
    def _theta(st: dict, m: str):
        """The AUC of model ``m`` as a Fraction, or None where it is undefined."""
        if st["nans_a"] or st["nans_b"] or st["P"] < 1 or st["N"] < 1:
            return None
        return Fraction(st["U2_" + m], 2 * st["P"] * st["N"])

    @staticmethod
    def _cov(st: dict, x: str, y: str):
        """cov(theta_x, theta_y) as a Fraction, or None where it is undefined."""
        P, N = st["P"], st["N"]
        if st["nans_a"] or st["nans_b"] or P < 2 or N < 2:
            return None
        uu = st["U2_" + x] * st["U2_" + y]
        s10 = Fraction(st["m_pos_" + x + y] * P - uu, 4 * N * N * P * (P - 1))
        s01 = Fraction(st["m_neg_" + x + y] * N - uu, 4 * P * P * N * (N - 1))
        return s10 / P + s01 / N

    def auc(self) -> float:
        """U2_a / (2 P N), the value ``auc`` returns."""
        t = self._theta(self.stats(), "a")
        return _NAN if t is None else float(t)

    def auc_other(self) -> float:
        """The other model's AUC."""
        t = self._theta(self._stats_for(True), "b")
        return _NAN if t is None else float(t)

    def variance(self) -> float:
        """DeLong's variance of the AUC: S10 / P + S01 / N."""
        v = self._cov(self.stats(), "a", "a")
        return _NAN if v is None else float(v)

    def std_error(self) -> float:
        v = self.variance()
        return _NAN if v != v else math.sqrt(v)

    def interval(self, level: float = 0.95) -> tuple:
        """(lo, hi) = AUC -+ z se clipped to [0, 1], z the normal quantile of (1 + level) / 2."""
        _check(isinstance(level, (int, float)) and 0.0 < level < 1.0, "auc_delong: the level must be in (0, 1)")
        a, se = self.auc(), self.std_error()
        if a != a or se != se:
            return _NAN, _NAN
        z = statistics.NormalDist().inv_cdf((1 + level) / 2)
        return max(0.0, a - z * se), min(1.0, a + z * se)

    def covariance(self) -> float:
        """DeLong's covariance of the two models' AUCs."""
        v = self._cov(self._stats_for(True), "a", "b")
        return _NAN if v is None else float(v)

    def difference(self) -> tuple:
        """(AUC - other's AUC, its standard error, z, two-sided p) of the paired comparison: var = var_a + var_b -
        2 cov, z = diff / se, p = erfc(|z| / sqrt 2).  Without variance: z 0 and p 1 for equal AUCs, else z +-inf
        and p 0."""
        st = self._stats_for(True)
        ta, tb = self._theta(st, "a"), self._theta(st, "b")
        if ta is None:
            return _NAN, _NAN, _NAN, _NAN
        diff = ta - tb
        va = self._cov(st, "a", "a")
        if va is None:
            return float(diff), _NAN, _NAN, _NAN
        var = va + self._cov(st, "b", "b") - 2 * self._cov(st, "a", "b")
        se = math.sqrt(float(var)) if var > 0 else 0.0
        if var > 0 and se > 0.0:
            z = float(diff) / se
        else:
            z = 0.0 if diff == 0 else math.copysign(math.inf, diff)
        return float(diff), se, z, math.erfc(abs(z) / math.sqrt(2.0))


def delong_workspace(n: int, device: torch.device, two_models: bool = True) -> torch.Tensor:
    """Device scratch of ``auc_delong`` for up to ``n`` scores of one or (also) two models (GPU)."""
    return torch.empty(int(native.hip().delong_workspace_bytes(int(n), bool(two_models))), dtype=torch.uint8,
                       device=device)


def auc_delong(scores: torch.Tensor, labels: torch.Tensor, other: torch.Tensor | None = None, *,
               ws: torch.Tensor | None = None) -> DelongStats:
    """DeLong, DeLong & Clarke-Pearson (1988) statistics of raw scores: the variance of the ROC AUC and, with the
    scores ``other`` of a second model on the same examples in the same order, the covariance of the two AUCs --
    a confidence interval and a paired test without resampling.

    With ``auc``'s conventions (positive iff ``label > 0``, scores compare as IEEE fp32 values, -0.0 == +0.0, NaN
    scores are counted per model and make every value NaN) a positive's placement is a_i = Nlt(s_i) + Nle(s_i)
    (the negatives below plus the negatives not above) and a negative's b_j = Pgt(s_j) + Pge(s_j); U2 = sum of the
    a_i = sum of the b_j, AUC = U2 / (2 P N), and with M_pos(x, y) / M_neg(x, y) the sums of the products of the
    positives' / negatives' placements under models x and y
        S10 = (M_pos P - U2_x U2_y) / (4 N^2 P (P - 1)),  S01 = (M_neg N - U2_x U2_y) / (4 P^2 N (N - 1)),
        cov(x, y) = S10 / P + S01 / N,  var(x) = cov(x, x).
    Every statistic is an integer (the same on GPU and CPU, whatever the order of the sums).  There are no
    ``weights``: the variance of a weighted AUC depends on what the weights mean (frequencies, costs, sampling
    rates), and ``evaluate``, the user of this op, has none.  GPU: hip/auc_delong.hip on the current stream
    (``ws``: reusable ``delong_workspace``; graph capture as for ``auc``); CPU: a sort per model and two passes.
    ``n == 0`` launches nothing.
    """
    dev, n, _, rdt = _sorted_score_inputs("auc_delong", scores, labels, None)
    if other is not None:
        _check(other.device == dev, "auc_delong: other must be on the scores' device")
        _chk_vec(other, torch.float32, n, "other", dev)
        _check(other.numel() == n, "auc_delong: one score of the other model per score")
    if n == 0:
        rec = torch.zeros(_DELONG_WORDS, dtype=rdt)  # (a host record: nothing is launched)
        rec[18] = int(other is not None)
        return DelongStats(rec, False, 0)
    rec = torch.empty(_DELONG_WORDS, dtype=rdt, device=dev)
    if _is_gpu(scores):
        h = native.hip()
        _, done = _sorted_score_launch(
            "auc_delong", dev, int(h.delong_workspace_bytes(n, other is not None)), ws, lambda w: h.auc_delong(
                scores_a=_p(scores), scores_b=_p(other), labels=_p(labels), n=n, out=_p(rec), ws=_p(w),
                ws_bytes=w.numel(), stream=_stream(scores)))
        return DelongStats(rec, False, n, done)
    _check(ws is None, "auc_delong: the workspace is a GPU argument")
    native.cpu().auc_delong(n=n, scores_a=_p(scores), scores_b=_p(other), labels=_p(labels), out=_p(rec))
    return DelongStats(rec, False, n)


def placement_moments(pl_a: torch.Tensor, pl_b: torch.Tensor | None, labels: torch.Tensor) -> torch.Tensor:
    """The moments step of ``auc_delong`` on its own: the 12 int64 words (hi, lo) of M_pos(a,a), M_neg(a,a),
    M_pos(b,b), M_neg(b,b), M_pos(a,b), M_neg(a,b) of placements given as int32 vectors (read as uint32; ``pl_b``
    None: the (a,a) words, the rest 0), on the placements' device.  Every product t adds ``t >> 32`` to its hi
    word and ``t & 0xffffffff`` to its lo word."""
    dev, n = pl_a.device, pl_a.numel()
    _chk_vec(pl_a, torch.int32, n, "pl_a", dev)
    _chk_vec(pl_b, torch.int32, n, "pl_b", dev)
    _chk_vec(labels, torch.float32, n, "labels", dev)
    _check(labels.numel() == n and (pl_b is None or pl_b.numel() == n), "placement_moments: one label per placement")
    _check(n < 2**30, "placement_moments: n must be < 2^30")
    if n == 0:
        return torch.zeros(12, dtype=torch.int64, device=dev)
    out = torch.empty(12, dtype=torch.int64, device=dev)
    if _is_gpu(pl_a):
        h = native.hip()
        ws = torch.empty(int(h.delong_moments_workspace_bytes(n)), dtype=torch.uint8, device=dev)
        h.delong_moments(pl_a=_p(pl_a), pl_b=_p(pl_b), labels=_p(labels), n=n, out=_p(out), ws=_p(ws),
                         ws_bytes=ws.numel(), stream=_stream(pl_a))
    else:
        native.cpu().delong_moments(n=n, pl_a=_p(pl_a), pl_b=_p(pl_b), labels=_p(labels), out=_p(out))
    return out


# ---------------------------------------------------------------------------
# threshold metrics: average precision, KS, best F1, operating points
# ---------------------------------------------------------------------------
_THR_MAX_TARGETS = 4                                 # csrc/threshold_rule.h: kMaxTargets
_THR_POINT0, _THR_POINTS = 3, 2 + 2 * _THR_MAX_TARGETS  # ... kPoint0, kPoints
_THR_WORDS = _THR_POINT0 + 3 * _THR_POINTS + 2       # ... kRecWords
_NAN = float("nan")


def threshold_targets(targets, what: str = "targets") -> tuple:
    """``targets`` (a number or a sequence) as a tuple of floats: 0 to 4 values, each in (0, 1]."""
    if isinstance(targets, (int, float)):
        targets = (targets,)
    t = tuple(float(x) for x in targets)
    _check(len(t) <= _THR_MAX_TARGETS and all(0.0 < x <= 1.0 for x in t),
           f"threshold_metrics: {what} must be 0 to {_THR_MAX_TARGETS} values in (0, 1]")
    return t


class ThresholdStats(_SortedScoreRecord):
    """The record of one ``threshold_metrics`` call, on the op's device: 35 64-bit words (csrc/threshold_rule.h)
    ``[AP numerator (fp64 bits), P, N, 10 points of (TP, FP, fp32 bits of the threshold): KS, best F1, the
    precision targets, the recall targets, NaN scores, sort error word]`` -- int64 (unweighted: exact) or float64
    (weighted).  The readers synchronise with the launch chain on the GPU and raise when the GPU sort reported a
    failed look-back: never a number then."""

    __slots__ = ("precision_targets", "recall_targets")
    _op, _result = "threshold_metrics", "threshold metrics"

    def __init__(self, rec: torch.Tensor, weighted: bool, n: int, precision_targets: tuple, recall_targets: tuple,
                 done: "torch.cuda.Event | None" = None):
        super().__init__(rec, weighted, n, done)
        self.precision_targets, self.recall_targets = precision_targets, recall_targets

    def stats(self) -> dict:
        """The record on the host: ``ap_num`` (float), ``P``, ``N`` (Python ints unweighted, else floats),
        ``nans``, and the points ``ks``, ``best_f1``, ``precision`` (one per target), ``recall`` (one per target):
        each ``(TP, FP, threshold)`` or None when there is no such threshold."""
        r = self._host_rec()
        ap_num = float(r[:1].view(torch.float64)[0])
        w = r.tolist()

        def point(s: int):
            tp, fp, bits = w[_THR_POINT0 + 3 * s: _THR_POINT0 + 3 * s + 3]
            if not tp + fp > 0:
                return None
            return tp, fp, struct.unpack("<f", struct.pack("<I", int(bits)))[0]

        np_, nr = len(self.precision_targets), len(self.recall_targets)
        return {"ap_num": ap_num, "P": w[1], "N": w[2], "nans": int(w[-2]), "ks": point(0), "best_f1": point(1),
                "precision": [point(2 + i) for i in range(np_)],
                "recall": [point(2 + _THR_MAX_TARGETS + i) for i in range(nr)]}

    @staticmethod
    def _defined(st: dict) -> bool:
        return not st["nans"] and st["P"] > 0 and st["N"] > 0

    def ap(self) -> float:
        """Average precision; NaN when a score is NaN or a class has no weight (undefined, not an error)."""
        st = self.stats()
        return st["ap_num"] / st["P"] if self._defined(st) else _NAN

    def ks(self) -> tuple:
        """(KS, its threshold): max over thresholds of |TP / P - FP / N|, at the highest such score."""
        st = self.stats()
        if not self._defined(st) or st["ks"] is None:
            return _NAN, _NAN
        tp, fp, t = st["ks"]
        P, N = st["P"], st["N"]
        return (abs(tp / P - fp / N) if self.weighted else abs(tp * N - fp * P) / (P * N)), t

    @staticmethod
    def _pr(point, P) -> tuple:
        tp, fp, t = point
        return t, tp / (tp + fp), tp / P

    def best_f1(self) -> tuple:
        """(F1, threshold, precision, recall) of the threshold with the greatest F1 (the highest such score)."""
        st = self.stats()
        if not self._defined(st) or st["best_f1"] is None:
            return _NAN, _NAN, _NAN, _NAN
        tp, fp, _ = st["best_f1"]
        return (2 * tp / ((tp + fp) + st["P"]), *self._pr(st["best_f1"], st["P"]))

    def _at(self, kind: str, targets: tuple, target: float) -> tuple:
        _check(float(target) in targets, f"threshold_metrics: {target} is not one of the call's {kind} targets")
        st = self.stats()
        point = st[kind][targets.index(float(target))]
        if not self._defined(st) or point is None:
            return _NAN, _NAN, _NAN
        return self._pr(point, st["P"])

    def at_precision(self, target: float) -> tuple:
        """(threshold, precision, recall) of the greatest recall with precision >= ``target`` (one of the call's
        ``precision_targets``); NaNs when no threshold reaches it."""
        return self._at("precision", self.precision_targets, target)

    def at_recall(self, target: float) -> tuple:
        """(threshold, precision, recall) of the highest threshold with recall >= ``target`` (one of the call's
        ``recall_targets``)."""
        return self._at("recall", self.recall_targets, target)


def threshold_workspace(n: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``threshold_metrics`` for up to ``n`` scores (GPU)."""
    return torch.empty(int(native.hip().threshold_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def threshold_metrics(scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None = None, *,
                      precision_targets=(), recall_targets=(), ws: torch.Tensor | None = None) -> ThresholdStats:
    """Average precision, KS, best F1 and operating points of raw scores, with ``auc``'s conventions: an example
    is positive iff ``label > 0``, ``weights`` None = all ones, scores compare as IEEE fp32 values (-0.0 == +0.0),
    NaN scores are counted and make every value NaN, as does a class without weight.

    Every distinct score t is a candidate threshold "positive iff score >= t" (a run of equal scores is never
    split) with TP(t) / FP(t) the weight of the positives / negatives at or above it and PP = TP + FP > 0:
    AP = (1 / P) sum over the positives of w_i TP(s_i) / PP(s_i) (scikit-learn's ``average_precision_score``);
    KS = max |TP / P - FP / N|; best F1 = max 2 TP / (PP + P); a precision target pi (0 to 4, each in (0, 1]):
    the greatest TP among the thresholds with TP >= pi PP; a recall target rho: the highest threshold with
    TP >= rho P.  Equal maxima resolve to the highest score; a reported threshold is the run's score (+0.0 for
    either zero).  Unweighted statistics are integers and every selection is exact (the same on GPU and CPU);
    weighted ones are fp64 sums of non-negative terms from the highest score down, in a fixed order (bitwise the
    same run to run).  GPU: hip/threshold_metrics.hip on the current stream (``ws``: reusable
    ``threshold_workspace``; graph capture as for ``auc``); CPU: a sort and one pass.  ``n == 0`` launches nothing.
    """
    dev, n, weighted, rdt = _sorted_score_inputs("threshold_metrics", scores, labels, weights)
    pt = threshold_targets(precision_targets, "precision_targets")
    rt = threshold_targets(recall_targets, "recall_targets")
    if _DEBUG and weighted and n > 0 and not (scores.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check(bool(weights.min() >= 0), "weights: must be >= 0")
    if n == 0:
        return ThresholdStats(torch.zeros(_THR_WORDS, dtype=rdt), weighted, 0, pt, rt)  # (nothing is launched)
    rec = torch.empty(_THR_WORDS, dtype=rdt, device=dev)
    if _is_gpu(scores):
        h = native.hip()
        _, done = _sorted_score_launch(
            "threshold_metrics", dev, int(h.threshold_workspace_bytes(n)), ws, lambda w: h.threshold_metrics(
                scores=_p(scores), labels=_p(labels), weights=_p(weights), n=n, precision_targets=list(pt),
                recall_targets=list(rt), out=_p(rec), ws=_p(w), ws_bytes=w.numel(), stream=_stream(scores)))
        return ThresholdStats(rec, weighted, n, pt, rt, done)
    _check(ws is None, "threshold_metrics: the workspace is a GPU argument")
    native.cpu().threshold_metrics(n=n, scores=_p(scores), labels=_p(labels), weights=_p(weights),
                                   precision_targets=list(pt), recall_targets=list(rt), out=_p(rec))
    return ThresholdStats(rec, weighted, n, pt, rt)


# ---------------------------------------------------------------------------
# validation metric: grouped AUC (GAUC)
# ---------------------------------------------------------------------------
class GaucStats(_SortedScoreRecord):
    """The record of one ``gauc`` call, on the op's device: six 64-bit words ``[sum over the valid groups of
    W_g AUC_g (fp64), their sum of W_g, valid groups, examples in valid groups, NaN scores, sort error word]``
    (the sum of W_g is an integer without weights, fp64 with them) and ``groups``, the ``[G, 3]`` per-group
    ``(U2_g, P_g, N_g)`` (int64 / float64).  The readers synchronise with the launch chain on the GPU and raise
    when its sort reported a failed look-back: never a number then."""

    __slots__ = ("groups", "num_groups")
    _op, _result = "gauc", "GAUC"

    def __init__(self, rec: torch.Tensor, groups: torch.Tensor, weighted: bool, n: int, num_groups: int,
                 done: "torch.cuda.Event | None" = None):
        super().__init__(rec, weighted, n, done)
        self.groups, self.num_groups = groups, num_groups

    def stats(self) -> tuple:
        """(sum W AUC, sum W, valid groups, examples in valid groups, nans) on the host."""
        r = self._host_rec()
        f = r.view(torch.float64).tolist()
        i = r.tolist()
        return f[0], (f[1] if self.weighted else i[1]), i[2], i[3], i[4]

    def value(self) -> float:
        """sum W_g AUC_g / sum W_g over the valid groups; NaN when there is none or a score is NaN."""
        wa, w, valid, _, nans = self.stats()
        if nans or not valid or not w > 0:
            return float("nan")
        return wa / w

    def valid_groups(self) -> int:
        """Groups with positive and negative weight (the ones GAUC averages)."""
        return self.stats()[2]

    def coverage(self) -> float:
        """Share of the examples that lie in valid groups (NaN for an empty set)."""
        return self.stats()[3] / self.n if self.n else float("nan")

    def per_group(self) -> torch.Tensor:
        """The ``[G, 3]`` tensor ``(U2_g, P_g, N_g)`` on the op's device; zeros for empty groups."""
        self.stats()
        return self.groups


def gauc_workspace(n: int, num_groups: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``gauc`` for up to ``n`` scores in ``num_groups`` groups (GPU)."""
    return torch.empty(int(native.hip().gauc_workspace_bytes(int(n), int(num_groups))), dtype=torch.uint8,
                       device=device)


def gauc(scores: torch.Tensor, labels: torch.Tensor, groups: torch.Tensor, num_groups: int,
         weights: torch.Tensor | None = None, *, ws: torch.Tensor | None = None) -> GaucStats:
    """Grouped AUC statistics of raw scores: ``auc``'s statistics of every group on its own, and their mean.

    ``groups``: int32 ids in ``[0, num_groups)``, one per score (a user, a query, a session).  Per group g, with
    ``auc``'s conventions (positive iff ``label > 0``, the same score order, a tie counts one half): P_g, N_g,
    U2_g over the group's examples only; g is valid iff P_g > 0 and N_g > 0, AUC_g = U2_g / (2 P_g N_g), W_g =
    P_g + N_g and GAUC = sum_valid W_g AUC_g / sum_valid W_g -- NaN without a valid group or with a NaN score.
    Unweighted per-group records are integers (exact, the same on GPU and CPU); weighted ones are fp64 sums of
    the group's own non-negative terms in a fixed order (bitwise the same run to run).  GPU: hip/gauc.hip on
    the current stream (``ws``: reusable ``gauc_workspace``); CPU: a sort and one pass per group.  ``n == 0``
    launches nothing (NaN).  Ids outside the range are an error with FM_DEBUG_CHECKS=1 and count as the last
    group without it.
    """
    G = int(num_groups)
    dev, n, weighted, rdt = _sorted_score_inputs("gauc", scores, labels, weights, groups)
    _check(1 <= G < 2**31, "gauc: num_groups must be in [1, 2^31)")
    if _DEBUG and n > 0 and not (scores.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check(bool(groups.min() >= 0) and bool(groups.max() < G), "groups: ids must be in [0, num_groups)")
        if weighted:
            _check(bool(weights.min() >= 0), "weights: must be >= 0")
    if n == 0:  # (host records: nothing is launched)
        return GaucStats(torch.zeros(6, dtype=torch.int64), torch.zeros((G, 3), dtype=rdt), weighted, 0, G)
    rec = torch.empty(6, dtype=torch.int64, device=dev)
    per = torch.empty((G, 3), dtype=rdt, device=dev)
    if _is_gpu(scores):
        h = native.hip()
        _, done = _sorted_score_launch("gauc", dev, int(h.gauc_workspace_bytes(n, G)), ws, lambda w: h.gauc(
            scores=_p(scores), labels=_p(labels), weights=_p(weights), groups=_p(groups), n=n, G=G, out=_p(rec),
            rec=_p(per), ws=_p(w), ws_bytes=w.numel(), stream=_stream(scores)))
        return GaucStats(rec, per, weighted, n, G, done)
    _check(ws is None, "gauc: the workspace is a GPU argument")
    native.cpu().gauc(n=n, G=G, scores=_p(scores), labels=_p(labels), weights=_p(weights), groups=_p(groups),
                      out=_p(rec), rec=_p(per))
    return GaucStats(rec, per, weighted, n, G)


# ---------------------------------------------------------------------------
# ranking metrics per group: NDCG@k, recall@k, precision@k
# ---------------------------------------------------------------------------
RANK_MAX_CUTOFF = 4096  # csrc/rank_table.h
RANK_MAX_CUTOFFS = 4


def rank_cutoffs(cutoffs) -> tuple:
    """``cutoffs`` as a tuple of ints; ``ValueError`` unless 1 to 4 strictly ascending integers in [1, 4096]."""
    try:
        ks = tuple(cutoffs)
    except TypeError:
        ks = (cutoffs,)
    ok = 1 <= len(ks) <= RANK_MAX_CUTOFFS and all(
        isinstance(k, int) and not isinstance(k, bool) and 1 <= k <= RANK_MAX_CUTOFF for k in ks)
    if not ok or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError("rank_metrics: cutoffs must be 1 to %d strictly ascending integers in [1, %d], got %r"
                         % (RANK_MAX_CUTOFFS, RANK_MAX_CUTOFF, cutoffs))
    return ks


class RankStats(_SortedScoreRecord):
    """The record of one ``rank_metrics`` call, on the op's device: ``3 nk + 4`` 64-bit words ``[per cutoff the
    sums over the ranked groups of NDCG_g, recall_g, precision_g (fp64); ranked groups, examples in ranked
    groups, NaN scores, sort error word]`` and ``groups``, the ``[G, 2 + 3 nk]`` float64 per-group ``(n_g, P_g,
    then DCG, IDCG, hits per cutoff)``.  The readers synchronise with the launch chain on the GPU and raise when
    its sort reported a failed look-back: never a number then."""

    __slots__ = ("groups", "num_groups", "cutoffs")
    _op, _result = "rank_metrics", "ranking metric"

    def __init__(self, rec: torch.Tensor, groups: torch.Tensor, cutoffs: tuple, n: int, num_groups: int,
                 done: "torch.cuda.Event | None" = None):
        super().__init__(rec, False, n, done)
        self.groups, self.num_groups, self.cutoffs = groups, num_groups, cutoffs

    def stats(self) -> tuple:
        """(the ``3 nk`` sums as floats, ranked groups, examples in ranked groups, nans) on the host."""
        r = self._host_rec()
        m = 3 * len(self.cutoffs)
        i = r.tolist()
        return r.view(torch.float64).tolist()[:m], i[m], i[m + 1], i[m + 2]

    def _mean(self, k: int, which: int) -> float:
        if isinstance(k, bool) or not isinstance(k, int):
            raise ValueError(f"rank_metrics: a cutoff is an integer, got {k!r}")
        if k not in self.cutoffs:
            raise KeyError(f"rank_metrics: cutoff {k} is not one of this call's {self.cutoffs}")
        sums, ranked, _, nans = self.stats()
        if nans or not ranked:
            return float("nan")
        return sums[3 * self.cutoffs.index(k) + which] / ranked

    def ndcg(self, k: int) -> float:
        """Mean NDCG@k over the ranked groups; NaN when there is none or a score is NaN."""
        return self._mean(k, 0)

    def recall(self, k: int) -> float:
        """Mean recall@k over the ranked groups (NaN as ``ndcg``)."""
        return self._mean(k, 1)

    def precision(self, k: int) -> float:
        """Mean precision@k over the ranked groups (NaN as ``ndcg``)."""
        return self._mean(k, 2)

    def ranked_groups(self) -> int:
        """Groups with a positive (the ones the means run over)."""
        return self.stats()[1]

    def coverage(self) -> float:
        """Share of the examples that lie in ranked groups (NaN for an empty set)."""
        return self.stats()[2] / self.n if self.n else float("nan")

    def per_group(self) -> torch.Tensor:
        """The ``[G, 2 + 3 nk]`` float64 tensor on the op's device; zeros for empty groups."""
        self.stats()
        return self.groups


def rank_metrics_workspace(n: int, num_groups: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``rank_metrics`` for up to ``n`` scores in ``num_groups`` groups (GPU)."""
    return torch.empty(int(native.hip().rank_metrics_workspace_bytes(int(n), int(num_groups))), dtype=torch.uint8,
                       device=device)


def rank_metrics(scores: torch.Tensor, labels: torch.Tensor, groups: torch.Tensor, num_groups: int, cutoffs, *,
                 ws: torch.Tensor | None = None) -> RankStats:
    """NDCG@k, recall@k and precision@k of every group and their means over the ranked groups.

    ``groups``: int32 ids in ``[0, num_groups)``, one per score; ``cutoffs``: 1 to 4 strictly ascending integers
    in [1, 4096].  The gain of an example is its label when that is > 0, else 0; it is positive iff ``label > 0``.
    Within a group rank 1 is the highest score (``auc``'s score order); a run of equal scores at the ranks a..b
    gives every member the run's mean position weight ``(C_k(b) - C_k(a - 1)) / (b - a + 1)`` -- the exact
    expectation under uniformly random tie-breaking, independent of the input order.  Per group and cutoff:
    DCG = sum gain * mean weight with c(j) = 1 / log2(j + 1), IDCG = the same with the gains as the scores, hits =
    the expected number of positives in the top k; NDCG = DCG / IDCG, recall = hits / P_g, precision = hits / k.
    A group is ranked iff it has a positive; each metric is the plain mean over the ranked groups -- NaN without
    one or with a NaN score.  Everything is fp64 summed in a fixed order (bitwise the same run to run); the
    discount sums come from one host-built table that GPU and CPU share.  There are no example weights.  GPU:
    hip/rank_metrics.hip on the current stream (``ws``: reusable ``rank_metrics_workspace``; capturable after
    one eager call on the device, as ``auc``); CPU: a sort and one pass per group.  ``n == 0`` launches nothing
    (NaN).  Ids outside the range are an error with FM_DEBUG_CHECKS=1 and count as the last group without it.
    """
    ks = rank_cutoffs(cutoffs)
    G = int(num_groups)
    dev, n, _, _ = _sorted_score_inputs("rank_metrics", scores, labels, None, groups)
    _check(1 <= G < 2**31, "rank_metrics: num_groups must be in [1, 2^31)")
    if _DEBUG and n > 0 and not (scores.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check(bool(groups.min() >= 0) and bool(groups.max() < G), "groups: ids must be in [0, num_groups)")
    nk = len(ks)
    if n == 0:  # (host records: nothing is launched)
        return RankStats(torch.zeros(3 * nk + 4, dtype=torch.int64), torch.zeros((G, 2 + 3 * nk), dtype=torch.float64),
                         ks, 0, G)
    rec = torch.empty(3 * nk + 4, dtype=torch.int64, device=dev)
    per = torch.empty((G, 2 + 3 * nk), dtype=torch.float64, device=dev)
    if _is_gpu(scores):
        h = native.hip()
        _, done = _sorted_score_launch(
            "rank_metrics", dev, int(h.rank_metrics_workspace_bytes(n, G)), ws, lambda w: h.rank_metrics(
                scores=_p(scores), labels=_p(labels), groups=_p(groups), n=n, G=G, cutoffs=list(ks), out=_p(rec),
                per=_p(per), ws=_p(w), ws_bytes=w.numel(), stream=_stream(scores)))
        return RankStats(rec, per, ks, n, G, done)
    _check(ws is None, "rank_metrics: the workspace is a GPU argument")
    native.cpu().rank_metrics(n=n, G=G, scores=_p(scores), labels=_p(labels), groups=_p(groups), cutoffs=list(ks),
                              out=_p(rec), per=_p(per))
    return RankStats(rec, per, ks, n, G)


# ---------------------------------------------------------------------------
# listwise ranking loss: softmax cross-entropy per group of one batch
# ---------------------------------------------------------------------------
RANK_LOSS = "rank_softmax"  # [Train] loss_type: not one of LOSS_TYPES, the forward kernels do not know it


class GroupPlan:
    """The batch half of the listwise loss (``group_plan``): ``sidx`` the examples in (group, batch) order, the
    excluded ones last, and ``first`` / ``end``, every sorted position's group range (``end == 0``: excluded) --
    int32 ``[n]`` each; on the GPU views of ``ws``, the workspace the plan lives in (``err``: the sort's error
    word there), which must stay untouched until the last ``group_softmax_loss`` that reads the plan has run."""

    __slots__ = ("n", "key_bits", "ws", "sidx", "first", "end", "err")

    def __init__(self, n, key_bits, ws, sidx, first, end, err=None):
        self.n, self.key_bits, self.ws = n, key_bits, ws
        self.sidx, self.first, self.end, self.err = sidx, first, end, err


def group_loss_tile() -> int:
    """Sorted positions per workgroup of the GPU op (hip/group_loss.hip kGlTile): where its tests put their sizes."""
    return int(native.hip().GROUP_LOSS_TILE)


def group_loss_workspace(n: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``group_plan`` / ``group_softmax_loss`` for up to ``n`` examples (GPU): one workspace
    serves both halves of one batch."""
    return torch.empty(int(native.hip().group_loss_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def group_keys(offsets: torch.Tensor, rows: torch.Tensor, pos: int, num_rows: int, *,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Group key of every example of a CSR batch: ``rows[offsets[i] + pos]``, the table row of its ``pos``-th
    feature (0-based; after hashing or the modulo); -1 -- excluded from the listwise loss -- for an example with
    fewer than ``pos + 1`` features.  int32 ``[B]``, asynchronous on the current stream."""
    dev = rows.device
    B = offsets.numel() - 1
    _check(B >= 0, "offsets: needs B + 1 entries")
    _check(isinstance(pos, int) and not isinstance(pos, bool) and pos >= 0,
           f"group_keys: pos must be an int >= 0, got {pos!r}")
    _check(1 <= int(num_rows) < 2**31 - 1, "group_keys: num_rows must be in [1, 2^31 - 1)")
    _chk_vec(offsets, torch.int32, B + 1, "offsets", dev)
    _chk_vec(rows, torch.int32, None, "rows", dev)
    if out is None:
        out = torch.empty(B, dtype=torch.int32, device=dev)
    _chk_vec(out, torch.int32, B, "out", dev)
    if B == 0:
        return out[:0]
    if _is_gpu(rows):
        native.hip().group_keys(B=B, offsets=_p(offsets), rows=_p(rows), pos=pos, num_rows=int(num_rows), keys=_p(out),
                                stream=_stream(rows))
    else:
        native.cpu().group_keys(B=B, offsets=_p(offsets), rows=_p(rows), pos=pos, num_rows=int(num_rows), keys=_p(out))
    return out[:B]


def group_plan(keys: torch.Tensor, key_bits: int, *, ws: torch.Tensor | None = None) -> GroupPlan:
    """Group the examples of one batch by their int32 ``keys``: ids in ``[0, 2^key_bits - 1)``; an id ``< 0`` (or
    at or above that bound: the sort's all-ones key is theirs) marks an excluded example.  ``key_bits`` in [1, 31]:
    ``bits_for(num_rows + 1)`` for keys that are table rows.  GPU: hip/group_loss.hip on the current stream into
    ``ws`` (``group_loss_workspace``; allocated when None) -- the stable in-tree radix sort over ``key_bits``, a
    sort error goes to the sticky device error word (``check_device_errors``); capturable after one eager call on
    the device.  CPU: a stable sort.  The plan depends on the batch alone, not on the model."""
    dev = keys.device
    n = keys.numel()
    _chk_vec(keys, torch.int32, n, "keys", dev)
    _check(isinstance(key_bits, int) and not isinstance(key_bits, bool) and 1 <= key_bits <= 31,
           f"group_plan: key_bits must be an int in [1, 31], got {key_bits!r}")
    _check(n < 2**30, "group_plan: n must be < 2^30 (the radix sort's bound)")
    if _DEBUG and n > 0 and not (keys.is_cuda and torch.cuda.is_current_stream_capturing()):
        _check(int(keys.max()) < (1 << key_bits) - 1, "keys: ids must be below 2^key_bits - 1")
    if not _is_gpu(keys):
        _check(ws is None, "group_plan: the workspace is a GPU argument")
        sidx, first, end = (torch.empty(n, dtype=torch.int32) for _ in range(3))
        native.cpu().group_plan(n=n, ids=_p(keys), key_bits=key_bits, sidx=_p(sidx), first=_p(first), end=_p(end))
        return GroupPlan(n, key_bits, None, sidx, first, end)
    h = native.hip()
    need = int(h.group_loss_workspace_bytes(n))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk_vec(ws, torch.uint8, need, "ws", dev)
    o = h.group_plan_offsets(n)
    sidx, first, end = (ws[o[i]: o[i] + 4 * n].view(torch.int32) for i in range(3))
    err = ws[o[3]: o[3] + 4].view(torch.int32)
    if n > 0:
        _sort_selfcheck(dev)
        h.group_plan(ids=_p(keys), n=n, key_bits=key_bits, ws=_p(ws), ws_bytes=ws.numel(), stream=_stream(keys))
    return GroupPlan(n, key_bits, ws, sidx, first, end, err)


def group_softmax_loss(plan: GroupPlan, scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None,
                       grad_scale: float = 1.0, *, dpred: torch.Tensor | None = None,
                       ws: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Listwise softmax cross-entropy of the groups of ``plan``: ``(dpred [n] fp32, loss_sum 0-d fp32)``.

    With the gain ``a_i = w_i max(y_i, 0)`` (``rank_metrics``' gain times the example weight) and, per group g over
    its examples, ``m = max s_i, Z = sum exp(s_i - m), A = sum a_i, T = sum a_i s_i``:
    ``L_g = A (m + log Z) - T = -sum a_i log softmax_g(s)_i``, ``dL/ds_i = A exp(s_i - m) / Z - a_i``,
    ``dpred_i = grad_scale dL/ds_i`` and ``loss_sum = sum_g L_g``.  A group without a positive (``A == 0``), a
    group of one and an excluded example add exactly 0 loss and 0 gradient; the gradient sums to zero within every
    group.  Everything is fp64 (exp and log too) summed in a fixed order and rounded to fp32 once: bitwise the
    same run to run.  GPU: hip/group_loss.hip on the current stream, no host read (capturable); ``ws``: the
    workspace of the intermediates, the plan's own by default.  CPU: a loop over the plan."""
    dev = scores.device
    n = plan.n
    _check(scores.numel() == n, f"group_softmax_loss: the plan has {n} examples, scores {scores.numel()}")
    _chk_vec(scores, torch.float32, n, "scores", dev)
    _chk_vec(labels, torch.float32, n, "labels", dev)
    _chk_vec(weights, torch.float32, n, "weights", dev)
    _check(plan.sidx.device == dev, "group_softmax_loss: the plan lives on another device")
    if dpred is None:
        dpred = torch.empty(n, dtype=torch.float32, device=dev)
    _chk_vec(dpred, torch.float32, n, "dpred", dev)
    if n == 0:
        return dpred[:0], torch.zeros((), dtype=torch.float32, device=dev)
    if not _is_gpu(scores):
        _check(ws is None, "group_softmax_loss: the workspace is a GPU argument")
        ls = native.cpu().group_softmax(n=n, sidx=_p(plan.sidx), first=_p(plan.first), end=_p(plan.end),
                                        scores=_p(scores), labels=_p(labels), weights=_p(weights),
                                        grad_scale=float(grad_scale), dpred=_p(dpred))
        return dpred[:n], torch.tensor(ls, dtype=torch.float32)
    h = native.hip()
    if ws is None:
        ws = plan.ws
    _chk_vec(ws, torch.uint8, int(h.group_loss_workspace_bytes(n)), "ws", dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    h.group_softmax(plan=_p(plan.ws), plan_bytes=plan.ws.numel(), n=n, scores=_p(scores), labels=_p(labels),
                    weights=_p(weights), grad_scale=float(grad_scale), dpred=_p(dpred), loss=_p(loss), ws=_p(ws),
                    ws_bytes=ws.numel(), stream=_stream(scores))
    return dpred[:n], loss


# ---------------------------------------------------------------------------
# pairwise ranking loss: logistic loss of every (positive, negative) pair of a group of one batch
# ---------------------------------------------------------------------------
RANK_PAIR_LOSS = "rank_pairwise"  # [Train] loss_type: the second group loss over the same plan
RANK_LOSSES = (RANK_LOSS, RANK_PAIR_LOSS)


def group_pair_geometry() -> tuple[int, int, int]:
    """``(rows, chunk, slabs)`` of the GPU op (hip/group_pair.hip): sorted positions per row tile, columns per
    chunk (chunks start at multiples of it), column slabs of a row tile's span -- where its tests put their sizes."""
    h = native.hip()
    return int(h.GROUP_PAIR_ROWS), int(h.GROUP_PAIR_CHUNK), int(h.GROUP_PAIR_SLABS)


def group_pair_workspace(n: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``group_pairwise_loss`` for up to ``n`` examples (GPU); the plan's workspace is not it."""
    return torch.empty(int(native.hip().group_pair_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def group_pairwise_loss(plan: GroupPlan, scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None,
                        grad_scale: float = 1.0, *, dpred: torch.Tensor | None = None,
                        ws: torch.Tensor | None = None) -> tuple[torch.Tensor, torch.Tensor]:
    """Pairwise logistic loss of the groups of ``plan``: ``(dpred [n] fp32, loss_sum 0-d fp32)``.

    Example i is positive iff ``y_i > 0``; ``p_i = w_i`` for a positive (else 0), ``q_i = w_i`` for a non-positive
    (else 0); per group g over its examples ``P = sum p_i, N = sum q_j, c = (P + N) / (P N)``:
    ``L_g = c sum_{i,j} p_i q_j softplus(s_j - s_i)``, ``dL/ds_i = -c p_i sum_j q_j sigma(s_j - s_i)`` for a
    positive, ``dL/ds_j = +c q_j sum_i p_i sigma(s_j - s_i)`` for a negative, ``dpred_i = grad_scale dL/ds_i`` and
    ``loss_sum = sum_g L_g``.  ``L_g / ln 2 >= W_g (1 - AUC_g)`` with ``gauc``'s ``W_g = P + N``.  A group without
    a positive or without a negative, a group of one, an excluded example and an example of weight 0 add exactly 0
    loss and get exactly 0 gradient, whatever their scores hold; the gradient sums to zero within every group.
    Everything is fp64 (exp, log1p and the division too), sums of non-negative terms in a fixed order, rounded to
    fp32 once: bitwise the same run to run.  The cost is ``sum_g P_g N_g`` pairs.  GPU: hip/group_pair.hip on the
    current stream, no host read (capturable); the plan is only read; ``ws``: ``group_pair_workspace`` (allocated
    when None).  CPU: a loop over the plan."""
    dev = scores.device
    n = plan.n
    _check(scores.numel() == n, f"group_pairwise_loss: the plan has {n} examples, scores {scores.numel()}")
    _chk_vec(scores, torch.float32, n, "scores", dev)
    _chk_vec(labels, torch.float32, n, "labels", dev)
    _chk_vec(weights, torch.float32, n, "weights", dev)
    _check(plan.sidx.device == dev, "group_pairwise_loss: the plan lives on another device")
    if dpred is None:
        dpred = torch.empty(n, dtype=torch.float32, device=dev)
    _chk_vec(dpred, torch.float32, n, "dpred", dev)
    if n == 0:
        return dpred[:0], torch.zeros((), dtype=torch.float32, device=dev)
    if not _is_gpu(scores):
        _check(ws is None, "group_pairwise_loss: the workspace is a GPU argument")
        ls = native.cpu().group_pairwise(n=n, sidx=_p(plan.sidx), first=_p(plan.first), end=_p(plan.end),
                                         scores=_p(scores), labels=_p(labels), weights=_p(weights),
                                         grad_scale=float(grad_scale), dpred=_p(dpred))
        return dpred[:n], torch.tensor(ls, dtype=torch.float32)
    h = native.hip()
    need = int(h.group_pair_workspace_bytes(n))
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    _chk_vec(ws, torch.uint8, need, "ws", dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    h.group_pairwise(plan=_p(plan.ws), plan_bytes=plan.ws.numel(), n=n, scores=_p(scores), labels=_p(labels),
                     weights=_p(weights), grad_scale=float(grad_scale), dpred=_p(dpred), loss=_p(loss), ws=_p(ws),
                     ws_bytes=ws.numel(), stream=_stream(scores))
    return dpred[:n], loss


# ---------------------------------------------------------------------------
# calibration: exact isotonic regression of (score, label, weight)
# ---------------------------------------------------------------------------
class IsotonicFit(_SortedScoreRecord):
    """The record of one ``isotonic_fit`` call, on the op's device: ``[blocks, total weight, positive weight,
    NaN scores, sort error word]`` -- int64 (unweighted: exact) or float64 (weighted) -- and the block arrays.
    The readers (``count`` / ``totals`` / ``blocks`` / ``fitted`` / ``calibrator``) read the record (a host
    sync on the GPU) and raise when a score is NaN (there is no fit then) or when the GPU sort reported a
    failed look-back.  On the GPU the block arrays live in the call's workspace: read them before the
    workspace is used again (``blocks`` copies)."""

    __slots__ = ("arrays", "fit", "keep", "scores", "_head")
    _op, _result = "isotonic_fit", "fit"

    def __init__(self, rec: torch.Tensor, weighted: bool, n: int, arrays: tuple | None = None,
                 fit: torch.Tensor | None = None, done: "torch.cuda.Event | None" = None,
                 keep: torch.Tensor | None = None, scores: torch.Tensor | None = None):
        super().__init__(rec, weighted, n, done)
        self.arrays, self.fit = arrays, fit
        self.keep, self.scores = keep, scores  # zero-weight examples were dropped: the mask, every score
        self._head = None

    def _read(self) -> tuple:
        if self._head is None:
            m, w, y, nans, _ = self._host_rec().tolist()
            if nans:
                raise ValueError(f"isotonic_fit: {int(nans)} NaN score(s); there is no fit")
            self._head = (int(m), w, y)
        return self._head

    def count(self) -> int:
        """Number of blocks (0: no example with weight)."""
        return self._read()[0]

    def totals(self) -> tuple:
        """(total weight, positive weight): Python ints (unweighted) or floats."""
        return self._read()[1:]

    def blocks(self) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(lo, hi, weight, positives, value) of the blocks in ascending score order: the fp32 scores of a
        block's first / last example, its weight and positive weight (int64 / float64) and value (float64,
        strictly increasing)."""
        m = self.count()
        if self.arrays is None or m == 0:
            dt = torch.float64 if self.weighted else torch.int64
            dev = self.rec.device
            return (torch.empty(0, dtype=torch.float32, device=dev), torch.empty(0, dtype=torch.float32, device=dev),
                    torch.empty(0, dtype=dt, device=dev), torch.empty(0, dtype=dt, device=dev),
                    torch.empty(0, dtype=torch.float64, device=dev))
        return tuple(a[:m].clone() for a in self.arrays)

    def calibrator(self) -> tuple[torch.Tensor, torch.Tensor]:
        """The fp32 threshold list ``x = [lo_0, hi_0, lo_1, hi_1, ...]`` and ``y = [v_0, v_0, v_1, v_1, ...]``
        (``calibrate_apply``'s arguments), on the op's device."""
        lo, hi, _, _, v = self.blocks()
        _check(lo.numel() > 0, "isotonic_fit: no example with weight, so no calibrator")
        v32 = v.to(torch.float32)
        return torch.stack((lo, hi), dim=1).reshape(-1).contiguous(), torch.stack((v32, v32), dim=1).reshape(-1)

    def fitted(self) -> torch.Tensor:
        """The fitted value of every example in input order (float64; needs ``want_fitted``).  An example that
        was dropped for its zero weight gets the calibrator's value at its score."""
        _check(self.fit is not None, "isotonic_fit: fitted values need want_fitted=True")
        m = self.count()
        if self.keep is None:
            return self.fit
        out = torch.full((self.keep.numel(),), float("nan"), dtype=torch.float64, device=self.keep.device)
        if m:
            out[self.keep] = self.fit
            x, y = self.calibrator()
            out[~self.keep] = calibrate_apply(self.scores[~self.keep].contiguous(), x, y).to(torch.float64)
        return out


def isotonic_workspace(n: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``isotonic_fit`` for up to ``n`` scores (GPU)."""
    return torch.empty(int(native.hip().isotonic_workspace_bytes(int(n))), dtype=torch.uint8, device=device)


def isotonic_fit(scores: torch.Tensor, labels: torch.Tensor, weights: torch.Tensor | None = None, *,
                 want_fitted: bool = False, ws: torch.Tensor | None = None, _cpu_tile: int = 0) -> IsotonicFit:
    """Exact isotonic regression: the non-decreasing map from raw score to P(positive) with the least weighted
    squared error (equally: the least log loss) on these examples.

    ``auc``'s conventions: an example is positive iff ``label > 0``, ``weights`` None = all ones, scores compare
    as IEEE fp32 values (-0.0 == +0.0, infinities and denormals ordered as usual), NaN scores are counted and
    make the readers raise.  With the examples sorted by score, the fit is the slope of the lower convex hull of
    the cumulative (weight, positive weight) diagram over the ends of the runs of tied scores, with the minimal
    vertex set; consecutive vertices bound a block of examples that share one value ``positives / weight``.
    Unweighted fits are integers (exact, the same on GPU and CPU); weighted ones are fp64 in a fixed order
    (bitwise the same run to run).  Examples with weight 0 are dropped here (the kernels need ``w > 0``: one host
    read of the weights' signs, so a weighted fit is no step of a captured graph).
    GPU: hip/isotonic.hip on the current stream (``ws``: reusable ``isotonic_workspace``); CPU: a sort and the
    serial stack.  ``n == 0`` or no weight at all launches nothing and has no blocks.
    """
    dev, n, weighted, rdt = _sorted_score_inputs("isotonic_fit", scores, labels, weights)
    keep = all_scores = None
    if weighted and n > 0:
        _check(bool((weights >= 0).all()), "weights: must be >= 0")  # (NaN weights fail too)
        pos = weights > 0
        if not bool(pos.all()):
            keep, all_scores = pos, scores
            scores, labels, weights = scores[pos].contiguous(), labels[pos].contiguous(), weights[pos].contiguous()
            n = scores.numel()
    if n == 0:  # (a host record: nothing is launched)
        fit = torch.empty(0, dtype=torch.float64, device=dev) if want_fitted else None
        return IsotonicFit(torch.zeros(5, dtype=rdt), weighted, 0, None, fit, None, keep, all_scores)
    rec = torch.empty(5, dtype=rdt, device=dev)
    fit = torch.empty(n, dtype=torch.float64, device=dev) if want_fitted else None
    if _is_gpu(scores):
        h = native.hip()
        ws, done = _sorted_score_launch("isotonic_fit", dev, int(h.isotonic_workspace_bytes(n)), ws, lambda w: (
            h.isotonic(scores=_p(scores), labels=_p(labels), weights=_p(weights), n=n, fitted=_p(fit), out=_p(rec),
                       ws=_p(w), ws_bytes=w.numel(), stream=_stream(scores))))
        off = h.isotonic_block_offsets(n)
        dts = (torch.float32, torch.float32, rdt, rdt, torch.float64)
        arrays = tuple(ws[o:o + n * d.itemsize].view(d) for o, d in zip(off, dts))
        return IsotonicFit(rec, weighted, n, arrays, fit, done, keep, all_scores)
    _check(ws is None, "isotonic_fit: the workspace is a GPU argument")
    arrays = (torch.empty(n, dtype=torch.float32), torch.empty(n, dtype=torch.float32), torch.empty(n, dtype=rdt),
              torch.empty(n, dtype=rdt), torch.empty(n, dtype=torch.float64))
    native.cpu().isotonic(n=n, scores=_p(scores), labels=_p(labels), weights=_p(weights), lo=_p(arrays[0]),
                          hi=_p(arrays[1]), W=_p(arrays[2]), Y=_p(arrays[3]), v=_p(arrays[4]), fitted=_p(fit),
                          out=_p(rec), tile=int(_cpu_tile))
    return IsotonicFit(rec, weighted, n, arrays, fit, None, keep, all_scores)


def calibrate_apply(scores: torch.Tensor, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Calibrated probabilities of raw scores from a fit's thresholds ``x = [lo_0, hi_0, lo_1, hi_1, ...]`` and
    values ``y = [v_0, v_0, v_1, v_1, ...]`` (fp32, ``IsotonicFit.calibrator``): NaN for NaN; the first / last
    block's value at and beyond the ends; exactly ``v_b`` for ``lo_b <= s <= hi_b``; between two blocks
    ``fmaf(t, v_{b+1} - v_b, v_b)`` with ``t = (s - hi_b) / (lo_{b+1} - hi_b)``, clamped into ``[v_b, v_{b+1}]``
    (``t`` = 0 / 1 / 0.5 when the gap's upper / lower / both ends are infinite).  Monotone in the score.
    GPU: hip/isotonic.hip calib_apply_kernel on the current stream; CPU: the same formula."""
    dev = scores.device
    n = scores.numel()
    m2 = x.numel()
    _chk_vec(scores, torch.float32, n, "scores", dev)
    _chk_vec(x, torch.float32, m2, "x", dev)
    _chk_vec(y, torch.float32, m2, "y", dev)
    _check(m2 >= 2 and m2 % 2 == 0 and y.numel() == m2, "calibrate_apply: x, y hold two entries per block")
    out = torch.empty(n, dtype=torch.float32, device=dev)
    if n == 0:
        return out
    if _is_gpu(scores):
        native.hip().calib_apply(scores=_p(scores), n=n, x=_p(x), y=_p(y), m2=m2, out=_p(out),
                                 stream=_stream(scores))
    else:
        native.cpu().calib_apply(n=n, scores=_p(scores), x=_p(x), y=_p(y), m2=m2, out=_p(out))
    return out


# ---------------------------------------------------------------------------
# top-k recommendation: rank a candidate set per query from FM profiles
# ---------------------------------------------------------------------------
TOPK_MAX_K = 128
TOPK_MAX_KP = 256


def topk_plan(nq: int, nc: int, k: int) -> tuple[int, int]:
    """``(slab, parts)`` of an ``fm_topk`` call on the GPU: the candidates per slab and the partial lists per
    query (csrc/topk_order.h; a pure function of the sizes, the same from the host module)."""
    return tuple(native.cpu().topk_plan(int(nq), int(nc), int(k)))


def topk_workspace(nq: int, nc: int, k: int, device: torch.device) -> torch.Tensor:
    """Device scratch of ``fm_topk`` (GPU): the slabs' partial key lists."""
    return torch.empty(int(native.hip().topk_workspace_bytes(int(nq), int(nc), int(k))), dtype=torch.uint8,
                       device=device)


def _chk_profiles(t: torch.Tensor, base: torch.Tensor, name: str, dev: torch.device) -> tuple[int, int, int]:
    """Validate a profile matrix [n, Kp] (+ its base scores [n]); returns (n, Kp, row stride)."""
    _check(t.dim() == 2, f"{name}_prof: expected [n, Kp]")
    _check(t.dtype == torch.float32, f"{name}_prof: expected {torch.float32}, got {t.dtype}")
    _check(t.device == dev, f"{name}_prof: expected device {dev}, got {t.device}")
    n, Kp = t.shape
    _check(Kp % 4 == 0 and 4 <= Kp <= TOPK_MAX_KP, f"{name}_prof: Kp={Kp} must be a multiple of 4 in 4..{TOPK_MAX_KP}")
    _check(t.stride(1) == 1, f"{name}_prof: rows must be contiguous")
    stride = t.stride(0) if n > 1 else Kp  # (the stride of a single row is never used)
    _check(stride >= Kp and stride % 4 == 0, f"{name}_prof: row stride {stride} must be a multiple of 4 >= Kp")
    _check(n == 0 or t.data_ptr() % 16 == 0, f"{name}_prof: base must be 16-byte aligned")
    _chk_vec(base, torch.float32, n, f"{name}_base", dev)
    _check(base.numel() == n, f"{name}_base: one base score per profile row")
    return n, Kp, stride


def fm_topk(q_prof: torch.Tensor, q_base: torch.Tensor, c_prof: torch.Tensor, c_base: torch.Tensor, k: int, *,
            idx: torch.Tensor | None = None, score: torch.Tensor | None = None, ws: torch.Tensor | None = None,
            threads: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """The ``k`` best candidates of every query from FM profiles (hip/fm_topk.hip; the reference only scores).

    ``s(q, c) = ((q_base[q] + c_base[c]) + dot) + 0`` with ``dot`` the fp32 fmaf chain of ``q_prof[q]`` and
    ``c_prof[c]`` over the columns in the fixed order of csrc/topk_order.h.  Returns ``(idx [nq, k] int32,
    score [nq, k] fp32)``: greater score first, equal scores by ascending candidate, ``-1`` / ``-inf`` where
    there are fewer than ``k`` candidates.  Exact fp32 on the matrix cores (gfx950's fp32-input MFMA), bitwise
    reproducible, and bit for bit the same on the CPU.  GPU: current stream, no host synchronisation (``ws``:
    reusable ``topk_workspace``).  Profiles are expected to be finite."""
    dev = q_prof.device
    _check(isinstance(k, int) and 1 <= k <= TOPK_MAX_K, f"fm_topk: k must be in 1..{TOPK_MAX_K}, got {k}")
    nq, Kp, q_stride = _chk_profiles(q_prof, q_base, "q", dev)
    nc, Kc, c_stride = _chk_profiles(c_prof, c_base, "c", dev)
    _check(Kp == Kc, f"fm_topk: profile widths differ ({Kp} and {Kc})")
    _check(nc < 2**31 and nq < 2**31, "fm_topk: nq and nc must be below 2^31")
    if idx is None:
        idx = torch.empty((nq, k), dtype=torch.int32, device=dev)
    if score is None:
        score = torch.empty((nq, k), dtype=torch.float32, device=dev)
    _chk_vec(idx, torch.int32, nq * k, "idx", dev)
    _chk_vec(score, torch.float32, nq * k, "score", dev)
    _check(tuple(idx.shape) == (nq, k) and tuple(score.shape) == (nq, k), "idx / score: expected [nq, k]")
    if nq == 0:
        return idx, score
    kw = dict(nq=nq, nc=nc, Kp=Kp, k=k, q=_p(q_prof), q_stride=q_stride, c=_p(c_prof), c_stride=c_stride,
              qb=_p(q_base), cb=_p(c_base), idx=_p(idx), score=_p(score))
    if _is_gpu(q_prof):
        h = native.hip()
        need = int(h.topk_workspace_bytes(nq, nc, k))
        if ws is None:
            ws = torch.empty(need, dtype=torch.uint8, device=dev)
        _chk_vec(ws, torch.uint8, need, "ws", dev)
        _check(ws.data_ptr() % 8 == 0, "ws: must be 8-byte aligned")
        h.topk(ws=_p(ws), ws_bytes=ws.numel(), stream=_stream(q_prof), **kw)
    else:
        _check(ws is None, "fm_topk: the workspace is a GPU argument")
        native.cpu().topk(threads=threads, **kw)
    return idx, score


# ---------------------------------------------------------------------------
# sparse checkpoints: rows that differ from their initial state
# ---------------------------------------------------------------------------
def _bits_of(value: float, dtype: torch.dtype) -> int:
    """The bit pattern torch stores for ``value`` in ``dtype`` (what ``torch.full`` wrote), as an int."""
    t = torch.full((1,), value, dtype=dtype)
    return int(t.view(torch.int16 if dtype == torch.bfloat16 else torch.int32).item()) & (
        0xFFFF if dtype == torch.bfloat16 else 0xFFFFFFFF)


def slot_init_values(opt: OptConfig) -> tuple[float, float]:
    """Initial values of optimizer slot 0 and slot 1 of a table with ``opt`` (models/table.py)."""
    return (float(opt.initial_accumulator) if opt.name in ("adagrad", "ftrl") else 0.0, 0.0)


def changed_rows(table, *, seed: int | None = None) -> torch.Tensor:
    """Ascending local rows (int64, on ``table.device``) of an ``FMTable`` shard that differ, bit for bit
    over columns ``0 .. K-1``, from their initial state: ``v`` / ``w`` from what ``init_rows`` writes for
    (``seed``, ``table.init_range``) -- fp8: the stored bytes and the row scale; the norm word is derived
    and ignored --, the optimizer slots from the constants they start from.  Only rows with a real global
    id (``< vocab_size``) are looked at.  ``seed``: the init seed to compare against (default: the one the
    table recorded, ``table.init_seed``).

    GPU: hip/ckpt.hip on the current stream -- one pass over the table, a bitmap, an ordered compaction;
    one host read (the count).  CPU: the same definition (cpu/kernels.cpp), fp32 and bf16 tables."""
    dev = table.device
    seed = int(table.init_seed if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
    rows = min(table.rows, table.real_rows)
    _check(rows <= 2**31, "changed_rows: at most 2^31 rows per shard")
    s0, s1 = slot_init_values(table.opt)
    sdt = table.state_dtype
    sv0, sv1 = _bits_of(s0, sdt), _bits_of(s1, sdt)
    sw0, sw1 = _bits_of(s0, torch.float32), _bits_of(s1, torch.float32)
    v, w = table.v, table.wx if table.fp8 else table.w
    v_stride = _chk_rows(v, table.Kp, "v")
    for name in ("s0v", "s1v"):
        t = getattr(table, name)
        if t is not None:
            _check(t.dtype == sdt and t.stride(1) == 1 and t.stride(0) == table.s0v.stride(0)
                   and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0, f"{name}: state rows of {sdt}, 16-byte aligned")
    for name in ("w", "s0w", "s1w"):
        t = getattr(table, name)
        _check(t is None or t.dtype == torch.float32, f"{name}: fp32")
    common = dict(v=_p(v), v_stride=v_stride, w=_p(w), w_stride=w.stride(0), s0v=_p(table.s0v), s1v=_p(table.s1v),
                  s_stride=table.s0v.stride(0), s0w=_p(table.s0w), s1w=_p(table.s1w), rows=rows, K=table.K,
                  dtype=dtype_code(table.dtype), gid_mul=table.world, gid_add=table.rank, seed=seed,
                  range=float(table.init_range), sv0=sv0, sv1=sv1, sw0=sw0, sw1=sw1)
    if dev.type == "cuda":
        h = native.hip()
        need = int(h.changed_workspace_bytes(rows))
        ws = torch.empty((need + 7) // 8, dtype=torch.int64, device=dev)
        st = _stream(v)
        h.changed_scan(**common, Kp=table.Kp, ws=_p(ws), ws_bytes=ws.numel() * 8, stream=st)
        n = int(ws[int(h.changed_total_offset(rows)) // 8].item())  # the one host read
        out = torch.empty(n, dtype=torch.int64, device=dev)
        if n:
            h.changed_emit(rows=rows, ws=_p(ws), out=_p(out), stream=st)
        return out
    _check(not table.fp8, "changed_rows: fp8 tables run on the GPU kernels only")
    c = native.cpu()
    flags = torch.empty(max(rows, 1), dtype=torch.uint8)
    n = int(c.changed_rows(**common, flags=_p(flags)))
    out = torch.empty(n, dtype=torch.int64)
    if n:
        c.changed_rows_emit(flags=_p(flags), rows=rows, out=_p(out))
    return out


# ---------------------------------------------------------------------------
# row-sharded helpers
# ---------------------------------------------------------------------------
def gather_rows(req: torch.Tensor, table: TableState, Kp: int, out: torch.Tensor, threads: int = 0,
                skip: tuple[int, int] | None = None) -> torch.Tensor:
    """out[p] = [v[req[p]], w[req[p]], 0...] (fp32), the owner side of a sharded lookup.
    ``skip`` (GPU): requests [s0, s1) are left out (their ``out`` rows are not written)."""
    dev = req.device
    R = req.numel()
    _chk_vec(req, torch.int32, R, "req", dev)
    v_stride = _chk_rows(table.v, Kp, "v")
    _check(out.dtype == torch.float32 and out.stride(1) == 1 and out.shape[0] >= R, "out: fp32 rows")
    _check(out.stride(0) >= Kp + 4 and out.stride(0) % 4 == 0, "out row stride")
    _range_check(req, table.v.shape[0], "req")
    dt = dtype_code(table.v.dtype)
    if _is_gpu(req):
        s0, s1 = skip or (0, 0)
        _check(0 <= s0 <= s1 <= R, "gather skip range")
        native.hip().gather_rows(R=R, req=_p(req), v=_p(table.v), v_stride=v_stride, w=_p(table.w),
                                 w_stride=table.w.stride(0), Kp=Kp, dtype=dt, out=_p(out), o_stride=out.stride(0),
                                 stream=_stream(req), skip0=s0, skip1=s1)
    else:
        _check(skip is None, "gather skip ranges are a GPU path")
        native.cpu().gather_rows(R=R, req=_p(req), v=_p(table.v), v_stride=v_stride, w=_p(table.w),
                                 w_stride=table.w.stride(0), Kp=Kp, dtype=dt, out=_p(out), o_stride=out.stride(0),
                                 threads=threads)
    return out


def shard_keys(ids: torch.Tensor, world: int, rows_per_shard: int, out: torch.Tensor) -> torch.Tensor:
    """Sharded key of every occurrence: (id % world) * rows_per_shard + id // world (int32)."""
    n = ids.numel()
    _check(world * rows_per_shard < 2**31, "sharded keys must fit int32")
    if _is_gpu(ids) and ids.dtype == torch.int32:
        _chk_vec(out, torch.int32, None, "out", ids.device)
        _check(out.numel() >= n, "out too small")
        native.hip().shard_keys(n=n, ids=_p(ids), W=int(world), Rps=int(rows_per_shard), keys=_p(out),
                                stream=_stream(ids))
        return out[:n]
    keys = (ids % world) * rows_per_shard + torch.div(ids, world, rounding_mode="floor")
    out[:n].copy_(keys)
    return out[:n]


def owner_counts(dd: DedupOut, rows_per_shard: int, world: int, out: torch.Tensor | None = None,
                 out2: torch.Tensor | None = None) -> torch.Tensor:
    """int64[world]: unique keys (owner * rows_per_shard + row) per owner, computed without a host sync.
    ``out`` / ``out2``: 1-D int64 views (any stride) to write (``out2``: a second copy, GPU)."""
    if out is None:
        out = torch.empty(world, dtype=torch.int64, device=dd.uniq.device)
    _check(out.dtype == torch.int64 and out.dim() == 1 and out.numel() == world, "owner_counts out: int64[world]")
    if dd.uniq.device.type == "cuda":
        if out2 is not None:
            _check(out2.dtype == torch.int64 and out2.shape == out.shape and out2.stride() == out.stride()
                   and out2.device == out.device, "owner_counts out2: like out")
        native.hip().owner_counts(uniq=_p(dd.uniq), num_unique=_p(dd.num_unique), Rps=int(rows_per_shard), W=world,
                                  out=_p(out), stream=_stream(dd.uniq), stride=out.stride(0),
                                  out2=_p(out2) if out2 is not None else 0)
    else:
        owner = torch.div(dd.uniq[: dd.sync()].to(torch.int64), rows_per_shard, rounding_mode="floor")
        out.copy_(torch.bincount(owner, minlength=world))
        if out2 is not None:
            out2.copy_(out)
    return out


def apply_rows(dd: DedupOut, grad_in: torch.Tensor, table: TableState, opt: OptConfig, Kp: int,
               threads: int = 0, sr_counter: torch.Tensor | None = None) -> None:
    """Owner side of a sharded update: sum received grad rows per table row, then one optimizer step."""
    v_stride = _chk_rows(table.v, Kp, "v")
    _check(grad_in.dtype == torch.float32 and grad_in.stride(1) == 1, "grad_in: fp32 rows")
    dt = dtype_code(table.v.dtype)
    s_stride = table.s0v.stride(0) if table.s0v is not None else 0
    if _is_gpu(grad_in):
        native.hip().apply_rows(num_unique=_p(dd.num_unique), seg_start=_p(dd.seg_start), uniq=_p(dd.uniq),
                                perm=_p(dd.perm), grad_in=_p(grad_in), g_stride=grad_in.stride(0), Kp=Kp,
                                v=_p(table.v), v_stride=v_stride, w=_p(table.w), w_stride=table.w.stride(0),
                                s0v=_p(table.s0v), s1v=_p(table.s1v), s_stride=s_stride, s0w=_p(table.s0w),
                                s1w=_p(table.s1w), opt_type=opt.code, lr=float(opt.lr), l1=float(opt.l1),
                                l2=float(opt.l2), beta=float(opt.beta), dtype=dt, max_unique=max(dd.n, 1),
                                stream=_stream(grad_in), sr_counter=_p(sr_counter))
    else:
        native.cpu().apply_rows(U=dd.sync(), seg_start=_p(dd.seg_start), uniq=_p(dd.uniq), perm=_p(dd.perm),
                                grad_in=_p(grad_in), g_stride=grad_in.stride(0), Kp=Kp, v=_p(table.v),
                                v_stride=v_stride, w=_p(table.w), w_stride=table.w.stride(0), s0v=_p(table.s0v),
                                s1v=_p(table.s1v), s_stride=s_stride, s0w=_p(table.s0w), s1w=_p(table.s1w),
                                opt_type=opt.code, lr=float(opt.lr), l1=float(opt.l1), l2=float(opt.l2),
                                beta=float(opt.beta), dtype=dt, threads=threads)


def dense_apply(grad: torch.Tensor, table: TableState, opt: OptConfig, Kp: int, row0: int = 0,
                rows: int | None = None, zero: bool = True, sr_counter: torch.Tensor | None = None) -> None:
    """Replicated-table update from a dense gradient buffer ``grad`` [n, Kp+4] (rows
    [g_v | g_w | touch | pad], e.g. all-reduced over the data-parallel ranks): every row whose
    touch word is non-zero gets one optimizer step on table row ``row0 + i`` and (``zero``) is
    cleared for the next step; untouched rows cost one word read.  GPU only; no host sync."""
    _check(_is_gpu(grad), "dense_apply is a GPU path")
    n = grad.shape[0] if rows is None else int(rows)
    v_stride = _chk_rows(table.v, Kp, "v")
    _check(grad.dtype == torch.float32 and grad.is_contiguous() and grad.shape[1] >= Kp + 2
           and grad.shape[1] % 4 == 0, "grad: contiguous fp32 [n, Kp+4]")
    _check(row0 >= 0 and row0 + n <= table.v.shape[0], "dense_apply rows outside the table")
    s_stride = table.s0v.stride(0) if table.s0v is not None else 0
    native.hip().dense_apply(R=n, row0=row0, grad=_p(grad), g_stride=grad.stride(0), touch_col=Kp + 1,
                             zero=int(zero), Kp=Kp, v=_p(table.v), v_stride=v_stride, w=_p(table.w),
                             w_stride=table.w.stride(0), s0v=_p(table.s0v), s1v=_p(table.s1v), s_stride=s_stride,
                             s0w=_p(table.s0w), s1w=_p(table.s1w), opt_type=opt.code, lr=float(opt.lr),
                             l1=float(opt.l1), l2=float(opt.l2), beta=float(opt.beta),
                             dtype=dtype_code(table.v.dtype), stream=_stream(grad), sr_counter=_p(sr_counter))


def zero_listed_rows(buf: torch.Tensor, rows: torch.Tensor, count: torch.Tensor, max_n: int) -> None:
    """buf[rows[i]] = 0 for i < count (device int32 scalar, capped at ``max_n``); GPU, no host sync."""
    _check(_is_gpu(buf) and buf.dtype == torch.float32 and buf.is_contiguous() and buf.shape[1] % 4 == 0,
           "buf: contiguous fp32 rows, width a multiple of 4")
    _chk_vec(rows, torch.int32, None, "rows", buf.device)
    _chk_vec(count, torch.int32, 1, "count", buf.device)
    native.hip().zero_listed_rows(buf=_p(buf), row_words=buf.stride(0), list=_p(rows), count=_p(count),
                                  max_n=int(min(max_n, rows.numel())), stream=_stream(buf))


def apply_runs(req: torch.Tensor, run_off: torch.Tensor, splits: list[int], grad_in: torch.Tensor,
               table: TableState, opt: OptConfig, Kp: int, match: torch.Tensor | None = None,
               threads: int = 0, ws: DedupWorkspace | None = None, grad_bf16: bool = False,
               sr_counter: torch.Tensor | None = None, self_run: int = -1,
               self_excl: torch.Tensor | None = None) -> None:
    """Owner side of a sharded update over the received requests as W ascending runs.

    ``req`` [R] holds the local rows requested by each source rank, rank-major
    (``splits[q]`` rows from rank q, ascending and distinct within a run);
    ``grad_in`` [R, >= Kp+1] the matching gradient rows.  Every distinct row gets
    the sum of its gradient rows in source-rank order and one optimizer step.
    On the GPU the grouping is a cross-run binary-search match (``run_off`` =
    device int32 [W+1] prefix of ``splits``, ``match`` int32 scratch of R*W when
    W > 1) instead of a sort; on the CPU a stable sort of ``req`` (``ws``).
    ``self_run`` >= 0 (GPU): the rows of that run flagged in ``self_excl`` (None: all of them)
    were updated in place by the backward (``SelfRows``) and are skipped.
    """
    R, W = int(sum(splits)), len(splits)
    _chk_vec(req, torch.int32, R, "req", req.device)
    _check(grad_in.dtype == torch.float32 and grad_in.stride(1) == 1 and grad_in.shape[0] >= R, "grad_in: fp32 rows")
    if R == 0:
        return
    if not _is_gpu(grad_in):
        _check(not grad_bf16 and self_run < 0, "bf16 gradient rows and self runs are a GPU path")
        dd = dedup(req[:R], ws=ws, key_bits=32, want_perm=True)
        apply_rows(dd, grad_in, table, opt, Kp, threads=threads)  # (CPU tables: fp32 / bf16, nearest)
        return
    v_stride = _chk_rows(table.v, Kp, "v")
    _range_check(req[:R], table.v.shape[0], "req")
    _chk_vec(run_off, torch.int32, W + 1, "run_off", req.device)
    if W > 1:
        _chk_vec(match, torch.int32, R * W, "match", req.device)
    dt = dtype_code(table.v.dtype)
    s_stride = table.s0v.stride(0) if table.s0v is not None else 0
    native.hip().apply_runs(R=R, W=W, run_off=_p(run_off), req=_p(req), match=_p(match) if W > 1 else 0,
                            grad_in=_p(grad_in), g_stride=grad_in.stride(0), Kp=Kp, v=_p(table.v), v_stride=v_stride,
                            w=_p(table.w), w_stride=table.w.stride(0), s0v=_p(table.s0v), s1v=_p(table.s1v),
                            s_stride=s_stride, s0w=_p(table.s0w), s1w=_p(table.s1w), opt_type=opt.code,
                            lr=float(opt.lr), l1=float(opt.l1), l2=float(opt.l2), beta=float(opt.beta), dtype=dt,
                            stream=_stream(grad_in), g_wcol=(Kp * 2 + 15) // 16 * 4 if grad_bf16 else Kp,
                            g_bf16=int(bool(grad_bf16)), sr_counter=_p(sr_counter), self_run=int(self_run),
                            self_excl=_p(self_excl))


def self_excl(req: torch.Tensor, W: int, run_off: torch.Tensor, me: int, n: int, out: torch.Tensor) -> torch.Tensor:
    """GPU: out[i] = 1 when request ``run_off[me] + i`` (this rank's own run) is in no other run."""
    _chk_vec(out, torch.int32, None, "excl", req.device)
    _check(out.numel() >= n, "excl too short")
    native.hip().self_excl(req=_p(req), W=int(W), run_off=_p(run_off), me=int(me), n=int(n), excl=_p(out),
                           stream=_stream(req))
    return out


@dataclass
class WireFormat:
    """Row layout of the row-sharded exchange (owner gather -> all-to-all -> fwd/bwd).

    A wire row is ``rb`` bytes: the Kp factor values in ``dtype`` (padded to
    ``vb`` bytes), then ``[w, scale, |v|^2, tag]`` fp32 (scale and the stored row norm for fp8 only;
    tag: patch gathers).  bf16 /
    fp8 tables travel at their storage size (the stored bits); an fp32 table
    travels as fp32 (``[v | w | pad]``, the same bytes as a [Kp+4] fp32 row) or,
    with ``comm_dtype = bf16``, as bf16 (rounded to nearest even).
    """

    dtype: torch.dtype
    Kp: int
    vb: int
    rb: int
    table_dtype: torch.dtype
    grad_bf16: bool = False   # gradient rows: [Kp bf16 | pad to gvb][gw fp32, 0, 0, 0] instead of [Kp fp32 | gw | pad]
    g_words: int = 0          # 4-byte words per gradient row
    g_wcol: int = 0           # word index of the w-gradient

    @staticmethod
    def make(table_dtype: torch.dtype, Kp: int, comm_dtype: str = "auto") -> "WireFormat":
        if comm_dtype not in ("auto", "bf16", "fp32", "storage"):
            raise ValueError(f"comm_dtype must be auto|storage|fp32|bf16, got {comm_dtype}")
        dt = table_dtype
        if comm_dtype == "bf16" and table_dtype == torch.float32 and Kp % 8 == 0:
            dt = torch.bfloat16
        if comm_dtype == "fp32":
            dt = torch.float32
        esz = torch.tensor([], dtype=dt).element_size()
        vb = (Kp * esz + 15) // 16 * 16
        gbf = comm_dtype == "bf16"
        gvb = (Kp * 2 + 15) // 16 * 16
        g_words, g_wcol = ((gvb + 16) // 4, gvb // 4) if gbf else (Kp + 4, Kp)
        return WireFormat(dt, Kp, vb, vb + 16, table_dtype, gbf, g_words, g_wcol)

    def empty_grads(self, n: int, device) -> torch.Tensor:
        """Gradient rows in the wire's gradient layout (fp32 words; bf16 pairs packed when ``grad_bf16``)."""
        return torch.empty((n, self.g_words), dtype=torch.float32, device=device)

    @property
    def fp32(self) -> bool:
        return self.dtype == torch.float32

    def empty(self, n: int, device) -> torch.Tensor:
        if self.fp32:
            return torch.empty((n, self.rb // 4), dtype=torch.float32, device=device)
        return torch.empty((n, self.rb), dtype=torch.uint8, device=device)

    def views(self, buf: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
        """(v [n, Kp] in the wire dtype, w [n] fp32 strided view; fp8 scale at w + 1) of a wire buffer."""
        if self.fp32:
            return buf[:, : self.Kp], buf[:, self.Kp]
        return buf.view(self.dtype)[:, : self.Kp], buf.view(torch.float32)[:, self.vb // 4]


def gather_wire(req: torch.Tensor, table: TableState, fmt: WireFormat, out: torch.Tensor,
                threads: int = 0, idx: torch.Tensor | None = None, run_off: torch.Tensor | None = None,
                W: int = 1, skip: tuple[int, int] | None = None) -> torch.Tensor:
    """Owner side of a sharded lookup: wire rows of table rows ``req`` into ``out`` (``fmt.empty``).

    With ``idx`` (GPU; patch gathers of the early row exchange) row p is ``req[idx[p]]``
    and its last tail word gets the tag ``idx[p] - run_off[run]`` (W ascending runs).
    ``skip`` (GPU, without ``idx``): requests [s0, s1) are left out (self rows)."""
    if fmt.fp32 and table.v.dtype == torch.float32 and idx is None:
        return gather_rows(req, table, fmt.Kp, out, threads=threads, skip=skip)
    _check(skip is None or idx is None, "skip ranges are for plain gathers")
    _check(_is_gpu(req), "non-fp32 wire formats and tagged gathers are a GPU path")
    R = req.numel() if idx is None else idx.numel()
    _chk_vec(req, torch.int32, None, "req", req.device)
    if idx is not None:
        _chk_vec(idx, torch.int32, R, "idx", req.device)
        _chk_vec(run_off, torch.int32, W + 1, "run_off", req.device)
    ok = out.is_contiguous() and out.shape[0] >= R and out.shape[1] * out.element_size() == fmt.rb
    _check(ok and out.dtype in (torch.uint8, torch.float32), "out: [R, rb bytes] wire buffer")
    v = table.v
    _chk_rows(v, fmt.Kp, "v")
    _range_check(req, v.shape[0], "req")
    to_bf16 = v.dtype == torch.float32 and fmt.dtype == torch.bfloat16
    _check(to_bf16 or v.dtype == fmt.dtype, f"wire dtype {fmt.dtype} cannot carry a {v.dtype} table")
    native.hip().gather_wire(R=R, req=_p(req), v=_p(v), v_bytes_stride=v.stride(0) * v.element_size(),
                             w=_p(table.w), w_stride=table.w.stride(0), vbytes=fmt.Kp * v.element_size(),
                             scaled=int(v.dtype == FP8), to_bf16=int(to_bf16), out=_p(out), rb=fmt.rb, vb=fmt.vb,
                             stream=_stream(req), idx=_p(idx), run_off=_p(run_off), W=int(W),
                             skip0=(skip or (0, 0))[0], skip1=(skip or (0, 0))[1])
    return out


def dirty_scan(req: torch.Tensor, run_off: torch.Tensor, W: int, prev: torch.Tensor, prev_off: torch.Tensor,
               Wp: int, flag: torch.Tensor, dcount: torch.Tensor, skip: tuple[int, int] | None = None) -> None:
    """GPU: flag[i] = req[i] in any of the Wp runs of ``prev``; dcount[q] = flagged per run q of ``req``.
    Requests in ``skip`` = [s0, s1) (self rows, read from the table) are never flagged."""
    R = req.numel()
    s0, s1 = skip or (0, 0)
    native.hip().dirty_scan(R=R, req=_p(req), W=int(W), run_off=_p(run_off), Wp=int(Wp), prev_off=_p(prev_off),
                            prev=_p(prev), flag=_p(flag), dcount=_p(dcount), stream=_stream(req), skip0=s0,
                            skip1=s1)


def select_flagged(flag: torch.Tensor, out: torch.Tensor, count: torch.Tensor, ws: torch.Tensor) -> None:
    """GPU stream compaction: out[0..count) = ascending i with flag[i] != 0 (no host sync)."""
    n = flag.numel()
    native.hip().select_flagged(n=n, flag=_p(flag), out=_p(out), count=_p(count), ws=_p(ws), ws_bytes=ws.numel(),
                                stream=_stream(flag))


def select_workspace(n: int, device) -> torch.Tensor:
    return torch.empty(max(native.hip().select_workspace_bytes(max(n, 1)), 1), dtype=torch.uint8, device=device)


def patch_scatter(recv: torch.Tensor, n: int, W: int, recv_off: torch.Tensor, sc_start: torch.Tensor,
                  gathered: torch.Tensor) -> None:
    """GPU: wire row p of ``recv`` (rank-major by owner, ``recv_off``) -> ``gathered[sc_start[owner] + tag]``."""
    rb = recv.shape[1] * recv.element_size()
    native.hip().patch_scatter(D=int(n), recv=_p(recv), rb=rb, W=int(W), recv_off=_p(recv_off),
                               sc_start=_p(sc_start), gathered=_p(gathered), stream=_stream(recv))


# ---------------------------------------------------------------------------
# GPU libsvm tokenizer (hip/parse.hip)
# ---------------------------------------------------------------------------
@dataclass
class ParsedGpu:
    labels: torch.Tensor     # [n] f32
    offsets: torch.Tensor    # [n+1] i32
    ids: torch.Tensor        # [nnz] i32
    vals: torch.Tensor | None  # [nnz] f32, None when every value is 1
    nnz: int
    max_feats: int
    fallback: bool           # syntax outside the GPU subset (or an error): re-parse on the CPU


class ParsePending:
    """A launched GPU tokenizer pass whose (fallback, max_feats, non-unit, nnz) summary is on its
    way to pinned host memory; ``finish()`` waits for it (an event, not a stream sync), so the
    caller can stage and launch the next batch in between."""

    def __init__(self, labels, offsets, ids, vals, info_h, ev):
        self.labels, self.offsets, self.ids, self.vals = labels, offsets, ids, vals
        self.info_h, self.ev = info_h, ev

    def finish(self) -> ParsedGpu:
        self.ev.synchronize()
        info = self.info_h
        fb, mf, nonunit, nnz = int(info[0]), int(info[1]), int(info[2]), int(info[4])
        return ParsedGpu(self.labels, self.offsets, self.ids[:nnz], self.vals[:nnz] if nonunit else None, nnz, mf,
                         bool(fb))


def parse_gpu_start(buf: torch.Tensor, line_start: torch.Tensor, vocab_size: int, hash_feature_id: bool = False,
                    stream: torch.cuda.Stream | None = None, require_vals: bool = False) -> ParsePending:
    """Launch the tokenizer of n '\n'-terminated libsvm lines (``buf`` uint8 on the GPU, line ``i``
    = ``buf[line_start[i]:line_start[i+1]]``) into CSR on the device, asynchronously on
    ``stream``; see ``parse_gpu``."""
    _check(_is_gpu(buf) and buf.dtype == torch.uint8 and buf.is_contiguous(), "buf: uint8 GPU bytes")
    _check(line_start.dtype == torch.int64 and line_start.device == buf.device, "line_start: int64 on buf's device")
    n = line_start.numel() - 1
    dev = buf.device
    st = stream or torch.cuda.current_stream(dev)
    h = native.hip()
    cap = buf.numel() // 2 + n + 1          # a token takes >= 2 bytes (separator + 1 char)
    i32 = dict(dtype=torch.int32, device=dev)
    with torch.cuda.stream(st):
        offsets = torch.empty(n + 1, **i32)
        counts = torch.empty(n + 1, **i32)
        labels = torch.empty(n, dtype=torch.float32, device=dev)
        ids = torch.empty(cap, **i32)
        vals = torch.empty(cap, dtype=torch.float32, device=dev)
        status = torch.empty(5, **i32)
        wsb = h.parse_workspace_bytes(max(n, 1))
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=dev)
        h.parse(buf=_p(buf), line_start=_p(line_start), n=n, vocab=int(vocab_size), hash=int(bool(hash_feature_id)),
                counts=_p(counts), offsets=_p(offsets), labels=_p(labels), ids=_p(ids), vals=_p(vals),
                status=_p(status), ws=_p(ws), ws_bytes=wsb, stream=st.cuda_stream,
                require_vals=int(bool(require_vals)))
        status[4:5].copy_(offsets[n:])   # (fallback, max_feats, non-unit, -, nnz)
        info_h = torch.empty(5, dtype=torch.int32, pin_memory=True)
        info_h.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(st)
    return ParsePending(labels, offsets, ids, vals, info_h, ev)


def parse_gpu(buf: torch.Tensor, line_start: torch.Tensor, vocab_size: int, hash_feature_id: bool = False,
              stream: torch.cuda.Stream | None = None, require_vals: bool = False) -> ParsedGpu:
    """Tokenize n '\n'-terminated libsvm lines on the GPU (launch + wait, see
    ``parse_gpu_start``).  When ``fallback`` is set the outputs are incomplete and the caller
    must parse the lines with the CPU parser (exact reference semantics and error messages)."""
    return parse_gpu_start(buf, line_start, vocab_size, hash_feature_id, stream, require_vals).finish()


def run_member(req: torch.Tensor, prev: torch.Tensor, prev_run_off: torch.Tensor | None,
               prev_splits: list[int]) -> torch.Tensor:
    """int32 flag per element of ``req``: 1 when the row is in ``prev`` (W ascending runs of
    ``prev_splits`` rows, device offsets ``prev_run_off`` on the GPU), else 0."""
    R = req.numel()
    flag = torch.empty(R, dtype=torch.int32, device=req.device)
    if R == 0:
        return flag
    P = int(sum(prev_splits))
    if not _is_gpu(req):
        return torch.isin(req, prev[:P]).to(torch.int32)
    _chk_vec(req, torch.int32, R, "req", req.device)
    _chk_vec(prev, torch.int32, P, "prev", req.device)
    _chk_vec(prev_run_off, torch.int32, len(prev_splits) + 1, "prev_run_off", req.device)
    native.hip().run_member(R=R, req=_p(req), W=len(prev_splits), run_off=_p(prev_run_off), prev=_p(prev),
                            flag=_p(flag), stream=_stream(req))
    return flag
