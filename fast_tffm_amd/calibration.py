"""Calibrated probabilities: a monotone map from raw score to P(positive), fitted on held-out data.

``Calibrator`` holds the thresholds of an exact isotonic fit (ops/kernels.py ``isotonic_fit`` /
``calibrate_apply``) and what it was fitted on.  ``run.py calibrate`` writes one as ``calibration.json``
into the checkpoint's directory, ``run.py predict --calibrated`` and ``ServingModel.predict_proba`` apply it.
"""

from __future__ import annotations

import json
import os

import numpy as np
import torch

FILE_NAME = "calibration.json"
FORMAT = "fast_tffm_amd/calibration-v1"


class CalibrationError(RuntimeError):
    """``calibrate`` / ``predict --calibrated`` cannot run as asked (the command line prints it and exits 1)."""


class Calibrator:
    """``x = [lo_0, hi_0, lo_1, hi_1, ...]`` (fp32 scores, ascending) and ``y = [v_0, v_0, v_1, v_1, ...]`` (fp32
    probabilities, non-decreasing): a score inside block b maps to ``v_b``, one between two blocks is
    interpolated (``calibrate_apply``).  ``meta``: examples, total weight, positives, blocks, the checkpoint's
    global step and whether the fit was weighted."""

    def __init__(self, x, y, meta: dict | None = None):
        self.x = torch.as_tensor(x, dtype=torch.float32).cpu().contiguous()
        self.y = torch.as_tensor(y, dtype=torch.float32).cpu().contiguous()
        if self.x.dim() != 1 or self.x.numel() < 2 or self.x.numel() % 2 or self.y.shape != self.x.shape:
            raise ValueError("Calibrator: x and y hold two entries per block, at least one block")
        if bool(torch.isnan(self.x).any()) or bool(torch.isnan(self.y).any()):
            raise ValueError("Calibrator: NaN threshold or value")
        if bool((self.x[1:] < self.x[:-1]).any()) or bool((self.y[1:] < self.y[:-1]).any()):
            raise ValueError("Calibrator: thresholds and values must ascend")
        self.meta = dict(meta or {})
        self._dev: dict = {}

    @classmethod
    def from_fit(cls, fit, **meta) -> "Calibrator":
        """From an ``IsotonicFit`` (one host read of its blocks)."""
        x, y = fit.calibrator()
        w, p = fit.totals()
        info = {"examples": int(fit.n), "total_weight": w, "positives": p, "blocks": x.numel() // 2,
                "weighted": bool(fit.weighted)}
        info.update(meta)
        return cls(x, y, info)

    @property
    def blocks(self) -> int:
        return self.x.numel() // 2

    def __call__(self, scores) -> torch.Tensor:
        """Calibrated probabilities of raw scores (fp32 tensor or array), on the scores' device."""
        from .ops.kernels import calibrate_apply

        s = scores if isinstance(scores, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(scores, np.float32))
        s = s.to(torch.float32).reshape(-1).contiguous()
        if s.device not in self._dev:
            self._dev[s.device] = (self.x.to(s.device), self.y.to(s.device))
        x, y = self._dev[s.device]
        return calibrate_apply(s, x, y)

    def save(self, path: str) -> str:
        """JSON; the fp32 thresholds and values are written as Python floats, which round-trip exactly."""
        doc = {"format": FORMAT, **self.meta, "x": self.x.tolist(), "y": self.y.tolist()}
        tmp = path + ".tmp"
        with open(tmp, "w") as f:
            json.dump(doc, f, indent=1)
        os.replace(tmp, path)
        return path

    @classmethod
    def load(cls, path: str) -> "Calibrator":
        with open(path) as f:
            doc = json.load(f)  # (an infinite threshold is written, and read back, as Infinity)
        if doc.get("format") != FORMAT:
            raise ValueError(f"{path}: not a {FORMAT} file")
        x, y = doc.pop("x"), doc.pop("y")
        doc.pop("format")
        return cls(x, y, doc)


def log_loss_sum_of_blocks(weight, positives, value) -> float:
    """Weighted log loss sum of a fit's own values over its own examples, from the blocks (host, fp64): block b
    adds -(Y_b log v_b + (W_b - Y_b) log(1 - v_b)); a block with v of 0 or 1 adds 0."""
    w = np.asarray(weight, np.float64)
    y = np.asarray(positives, np.float64)
    v = np.asarray(value, np.float64)
    inner = (v > 0) & (v < 1)
    return float(-(y[inner] * np.log(v[inner]) + (w[inner] - y[inner]) * np.log1p(-v[inner])).sum())
