"""What a training step returns: shared by the model and the multi-rank executors."""

from __future__ import annotations

from dataclasses import dataclass

import torch


@dataclass
class StepOut:
    loss_sum: torch.Tensor            # 0-d, summed weighted loss of this rank's batch
    n: int                            # examples in this rank's batch

    def mean_loss(self) -> float:
        return float(self.loss_sum) / max(self.n, 1)
