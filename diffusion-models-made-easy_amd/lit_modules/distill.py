"""LitDistill: the training facade of progressive distillation (diffusion_models/distill.py).  It exposes `.diffusion_model` like every
Lit module here, so `train_loop.train_step`, the gradient reducer and the AMP path drive it unchanged.  The reference project has no such
module."""

from __future__ import annotations

from torch import Tensor, nn

from ..diffusion_models.distill import ProgressiveDistillation
from ..lr_scheduler import LinearDecayLR
from .ddpm import _Base


class LitDistill(_Base):
    def __init__(self, diffusion_model: ProgressiveDistillation, lr: float = 1e-4, stage_steps: int = 50_000, ema_decay: float = 0.0) -> None:
        """`stage_steps`: optimiser steps of one halving stage, over which the rate falls linearly to zero.  `ema_decay` defaults to 0: the
        next stage's teacher is the student as trained."""
        super().__init__()
        if not isinstance(diffusion_model, ProgressiveDistillation):
            raise TypeError("LitDistill wraps a ProgressiveDistillation process")
        self.lr = lr
        self.stage_steps = int(stage_steps)
        self.ema_decay = ema_decay
        self.diffusion_model = diffusion_model

    def forward(self, x: Tensor, i: int):
        r"""one step of the sampler the student is trained for: x_{tau_i} -> x_{tau_{i-1}} on its N-point grid"""
        s = getattr(self, "_sampler", None)
        if s is None or s.sub_timesteps != self.diffusion_model.steps or s.model is not self.diffusion_model.model:
            s = self.diffusion_model.sampler()
            object.__setattr__(self, "_sampler", s)
        return s.denoise_once(x, int(i))

    def training_step(self, batch, batch_idx):
        loss = self.diffusion_model.training_step(batch[0])
        if hasattr(self, "log") and _Base is not nn.Module:
            self.log("train/loss", loss)
        return loss

    def generate(self, img_size):
        return self.diffusion_model.sampler().generate(img_size)

    def configure_optimizers(self):
        """Adam over the student only, its rate falling linearly to zero over the stage; built fresh for every stage"""
        from ..optim import FusedAdam

        optimizer = FusedAdam(self.diffusion_model.parameters(), lr=self.lr, ema_decay=self.ema_decay)
        scheduler = {"scheduler": LinearDecayLR(optimizer, self.stage_steps), "interval": "step", "frequency": 1}
        return [optimizer], [scheduler]
