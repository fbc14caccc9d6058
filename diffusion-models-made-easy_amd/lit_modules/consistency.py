"""LitConsistency: the training facade of consistency distillation (diffusion_models/consistency.py).  It exposes `.diffusion_model` like
every Lit module here, so `train_loop.train_step`, the gradient reducer and the AMP path drive it unchanged; the fit loop calls the
process's `after_step()` after every optimiser step.  The reference project has no such module."""

from __future__ import annotations

from torch import Tensor, nn

from ..diffusion_models.consistency import ConsistencyDistillation
from .ddpm import _Base


class LitConsistency(_Base):
    def __init__(self, diffusion_model: ConsistencyDistillation, lr: float = 1e-4, sample_steps: int = 1, ema_decay: float = 0.0) -> None:
        """`sample_steps`: the K of the sampler `forward` and `generate` run (K divides the training grid's N).  `ema_decay` defaults to 0:
        the checkpoint holds the student as trained."""
        super().__init__()
        if not isinstance(diffusion_model, ConsistencyDistillation):
            raise TypeError("LitConsistency wraps a ConsistencyDistillation process")
        self.lr = lr
        self.sample_steps = int(sample_steps)
        self.ema_decay = ema_decay
        self.diffusion_model = diffusion_model

    def _the_sampler(self):
        s = getattr(self, "_sampler", None)
        if s is None or s.sub_timesteps != self.sample_steps or s.model is not self.diffusion_model.model:
            s = self.diffusion_model.sampler(self.sample_steps)
            object.__setattr__(self, "_sampler", s)
        return s

    def forward(self, x: Tensor, i: int):
        r"""one step of the K-step consistency sampler: x_{tau_i} -> x_{tau_{i-1}} on its K-point grid"""
        return self._the_sampler().denoise_once(x, int(i))

    def training_step(self, batch, batch_idx):
        loss = self.diffusion_model.training_step(batch[0])
        if hasattr(self, "log") and _Base is not nn.Module:
            self.log("train/loss", loss)
        return loss

    def generate(self, img_size):
        return self._the_sampler().generate(img_size)

    def configure_optimizers(self):
        """Adam over the student only, at a constant rate"""
        from ..optim import FusedAdam

        return [FusedAdam(self.diffusion_model.parameters(), lr=self.lr, ema_decay=self.ema_decay)], []
