"""LitClassifierFreeDDPM: LitDDPM over a class-conditional network trained with label dropout (classifier-free guidance,
Ho & Salimans 2021).  The batch is (images, labels), as the data modules yield it."""

from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from ..models.cond import ConditionalUNet
from .ddpm import LitDDPM, _Base


class LitClassifierFreeDDPM(LitDDPM):
    conditional = True  # train_loop: the step takes the loader's labels

    def __init__(
        self,
        lr: float = 2e-4,
        warmup: int = 5000,
        decay: float = 0.9999,
        diffusion_model: Optional[nn.Module] = None,
        model: Optional[nn.Module] = None,
        timesteps: int = 1000,
        num_classes: int = 10,
        guidance_scale: float = 1.0,
        p_uncond: float = 0.1,
        prediction: str = "eps",
        loss_weight: str = "uniform",
        snr_gamma: float = 5.0,
    ) -> None:
        if diffusion_model is None:
            from ..guidance.cfg import ClassifierFreeDDPM

            if model is None:
                model = ConditionalUNet(num_classes=num_classes)
            diffusion_model = ClassifierFreeDDPM(model, timesteps, guidance_scale, p_uncond, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma)
        super().__init__(lr, warmup, decay, diffusion_model)

    def forward(self, x_t: Tensor, t, y):
        r"""denoise once with guidance: x_t -> x_{t-1} for the labels y"""
        return self.diffusion_model.sampling_step(x_t, torch.as_tensor(t, device=x_t.device).reshape(1), y)

    def training_step(self, batch, batch_idx):
        r"""L_simple on (batch[0], batch[1]) with label dropout"""
        loss = self.diffusion_model.training_step(batch[0], batch[1])
        if hasattr(self, "log") and _Base is not nn.Module:
            self.log("train/loss", loss)
        return loss

    def generate(self, img_size, y):
        return self.diffusion_model.generate(img_size=img_size, y=y)
