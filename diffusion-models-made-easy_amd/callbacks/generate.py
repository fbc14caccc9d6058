"""GenerateImage: samples that show how training is going (reference: src/dmme/callbacks/generate.py:10-88).

Same constructor as the reference's callback.  `generate_img` is its host loop, step by step through the module's forward;
`grid` is the same picture from ONE device-resident chain with a HistoryRecorder (a launch per kept frame instead of a clone and
a denorm per frame and a make_grid at the end).  There is no logger here, so nothing calls the callback by itself: the bundled
runner writes `grid` to PNG files (`trainer fit --preview-dir`)."""

from __future__ import annotations

from typing import Tuple

import torch

from ..common.noise import gaussian
from ..common.norm import denorm
from ..diffusion_models.ddpm import HistoryRecorder, history_ordinals


class GenerateImage:
    """Sample from the model being trained and show the chain.  Constructor as in the reference's callback:

    imgsize (C, H, W) of one image; timesteps: steps of `generate_img`'s host loop; batch_size: images sampled; vis_length: frames
    of each image's chain that are kept; every_n_epochs: read from the reference's YAML files and kept, not used (the bundled
    runner counts optimiser steps: `--preview-every`)."""

    def __init__(self, imgsize: Tuple[int, int, int], timesteps: int, batch_size: int = 8, vis_length: int = 20, every_n_epochs: int = 5):
        self.imgsize = tuple(int(v) for v in imgsize)
        self.timesteps = timesteps
        self.batch_size = batch_size
        self.vis_length = vis_length
        self.every_n_epochs = every_n_epochs
        self._recorder = None

    @staticmethod
    def _device(pl_module):
        return next(pl_module.parameters()).device

    def _frame(self, x_t):
        return denorm(x_t.detach().clone())

    @torch.no_grad()
    def generate_img(self, pl_module):
        """the host loop of the reference (callbacks/generate.py:64-88), one `pl_module(x_t, t)` per step from t = timesteps down to 1:
        the list of denormed frames, x_t in front of the step from each t = int(timesteps / (vis_length - 1) * i), then the result.
        Runs in eval mode and puts the module back into the mode it found."""
        was_training = pl_module.training
        pl_module.eval()
        try:
            L, total = self.vis_length, self.timesteps
            wanted = {int(total / (L - 1) * i) for i in range(1, L)}
            x_t = gaussian((self.batch_size, *self.imgsize), device=self._device(pl_module))
            frames = []
            for t in range(total, 0, -1):
                if t in wanted:
                    frames.append(self._frame(x_t))
                x_t = pl_module(x_t, t)
            frames.append(self._frame(x_t))
        finally:
            pl_module.train(was_training)
        return frames

    def recorder(self, count: int, out_kind: int, device) -> HistoryRecorder:
        """the recorder of a `count`-step chain, kept between calls (one canvas per callback, not one per preview)"""
        key = (int(count), int(out_kind), torch.device(device))
        if self._recorder is None or self._recorder[0] != key:
            rec = HistoryRecorder(self.batch_size, *self.imgsize, history_ordinals(count, self.vis_length), out_kind, device)
            self._recorder = (key, rec)
        return self._recorder[1]

    @torch.no_grad()
    def grid(self, pl_module, out_kind: int = 0, y=None):
        """the history grid, (Cg, batch_size rows, vis_length columns of images), from one `generate(..., history=recorder)` of the
        module's diffusion process: its own chain (a DDIM module: its S steps), frames spread over it as the reference spreads them over
        `timesteps`.  For a LitDDPM with `timesteps` = T this equals `make_history(generate_img(pl_module))` under the same seed.
        out_kind 0: float32 in [0, 1]; 1: uint8.  `y`: labels for a class-conditional module (default: the null label).
        The chain is the process's own, with its x0 thresholding (`threshold=` / `set_threshold`) as it is set.
        The canvas belongs to the callback: the next call overwrites it."""
        dm = pl_module.diffusion_model
        was_training = pl_module.training
        pl_module.eval()
        try:
            dev = self._device(pl_module)
            rec = self.recorder(dm.chain_length(), out_kind, dev)
            shape = (self.batch_size, *self.imgsize)
            if getattr(pl_module, "conditional", False):
                dm.generate(shape, [dm.model.null_label] * self.batch_size if y is None else y, history=rec)
            else:
                dm.generate(shape, history=rec)
        finally:
            pl_module.train(was_training)
        return rec.canvas
