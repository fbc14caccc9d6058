"""DDNM (Wang, Yu, Zhang 2023, "Zero-Shot Image Restoration Using Denoising Diffusion Null-Space Model"): super-resolution, colourisation,
inpainting and their compositions over any unconditionally trained network of the package, training-free, as device-resident chains.

The degradation is A = M o Pool_s o Gray_g on images (B, C, H, W): Gray_g the mean over the channels (`gray=True`, Cm = 1) or the identity
(Cm = C), Pool_s the mean over s x s blocks, to (B, Cm, h, w) = (B, Cm, H/s, W/s), M a binary mask at measurement resolution (1 =
measured).  A cell is the n = (C if gray else 1) s s image elements one measurement value averages; the pseudo-inverse A+ y gives every
element of a cell the cell's value m y, and A A+ A = A, A+ A A+ = A+ hold exactly (a fractional mask would break the first).

Grid 0 = tau_0 < tau_1 < ... < tau_n = T (`solver_grid(alpha_bar, sub_timesteps, "linear")`, RePaint's); the walk is
`repaint_levels(n, travel_length, travel_repeat)`, the paper's "time travel" (1 / 1: straight down).  Every downward transition
a -> b = a - 1 is one network evaluation and one table row (DDNM+, eq. 17-19; alpha = abar_a / abar_b, beta = 1 - alpha):

    x0 = A_t x - B_t eps                       the network's x0 prediction
    r  = m (mean_cell(x0) - y)                 one value per cell: what A x0 misses of the measurement
    xh = x0 - lambda r                         x0 with its range-space part rectified: A xh = y on measured cells where lambda = 1
    u  = ca xh + cb x [+ cz z0]                the posterior q(x_b | x_a, xh) with the measurement's noise taken off its variance
    x' = u, or r0 u + r1 z1                    the walk's next upward run b -> c, folded into one Gaussian as `repaint_rows` folds it

With sigma_y > 0 the last row has lambda = 0: a noisy measurement is not imposed on the final image (the paper's behaviour).  The host
computes the rows in float64 and rounds them to fp32 once (include/dmme_hip.h: dmme_ddnm_step); the cell reduction is the device's work
(csrc/ddnm.hip)."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian
from .chain import ROW_DRAWS, ChainRunner, eager_chain
from .conditioned import GridProcess, check_mask, fp32_tables
from .dpm_solver import _row_arg
from .repaint import repaint_levels

ROW = 8  # floats per table row: ca, cb, cz, A_t, B_t, lambda, r0, r1
STREAMS = 2  # normal streams a step owns: z0 (the posterior's noise), z1 (the jump)
ROW_DRAWS[_lib.CHAIN_DDNM] = lambda row: row[2] != 0.0 or row[7] != 0.0  # (cz of the posterior's noise, r1 of a folded jump)


def ddnm_rows(alpha_bar, grid: Sequence[int], walk: Sequence[int], sigma_y: float = 0.0) -> Tuple[np.ndarray, List[int]]:
    """(float64 rows [n_rows + 1][8], t_table [n_rows + 1]) of a level walk: one row {ca, cb, cz, A_t, B_t, lambda, r0, r1} per downward
    transition a -> b with the upward run b -> c behind it folded in; the k-th transition sits at loop index n_rows - k, t_table there is
    tau_a.  Row 0 is never stepped from.  With var = beta (1 - abar_b)/(1 - abar_a) and sigma = sqrt(var): lambda = 1 where
    sigma_y = 0 or sigma >= ca sigma_y, else sigma / (ca sigma_y); cz = sqrt(max(var - (ca lambda sigma_y)^2, 0)) (the difference comes
    out a few 1e-18 below zero where lambda < 1).  For b = 0 the row is exactly (1, 0, 0, A_t, B_t, lambda, 1, 0)."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    sy = float(sigma_y)
    if not sy >= 0.0:
        raise ValueError(f"ddnm_rows: sigma_y = {sigma_y!r} must be at least 0")
    walk = [int(v) for v in walk]
    steps, p, last = [], 0, len(walk) - 1
    while p < last:
        a, b = walk[p], walk[p + 1]
        if b != a - 1 or b < 0:
            raise ValueError(f"ddnm_rows: the walk goes {a} -> {b} where a step down by one level was due")
        p += 1
        c = b
        while p < last and walk[p + 1] == walk[p] + 1:
            p, c = p + 1, c + 1
        steps.append((a, b, c))
    n_rows = len(steps)
    rows = np.zeros((n_rows + 1, ROW), dtype=np.float64)
    rows[0] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 1.0, 0.0)
    ttab = [0] * (n_rows + 1)
    for k, (a, b, c) in enumerate(steps):
        i = n_rows - k
        ab_a, ab_b, ab_c = ab[grid[a]], ab[grid[b]], ab[grid[c]]
        A_t, B_t = 1.0 / np.sqrt(ab_a), np.sqrt(1.0 - ab_a) / np.sqrt(ab_a)
        if b == 0:
            rows[i] = (1.0, 0.0, 0.0, A_t, B_t, 1.0 if sy == 0.0 else 0.0, 1.0, 0.0)
        else:
            alpha = ab_a / ab_b
            beta = 1.0 - alpha
            ca, cb = np.sqrt(ab_b) * beta / (1.0 - ab_a), np.sqrt(alpha) * (1.0 - ab_b) / (1.0 - ab_a)
            var = beta * (1.0 - ab_b) / (1.0 - ab_a)
            sigma = np.sqrt(var)
            lam = 1.0 if sy == 0.0 or sigma >= ca * sy else sigma / (ca * sy)
            cz = np.sqrt(max(var - (ca * lam * sy) ** 2, 0.0))
            r0, r1 = (1.0, 0.0) if c == b else (np.sqrt(ab_c / ab_b), np.sqrt(1.0 - ab_c / ab_b))
            rows[i] = (ca, cb, cz, A_t, B_t, lam, r0, r1)
        ttab[i] = int(grid[a])
    return rows, ttab


class RestoreChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_ddnm_chain_step: tables of 8 floats per index, the measurement and its mask in fixed buffers
    of measurement shape (B, Cm, h, w) (read only: a chain fills them once), two normal streams per step"""

    _side = ("y", "mask")

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        self.scale, self.gray = process.scale, int(process.gray)
        shape = process.measurement_shape(x.shape)
        self.y = torch.zeros(shape, dtype=torch.float32, device=x.device)
        self.mask = torch.zeros(shape, dtype=torch.float32, device=x.device)
        self.noise_numel = STREAMS * x.numel()

    def _call(self, packed):
        _lib.check(
            _lib.lib().dmme_ddnm_chain_step(self.plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.plan.workspace), _lib.ptr(self.y),
                                            _lib.ptr(self.mask), self.scale, self.gray, _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state),
                                            _lib.stream_ptr()),
            "dmme_ddnm_chain_step",
        )

    def restore(self, x: Tensor, y: Tensor, mask: Tensor, first: int, recorder=None) -> Tensor:
        return self.run_copies(x, (y, mask), first, recorder)


class DDNM(GridProcess):
    r"""DDNM+ over any unconditional noise-prediction network of the package (an IDDPM network's learned variance is not used), or an
    x0 / v network (`prediction=`).

    `sub_timesteps`: levels of the grid; `scale`: s of the s x s average pooling (1: none), a divisor of the height and width of the images
    restored; `gray`: the measurement is the mean of the channels; `sigma_y`: the noise level of the measurement (0: noiseless);
    `travel_length`, `travel_repeat`: the walk of `repaint_levels` (1 / 1: straight down).  `alpha_bar`: a (T+1) table in place of the
    linear schedule's (`from_process` takes it from a DDPM / IDDPM instance)."""

    _chain_kind = _lib.CHAIN_DDNM
    _runner_class = RestoreChainRunner
    _whole_chains = "DDNM runs whole chains: restore / generate"

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 100, scale: int = 1, gray: bool = False, sigma_y: float = 0.0,
                 travel_length: int = 1, travel_repeat: int = 1, start: float = 0.0001, end: float = 0.02, alpha_bar: Optional[Tensor] = None, *,
                 prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        for name, v in (("scale", scale), ("travel_length", travel_length), ("travel_repeat", travel_repeat)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError(f"{name} = {v!r}; an integer of at least 1")
        if isinstance(sigma_y, bool) or not float(sigma_y) >= 0.0 or not np.isfinite(float(sigma_y)):
            raise ValueError(f"sigma_y = {sigma_y!r}; a finite noise level of at least 0")
        self._set_grid(sub_timesteps, alpha_bar)
        self.scale, self.gray, self.sigma_y = int(scale), bool(gray), float(sigma_y)
        self.travel_length, self.travel_repeat = int(travel_length), int(travel_repeat)
        self._walk = repaint_levels(self.n_levels, self.travel_length, self.travel_repeat)
        self._tables = fp32_tables(*ddnm_rows(self._ab64, self._tau_host, self._walk, self.sigma_y))
        self.n_rows = self._tables[0]

    # ------------------------------------------------------------------ the operator
    def measurement_shape(self, image_shape) -> Tuple[int, int, int, int]:
        """(B, Cm, h, w) of A x for images of `image_shape`; refuses a size the scale does not divide"""
        B, Cc, H, W = (int(v) for v in image_shape)
        s = self.scale
        if H % s != 0 or W % s != 0:
            raise ValueError(f"DDNM: the image size {H} x {W} is not divisible by scale = {s}")
        return B, 1 if self.gray else Cc, H // s, W // s

    def _channels(self, Cm: int) -> int:
        """the channels of the images a measurement of Cm channels comes from"""
        return int(getattr(self.model, "in_channels", 3)) if self.gray else int(Cm)

    @staticmethod
    def _mask(mask, shape, device, none_value: float) -> Tensor:
        """(B|1, Cm|1, h, w) with values 0 or 1 -> contiguous fp32 of the measurement's shape; None: `none_value` everywhere"""
        return check_mask(mask, shape, device, none_value, channels="Cm", why=": a fractional mask has no pseudo-inverse of this form")

    @torch.no_grad()
    def degrade(self, x: Tensor, mask=None) -> Tensor:
        """A x on the device (dmme_ddnm_measure): the measurement (B, Cm, h, w) of an image batch; unmeasured cells are 0"""
        src = self._image(x, "degrade")
        B, Cc, H, W = src.shape
        shape = self.measurement_shape(src.shape)
        m = None if mask is None else self._mask(mask, shape, src.device, 1.0)
        y = torch.empty(shape, dtype=torch.float32, device=src.device)
        _lib.check(_lib.lib().dmme_ddnm_measure(_lib.ptr(src), _lib.ptr(m), _lib.ptr(y), B, Cc, H, W, self.scale, int(self.gray), _lib.stream_ptr()), "dmme_ddnm_measure")
        return y

    def pinv(self, y: Tensor, mask=None) -> Tensor:
        """A+ y on the host: every element of a cell gets the cell's value m y; (B, Cm, h, w) -> (B, C, H, W)"""
        if not (isinstance(y, Tensor) and y.dim() == 4 and y.is_floating_point()):
            raise ValueError("pinv: a floating-point measurement batch (B, Cm, h, w)")
        if self.gray and y.shape[1] != 1:
            raise ValueError(f"pinv: a grey measurement has one channel, got {y.shape[1]}")
        if mask is not None:
            y = y * self._mask(mask, tuple(y.shape), y.device, 1.0).to(y.dtype)
        out = y.repeat_interleave(self.scale, dim=2).repeat_interleave(self.scale, dim=3)
        return out.repeat_interleave(self._channels(y.shape[1]), dim=1) if self.gray else out

    # ------------------------------------------------------------------ chains
    def _eager_chain(self, x: Tensor, y: Tensor, mask: Tensor, history=None) -> Tensor:
        """the host loop over dmme_ddnm_step (`eager_chain`), in place on x"""
        B, Cc, H, W = x.shape

        def call(row, t, z):
            eps = self._eps(x, t).detach().to(torch.float32).contiguous()
            _lib.check(_lib.lib().dmme_ddnm_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(y), _lib.ptr(mask), _lib.ptr(z), _row_arg(row), B, Cc, H, W, self.scale,
                                                 int(self.gray), eps[0].numel() // x[0].numel(), _lib.stream_ptr()), "dmme_ddnm_step")

        return eager_chain(x, _lib.CHAIN_DDNM, self._tables, self._tables[0], STREAMS, call, history)

    def _chain(self, x: Tensor, y: Tensor, mask: Tensor, history=None) -> Tensor:
        runner = self._buffered_runner("_runner", x.shape, x.device)
        if runner is None:
            return self._eager_chain(x, y, mask, history)
        return runner.restore(x, y, mask, self._tables[0], history)

    @torch.no_grad()
    def restore(self, y: Tensor, mask=None, history=None) -> Tensor:
        r"""images (B, C, H, W) = (B, C, s h, s w) whose degradation reproduces the measurement `y` (B, Cm, h, w) where `mask` (B|1, Cm|1,
        h, w; None: everywhere) is 1, and that the network finds plausible elsewhere: x_T ~ N(0, I), then the whole walk through the
        captured step.  `history`: a HistoryRecorder for the walk's frames (`n_rows` steps)."""
        meas = self._image(y, "restore")
        B, Cm, h, w = meas.shape
        if self.gray and Cm != 1:
            raise ValueError(f"restore: a grey measurement has one channel, got {Cm}")
        shape = (B, self._channels(Cm), h * self.scale, w * self.scale)
        if self.measurement_shape(shape) != tuple(meas.shape):
            raise ValueError(f"restore: a measurement of shape {tuple(meas.shape)} does not come from images of {shape}")
        m = self._mask(mask, tuple(meas.shape), meas.device, 1.0)
        return self._chain(gaussian(shape, device=meas.device), meas, m, history)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """`restore` with nothing measured (an all-zero mask): the unconditioned walk from pure noise"""
        shape = self.measurement_shape(img_size)
        zeros = torch.zeros(shape, dtype=torch.float32, device=self.beta.device)
        return self._chain(gaussian(tuple(img_size), device=zeros.device), zeros, zeros, history)
