"""DPS (Chung et al., ICLR 2023, "Diffusion Posterior Sampling for General Noisy Inverse Problems", Algorithm 1): restoration from a
noisy linear measurement y = A x + n over any unconditional eps network of the package, training-free, as device-resident chains.

The operator acts on each channel plane: A x = M o (Kh x_c Kw^T) on images (B, C, H, W), to (B, C, h, w); Kh [h][H] and Kw [w][W] are
dense matrices (`SeparableOperator`: identity, Gaussian blur, bicubic and average down-sampling presets, built in float64 and rounded to
fp32 once; the device reads them as dense and assumes nothing else), M a binary mask at measurement resolution (1 = measured).  Unlike
DDNM's, the family needs no closed-form pseudo-inverse: blur is in it, and a noisy measurement is handled by the method itself.

Grid 0 = tau_0 < tau_1 < ... < tau_n = T (`solver_grid(alpha_bar, sub_timesteps, "linear")`, RePaint's); the walk goes straight down.
Every transition a -> b = a - 1 is one network evaluation, one input gradient and one table row (alpha = abar_a / abar_b):

    x0 = A_t x - B_t eps                       the network's x0 prediction
    r  = m (y - A x0)                          the residual, at measurement resolution
    g  = A^T r;   dx = J_eps(x)^T (B_t g)      the adjoint (csrc/dps.hip) and the network's input-only backward
    u  = c0 (x - c1 eps) [+ c2 z]              DDPM's reverse step (sigma^2 = 1 - alpha)
    x' = u + (zeta / ||r_b||) (A_t g - dx)     = u - zeta grad_x ||y - A x0(x)||, per image b

A step costs one keep-forward plus one input-backward of the network.  The host computes the rows in float64 and rounds them to fp32
once (include/dmme_hip.h: dmme_dps_step)."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like
from .chain import ROW_DRAWS, KeepForwardRunner, eager_chain
from .conditioned import GridProcess, check_mask, fp32_tables
from .dpm_solver import _row_arg
from .ilvr import resize_matrix

ROW = 8  # floats per table row: c0, c1, c2, A_t, B_t, zeta, -, -
STREAMS = 1  # normal streams a step owns: z (the reverse step)
ROW_DRAWS[_lib.CHAIN_DPS] = lambda row: row[2] != 0.0  # (c2 of the reverse step's noise)
OPERATORS = ("identity", "blur", "bicubic", "average")


def _size(name: str, v) -> int:
    if isinstance(v, bool) or int(v) != v or v < 1:
        raise ValueError(f"{name} = {v!r}; an integer of at least 1")
    return int(v)


class SeparableOperator:
    """A = Kh . Kw^T per channel plane: float64 Kh [h][H] and Kw [w][W] with h <= H, w <= W, and their fp32 device copies (rounded once,
    cached per device).  The presets are the class methods; any pair of dense matrices of these shapes is an operator."""

    def __init__(self, Kh, Kw, name: str = "custom"):
        Kh, Kw = np.ascontiguousarray(Kh, dtype=np.float64), np.ascontiguousarray(Kw, dtype=np.float64)
        if Kh.ndim != 2 or Kw.ndim != 2 or Kh.shape[0] > Kh.shape[1] or Kw.shape[0] > Kw.shape[1] or 0 in Kh.shape or 0 in Kw.shape:
            raise ValueError(f"SeparableOperator: Kh {Kh.shape} and Kw {Kw.shape} must be [h][H] and [w][W] with 1 <= h <= H, 1 <= w <= W")
        if not (np.isfinite(Kh).all() and np.isfinite(Kw).all()):
            raise ValueError("SeparableOperator: the matrices must be finite")
        self.Kh, self.Kw, self.name = Kh, Kw, str(name)
        self._dev = {}

    h = property(lambda self: self.Kh.shape[0])
    H = property(lambda self: self.Kh.shape[1])
    w = property(lambda self: self.Kw.shape[0])
    W = property(lambda self: self.Kw.shape[1])

    def __repr__(self):
        return f"SeparableOperator({self.name}: {self.H} x {self.W} -> {self.h} x {self.w})"

    def device(self, device) -> Tuple[Tensor, Tensor]:
        """the fp32 copies of (Kh, Kw) on `device`, built once"""
        key = torch.device(device)
        if key not in self._dev:
            self._dev[key] = tuple(torch.from_numpy(K.astype(np.float32)).contiguous().to(key) for K in (self.Kh, self.Kw))
        return self._dev[key]

    def measurement_shape(self, image_shape) -> Tuple[int, int, int, int]:
        B, Cc, H, W = (int(v) for v in image_shape)
        if (H, W) != (self.H, self.W):
            raise ValueError(f"{self!r} does not act on images of {H} x {W}")
        return B, Cc, self.h, self.w

    # ------------------------------------------------------------------ presets
    @classmethod
    def identity(cls, H: int, W: int) -> "SeparableOperator":
        return cls(np.eye(_size("H", H)), np.eye(_size("W", W)), "identity")

    @staticmethod
    def _blur_matrix(n: int, size: int, sigma: float) -> np.ndarray:
        K = np.zeros((n, n), dtype=np.float64)
        half = size // 2
        for i in range(n):
            lo, hi = max(i - half, 0), min(i + half + 1, n)
            wts = np.exp(-0.5 * ((np.arange(lo, hi, dtype=np.float64) - i) / sigma) ** 2)
            K[i, lo:hi] = wts / wts.sum()
        return K

    @classmethod
    def gaussian_blur(cls, H: int, W: int, size: int = 9, sigma: float = 2.0) -> "SeparableOperator":
        """a Gaussian kernel of `size` taps (odd) and standard deviation `sigma` along each axis, as a band matrix: windows clipped to
        the image and renormalised, so every row sums to 1"""
        H, W, size = _size("H", H), _size("W", W), _size("size", size)
        if size % 2 != 1:
            raise ValueError(f"size = {size}; an odd number of taps")
        if isinstance(sigma, bool) or not float(sigma) > 0.0 or not np.isfinite(float(sigma)):
            raise ValueError(f"sigma = {sigma!r}; a positive standard deviation")
        return cls(cls._blur_matrix(H, size, float(sigma)), cls._blur_matrix(W, size, float(sigma)), f"blur {size} / {float(sigma):g}")

    @staticmethod
    def _scaled(H: int, W: int, scale: int) -> Tuple[int, int, int]:
        H, W, s = _size("H", H), _size("W", W), _size("scale", scale)
        if H % s != 0 or W % s != 0:
            raise ValueError(f"scale = {s} does not divide the image size {H} x {W}")
        return H, W, s

    @classmethod
    def bicubic(cls, H: int, W: int, scale: int) -> "SeparableOperator":
        """antialiased bicubic down-sampling by `scale` (ILVR's resize matrix: torch's interpolate(mode="bicubic", antialias=True))"""
        H, W, s = cls._scaled(H, W, scale)
        return cls(resize_matrix(H, H // s), resize_matrix(W, W // s), f"bicubic / {s}")

    @classmethod
    def average(cls, H: int, W: int, scale: int) -> "SeparableOperator":
        """the mean over scale x scale blocks"""
        H, W, s = cls._scaled(H, W, scale)
        pool = lambda n: np.kron(np.eye(n // s), np.full((1, s), 1.0 / s))
        return cls(pool(H), pool(W), f"average / {s}")

    @classmethod
    def preset(cls, name: str, H: int, W: int, *, blur_size: int = 9, blur_sigma: float = 2.0, scale: int = 4) -> "SeparableOperator":
        if name == "identity":
            return cls.identity(H, W)
        if name == "blur":
            return cls.gaussian_blur(H, W, blur_size, blur_sigma)
        if name == "bicubic":
            return cls.bicubic(H, W, scale)
        if name == "average":
            return cls.average(H, W, scale)
        raise ValueError(f"operator = {name!r}; use one of {OPERATORS}")


def dps_rows(alpha_bar, grid: Sequence[int], zeta: float = 1.0) -> Tuple[np.ndarray, List[int]]:
    """(float64 rows [n + 1][8], t_table [n + 1]) of the straight walk n -> 0: row i = {c0, c1, c2, A_t, B_t, zeta, 0, 0} of the transition
    a = i -> b = i - 1 with alpha = abar_a / abar_b: c0 = 1/sqrt(alpha), c1 = (1 - alpha)/sqrt(1 - abar_a), c2 = sqrt(1 - alpha) (0 in the
    last row, b = 0), A_t = 1/sqrt(abar_a), B_t = sqrt(1 - abar_a)/sqrt(abar_a); t_table[i] = tau_i.  Row 0 is never stepped from."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    n = len(grid) - 1
    rows = np.zeros((n + 1, ROW), dtype=np.float64)
    rows[0, :6] = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    for a in range(1, n + 1):
        b = a - 1
        ab_a, ab_b = ab[grid[a]], ab[grid[b]]
        alpha = ab_a / ab_b
        beta = 1.0 - alpha
        rows[a, :6] = (1.0 / np.sqrt(alpha), beta / np.sqrt(1.0 - ab_a), np.sqrt(beta) if b > 0 else 0.0, 1.0 / np.sqrt(ab_a), np.sqrt(1.0 - ab_a) / np.sqrt(ab_a),
                       float(zeta))
    return rows, [int(t) for t in grid]


class PosteriorChainRunner(KeepForwardRunner):
    """ChainRunner whose captured step is dmme_dps_chain_step: the keep form of the forward, the adjoint kernel, the input-only backward
    and the update.  Tables of 8 floats per index; the measurement and its mask in fixed buffers (read only: a chain fills them once), the
    device copies of the operator's matrices, and the step's own buffers g, d_out, dx, sumsq; one normal stream per step."""

    _side = ("y", "mask")

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        B, Cc, H, W = x.shape
        op = process._operator_for(H, W)
        self.h, self.w = op.h, op.w
        self.Kh, self.Kw = op.device(x.device)
        self.y = torch.zeros((B, Cc, op.h, op.w), dtype=torch.float32, device=x.device)
        self.mask = torch.zeros_like(self.y)
        self.g, self.dx = torch.zeros_like(x), torch.zeros_like(x)
        self.d_out = torch.zeros_like(self.out)
        self.sumsq = torch.zeros((B, Cc), dtype=torch.float32, device=x.device)

    def _call(self, packed):
        p = self.plan
        _lib.check(
            _lib.lib().dmme_dps_chain_step(p.h, _lib.ptr(packed), _lib.ptr(p.packed_bwd), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(p.workspace), _lib.ptr(p.bws),
                                           _lib.ptr(self.y), _lib.ptr(self.mask), _lib.ptr(self.Kh), _lib.ptr(self.Kw), self.h, self.w, _lib.ptr(self.g),
                                           _lib.ptr(self.d_out), _lib.ptr(self.dx), _lib.ptr(self.sumsq), _lib.ptr(self.coef), _lib.ptr(self.ttab),
                                           _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_dps_chain_step",
        )

    def restore(self, x: Tensor, y: Tensor, mask: Tensor, first: int, recorder=None) -> Tensor:
        return self.run_copies(x, (y, mask), first, recorder)


class DPS(GridProcess):
    r"""DPS over any unconditional noise-prediction network of the package (an IDDPM network's learned variance is not used: the reverse
    step's variance is 1 - alpha).

    `sub_timesteps`: levels of the grid (the paper walks every timestep); `operator`: a `SeparableOperator` for the image size restored
    (None: the identity, plain denoising / inpainting); `zeta`: the step size of the gradient step on ||y - A x0|| (0: the strided
    DDPM chain); `sigma_y`: the standard deviation of the Gaussian noise `degrade` adds to a measurement.  `alpha_bar`: a (T+1) table in
    place of the linear schedule's (`from_process` takes it from a DDPM / IDDPM instance).  Not built: x0 / v networks and x0
    thresholding (the derivative of the adapter and of the clip), conditional plans."""

    _chain_kind = _lib.CHAIN_DPS
    _runner_class = PosteriorChainRunner
    _whole_chains = "DPS runs whole chains: restore / generate"

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 1000, operator: Optional[SeparableOperator] = None, zeta: float = 1.0,
                 sigma_y: float = 0.0, start: float = 0.0001, end: float = 0.02, alpha_bar: Optional[Tensor] = None, *, prediction: str = "eps",
                 loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        if self.prediction != "eps":
            raise NotImplementedError(f"DPS: prediction = {prediction!r}; the derivative of the x0 / v adapter is not built: an eps network only")
        if self.threshold != "none":
            raise NotImplementedError(f"DPS: threshold = {threshold!r}; the derivative of the clip is not built: threshold \"none\" only")
        for name, v in (("zeta", zeta), ("sigma_y", sigma_y)):
            if isinstance(v, bool) or not float(v) >= 0.0 or not np.isfinite(float(v)):
                raise ValueError(f"{name} = {v!r}; a finite number of at least 0")
        if operator is not None and not isinstance(operator, SeparableOperator):
            raise ValueError(f"operator = {operator!r}; a SeparableOperator (or None: the identity)")
        self._set_grid(sub_timesteps, alpha_bar)
        self.operator, self.zeta, self.sigma_y = operator, float(zeta), float(sigma_y)
        self._tables = fp32_tables(*dps_rows(self._ab64, self._tau_host, self.zeta))
        self.n_rows = self._tables[0]
        self._identities = {}

    def set_threshold(self, mode: str, percentile: Optional[float] = None):
        if mode != "none":
            raise NotImplementedError(f"DPS: threshold = {mode!r}; the derivative of the clip is not built: threshold \"none\" only")
        return super().set_threshold(mode, percentile)

    # ------------------------------------------------------------------ the operator
    def _operator_for(self, H: int, W: int) -> SeparableOperator:
        """the process's operator, checked against the image size (None: the identity of that size, built once)"""
        op = self.operator
        if op is None:
            key = (int(H), int(W))
            if key not in self._identities:
                self._identities[key] = SeparableOperator.identity(*key)
            return self._identities[key]
        if (op.H, op.W) != (int(H), int(W)):
            raise ValueError(f"DPS: {op!r} does not act on images of {H} x {W}")
        return op

    _mask = staticmethod(check_mask)  # (B|1, C|1, h, w) with values 0 or 1 -> contiguous fp32 of the measurement's shape

    @torch.no_grad()
    def degrade(self, x: Tensor, mask=None, noise: bool = True) -> Tensor:
        """A x on the device (dmme_dps_measure), plus sigma_y N(0, I) on the measured cells where `noise`: the measurement (B, C, h, w)
        of an image batch; unmeasured cells are exactly 0"""
        src = self._image(x, "degrade")
        B, Cc, H, W = src.shape
        op = self._operator_for(H, W)
        shape = op.measurement_shape(src.shape)
        m = None if mask is None else self._mask(mask, shape, src.device, 1.0)
        Kh, Kw = op.device(src.device)
        y = torch.empty(shape, dtype=torch.float32, device=src.device)
        _lib.check(_lib.lib().dmme_dps_measure(_lib.ptr(src), _lib.ptr(Kh), _lib.ptr(Kw), _lib.ptr(m), _lib.ptr(y), B, Cc, H, W, op.h, op.w, _lib.stream_ptr()),
                   "dmme_dps_measure")
        if noise and self.sigma_y > 0.0:
            z = gaussian_like(y) * self.sigma_y
            y += z if m is None else z * m
        return y

    # ------------------------------------------------------------------ chains
    def _eager_chain(self, x: Tensor, y: Tensor, mask: Tensor, history=None) -> Tensor:
        """the host loop over the eager entry points (keep-forward, dmme_dps_adjoint, input-only backward, dmme_dps_step; `eager_chain`),
        in place on x"""
        model = self.model
        if not hasattr(model, "_forward_impl") or model.training:
            raise _lib.DmmeError("DPS differentiates the denoiser on the device: a dmme_amd UNet in eval mode")
        lib = _lib.lib()
        B, Cc, H, W = x.shape
        op = self._operator_for(H, W)
        Kh, Kw = op.device(x.device)
        g, sumsq = torch.empty_like(x), torch.empty((B, Cc), dtype=torch.float32, device=x.device)

        def call(row, t, z):
            eps, saved = model._forward_impl(x, t, want_ctx=True)
            planes = eps[0].numel() // x[0].numel()
            d_out = torch.empty_like(eps)
            _lib.check(lib.dmme_dps_adjoint(_lib.ptr(x), _lib.ptr(eps), planes, _row_arg(row), _lib.ptr(y), _lib.ptr(mask), _lib.ptr(Kh), _lib.ptr(Kw), _lib.ptr(g),
                                            _lib.ptr(d_out), _lib.ptr(sumsq), B, Cc, H, W, op.h, op.w, _lib.stream_ptr()), "dmme_dps_adjoint")
            dx = model._backward_input_impl(saved, d_out)
            _lib.check(lib.dmme_dps_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(g), _lib.ptr(dx), _lib.ptr(sumsq), _lib.ptr(z), _row_arg(row), B, Cc, H, W, planes,
                                         _lib.stream_ptr()), "dmme_dps_step")

        return eager_chain(x, _lib.CHAIN_DPS, self._tables, self._tables[0], STREAMS, call, history)

    def _chain(self, x: Tensor, y: Tensor, mask: Tensor, history=None) -> Tensor:
        runner = self._buffered_runner("_runner", x.shape, x.device)
        if runner is None:
            return self._eager_chain(x, y, mask, history)
        return runner.restore(x, y, mask, self._tables[0], history)

    def _measured(self, y: Tensor, what: str) -> Tuple[Tensor, SeparableOperator, Tuple[int, int, int, int]]:
        meas = self._image(y, what)
        B, Cc, h, w = meas.shape
        op = self.operator
        if op is None:
            op = self._operator_for(h, w)
        if (op.h, op.w) != (h, w):
            raise ValueError(f"{what}: a measurement of shape {tuple(meas.shape)} does not come from {op!r}")
        return meas, op, (B, Cc, op.H, op.W)

    @torch.no_grad()
    def restore(self, y: Tensor, mask=None, history=None) -> Tensor:
        r"""images (B, C, H, W) whose degradation explains the measurement `y` (B, C, h, w) where `mask` (B|1, C|1, h, w; None: everywhere)
        is 1, and that the network finds plausible: x_T ~ N(0, I), then the whole walk through the captured step.  `history`: a
        HistoryRecorder for the walk's frames (`n_rows` steps)."""
        meas, op, shape = self._measured(y, "restore")
        m = self._mask(mask, tuple(meas.shape), meas.device, 1.0)
        return self._chain(gaussian(shape, device=meas.device), meas, m, history)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """`restore` with nothing measured (an all-zero mask): the unconditioned strided DDPM walk from pure noise"""
        B, Cc, H, W = (int(v) for v in img_size)
        shape = self._operator_for(H, W).measurement_shape((B, Cc, H, W))
        zeros = torch.zeros(shape, dtype=torch.float32, device=self.beta.device)
        return self._chain(gaussian((B, Cc, H, W), device=zeros.device), zeros, zeros, history)
