"""ILVR (Choi et al. 2021, "Conditioning Method for Denoising Diffusion Probabilistic Models"): samples of an unconditional network that
share the coarse content of a reference image, as device-resident chains.

Grid 0 = tau_0 < tau_1 < ... < tau_n = T (`solver_grid(alpha_bar, sub_timesteps, "linear")`, RePaint's); the walk goes straight down,
n -> 0.  Every transition a -> b = a - 1 is one network evaluation and one table row; with y the clean reference:

    u  = c0 (x - c1 eps) [+ c2 z0]        DDPM's reverse step (sigma^2 = beta)
    k  = ka y [+ ks z1]                   the reference noised to level b
    x' = u + phi(k - u)                   while the step is conditioned (b >= range_level), else x' = u

phi = up o down is linear, so u + phi(k - u) is the paper's phi(y_b) + u - phi(u) with one filter application.  Both directions use the
bicubic kernel (a = -0.5), antialiased on the way down: torch.nn.functional.interpolate(mode="bicubic", antialias=True,
align_corners=False), which is PIL's convention.  Per axis of length n the filter is the dense n x n matrix
P(n, N) = R(n/N -> n) R(n -> n/N) (`lowpass_matrix`), built in float64 and rounded to fp32 once; phi(d) = Ph d Pw^T per channel plane is
the device's work (csrc/ilvr.hip, include/dmme_hip.h: dmme_ilvr_step).  P is not idempotent (|P P - P| reaches 0.01 - 0.06).

`down_factor` N trades fidelity to the reference (small N) against diversity (large N); `range_level` r stops the conditioning early:
transitions with b >= r are conditioned, r = 0 (the default) conditions every step, the last included."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian
from .chain import ROW_DRAWS, ChainRunner, eager_chain
from .conditioned import GridProcess, fp32_tables
from .dpm_solver import _row_arg

ROW = 8  # floats per table row: c0, c1, c2, ka, ks, g, -, -
STREAMS = 2  # normal streams a step owns: z0 (reverse step), z1 (the reference's noise)
ROW_DRAWS[_lib.CHAIN_ILVR] = lambda row: row[2] != 0.0 or row[5] != 0.0 and row[4] != 0.0  # (z0, or z1 of a conditioned row: a stream whose coefficient is zero is not read)


def _cubic(x: np.ndarray, a: float = -0.5) -> np.ndarray:
    x = np.abs(x)
    return np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))


def resize_matrix(n_in: int, n_out: int) -> np.ndarray:
    """float64 [n_out][n_in]: the antialiased bicubic resize of one axis (align_corners=False).  Output i sits at centre
    s (i + 1/2), s = n_in / n_out; its window has half-width 2 max(s, 1), is clipped to the axis, and the kernel is stretched by
    max(s, 1); the weights are renormalised, so every row sums to 1."""
    s = n_in / n_out
    support = 2.0 * s if s >= 1.0 else 2.0
    inv = 1.0 / s if s >= 1.0 else 1.0
    R = np.zeros((n_out, n_in), dtype=np.float64)
    for i in range(n_out):
        centre = s * (i + 0.5)
        lo = max(int(centre - support + 0.5), 0)
        hi = min(int(centre + support + 0.5), n_in)
        w = _cubic((np.arange(lo, hi, dtype=np.float64) - centre + 0.5) * inv)
        R[i, lo:hi] = w / w.sum()
    return R


def lowpass_matrix(n: int, N: int) -> np.ndarray:
    """float64 [n][n]: P(n, N) = R(n/N -> n) R(n -> n/N), the low-pass filter phi_N along one axis of length n"""
    if isinstance(n, bool) or isinstance(N, bool) or int(n) != n or int(N) != N or n < 1 or N < 2 or n % N != 0:
        raise ValueError(f"lowpass_matrix: the down-sampling factor N = {N!r} must be an integer of at least 2 that divides the axis length n = {n!r}")
    n, N = int(n), int(N)
    return resize_matrix(n // N, n) @ resize_matrix(n, n // N)


def ilvr_rows(alpha_bar, grid: Sequence[int], range_level: int = 0, reverse=None) -> Tuple[np.ndarray, List[int]]:
    """(float64 rows [n + 1][8], t_table [n + 1]) of the straight walk n -> 0: row i = {c0, c1, c2, ka, ks, g, 0, 0} of the transition
    a = i -> b = i - 1, t_table[i] = tau_i; g = 1 where b >= range_level.  Row 0 is never stepped from.  `reverse`: per-timestep
    (1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), sqrt(beta_t)) of a process whose grid is every timestep, taken in place of the float64
    values so that the reverse half carries DDPM's bits (as `repaint_rows`)."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    n, r = len(grid) - 1, int(range_level)
    rows = np.zeros((n + 1, ROW), dtype=np.float64)
    rows[0, :6] = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    for a in range(1, n + 1):
        b = a - 1
        ab_a, ab_b = ab[grid[a]], ab[grid[b]]
        alpha = ab_a / ab_b
        beta = 1.0 - alpha
        if reverse is None:
            c0, c1, c2 = 1.0 / np.sqrt(alpha), beta / np.sqrt(1.0 - ab_a), np.sqrt(beta)
        else:
            c0, c1, c2 = (float(col[grid[a]]) for col in reverse)
        rows[a, :6] = (c0, c1, c2 if b > 0 else 0.0, np.sqrt(ab_b), np.sqrt(1.0 - ab_b), 1.0 if b >= r else 0.0)
    return rows, [int(t) for t in grid]


class LikeChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_ilvr_chain_step: tables of 8 floats per index, the reference image in a fixed buffer beside
    x (read only: a chain fills it once), the device copies of the two filter matrices, the streaming form's scratch, two normal streams
    per step"""

    _side = ("ref",)

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        B, Cc, H, W = x.shape
        self.ref = torch.zeros_like(x)
        self.Ph, self.Pw = process._filters(H, W, x.device)
        self.scratch = process._scratch(B * Cc, H, W, x.device)
        self.noise_numel = STREAMS * x.numel()

    def _call(self, packed):
        _lib.check(
            _lib.lib().dmme_ilvr_chain_step(self.plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.plan.workspace), _lib.ptr(self.ref),
                                            _lib.ptr(self.Ph), _lib.ptr(self.Pw), _lib.ptr(self.scratch), _lib.ptr(self.coef), _lib.ptr(self.ttab),
                                            _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_ilvr_chain_step",
        )

    def like(self, x: Tensor, ref: Tensor, first: int, recorder=None) -> Tensor:
        return self.run_copies(x, (ref,), first, recorder)


class ILVR(GridProcess):
    r"""ILVR over any unconditional noise-prediction network of the package (an IDDPM network's learned variance is not used: the reverse
    step's variance is beta), or an x0 / v network (`prediction=`).

    `sub_timesteps`: levels of the grid (`sub_timesteps = timesteps`: every timestep, and the reverse half is DDPM's update bit for bit);
    `down_factor`: N of the low-pass filter, an integer of at least 2 that must divide the height and width of the images sampled;
    `range_level`: the level below which steps are no longer conditioned (0: every step is).  `alpha_bar`: a (T+1) table in place of the
    linear schedule's (`from_process` takes it from a DDPM / IDDPM instance)."""

    _chain_kind = _lib.CHAIN_ILVR
    _runner_class = LikeChainRunner
    _whole_chains = "ILVR runs whole chains: sample_like / generate"
    _image_noun = "image batch"

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 250, down_factor: int = 4, range_level: int = 0, start: float = 0.0001,
                 end: float = 0.02, alpha_bar: Optional[Tensor] = None, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        if isinstance(down_factor, bool) or int(down_factor) != down_factor or down_factor < 2:
            raise ValueError(f"down_factor = {down_factor!r}; an integer of at least 2")
        self._set_grid(sub_timesteps, alpha_bar)
        self.down_factor = int(down_factor)
        if isinstance(range_level, bool) or int(range_level) != range_level or not 0 <= range_level <= self.n_levels:
            raise ValueError(f"range_level = {range_level!r} outside 0..{self.n_levels} (the grid's levels)")
        self.range_level = int(range_level)
        self._tables = self._make_tables(self.range_level)
        self._free_tables = self._make_tables(self.n_levels + 1)  # `generate`: g = 0 in every row
        self._filter_cache = {}

    def _make_tables(self, range_level: int):
        full = self.n_levels == self.timesteps
        return fp32_tables(*ilvr_rows(self._ab64, self._tau_host, range_level, (self._c1, self._c2, self._sigma) if full else None))

    # ------------------------------------------------------------------ the filter
    def _filters(self, H: int, W: int, device) -> Tuple[Tensor, Tensor]:
        """the fp32 device copies of Ph = P(H, N) and Pw = P(W, N), built once per (H, W, device)"""
        N = self.down_factor
        if H % N != 0 or W % N != 0:
            raise ValueError(f"ILVR: the image size {H} x {W} is not divisible by down_factor = {N}")
        key = (int(H), int(W), torch.device(device))
        if key not in self._filter_cache:
            self._filter_cache[key] = tuple(torch.from_numpy(lowpass_matrix(n, N).astype(np.float32)).contiguous().to(device) for n in (H, W))
        return self._filter_cache[key]

    @staticmethod
    def _scratch(planes: int, H: int, W: int, device) -> Tensor:
        """the buffer the streaming form hands T from its first launch to its second (the fused form does not touch it)"""
        return torch.empty(int(_lib.lib().dmme_lowpass_scratch_bytes(planes, H, W)) // 4, dtype=torch.float32, device=device)

    @torch.no_grad()
    def low_pass(self, x: Tensor) -> Tensor:
        """phi_N(x) per channel plane, a new tensor: what the sampler keeps of the reference (dmme_lowpass)"""
        src = self._image(x, "low_pass")
        B, Cc, H, W = src.shape
        Ph, Pw = self._filters(H, W, src.device)
        dst = torch.empty_like(src)
        _lib.check(_lib.lib().dmme_lowpass(_lib.ptr(src), _lib.ptr(dst), B * Cc, H, W, _lib.ptr(Ph), _lib.ptr(Pw), _lib.ptr(self._scratch(B * Cc, H, W, src.device)), 0,
                                           _lib.stream_ptr()), "dmme_lowpass")
        return dst

    # ------------------------------------------------------------------ chains
    def _eager_chain(self, x: Tensor, ref: Tensor, tables=None, history=None) -> Tensor:
        """the host loop over dmme_ilvr_step (`eager_chain`), in place on x"""
        tables = tables if tables is not None else self._tables
        B, Cc, H, W = x.shape
        Ph, Pw = self._filters(H, W, x.device)
        scratch = self._scratch(B * Cc, H, W, x.device)

        def call(row, t, z):
            eps = self._eps(x, t).detach().to(torch.float32).contiguous()
            _lib.check(_lib.lib().dmme_ilvr_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(ref), _lib.ptr(z), _row_arg(row), _lib.ptr(Ph), _lib.ptr(Pw), _lib.ptr(scratch), B,
                                                 Cc, H, W, eps[0].numel() // x[0].numel(), 0, _lib.stream_ptr()), "dmme_ilvr_step")

        return eager_chain(x, _lib.CHAIN_ILVR, tables, tables[0], STREAMS, call, history)

    def _chain(self, slot: str, x: Tensor, ref: Tensor, tables=None, history=None) -> Tensor:
        self._filters(x.shape[2], x.shape[3], x.device)  # (the size check, before a runner or a draw)
        runner = self._table_runner(slot, x.shape, x.device, tables)
        if runner is None:
            return self._eager_chain(x, ref, tables, history)
        return runner.like(x, ref, (tables if tables is not None else self._tables)[0], history)

    @torch.no_grad()
    def sample_like(self, reference: Tensor, history=None) -> Tensor:
        r"""images that share the reference's low frequencies phi_N(reference): x_T ~ N(0, I), then the whole walk through the captured
        step; a new tensor of the reference's shape.  `history`: a HistoryRecorder for the walk's frames (`n_levels` steps)."""
        ref = self._image(reference, "sample_like")
        self._filters(ref.shape[2], ref.shape[3], ref.device)
        return self._chain("_runner", gaussian(ref.shape, device=ref.device), ref, history=history)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """the walk from pure noise with no step conditioned (g = 0 in every row): the strided DDPM chain over the same grid"""
        zeros = torch.zeros(tuple(img_size), dtype=torch.float32, device=self.beta.device)
        self._filters(zeros.shape[2], zeros.shape[3], zeros.device)
        return self._chain("_free_runner", gaussian(img_size, device=zeros.device), zeros, self._free_tables, history)
