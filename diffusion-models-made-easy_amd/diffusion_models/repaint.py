"""RePaint inpainting (Lugmayr et al. 2022) and SDEdit image editing (Meng et al. 2022) over any unconditionally trained noise predictor
of the package, as device-resident chains.

Grid 0 = tau_0 < tau_1 < ... < tau_n = T (`solver_grid(alpha_bar, sub_timesteps, "linear")`); a level k is a sample at noise level
tau_k, level 0 a clean image.  RePaint walks the levels n -> 0, jumping back up `jump_length` levels `resamples - 1` times from every
`jump_length`-th level (`repaint_levels`).  Every downward transition a -> b = a - 1 is one network evaluation and one table row:

    u  = c0 (x - c1 eps) [+ c2 z0]        the reverse step of the pixels to generate      (DDPM's, sigma_t^2 = beta_t)
    k  = ka x0 [+ ks z1]                  the known pixels noised to level b
    y  = m k + (1 - m) u                  m: 1 = known pixel, 0 = generate
    x' = y, or r0 y + r1 z2               the walk's next upward run b -> c, folded

The fold: the upward transitions that follow a downward one use no network, and forward noising composes, so the run b -> c is ONE
Gaussian q(x_c | x_b) = N(sqrt(abar_c / abar_b) x_b, (1 - abar_c / abar_b) I) with one normal per element.  It has the distribution of
the `jump_length` single sqrt(1 - beta) x + sqrt(beta) z steps of the paper's Algorithm 1, not their draws.  So every replay of the
captured step is one forward pass plus one update, and no step runs a network pass whose result is thrown away.

The host computes the rows in float64 and rounds them to fp32 (include/dmme_hip.h: dmme_repaint_step); the walk is a table of timesteps
that goes up and down, which the replayed step's `t = t_table[i]` never minded.  SDEdit is the plain walk k -> 0 from a noised guide."""

from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like
from .chain import ROW_DRAWS, ChainRunner, eager_chain
from .conditioned import GridProcess, check_mask, fp32_tables
from .dpm_solver import _row_arg

ROW = 8  # floats per table row: c0, c1, c2, ka, ks, r0, r1, -
STREAMS = 3  # normal streams a step owns: z0 (reverse step), z1 (known pixels), z2 (jump)
ROW_DRAWS[_lib.CHAIN_REPAINT] = lambda row: row[2] != 0.0 or row[4] != 0.0 or row[6] != 0.0  # (a stream whose coefficient is zero is not read)


def repaint_levels(n: int, jump_length: int = 10, resamples: int = 10) -> List[int]:
    """the level walk n, n - 1, ..., 0 with its jumps back up: from each level l = 1, 1 + j, 1 + 2j, ... whose jump stays inside the grid
    (l + j <= n) the walk climbs j levels, resamples - 1 times.  j = 1 is the paper's Algorithm 1 (every step t >= 2 taken U = resamples
    times); n = 250, j = r = 10 the published schedule in 1-based levels.  n + (r - 1) j floor((n - 1) / j) downward transitions."""
    n, j, r = int(n), int(jump_length), int(resamples)
    if n < 1 or j < 1 or r < 1:
        raise ValueError(f"repaint_levels: n = {n}, jump_length = {j}, resamples = {r} must all be at least 1")
    left = {l: r - 1 for l in range(1, n - j + 1, j)}
    k, walk = n, [n]
    while k >= 1:
        k -= 1
        walk.append(k)
        if left.get(k, 0) > 0:
            left[k] -= 1
            for _ in range(j):
                k += 1
                walk.append(k)
    return walk


def repaint_rows(alpha_bar, grid: Sequence[int], walk: Sequence[int], reverse=None) -> Tuple[np.ndarray, List[int]]:
    """(float64 rows [n_rows + 1][8], t_table [n_rows + 1]) of a level walk: one row {c0, c1, c2, ka, ks, r0, r1, 0} per downward
    transition a -> b with the upward run b -> c behind it folded in; the k-th transition sits at loop index n_rows - k, t_table there is
    tau_a.  Row 0 is never stepped from.  `reverse`: per-timestep (1/sqrt(alpha_t), beta_t/sqrt(1-abar_t), sqrt(beta_t)) of a process
    whose grid is every timestep, taken in place of the float64 values so that the reverse half carries DDPM's bits."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    walk = [int(v) for v in walk]
    steps, p, last = [], 0, len(walk) - 1
    while p < last:
        a, b = walk[p], walk[p + 1]
        if b != a - 1 or b < 0:
            raise ValueError(f"repaint_rows: the walk goes {a} -> {b} where a step down by one level was due")
        p += 1
        c = b
        while p < last and walk[p + 1] == walk[p] + 1:
            p, c = p + 1, c + 1
        steps.append((a, b, c))
    n_rows = len(steps)
    rows = np.zeros((n_rows + 1, ROW), dtype=np.float64)
    rows[0, :7] = (1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0)
    ttab = [0] * (n_rows + 1)
    for k, (a, b, c) in enumerate(steps):
        i = n_rows - k
        ab_a, ab_b, ab_c = ab[grid[a]], ab[grid[b]], ab[grid[c]]
        alpha = ab_a / ab_b
        beta = 1.0 - alpha
        if reverse is None:
            c0, c1, c2 = 1.0 / np.sqrt(alpha), beta / np.sqrt(1.0 - ab_a), np.sqrt(beta)
        else:
            c0, c1, c2 = (float(col[grid[a]]) for col in reverse)
        r0, r1 = (1.0, 0.0) if c == b else (np.sqrt(ab_c / ab_b), np.sqrt(1.0 - ab_c / ab_b))
        rows[i, :7] = (c0, c1, c2 if b > 0 else 0.0, np.sqrt(ab_b), np.sqrt(1.0 - ab_b), r0, r1)
        ttab[i] = int(grid[a])
    return rows, ttab


class PaintChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_repaint_chain_step: tables of 8 floats per index, the known image and its mask in fixed
    buffers beside x (read only: a chain fills them once), three normal streams per step"""

    _side = ("known", "mask")

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        self.known = torch.zeros_like(x)
        self.mask = torch.zeros_like(x)
        self.noise_numel = STREAMS * x.numel()

    def _call(self, packed):
        _lib.check(
            _lib.lib().dmme_repaint_chain_step(self.plan.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(self.plan.workspace),
                                               _lib.ptr(self.known), _lib.ptr(self.mask), _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state),
                                               _lib.stream_ptr()),
            "dmme_repaint_chain_step",
        )

    def paint(self, x: Tensor, known: Tensor, mask: Tensor, first: int, recorder=None) -> Tensor:
        return self.run_copies(x, (known, mask), first, recorder)


class RePaint(GridProcess):
    r"""RePaint / SDEdit over any unconditional noise-prediction network of the package (an IDDPM network's learned variance is not used:
    the reverse step's variance is beta), or an x0 / v network (`prediction=`).

    `sub_timesteps`: levels of the grid (`sub_timesteps = timesteps`: every timestep, and the reverse half is DDPM's update bit for bit);
    `jump_length`, `resamples`: the walk of `repaint_levels`.  `alpha_bar`: a (T+1) table in place of the linear schedule's
    (`from_process` takes it from a DDPM / IDDPM instance)."""

    _chain_kind = _lib.CHAIN_REPAINT
    _runner_class = PaintChainRunner
    _whole_chains = "RePaint runs whole chains: inpaint / edit / generate"
    _image_noun = "image batch"

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 250, jump_length: int = 10, resamples: int = 10, start: float = 0.0001,
                 end: float = 0.02, alpha_bar: Optional[Tensor] = None, *, prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold, threshold_percentile=threshold_percentile)
        for name, v in (("jump_length", jump_length), ("resamples", resamples)):
            if isinstance(v, bool) or int(v) != v or v < 1:
                raise ValueError(f"{name} = {v!r}; an integer of at least 1")
        self._set_grid(sub_timesteps, alpha_bar)
        self.jump_length, self.resamples = int(jump_length), int(resamples)
        self._walk = repaint_levels(self.n_levels, self.jump_length, self.resamples)
        self._tables = self._make_tables(self._walk)
        self._plain_tables = self._make_tables(list(range(self.n_levels, -1, -1)))  # SDEdit's: loop index = level
        self.n_rows = self._tables[0]

    def _make_tables(self, walk):
        full = self.n_levels == self.timesteps
        return fp32_tables(*repaint_rows(self._ab64, self._tau_host, walk, (self._c1, self._c2, self._sigma) if full else None))

    @staticmethod
    def _mask(mask: Optional[Tensor], like: Tensor) -> Tensor:
        """(B|1, C|1, H, W) with values in [0, 1] -> contiguous fp32 of `like`'s shape; None: nothing is known"""
        return check_mask(mask, tuple(like.shape), like.device, 0.0, binary=False)

    # ------------------------------------------------------------------ chains
    def _eager_chain(self, x: Tensor, known: Tensor, mask: Tensor, tables=None, first: Optional[int] = None, history=None) -> Tensor:
        """the host loop over dmme_repaint_step (`eager_chain`), in place on x"""
        tables = tables if tables is not None else self._tables

        def call(row, t, z):
            eps = self._eps(x, t).detach().to(torch.float32).contiguous()
            _lib.check(_lib.lib().dmme_repaint_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(known), _lib.ptr(mask), _lib.ptr(z), _row_arg(row), x.shape[0], x[0].numel(),
                                                    eps[0].numel() // x[0].numel(), _lib.stream_ptr()), "dmme_repaint_step")

        return eager_chain(x, _lib.CHAIN_REPAINT, tables, tables[0] if first is None else int(first), STREAMS, call, history)

    def _chain(self, slot: str, x: Tensor, known: Tensor, mask: Tensor, tables=None, first: Optional[int] = None, history=None) -> Tensor:
        first = (tables if tables is not None else self._tables)[0] if first is None else first
        runner = self._table_runner(slot, x.shape, x.device, tables)
        if runner is None:
            return self._eager_chain(x, known, mask, tables, first, history)
        return runner.paint(x, known, mask, first, history)

    @torch.no_grad()
    def inpaint(self, x0: Tensor, mask: Tensor, history=None) -> Tensor:
        r"""the image batch whose pixels equal `x0` where `mask` is 1 (bit for bit) and are generated, in harmony with them, where it is 0:
        x_T ~ N(0, I), then the whole RePaint walk through the captured step.  mask: (B|1, C|1, H, W), values in [0, 1].
        `history`: a HistoryRecorder for the walk's frames, keyed on the step ordinal (`n_rows` steps: the level is not monotone)."""
        known = self._image(x0, "inpaint")
        m = self._mask(mask, known)
        return self._chain("_runner", gaussian(known.shape, device=known.device), known, m, history=history)

    @torch.no_grad()
    def edit(self, x_guide: Tensor, strength: float, mask: Optional[Tensor] = None, history=None) -> Tensor:
        r"""SDEdit: the guide noised to level k = max(1, round(strength n)) and denoised by the plain walk k -> 0 (no resampling,
        whatever `resamples` is).  strength in (0, 1]: 1 forgets the guide, small values stay close to it.  With a mask the pixels where
        it is 1 are kept exactly (SDEdit's masked variant).  `history`: a HistoryRecorder for the frames of the `edit_level(strength)` steps."""
        strength = float(strength)
        if not 0.0 < strength <= 1.0:
            raise ValueError(f"strength = {strength!r} outside (0, 1]")
        guide = self._image(x_guide, "edit")
        m = self._mask(mask, guide)
        k = self.edit_level(strength)
        t = torch.full((guide.shape[0],), self._tau_host[k], dtype=torch.int64, device=guide.device)
        x_k = self._noised(guide, t, gaussian_like(guide), target=False)[2]
        return self._chain("_edit_runner", x_k, guide, m, self._plain_tables, k, history)

    def edit_level(self, strength: float) -> int:
        """the level SDEdit starts from"""
        return min(self.n_levels, max(1, int(round(float(strength) * self.n_levels))))

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """`inpaint` with nothing known: the walk from pure noise"""
        zeros = torch.zeros(tuple(img_size), dtype=torch.float32, device=self.beta.device)
        return self._chain("_runner", gaussian(img_size, device=zeros.device), zeros, zeros, history=history)
