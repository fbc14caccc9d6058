"""The probability-flow ODE of a trained DDPM (Song et al., ICLR 2021, section 4.3 and appendix D.2): a second-order (Heun) sampler, the
latent encoding x_0 -> x_T, and the log-likelihood of an image, as device-resident chains over any unconditional eps network of the package.

With sig(t) = sqrt((1 - abar_t) / abar_t) and xbar = x / sqrt(abar) the ODE is d xbar / d sig = eps(x, t); along a solution
d log pbar / d sig = -sqrt(abar) tr(d eps / d x).  The network takes integer timesteps only, so the nodes are integers
g_0 = t_min < g_1 < ... < g_n = T: t_min and what `solver_grid(abar, nodes, schedule)` has above it.  A Heun step from node a to node b, in
either direction, has k0 = sqrt(abar_b / abar_a), k1 = sqrt(1 - abar_b) - k0 sqrt(1 - abar_a), h = sig(b) - sig(a) and two stages:

    A (at x_a, t = a):   e_a = eps(x_a, a);   x' = k0 x_a + k1 e_a                      the paper-form DDIM step, eta = 0
    B (at x', t = b):    e_b = eps(x', b);    x_b = k0 x_a + (k1 / 2)(e_a + e_b)

Every stage is one table row {c0, c1, c2, c3, w, save, 0, 0} of the update x_new = c0 x + c1 xs + c2 e + c3 es (xs <- x, es <- e where
save), folded in float64 and rounded once (include/dmme_hip.h: dmme_pf_stage).  With the likelihood on, a stage draws a Rademacher
probe z, takes J^T z from the network's input-only backward and adds w sum(z J^T z) to a per-image double on the device:
w_A = (h / 2) sqrt(abar_a), w_B = (h / 2) sqrt(abar_b).  Walking up from x_{g_0} := x_0 (the data is taken as the state at t_min: sig(1) =
0.01 on the linear schedule, where Song et al. start at 1e-5),

    log p(x_0) = log N(x_T; 0, I) + (D / 2)(ln abar_{g_n} - ln abar_{g_0}) + acc
    bits/dim   = -log p / (D ln 2) + log2(255 / 2)           (the data module's norm puts pixels 2 / 255 apart)

A sampling stage costs one no-grad forward, a likelihood stage one keep-forward plus one input-backward.  One probe per image and stage:
tile the batch to average probes."""

from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, philox_reserve
from .chain import ChainRunner, KeepForwardRunner, walk
from .conditioned import WholeChainProcess, fp32_tables
from .dpm_solver import TAU_SCHEDULES, _row_arg, solver_grid

ROW = 8  # floats per table row: c0, c1, c2, c3, w, save, -, -
DIRECTIONS = ("encode", "decode")


class LogLikelihood(NamedTuple):
    log_p: Tensor       # float64 [B]: log p(x_0) in nats
    prior: Tensor       # float64 [B]: log N(x_T; 0, I)
    divergence: Tensor  # float64 [B]: the accumulated trace term
    latent: Tensor      # fp32 (B, C, H, W): x_T


def pf_grid(alpha_bar, nodes: int, schedule: str = "linear", t_min: int = 1) -> List[int]:
    """g_0 = t_min < g_1 < ... < g_n = T: t_min and the timesteps of `solver_grid(alpha_bar, nodes, schedule)` above it"""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    T = ab.size - 1
    if isinstance(t_min, bool) or int(t_min) != t_min or not 1 <= t_min < T:
        raise ValueError(f"t_min = {t_min!r} outside 1..{T - 1}")
    if isinstance(nodes, bool) or int(nodes) != nodes or not 1 <= nodes <= T:
        raise ValueError(f"nodes = {nodes!r} outside 1..{T}")
    return [int(t_min)] + [t for t in solver_grid(ab, int(nodes), schedule)[1:] if t > t_min]


def _check_grid(grid: Sequence[int], T: int) -> List[int]:
    g = [int(t) for t in grid]
    if len(g) < 2 or g[0] < 1 or g[-1] > T or any(b <= a for a, b in zip(g, g[1:])) or any(int(t) != t for t in grid):
        raise ValueError(f"grid = {list(grid)!r}; at least two strictly increasing integer timesteps in 1..{T}")
    return g


def heun_scalars(alpha_bar, a: int, b: int) -> Tuple[float, float, float]:
    """(k0, k1, h) of the step from node a to node b, in float64"""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    sig = lambda t: np.sqrt((1.0 - ab[t]) / ab[t])
    k0 = np.sqrt(ab[b] / ab[a])
    return float(k0), float(np.sqrt(1.0 - ab[b]) - k0 * np.sqrt(1.0 - ab[a])), float(sig(b) - sig(a))


def pf_rows(alpha_bar, grid: Sequence[int], direction: str = "decode", likelihood: bool = False, final_denoise: bool = True) -> Tuple[np.ndarray, List[int]]:
    """(float64 rows [n + 1][8], t_table [n + 1]) of a walk over `grid`, one STAGE per loop index; the index runs down, so stage k of the
    walk sits at index n - k and row 0 is never stepped from.  "encode": g_0 -> g_n; "decode": g_n -> g_0, closed by one Euler stage
    g_0 -> 0 where `final_denoise`.  Stage A: (k0, 0, k1, 0, w_A, 1) at t = a; stage B: (0, k0, k1/2, k1/2, w_B, 0) at t = b;
    w = (h/2) sqrt(abar) of the stage's node where `likelihood`, else 0."""
    if direction not in DIRECTIONS:
        raise ValueError(f"direction = {direction!r}; use one of {DIRECTIONS}")
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    g = _check_grid(grid, ab.size - 1)
    m = len(g) - 1
    pairs = [(g[j], g[j + 1]) for j in range(m)] if direction == "encode" else [(g[m - j], g[m - j - 1]) for j in range(m)]
    stages, ts = [], []
    for a, b in pairs:
        k0, k1, h = heun_scalars(ab, a, b)
        wa, wb = ((0.5 * h) * np.sqrt(ab[a]), (0.5 * h) * np.sqrt(ab[b])) if likelihood else (0.0, 0.0)
        stages += [(k0, 0.0, k1, 0.0, wa, 1.0, 0.0, 0.0), (0.0, k0, 0.5 * k1, 0.5 * k1, wb, 0.0, 0.0, 0.0)]
        ts += [a, b]
    last = pairs[-1][1]
    if direction == "decode" and final_denoise:
        stages.append((1.0 / np.sqrt(ab[last]), 0.0, -np.sqrt(1.0 - ab[last]) / np.sqrt(ab[last]), 0.0, 0.0, 0.0, 0.0, 0.0))
        ts.append(last)
    n = len(stages)
    rows = np.zeros((n + 1, ROW), dtype=np.float64)
    rows[0, 0] = 1.0
    ttab = [last] * (n + 1)
    for k, (row, t) in enumerate(zip(stages, ts)):
        rows[n - k], ttab[n - k] = row, int(t)
    return rows, ttab


class FlowChainRunner(ChainRunner):
    """ChainRunner whose captured step is dmme_pf_chain_step: the no-grad forward and one Heun stage.  Tables of 8 floats per index; `xs`
    and `es`, the state and the prediction at a step's first node, are fixed buffers that travel with x and the loop state."""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        self.xs, self.es = torch.zeros_like(x), torch.zeros_like(x)

    def _carried(self):
        return [self.x, self.state, self.xs, self.es]

    def _call(self, packed):
        p = self.plan
        _lib.check(
            _lib.lib().dmme_pf_chain_step(p.h, _lib.ptr(packed), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(p.workspace), _lib.ptr(self.xs), _lib.ptr(self.es),
                                          _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_pf_chain_step",
        )


class LikelihoodChainRunner(KeepForwardRunner, FlowChainRunner):
    """ChainRunner whose captured step is dmme_pf_ll_chain_step: the keep form of the forward, the Rademacher probe written as d_out, the
    input-only backward, the probe dot into `acc` (a double per image, carried from stage to stage) and the Heun stage; one probe
    stream per stage.  `s` holds the last stage's per-image z^T J z, `dx` its J^T z."""

    def __init__(self, process, x: Tensor, use_graph: bool = True, spec=None):
        super().__init__(process, x, use_graph, spec)
        B = x.shape[0]
        self.d_out, self.dx = torch.zeros_like(self.out), torch.zeros_like(x)
        self.scratch = torch.zeros(int(_lib.lib().dmme_pf_scratch_floats(B, x[0].numel())), dtype=torch.float32, device=x.device)
        self.s = torch.zeros(B, dtype=torch.float32, device=x.device)
        self.acc = torch.zeros(B, dtype=torch.float64, device=x.device)

    def _carried(self):
        return super()._carried() + [self.acc]

    def _call(self, packed):
        p = self.plan
        _lib.check(
            _lib.lib().dmme_pf_ll_chain_step(p.h, _lib.ptr(packed), _lib.ptr(p.packed_bwd), _lib.ptr(self.x), _lib.ptr(self.out), _lib.ptr(p.workspace), _lib.ptr(p.bws),
                                             _lib.ptr(self.xs), _lib.ptr(self.es), _lib.ptr(self.d_out), _lib.ptr(self.dx), _lib.ptr(self.scratch), _lib.ptr(self.s),
                                             _lib.ptr(self.acc), _lib.ptr(self.coef), _lib.ptr(self.ttab), _lib.ptr(self.state), _lib.stream_ptr()),
            "dmme_pf_ll_chain_step",
        )


class ProbabilityFlow(WholeChainProcess):
    r"""The probability-flow ODE over any noise-prediction network of the package (an IDDPM network's learned variance is not used).

    `nodes`, `schedule` ("linear", "quadratic", "logsnr") and `t_min` give the integer grid (`pf_grid`); `grid=` gives it outright.
    `alpha_bar`: a (T+1) table in place of the linear schedule's (`from_process` takes it from a DDPM / IDDPM instance).
    `decode` / `generate` are the Heun sampler and work for x0 / v networks and with x0 thresholding like every sampler; `encode` and
    `log_likelihood` need an unconditional eps network in eval mode, no thresholding (the derivative of the adapter and of the clip is not
    built) and a precision with a backward (not fp16r32).  Classifier-free guidance is not built."""

    _chain_kind = _lib.CHAIN_PFODE
    _runner_class = FlowChainRunner
    _whole_chains = "ProbabilityFlow runs whole walks: decode / generate / encode / log_likelihood"

    def __init__(self, model: nn.Module, timesteps: int = 1000, nodes: int = 50, schedule: str = "linear", t_min: int = 1, start: float = 0.0001,
                 end: float = 0.02, alpha_bar: Optional[Tensor] = None, grid: Optional[Sequence[int]] = None, *, prediction: str = "eps",
                 loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, start, end, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold,
                         threshold_percentile=threshold_percentile)
        kind = str(schedule).lower()
        if kind not in TAU_SCHEDULES:
            raise ValueError(f"schedule = {schedule!r}; use one of {TAU_SCHEDULES}")
        if alpha_bar is not None:
            self._use_alpha_bar(alpha_bar)
        ab64 = self.alpha_bar.reshape(-1).to(torch.float64).cpu().numpy()
        g = _check_grid(grid, timesteps) if grid is not None else pf_grid(ab64, nodes, kind, t_min)
        if len(g) < 2:
            raise ValueError(f"nodes = {nodes!r}, t_min = {t_min!r}: the grid {g} has no step")
        self.nodes, self.schedule, self.t_min = len(g), kind, g[0]
        self.register_buffer("tau", torch.tensor(g, dtype=torch.int64), persistent=False)
        self._grid, self._ab64 = g, ab64
        self._tables = {
            "decode": fp32_tables(*pf_rows(ab64, g, "decode")),
            "decode_raw": fp32_tables(*pf_rows(ab64, g, "decode", final_denoise=False)),
            "encode": fp32_tables(*pf_rows(ab64, g, "encode")),
            "likelihood": fp32_tables(*pf_rows(ab64, g, "encode", likelihood=True)),
        }
        # log p(x_0) - log N(x_T) - acc, per dimension pair: (1/2)(ln abar_{g_n} - ln abar_{g_0})
        self._log_scale = 0.5 * (math.log(ab64[g[-1]]) - math.log(ab64[g[0]]))

    def _chain_tables(self):
        n, rows, ttab = self._tables["decode"]
        return n, list(rows), list(ttab)

    # ------------------------------------------------------------------ what the derivative-taking walks refuse, before anything is launched
    def _require_plain_eps(self, what: str) -> None:
        if self.prediction != "eps":
            raise NotImplementedError(f"ProbabilityFlow.{what}: prediction = {self.prediction!r}; the derivative of the x0 / v adapter is not built: an eps network only")
        if self.threshold != "none":
            raise NotImplementedError(f"ProbabilityFlow.{what}: threshold = {self.threshold!r}; the derivative of the clip is not built: threshold \"none\" only")
        model = self.model
        if getattr(model, "num_classes", None) is not None and hasattr(model, "label_embedding") or type(model).__name__ == "ConditionalUNet":
            raise NotImplementedError(f"ProbabilityFlow.{what}: a class-conditional network; conditional likelihood is not built")
        if not hasattr(model, "_forward_impl"):
            raise _lib.DmmeError(f"ProbabilityFlow.{what} differentiates the denoiser on the device: a dmme_amd UNet")
        if model.training:
            raise RuntimeError(f"ProbabilityFlow.{what}: the network is in train mode; the ODE needs a deterministic denoiser (call .eval())")
        if getattr(model, "_dtype", None) == _lib.F16R32:
            raise NotImplementedError(f"ProbabilityFlow.{what}: precision fp16r32 is an inference mode without a backward; use fp32, bf16, fp16 or bf16x3")

    # ------------------------------------------------------------------ runners: one per table, each on a buffer of its own
    def _flow_runner(self, name: str, shape, device, cls=FlowChainRunner) -> Optional[ChainRunner]:
        n, rows, ttab = self._tables[name]
        return self._buffered_runner(f"_pf_runner_{name}", shape, device, spec=lambda: (_lib.CHAIN_PFODE, (n, list(rows), list(ttab))), buf=f"_pf_buf_{name}", cls=cls)

    # ------------------------------------------------------------------ the eager host loops over the eager entry points
    def _eager_walk(self, x: Tensor, name: str, history=None, threshold: bool = True) -> Tensor:
        """the no-grad walk of table `name`, in place on x: `_eps` (the network, the x0 / v adapter, thresholding) and dmme_pf_stage"""
        n, rows, ttab = self._tables[name]
        lib = _lib.lib()
        B, chw = x.shape[0], x[0].numel()
        tt = torch.tensor(ttab, dtype=torch.int64, device=x.device).unsqueeze(1)
        xs, es = torch.zeros_like(x), torch.zeros_like(x)

        def step(k, i):
            eps = self._eps(x, tt[i], _threshold=threshold).contiguous()
            planes = eps[0].numel() // chw
            _lib.check(lib.dmme_pf_stage(_lib.ptr(x), _lib.ptr(eps), planes, _lib.ptr(xs), _lib.ptr(es), _row_arg(rows[i]), B, chw, _lib.stream_ptr()), "dmme_pf_stage")

        return walk(x, n, n, step, history)

    def _eager_likelihood(self, x: Tensor) -> Tuple[Tensor, Tensor]:
        """the likelihood walk on the host, in place on x: keep-forward, dmme_pf_probe, input-only backward, dmme_pf_dot, dmme_pf_stage,
        the probes from the (seed, offset) the captured chain's state walks through; (x_T, acc)"""
        n, rows, ttab = self._tables["likelihood"]
        model, lib = self.model, _lib.lib()
        B, chw, numel = x.shape[0], x[0].numel(), x.numel()
        quads = (numel + 3) // 4
        tt = torch.tensor(ttab, dtype=torch.int64, device=x.device).unsqueeze(1)
        xs, es = torch.zeros_like(x), torch.zeros_like(x)
        scratch = torch.zeros(int(lib.dmme_pf_scratch_floats(B, chw)), dtype=torch.float32, device=x.device)
        s = torch.zeros(B, dtype=torch.float32, device=x.device)
        acc = torch.zeros(B, dtype=torch.float64, device=x.device)
        span = []

        def step(k, i):
            eps, saved = model._forward_impl(x, tt[i], want_ctx=True)
            planes = eps[0].numel() // chw
            d_out = torch.empty_like(eps)
            _lib.check(lib.dmme_pf_probe(_lib.ptr(d_out), B, chw, planes, span[0], span[1] + k * quads, _lib.stream_ptr()), "dmme_pf_probe")
            dx = model._backward_input_impl(saved, d_out)
            _lib.check(lib.dmme_pf_dot(_lib.ptr(d_out), planes, _lib.ptr(dx), _row_arg(rows[i]), B, chw, _lib.ptr(scratch), _lib.ptr(s), _lib.ptr(acc),
                                       _lib.stream_ptr()), "dmme_pf_dot")
            _lib.check(lib.dmme_pf_stage(_lib.ptr(x), _lib.ptr(eps), planes, _lib.ptr(xs), _lib.ptr(es), _row_arg(rows[i]), B, chw, _lib.stream_ptr()), "dmme_pf_stage")

        walk(x, n, n, step, None, lambda: span.extend(philox_reserve(x.device, 4 * quads * n)))
        return x, acc

    # ------------------------------------------------------------------ the public walks
    @torch.no_grad()
    def decode(self, x_T: Tensor, history=None, final_denoise: bool = True) -> Tensor:
        """x_0 from the latent x_T: the Heun walk g_n -> g_0, closed by one Euler stage g_0 -> 0 (`final_denoise=False`: the state at
        t_min).  Deterministic: nothing is drawn.  `history`: a HistoryRecorder for the walk's frames (one per stage)."""
        name = "decode" if final_denoise else "decode_raw"
        x = self._image(x_T, "decode", copy=True)
        runner = self._flow_runner(name, x.shape, x.device)
        if runner is None:
            return self._eager_walk(x, name, history)
        return runner.run_copies(x, (), self._tables[name][0], history)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """`decode` from pure noise: the second-order deterministic sampler"""
        return self.decode(gaussian(tuple(int(v) for v in img_size), device=self.beta.device), history)

    @torch.no_grad()
    def encode(self, x_0: Tensor) -> Tensor:
        """the latent x_T of the images x_0, taken as the state at t_min: the Heun walk g_0 -> g_n"""
        self._require_plain_eps("encode")
        x = self._image(x_0, "encode", copy=True)
        runner = self._flow_runner("encode", x.shape, x.device)
        if runner is None:
            return self._eager_walk(x, "encode", threshold=False)
        return runner.run_copies(x, (), self._tables["encode"][0])

    @torch.no_grad()
    def log_likelihood(self, x_0: Tensor, dequantize: bool = False) -> LogLikelihood:
        """log p(x_0) in nats under the ODE, per image, with one Rademacher probe per image and stage (Hutchinson's estimator: unbiased,
        and the same probes under the same seed).  `dequantize`: uniform noise of one pixel step (2/255) is added first, as the published
        bits/dim figures do.  Returns (log_p, prior, divergence) in float64 and the latent x_T."""
        self._require_plain_eps("log_likelihood")
        x = self._image(x_0, "log_likelihood", copy=True)
        B, chw = x.shape[0], x[0].numel()
        lib = _lib.lib()
        if dequantize:
            seed, off = philox_reserve(x.device, x.numel())
            _lib.check(lib.dmme_pf_dequantize(_lib.ptr(x), x.numel(), seed, off, _lib.stream_ptr()), "dmme_pf_dequantize")
        runner = self._flow_runner("likelihood", x.shape, x.device, LikelihoodChainRunner)
        if runner is None:
            latent, acc = self._eager_likelihood(x)
        else:
            runner.acc.zero_()
            latent, acc = runner.run_copies(x, (), self._tables["likelihood"][0]), runner.acc.clone()
        scratch = torch.zeros(int(lib.dmme_pf_scratch_floats(B, chw)), dtype=torch.float32, device=x.device)
        prior = torch.zeros(B, dtype=torch.float64, device=x.device)
        _lib.check(lib.dmme_pf_prior(_lib.ptr(latent), B, chw, _lib.ptr(scratch), _lib.ptr(prior), _lib.stream_ptr()), "dmme_pf_prior")
        return LogLikelihood(prior + chw * self._log_scale + acc, prior, acc, latent)

    @torch.no_grad()
    def bits_per_dim(self, x_0: Tensor, dequantize: bool = False) -> Tensor:
        """-log2 p per dimension of the 8-bit image behind x_0 (float64 [B]): -log p / (D ln 2) + log2(255 / 2)"""
        ll = self.log_likelihood(x_0, dequantize)
        D = ll.latent[0].numel()
        return -ll.log_p / (D * math.log(2.0)) + math.log2(255.0 / 2.0)
