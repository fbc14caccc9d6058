"""DDPM training / sampling driver over the HIP kernels.

Drop-in for the reference's `dmme.diffusion_models.DDPM`
(src/dmme/diffusion_models/ddpm.py:15-144): same constructor, buffers
(beta / alpha / alpha_bar, shape (T+1,1,1,1), non-persistent) and methods.  The host
loop stays in Python as in the reference; every per-pixel operation (forward noising,
the reverse update, the MSE loss, the normal draws) is one fused HIP kernel."""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like, philox_reserve, uniform_int
from ..equations.ddpm import linear_schedule, sampling_coefficients
from .chain import ChainRunner, ChainTables, HistoryRecorder, chain_draws, history_ordinals, walk  # noqa: F401  (the samplers, tools and tests import them from here too)


def _scalar_index(t: Tensor, what: str) -> int:
    """the host integer of `sampling_step`'s index argument.  As in the reference only a tensor of shape (1,) is valid (the
    reference's `torch.where(t == 1, ...)` broadcasts t against the last image dimension)."""
    if t.numel() != 1:
        raise RuntimeError(f"sampling_step expects {what} tensor of shape (1,), got {tuple(t.shape)}")
    return int(t.reshape(-1)[0].item())


LOSS_WEIGHTS = ("uniform", "min-snr", "truncated-snr")


def prediction_table(alpha_bar, prediction: str) -> np.ndarray:
    """float64 [T+1][2] = (a_t, b_t) with eps = a_t * out + b_t * x_t for a network that predicts `prediction` (include/dmme_hip.h:
    dmme_pred_to_eps).  x0: a = -sqrt(abar)/sqrt(1-abar), b = 1/sqrt(1-abar), and (NaN, NaN) where abar = 1 (index 0: never stepped
    from, and a misuse should be loud); v: a = sqrt(abar), b = sqrt(1-abar); eps: the identity (1, 0)."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    out = np.empty((ab.size, 2), dtype=np.float64)
    if prediction == "x0":
        with np.errstate(divide="ignore", invalid="ignore"):
            out[:, 0], out[:, 1] = -np.sqrt(ab) / np.sqrt(1 - ab), 1.0 / np.sqrt(1 - ab)
        out[ab >= 1.0] = np.nan
    elif prediction == "v":
        out[:, 0], out[:, 1] = np.sqrt(ab), np.sqrt(1 - ab)
    elif prediction == "eps":
        out[:, 0], out[:, 1] = 1.0, 0.0
    else:
        raise ValueError(f"prediction = {prediction!r}; use one of {tuple(_lib.PREDICTIONS)}")
    return out


def threshold_table(alpha_bar) -> np.ndarray:
    """float64 [T+1][4] = (A_t, B_t, C_t, D_t) of x0 thresholding (include/dmme_hip.h: dmme_x0_threshold): x0 = A x_t - B eps and
    eps = C x_t - D x0, so A = 1/sqrt(abar), B = sqrt(1-abar)/sqrt(abar), C = 1/sqrt(1-abar), D = sqrt(abar)/sqrt(1-abar); NaN where
    abar = 1 (index 0: never stepped from, and a misuse should be loud), as in `prediction_table`."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    out = np.empty((ab.size, 4), dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        sa, sd = np.sqrt(ab), np.sqrt(1 - ab)
        out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 1.0 / sa, sd / sa, 1.0 / sd, sa / sd
    out[ab >= 1.0] = np.nan
    return out


def threshold_rank(percentile: float, n: int) -> Tuple[int, float]:
    """(k, frac) of the `percentile`-quantile of n values with linear interpolation, q = a_k + frac (a_{k+1} - a_k) over the ascending
    order statistics: k = floor(p (n - 1)) and the remainder, formed in float64; frac is what float32 holds of it.  p = 1: (n - 1, 0)."""
    p, n = float(percentile), int(n)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"threshold_percentile = {percentile!r}; a number in [0, 1]")
    if n < 1:
        raise ValueError(f"threshold_rank: {n} values")
    pos = p * (n - 1)
    k = min(int(np.floor(pos)), n - 1)
    frac = float(np.float32(pos - k))
    if k == n - 1:
        frac = 0.0
    return k, frac


def _check_threshold(mode, percentile) -> Tuple[str, float]:
    if mode not in _lib.THRESHOLDS:
        raise ValueError(f"threshold = {mode!r}; use one of {tuple(_lib.THRESHOLDS)}")
    if isinstance(percentile, bool) or not isinstance(percentile, (int, float, np.floating, np.integer)) or not 0.0 <= float(percentile) <= 1.0:
        raise ValueError(f"threshold_percentile = {percentile!r}; a number in [0, 1]")
    return mode, float(percentile)


def loss_weight_table(alpha_bar, prediction: str, loss_weight: str, snr_gamma: float = 5.0) -> np.ndarray:
    """float64 [T+1] weights of the per-timestep MSE.  "min-snr" (Hang et al. 2023) with snr = abar/(1-abar): min(snr, gamma)/snr for an
    eps network, min(snr, gamma) for x0, min(snr, gamma)/(snr + 1) for v - the same weight min(snr, gamma) on the x0 error each
    loss implies.  Where abar = 1 (index 0, snr infinite: never drawn) the limits 0, gamma, 0.  "uniform": ones.  "truncated-snr" (Salimans
    & Ho 2022, the weight progressive distillation trains under): max(snr, 1) on the x0 error, so max(snr, 1)/snr for eps, max(snr, 1)
    for x0, max(snr, 1)/(snr + 1) for v; where abar = 1: 1, NaN (the weight is unbounded there), 1."""
    ab = np.asarray(alpha_bar, dtype=np.float64).reshape(-1)
    if prediction not in _lib.PREDICTIONS:
        raise ValueError(f"prediction = {prediction!r}; use one of {tuple(_lib.PREDICTIONS)}")
    if loss_weight == "uniform":
        return np.ones_like(ab)
    if loss_weight not in LOSS_WEIGHTS:
        raise ValueError(f"loss_weight = {loss_weight!r}; use one of {LOSS_WEIGHTS}")
    one = ab >= 1.0
    snr = np.where(one, 1.0, ab) / np.where(one, 1.0, 1 - ab)
    if loss_weight == "truncated-snr":
        floored = np.maximum(snr, 1.0)
        if prediction == "eps":
            return np.where(one, 1.0, floored / snr)
        if prediction == "x0":
            return np.where(one, np.nan, floored)
        return np.where(one, 1.0, floored / (snr + 1.0))
    gamma = float(snr_gamma)
    clipped = np.minimum(snr, gamma)
    if prediction == "eps":
        return np.where(one, 0.0, clipped / snr)
    if prediction == "x0":
        return np.where(one, gamma, clipped)
    return np.where(one, 0.0, clipped / (snr + 1.0))


class DDPM(nn.Module):
    beta: Tensor
    alpha: Tensor
    alpha_bar: Tensor

    def __init__(self, model: nn.Module, timesteps: int = 1000, start: float = 0.0001, end: float = 0.02, *, prediction: str = "eps",
                 loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        """`prediction`: what the network's output is - "eps" (the noise), "x0", or "v" = sqrt(abar_t) eps - sqrt(1 - abar_t) x0 (Salimans
        & Ho 2022).  Training regresses on that target; sampling turns the output into an eps prediction with one elementwise launch
        behind the network (dmme_pred_to_eps) and runs today's updates on it.  `loss_weight`: "uniform", "min-snr" (Hang et al.
        2023, clipped at `snr_gamma`) or "truncated-snr" (Salimans & Ho 2022: max(snr, 1) on the x0 error).  `threshold`: sampling clips the x0 each eps prediction implies, in front of the update
        (dmme_x0_threshold) - "static" to [-1, 1] (the published samplers' clip_denoised), "dynamic" to the image's
        `threshold_percentile` quantile of |x0| where that exceeds 1, then rescaled (Saharia et al. 2022); see `set_threshold`."""
        super().__init__()
        self.model = model
        self.timesteps = timesteps
        self.threshold, self.threshold_percentile = _check_threshold(threshold, threshold_percentile)
        self._thr = _lib.THRESHOLDS[self.threshold]
        if prediction not in _lib.PREDICTIONS:
            raise ValueError(f"prediction = {prediction!r}; use one of {tuple(_lib.PREDICTIONS)}")
        if loss_weight not in LOSS_WEIGHTS:
            raise ValueError(f"loss_weight = {loss_weight!r}; use one of {LOSS_WEIGHTS}")
        if isinstance(snr_gamma, bool) or not float(snr_gamma) > 0.0:
            raise ValueError(f"snr_gamma = {snr_gamma!r}; a positive number")
        self.prediction, self.loss_weight, self.snr_gamma = prediction, loss_weight, float(snr_gamma)
        self._pred = _lib.PREDICTIONS[prediction]

        beta = linear_schedule(timesteps, start, end).reshape(-1, 1, 1, 1)
        alpha = 1 - beta
        alpha_bar = torch.cumprod(alpha, dim=0)  # alpha[0] = 1
        self.register_buffer("beta", beta, persistent=False)
        self.register_buffer("alpha", alpha, persistent=False)
        self.register_buffer("alpha_bar", alpha_bar, persistent=False)
        # fp32 tables for the forward-noising kernel, evaluated like forward_process does
        # (reference: equations/ddpm/ddpm.py:36-39); device-resident, not part of the state_dict
        self.register_buffer("_sqrt_alpha_bar", torch.sqrt(alpha_bar).reshape(-1).contiguous(), persistent=False)
        self.register_buffer("_sqrt_one_minus_alpha_bar", torch.sqrt(1 - alpha_bar).reshape(-1).contiguous(), persistent=False)
        # host copies of the per-step scalars of the reverse update (python floats)
        self._c1, self._c2, self._sigma = sampling_coefficients(beta, alpha, alpha_bar)
        self._all_t: Optional[Tensor] = None
        self._runner: Optional[ChainRunner] = None
        self._pred_setup()

    def _pred_setup(self) -> None:
        """the fp32 device tables of the x0 / v adapter ([T+1][2]) and of the loss weights ([T+1]), folded in float64 from alpha_bar and
        rounded once; an eps process with uniform weights registers neither"""
        ab64 = self.alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
        if self._pred != _lib.PRED_EPS:
            tab = prediction_table(ab64, self.prediction).astype(np.float32)
            self.register_buffer("_pred_ab", torch.from_numpy(tab).reshape(-1).contiguous(), persistent=False)
        if self.loss_weight != "uniform":
            w = loss_weight_table(ab64, self.prediction, self.loss_weight, self.snr_gamma).astype(np.float32)
            self.register_buffer("_loss_w", torch.from_numpy(w).contiguous(), persistent=False)
        self._thr_setup()

    def _thr_setup(self) -> None:
        """the fp32 device table of x0 thresholding ([T+1][4]), folded in float64 from alpha_bar and rounded once; a process that does
        not threshold registers none"""
        if self._thr != _lib.THRESHOLD_NONE:
            ab64 = self.alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
            tab = torch.from_numpy(threshold_table(ab64).astype(np.float32)).reshape(-1).contiguous()
            self.register_buffer("_thr_tab", tab.to(self.alpha_bar.device), persistent=False)

    def set_threshold(self, mode: str, percentile: Optional[float] = None):
        """another x0 thresholding for the sampling calls that follow: "none", "static" or "dynamic" (at `percentile`, default: the
        process's).  A cached runner is keyed by it: the next chain builds a runner and a graph with the new setting."""
        self.threshold, self.threshold_percentile = _check_threshold(mode, self.threshold_percentile if percentile is None else percentile)
        self._thr = _lib.THRESHOLDS[self.threshold]
        self._thr_setup()
        return self

    def _thr_table(self, device) -> Tensor:
        """the thresholding table on `device` (the buffer itself where the process lives there)"""
        tab = self._thr_tab
        return tab if tab.device == torch.device(device) else tab.to(device)

    def _threshold_eps(self, e: Tensor, x: Tensor, t: Tensor, halves: int = 1, guidance_scale: float = 1.0) -> Tensor:
        """the thresholding stage in place on the eps prediction `e` (a tensor this process owns): one plane per image, IDDPM's two, or
        (halves = 2) the two halves of a classifier-free batch, mixed at `guidance_scale`; `x`: the images the network saw (B of them)"""
        xx = x.detach().to(device=e.device, dtype=torch.float32).contiguous()
        tt = t.detach().reshape(-1).to(device=e.device, dtype=torch.int64).contiguous()
        B, chw = xx.shape[0], xx[0].numel()
        planes = e[0].numel() // chw
        if e.shape[0] != B * halves or planes * chw != e[0].numel() or planes not in (1, 2) or tt.numel() not in (1, B):
            raise ValueError(f"threshold = {self.threshold!r}: a prediction of shape {tuple(e.shape)} for {halves} x images {tuple(xx.shape)} at {tt.numel()} timesteps")
        k, frac = threshold_rank(self.threshold_percentile, chw) if self._thr == _lib.THRESHOLD_DYNAMIC else (0, 0.0)
        lib = _lib.lib()
        scratch = None
        if self._thr == _lib.THRESHOLD_DYNAMIC:
            scratch = getattr(self, "_thr_scratch", None)
            need = int(lib.dmme_x0_threshold_scratch_bytes(B, chw)) // 4
            if scratch is None or scratch.device != e.device or scratch.numel() < need:
                scratch = self._thr_scratch = torch.empty(need, dtype=torch.int32, device=e.device)
        _lib.check(lib.dmme_x0_threshold(self._thr, _lib.ptr(e), _lib.ptr(xx), _lib.ptr(self._thr_table(e.device)), self.timesteps, _lib.ptr(tt), tt.numel(), B, chw,
                                         planes, halves, float(guidance_scale), k, frac, _lib.ptr(scratch), _lib.stream_ptr()), "dmme_x0_threshold")
        return e

    def _pred_table(self, device) -> Tensor:
        """the adapter's table on `device` (the buffer itself where the process lives there)"""
        tab = self._pred_ab
        return tab if tab.device == torch.device(device) else tab.to(device)

    def _use_alpha_bar(self, alpha_bar) -> None:
        """a (T+1) alpha_bar table in place of the linear schedule's (samplers built over another process's schedule): the buffers and
        DDPM's host scalars follow it"""
        T = self.timesteps
        ab = torch.as_tensor(alpha_bar).detach().reshape(-1).to(dtype=torch.float32, device="cpu")
        if ab.numel() != T + 1 or float(ab[0]) != 1.0 or not bool(((ab[1:] > 0) & (ab[1:] < 1)).all()) or not bool((ab[1:] < ab[:-1]).all()):
            raise ValueError(f"alpha_bar: {T + 1} decreasing values, 1 at t = 0 and inside (0, 1) elsewhere")
        ab = ab.reshape(-1, 1, 1, 1)
        alpha = torch.cat([torch.ones_like(ab[:1]), ab[1:] / ab[:-1]])
        for name, v in (("beta", 1 - alpha), ("alpha", alpha), ("alpha_bar", ab), ("_sqrt_alpha_bar", torch.sqrt(ab).reshape(-1).contiguous()),
                        ("_sqrt_one_minus_alpha_bar", torch.sqrt(1 - ab).reshape(-1).contiguous())):
            self.register_buffer(name, v, persistent=False)
        self._c1, self._c2, self._sigma = sampling_coefficients(self.beta, self.alpha, self.alpha_bar)
        self._pred_setup()

    # ------------------------------------------------------------------ device-resident loop (replayable step)
    _chain_kind = _lib.CHAIN_DDPM

    def _chain_tables(self):
        """(number of steps, per-index update scalars [n+1][4], timestep at each loop index) of dmme_chain_step"""
        T = self.timesteps
        rows = [(self._c1[t], self._c2[t] if t > 0 else 0.0, self._sigma[t], 0.0) for t in range(T + 1)]  # index 0 is never stepped from
        return T, rows, list(range(T + 1))

    def chain_length(self) -> int:
        """steps of the chain `generate` runs (DDPM: T; the strided samplers: their sub-steps; RePaint: its walk's downward steps):
        what `history_ordinals` spreads a recorder's frames over"""
        return int(self._chain_tables()[0])

    def timestep_tensor(self, t: int, device) -> Tensor:
        """shape-(1,) device view holding t: indexes a resident arange instead of building `torch.tensor([t])` (a host-to-device
        copy per step in the reference, lit_modules/ddpm.py:77)"""
        n = self.timesteps + 1
        if self._all_t is None or self._all_t.device != torch.device(device) or self._all_t.numel() != n:
            self._all_t = torch.arange(0, n, device=device).unsqueeze(1)
        return self._all_t[t]

    def chain_runner(self, x: Tensor, use_graph: bool = True, slot: str = "_runner", spec=None, cls=None) -> Optional[ChainRunner]:
        """runner bound to the image buffer `x` (cached per buffer / shape); None when the replayable step does not apply
        (a model that is not a dmme_amd UNet, train mode, an image size that is not a multiple of 4).  `cls`: a runner class in place of
        the process's `_runner_class` (a process whose chains do not all take the same step)"""
        if not self._replayable(x):
            return None
        r = getattr(self, slot, None)
        key = self._runner_key(x, use_graph)
        if r is None or r._key != key:
            r = (cls or self._runner_class)(self, x, use_graph, spec() if spec is not None else None)  # (spec: a callable, evaluated only when a runner is built)
            r._key = key
            setattr(self, slot, r)
        return r

    _runner_class = ChainRunner

    def _replayable(self, x: Tensor) -> bool:
        model = self.model
        return hasattr(model, "_plan_for") and not model.training and x.is_cuda and x.dim() == 4 and x[0].numel() % 4 == 0 and x.dtype == torch.float32 and x.is_contiguous()

    def _runner_key(self, x: Tensor, use_graph: bool):
        """what a cached runner is good for: this buffer, this network (by identity) in this precision, this x0 thresholding"""
        return (x.data_ptr(), tuple(x.shape), self.model, self.model._dtype, use_graph, (self.threshold, self.threshold_percentile))

    def _buffered_runner(self, slot: str, shape, device, spec=None, buf: str = "_gen_buf", cls=None) -> Optional[ChainRunner]:
        """the runner in `slot`, bound to an internal image buffer (attribute `buf`) of this shape on this device; both outlive the call:
        a second chain of the same shape re-uses the captured graph, the device tables and the buffers.  None where `chain_runner` is."""
        b = getattr(self, buf, None)
        if b is None or tuple(b.shape) != tuple(shape) or b.device != torch.device(device):
            b = torch.empty(tuple(shape), dtype=torch.float32, device=device)
            setattr(self, buf, b)
        return self.chain_runner(b, slot=slot, spec=spec, cls=cls)

    def _run_chain(self, runner: Optional[ChainRunner], x: Tensor, first: int, count: int, step, history: Optional[HistoryRecorder] = None) -> Tensor:
        """`count` steps from loop index `first` downwards: x into the runner's buffer, one captured step (UNet + noise + update +
        state advance) replayed, a clone of the result; without a runner the eager `step(index)`, in place on x, index by index.
        `history`: a recorder for the chain's frames, on the same step ordinals either way"""
        if runner is not None:
            runner.x.copy_(x)
            return runner.run(first, count, history).clone()
        return walk(x, first, count, lambda s, i: step(i), history)

    def _once_via_runner(self, x_t: Tensor, index: int) -> Optional[Tensor]:
        """single step at loop index `index` through the captured graph, for callers that loop on the host one step at a time
        (LitDDPM.forward <- callbacks/generate.py:82): small batches are bound by the ~160 dependent launches of an eager step"""
        if self.model.training or not x_t.is_cuda or x_t.shape[0] > 64 or torch.is_grad_enabled() and x_t.requires_grad:
            return None
        runner = self._buffered_runner("_runner_once", x_t.shape, x_t.device, buf="_once_buf")
        if runner is None:
            return None
        runner.x.copy_(x_t)
        # (the paper-form DDIM kind at eta = 0 and the DPM-Solver++ kind reserve nothing, like their eager steps; every other kind keeps reserving one span per call,
        # the shipped DDIM kinds included, which draw nothing either)
        seed, off = (0, 0) if runner.kind in (_lib.CHAIN_GDDIM, _lib.CHAIN_DPMPP) and not runner.draws else philox_reserve(x_t.device, x_t.numel())
        runner.set(index, seed, off)
        with torch.no_grad():
            runner.step()
        # (per-step callers: `runner.step()` reads the engine's status word in front of every replay without synchronising - a
        # hand-off timeout raises one step late at most - and `model.check_engine()` is the synchronising check at the end of a loop)
        return runner.x.clone()

    # ------------------------------------------------------------------ training
    def _noised(self, x_0: Tensor, t: Tensor, noise: Tensor, target: bool = True):
        """forward noising for every loss here: (x0, t, x_t, target) = fp32 x_0, int64 t, x_t ~ q(x_t | x_0) built from `noise`, and the
        regression target of the process's `prediction` (None with target=False): for an eps network the noise as the loss re-derives it
        from x_t, for x0 the image, for v sqrt(abar_t) noise - sqrt(1 - abar_t) x_0.  The caller draws `t` and `noise`."""
        x0 = x_0.detach().to(torch.float32).contiguous()
        z = noise.detach().to(device=x0.device, dtype=torch.float32).contiguous()
        t = t.to(device=x0.device, dtype=torch.int64).contiguous()
        x_t = torch.empty_like(x0)
        tgt = torch.empty_like(x0) if target else None
        if self._pred == _lib.PRED_EPS:  # (the launch an eps process has always made; dmme_q_sample_pred writes the same bits)
            _lib.check(
                _lib.lib().dmme_q_sample(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(self._sqrt_alpha_bar), _lib.ptr(self._sqrt_one_minus_alpha_bar), _lib.ptr(t), x0.size(0), x0[0].numel(), _lib.ptr(x_t), _lib.ptr(tgt), _lib.stream_ptr()),
                "dmme_q_sample",
            )
        else:
            _lib.check(
                _lib.lib().dmme_q_sample_pred(self._pred, _lib.ptr(x0), _lib.ptr(z), _lib.ptr(self._sqrt_alpha_bar), _lib.ptr(self._sqrt_one_minus_alpha_bar), _lib.ptr(t), x0.size(0),
                                              x0[0].numel(), _lib.ptr(x_t), _lib.ptr(tgt), _lib.stream_ptr()),
                "dmme_q_sample_pred",
            )
        return x0, t, x_t, tgt

    def _loss(self, out: Tensor, target: Tensor, t: Tensor) -> Tensor:
        """the MSE of the network output against `_noised`'s target: plain (dmme_mse_loss, what an eps process has always called) with
        uniform weights, else weighted per image by the table entry of its timestep (dmme_mse_loss_rows)"""
        from ..autograd import mse_loss_apply, weighted_mse_loss_apply

        if self.loss_weight == "uniform":
            return mse_loss_apply(out, target)
        return weighted_mse_loss_apply(out, target, self._loss_w, t)

    def training_step(self, x_0: Tensor, t: Optional[Tensor] = None, noise: Optional[Tensor] = None) -> Tensor:
        r"""L_simple for one batch (reference: diffusion_models/ddpm.py:53-81), on the target of the process's `prediction` and with its
        `loss_weight`.

        `t` / `noise` may be injected for parity tests; by default t ~ randint(1, T)
        (never T itself, as in the reference) and noise ~ N(0, I)."""
        if t is None:
            t = uniform_int(1, self.timesteps, x_0.size(0), device=x_0.device)
        if noise is None:
            noise = gaussian_like(x_0)
        _, t, x_t, target = self._noised(x_0, t, noise)
        return self._loss(self.model(x_t, t), target, t)

    # ------------------------------------------------------------------ sampling
    def _eps(self, x: Tensor, t: Tensor, *labels, _threshold: bool = True, **kw) -> Tensor:
        """the network's noise prediction at (x, t): its output for an eps network; for an x0 / v network one dmme_pred_to_eps launch on
        the output (eps = a_t out + b_t x); with `threshold` set, the thresholding stage behind that (`_threshold=False`: a caller that
        must not clip, or applies the stage itself).  Every sampling call of the network goes through here; `forward` returns the raw output."""
        out = self.model(x, t, *labels, **kw)
        thr = _threshold and self._thr != _lib.THRESHOLD_NONE
        if self._pred == _lib.PRED_EPS and not thr:
            return out
        e = out.detach().to(torch.float32).contiguous()
        if out.requires_grad and e.data_ptr() == out.data_ptr():
            e = e.clone()  # (never in place on a tensor autograd may still read)
        if self._pred == _lib.PRED_EPS:
            return self._threshold_eps(e, x, t)
        xx = x.detach().to(device=e.device, dtype=torch.float32).contiguous()
        tt = t.detach().reshape(-1).to(device=e.device, dtype=torch.int64).contiguous()
        B = e.shape[0]
        if tuple(e.shape) != tuple(xx.shape) or tt.numel() not in (1, B):
            raise ValueError(f"prediction = {self.prediction!r}: a network output of shape {tuple(e.shape)} for images {tuple(xx.shape)} at {tt.numel()} timesteps")
        _lib.check(_lib.lib().dmme_pred_to_eps(self._pred, _lib.ptr(e), _lib.ptr(xx), _lib.ptr(self._pred_table(e.device)), self.timesteps, _lib.ptr(tt), tt.numel(), B,
                                               e[0].numel(), _lib.stream_ptr()), "dmme_pred_to_eps")
        return self._threshold_eps(e, xx, tt) if thr else e

    def _reverse_update(self, x_t: Tensor, eps: Tensor, t: int, noise: Optional[Tensor]) -> Tensor:
        if noise is None:
            noise = gaussian_like(x_t)  # drawn even when t == 1, then unused (reference :107-110)
        _lib.check(
            _lib.lib().dmme_ddpm_step(_lib.ptr(x_t), _lib.ptr(eps), _lib.ptr(noise), self._c1[t], self._c2[t], self._sigma[t], int(t != 1), x_t.numel(), _lib.stream_ptr()),
            "dmme_ddpm_step",
        )
        return x_t

    def sampling_step(self, x_t: Tensor, t: Tensor, noise: Optional[Tensor] = None) -> Tensor:
        r"""one draw from p_theta(x_{t-1} | x_t) (reference: diffusion_models/ddpm.py:83-111); t has shape (1,)"""
        step = _scalar_index(t, "a timestep")
        eps = self._eps(x_t, t.reshape(1))
        x = x_t.detach().to(torch.float32).clone()
        return self._reverse_update(x, eps, step, noise)

    def denoise_once(self, x_t: Tensor, t: int) -> Tensor:
        """x_{t-1} ~ p_theta(. | x_t) for a host integer t, as a new tensor: what `LitDDPM.forward(x_t, t)` returns
        (reference: lit_modules/ddpm.py:65-79) without the per-step `torch.tensor([t])` upload or a `.item()` read-back"""
        t = int(t)
        out = self._once_via_runner(x_t, t)
        if out is not None:
            return out
        eps = self._eps(x_t, self.timestep_tensor(t, x_t.device))
        x = x_t.detach().to(torch.float32).clone()
        return self._reverse_update(x, eps, t, None)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history: Optional[HistoryRecorder] = None) -> Tensor:
        """run the full T-step chain from pure noise (reference: diffusion_models/ddpm.py:113-133); `history`: a recorder for its frames"""
        dev = self.beta.device
        x_t = gaussian(img_size, device=dev)
        runner, T = self._buffered_runner("_runner", img_size, dev), self.timesteps
        return self._run_chain(runner, x_t, T, T, lambda t: self._reverse_update(x_t, self._eps(x_t, self.timestep_tensor(t, dev)), t, None), history)

    def forward(self, x: Tensor, t: Tensor) -> Tensor:
        """the raw network output (eps, x0 or v, as `prediction` says), not converted: sampling reads it through `_eps`"""
        return self.model(x, t)
