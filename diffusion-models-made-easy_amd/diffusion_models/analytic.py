"""Analytic-DPM (Bao et al., ICLR 2022) over the HIP kernels: the optimal reverse variance of a fixed-variance noise prediction network on
any sub-trajectory, without retraining.

One statistic per timestep, G_t = E_{x_0, eps} mean_j eps_theta(x_t, t)_j^2 (the paper's beta-bar_t Gamma_t), turns every `GeneralizedDDIM`
grid into its optimal sigma_i and makes the K-step variational bound of such a network computable.  With a = abar_{tau_i},
p = abar_{tau_{i-1}} and lambda_i^2 = eta^2 (1 - p) / (1 - a) (1 - a / p) (0 where p == 1):

    sigma_i^2 = lambda_i^2 + (sqrt((1 - a) p / a) - sqrt(1 - p - lambda_i^2))^2 (1 - G_{tau_i})

The sampling step is `GeneralizedDDIM`'s row {k0, k1, k2} with k2 = sigma_i (0 at i = 1: the last step returns the mean), so `generate`,
`decode`, `sampling_step`, the chain kernel and the capture path are the parent's.  New on the device: the statistics pass
(dmme_analytic_moment) and the rows of the bound (dmme_analytic_vlb_rows).  Left out: the paper's clipped-x0 variant (a second statistic),
guided kinds, data-parallel estimation."""

from __future__ import annotations

import math
from typing import List, Optional

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian_like
from .ddim import GeneralizedDDIM
from .ddpm import _scalar_index
from .iddpm import BitsPerDim

VARIANCES = ("analytic", "beta", "beta-tilde")
VAR_FLOOR = 1e-12  # under the logarithm of a variance that may be 0, as IDDPM floors beta~_1


def analytic_rows(ab, tau, eta: float, G) -> np.ndarray:
    """float64 [S+1][6] = {k0, k1, sigma_i^2, lambda_i^2, upper_i, lambda_i} per loop index (row 0: the identity, never stepped from): the
    mean's scalars as `GeneralizedDDIM` folds them, the optimal variance for the moments `G` (float64[T+1], read at tau_1 .. tau_S), the
    posterior's variance and the paper's upper bound (G = 0).  The grid is strictly increasing from tau_0 = 0."""
    ab = np.asarray(ab, dtype=np.float64).reshape(-1)
    G = np.asarray(G, dtype=np.float64).reshape(-1)
    S = len(tau) - 1
    rows = np.zeros((S + 1, 6), dtype=np.float64)
    rows[0, 0] = 1.0
    for i in range(1, S + 1):
        a, p = ab[tau[i]], ab[tau[i - 1]]
        lam = 0.0 if p == 1.0 or a == 1.0 else eta * np.sqrt((1 - p) / (1 - a)) * np.sqrt(1 - a / p)
        lam2 = lam * lam
        k0 = np.sqrt(p / a)
        root = np.sqrt(max(1 - p - lam2, 0.0))
        c = np.sqrt((1 - a) * p / a) - root
        rows[i] = (k0, root - k0 * np.sqrt(1 - a), lam2 + c * c * (1.0 - G[tau[i]]), lam2, lam2 + c * c, lam)
    return rows


def moment_schedule(timesteps: int, batch_size: int, images_per_timestep: int) -> List[np.ndarray]:
    """the timesteps of every pass of `estimate_moments`: image g of the run (g = b + k B in pass k) gets t = 1 + g mod T; passes of
    `batch_size` images, the last cut to what is left of T * images_per_timestep, so every timestep receives an equal count"""
    T, B, m = int(timesteps), int(batch_size), int(images_per_timestep)
    if T < 1 or B < 1 or m < 1:
        raise ValueError(f"moment_schedule: T = {T}, batch_size = {B}, images_per_timestep = {m}; all at least 1")
    total = T * m
    return [1 + np.arange(g, min(g + B, total), dtype=np.int64) % T for g in range(0, total, B)]


def moment_images(first: int, count: int, timesteps: int, n: int) -> np.ndarray:
    """which of a tensor's n images the run's images first .. first + count - 1 are: (g + g // T) mod n - every sweep over the timesteps
    starts one image further, so a timestep does not keep meeting the same images where n and T share a factor"""
    g = np.arange(int(first), int(first) + int(count), dtype=np.int64)
    return (g + g // int(timesteps)) % int(n)


class AnalyticDPM(GeneralizedDDIM):
    r"""`GeneralizedDDIM` with the optimal reverse variance of Analytic-DPM in place of the hand-set eta^2 beta~.  `estimate_moments` fills
    the per-timestep statistic from data (or `set_moments` installs a table); it travels in the state_dict.  `bits_per_dim` is the K-step
    variational bound of the network under that variance, or under the hand-set beta / beta~.  The moment is taken behind the x0 / v adapter,
    where every network's output is a noise prediction; an IDDPM network's eps plane is read and its learned variance is not used."""

    _table_version = 0  # counts the changes of the moments: part of a runner's key
    _analytic = None    # (float64 rows, fp32 sampling rows) of the current moments, built on first use

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 50, tau_schedule: str = "linear", eta: float = 1.0, *,
                 prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, sub_timesteps, tau_schedule, eta, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma,
                         threshold=threshold, threshold_percentile=threshold_percentile)
        tau = self._tau_host
        if tau[0] != 0 or any(tau[i] <= tau[i - 1] for i in range(1, len(tau))):
            i = next((i for i in range(1, len(tau)) if tau[i] <= tau[i - 1]), 0)
            raise ValueError(f"AnalyticDPM: the {self.tau_schedule} grid of {sub_timesteps} steps over T = {timesteps} is not strictly increasing from tau_0 = 0 "
                             f"(tau_{max(i - 1, 0)} = {tau[max(i - 1, 0)]}, tau_{i} = {tau[i]}): the posterior between equal timesteps has no variance")
        self._ab64 = self.alpha_bar.detach().reshape(-1).to(torch.float64).cpu().numpy()
        # the statistic: sum of the per-image moments and their number per timestep (entry 0 unused); persistent, of this class only
        self.register_buffer("_g_sum", torch.zeros(timesteps + 1, dtype=torch.float64))
        self.register_buffer("_g_count", torch.zeros(timesteps + 1, dtype=torch.int64))

    # ------------------------------------------------------------------ the statistic
    def _moments_changed(self) -> None:
        """the tables follow the moments: the next use rebuilds them, and a runner captured over the old ones is replaced (`_runner_key`)"""
        self._analytic = None
        self._table_version += 1

    def _load_from_state_dict(self, *args, **kw):
        super()._load_from_state_dict(*args, **kw)
        self._moments_changed()

    def _runner_key(self, x: Tensor, use_graph: bool):
        return super()._runner_key(x, use_graph) + (self._table_version,)

    def moments(self) -> np.ndarray:
        """float64[T+1]: G_t = clip(sum_t / count_t, 0, 1); NaN where nothing has been counted (entry 0 always)"""
        s, c = self._g_sum.detach().cpu().numpy(), self._g_count.detach().cpu().numpy()
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(c > 0, np.clip(s / np.maximum(c, 1), 0.0, 1.0), np.nan)

    def set_moments(self, G) -> "AnalyticDPM":
        """install a table G[T+1] (entry 0 is not read) in place of what has been counted, as ONE count per timestep: an `estimate_moments`
        that follows would average the table in as if it were a single image's moment - call `reset_moments` first where that is not meant"""
        G = np.asarray(G, dtype=np.float64).reshape(-1)
        T = self.timesteps
        if G.size != T + 1 or not bool(np.all((G[1:] >= 0.0) & (G[1:] <= 1.0))):
            raise ValueError(f"set_moments: {T + 1} values, those of t = 1..{T} in [0, 1]")
        s = torch.from_numpy(G.copy())
        s[0] = 0.0
        c = torch.ones(T + 1, dtype=torch.int64)
        c[0] = 0
        self._g_sum.copy_(s)
        self._g_count.copy_(c)
        self._moments_changed()
        return self

    def reset_moments(self) -> "AnalyticDPM":
        """forget every moment: sums and counts back to zero"""
        self._g_sum.zero_()
        self._g_count.zero_()
        self._moments_changed()
        return self

    def _require_eval(self, what: str) -> None:
        """the statistic and the bound are those of the network that samples: in train mode a UNet draws dropout masks, under no_grad too"""
        if getattr(self.model, "training", False):
            raise RuntimeError(f"AnalyticDPM.{what}: the network is in train mode; the moments and the bound need the deterministic denoiser that samples (call .eval())")

    @torch.no_grad()
    def estimate_moments(self, data, images_per_timestep: int = 64, batch_size: Optional[int] = None, seed: Optional[int] = 0) -> np.ndarray:
        r"""ADDS T * images_per_timestep per-image moments to the tables (to what earlier calls or `set_moments` left there; `reset_moments`
        starts over) and returns `moments()`.  `data`: a tensor of images in [-1, 1] or an iterable of batches (each a tensor, or a tuple
        whose first entry is one; walked again when it ends).  Image g of the run gets t = 1 + g mod T (`moment_schedule`); of a tensor of
        n images it is image (g + g // T) mod n (`moment_images`): every sweep over the timesteps starts one image further, so a timestep does not keep
        meeting the same images where n and T share a factor.  Per pass: a span of the Philox stream for the noise, dmme_q_sample, the
        network without gradient (behind its x0 / v adapter, in front of x0 thresholding), dmme_analytic_moment.  Nothing is read back
        inside the loop; the kernel's status word is read once at the end.  The network must be in eval mode.

        SIDE EFFECT of the default `seed=0`: the device's global generator is restarted at that seed, so the same call gives the same
        moments - and whatever samples afterwards draws from the restarted stream.  `seed=None` leaves the generator alone and draws from
        where it stands (what the trainer does)."""
        self._require_eval("estimate_moments")
        T, m = self.timesteps, int(images_per_timestep)
        dev = self._g_sum.device
        if dev.type != "cuda":
            raise RuntimeError("estimate_moments runs on the GPU: move the process there first")
        if seed is not None:
            torch.cuda.default_generators[dev.index if dev.index is not None else torch.cuda.current_device()].manual_seed(int(seed))
        total, done = T * m, 0
        lib = _lib.lib()
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        scratch = None

        def batches():
            if torch.is_tensor(data):
                n0 = data.shape[0]
                B = int(batch_size or min(n0, 128))
                g = 0
                while True:
                    yield data[torch.from_numpy(moment_images(g, B, T, n0)).to(data.device)]
                    g += B
            else:
                while True:
                    seen = False
                    for item in data:
                        seen = True
                        yield item[0] if isinstance(item, (tuple, list)) else item
                    if not seen:
                        raise ValueError("estimate_moments: the data yielded no batch")

        for x in batches():
            x = x[: total - done].to(device=dev, dtype=torch.float32)
            B, chw = x.shape[0], x[0].numel()
            t = 1 + (torch.arange(done, done + B, device=dev, dtype=torch.int64) % T)
            _, t, x_t, _ = self._noised(x, t, gaussian_like(x), target=False)
            out = self._eps(x_t, t, _threshold=False).detach().to(torch.float32).contiguous()
            if scratch is None or scratch.numel() < 32 * B:
                scratch = torch.empty(32 * B, dtype=torch.float32, device=dev)
            _lib.check(lib.dmme_analytic_moment(_lib.ptr(out), out[0].numel(), _lib.ptr(t), T, B, chw, _lib.ptr(self._g_sum), _lib.ptr(self._g_count), None,
                                                _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_analytic_moment")
            done += B
            if done >= total:
                break
        self._moments_changed()
        if int(status.item()) != 0:
            raise _lib.DmmeError("estimate_moments: a timestep left the moment tables")
        return self.moments()

    # ------------------------------------------------------------------ tables
    def _analytic_tables(self):
        """(float64 rows of `analytic_rows`, the fp32-rounded sampling rows {k0, k1, k2, 0}): built on first use after the moments change"""
        if self._analytic is None:
            tau = self._tau_host
            G = self.moments()
            for i in range(1, len(tau)):
                if not np.isfinite(G[tau[i]]):
                    raise RuntimeError(f"AnalyticDPM: no moment for timestep {tau[i]} (tau_{i}): run estimate_moments, set_moments or load a checkpoint that holds them")
            rows = analytic_rows(self._ab64, tau, self.eta, G)
            f32 = lambda v: float(np.float32(v))
            rev = [(1.0, 0.0, 0.0, 0.0)]
            for i in range(1, len(tau)):
                k0, k1, s2, l2, _, lam = rows[i]
                k2 = 0.0 if i == 1 else lam if s2 == l2 else np.sqrt(s2)  # (G = 1: the posterior's own deviation, GeneralizedDDIM's bits)
                rev.append((f32(k0), f32(k1), f32(k2), 0.0))
            self._analytic = (rows, rev)
        return self._analytic

    def sampling_rows(self):
        """the fp32 rows {k0, k1, k2, 0} per loop index the chain steps with (the parent's `_rev_rows` stay its hand-set ones)"""
        return self._analytic_tables()[1]

    def draws(self) -> bool:
        """does the chain draw noise?  (at eta = 0 too: the optimal variance of a deterministic mean is not zero)"""
        return any(r[2] != 0.0 for r in self.sampling_rows())

    # the three places GeneralizedDDIM reads its rows: the runner's tables, the eager chain's update, the public step
    def _chain_tables(self):
        return self.sub_timesteps, list(self.sampling_rows()), list(self._tau_host)

    def _ddim_update(self, x: Tensor, eps: Tensor, i: int) -> Tensor:
        return self._gddim_update(x, eps, self.sampling_rows()[i], None, self.draws())

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, noise: Optional[Tensor] = None) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i} under the analytic variance; arguments as `GeneralizedDDIM.sampling_step`"""
        idx = self._index(_scalar_index(i, "an index"), "sampling_step")
        eps = self._eps(x_tau_i, self.tau[idx].reshape(1))
        x = x_tau_i.detach().to(torch.float32).clone()
        return self._gddim_update(x, eps, self.sampling_rows()[idx], noise, self.draws())

    def variances(self) -> np.ndarray:
        """float64 [S+1][3] = (sigma_i^2, lambda_i^2, upper_i) of the current moments"""
        return self._analytic_tables()[0][:, 2:5].copy()

    # ------------------------------------------------------------------ the bound
    def _vlb_table(self, variance: str) -> np.ndarray:
        """float32 [S+1][8] of dmme_analytic_vlb_rows: {k0, k1, log sigma^2, log lambda^2, sqrt(abar), sqrt(1 - abar), 0, 0}"""
        if variance not in VARIANCES:
            raise ValueError(f"variance = {variance!r}; use one of {VARIANCES}")
        tau, ab = self._tau_host, self._ab64
        S = len(tau) - 1
        if variance == "analytic":
            rows = self._analytic_tables()[0]
        else:
            rows = analytic_rows(ab, tau, self.eta, np.ones(self.timesteps + 1))
        sa, s1 = self._sqrt_alpha_bar.detach().cpu().numpy(), self._sqrt_one_minus_alpha_bar.detach().cpu().numpy()  # dmme_q_sample's own fp32 tables
        tab = np.zeros((S + 1, 8), dtype=np.float64)
        tab[0, 0] = 1.0
        for i in range(1, S + 1):
            a, p = ab[tau[i]], ab[tau[i - 1]]
            l2 = rows[i][3]
            s2 = rows[i][2] if variance == "analytic" else 1.0 - a / p if variance == "beta" else l2
            tab[i] = (rows[i][0], rows[i][1], math.log(max(s2, VAR_FLOOR)), math.log(max(l2, VAR_FLOOR)), sa[tau[i]], s1[tau[i]], 0.0, 0.0)
        return tab.astype(np.float32)

    @torch.no_grad()
    def bits_per_dim(self, x_0: Tensor, variance: str = "analytic", noise: Optional[Tensor] = None) -> BitsPerDim:
        r"""the K-step variational bound on -log p(x_0) in bits/dim: (total[B], prior[B], terms[B, S]) with terms[:, i-1] the term of the step
        tau_i -> tau_{i-1} (the discretised-Gaussian NLL of x_0 at i = 1, KL(q(x_{tau_{i-1}} | x_{tau_i}, x_0) || p_theta) above),
        prior = KL(q(x_{tau_S} | x_0) || N(0, I)), total their sum, each a mean over the image's elements divided by ln 2.  `variance`: the
        reverse variance - "analytic" (sigma_i^2 of the moments), "beta" (1 - abar_{tau_i} / abar_{tau_{i-1}}) or "beta-tilde"
        (lambda_i^2, floored at 1e-12 at i = 1 as IDDPM floors beta~_1).  Needs eta = 1: the KL is infinite against a posterior without
        variance.  An eager loop over i = S .. 1 of dmme_q_sample at tau_i, the network and dmme_analytic_vlb_rows; `noise`
        (S, B, C, H, W): noise[i-1] is the draw of step i (default: fresh normals).  The status word is read once at the end."""
        self._require_eval("bits_per_dim")
        if self.eta != 1.0:
            raise ValueError(f"bits_per_dim needs eta = 1 (the posterior of eta = {self.eta} is narrower than DDPM's; at eta = 0 the KL is infinite)")
        tab = self._vlb_table(variance)
        tau, S, B = self._tau_host, self.sub_timesteps, x_0.size(0)
        x0 = x_0.detach().to(torch.float32).contiguous()
        dev, chw = x0.device, x0[0].numel()
        lib = _lib.lib()
        coef = torch.from_numpy(tab).reshape(-1).to(dev)
        rows = torch.empty(B, dtype=torch.float32, device=dev)
        scratch = torch.empty(32 * B, dtype=torch.float32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        terms = torch.empty((S, B), dtype=torch.float32, device=dev)
        prior = torch.empty(B, dtype=torch.float32, device=dev)
        for i in range(S, 0, -1):
            t = torch.full((B,), tau[i], dtype=torch.int64, device=dev)
            idx = torch.full((B,), i, dtype=torch.int64, device=dev)
            _, _, x_t, _ = self._noised(x0, t, gaussian_like(x0) if noise is None else noise[i - 1], target=False)
            out = self._eps(x_t, t, _threshold=False).detach().to(torch.float32).contiguous()
            _lib.check(lib.dmme_analytic_vlb_rows(_lib.ptr(out), out[0].numel(), _lib.ptr(x_t), _lib.ptr(x0), _lib.ptr(idx), _lib.ptr(coef), S, B, chw, _lib.ptr(rows),
                                                  _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_analytic_vlb_rows")
            terms[i - 1] = rows / math.log(2.0)
        _lib.check(lib.dmme_iddpm_prior_rows(_lib.ptr(x0), B, chw, float(self.alpha_bar.reshape(-1)[tau[S]]), _lib.ptr(prior), _lib.stream_ptr()), "dmme_iddpm_prior_rows")
        prior = prior / math.log(2.0)
        if int(status.item()) != 0:
            raise _lib.DmmeError("bits_per_dim: an index left the coefficient table")
        terms = terms.t().contiguous()
        return BitsPerDim(prior + terms.sum(dim=1), prior, terms)
