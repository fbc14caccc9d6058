"""DDIM strided sampler over the HIP kernels.

Drop-in for the reference's `dmme.diffusion_models.DDIM`
(src/dmme/diffusion_models/ddim.py:15-99).  The update is the one the reference ships
(numerically x - sqrt(1 - abar_tau_i) * eps), computed directly so the
`Normal(mean, 0)` ValueError of the reference at tau_{i-1} = 0 cannot occur."""

from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .. import _lib
from ..common.noise import gaussian, gaussian_like
from ..equations.ddim import linear_tau, quadratic_tau
from .ddpm import DDPM, ChainRunner, _scalar_index


class DDIM(DDPM):
    tau: Tensor

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 50, tau_schedule: str = "quadratic", *, prediction: str = "eps",
                 loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold,
                         threshold_percentile=threshold_percentile)  # start/end are not forwarded, as in the reference (:39)
        self.sub_timesteps = sub_timesteps
        kind = tau_schedule.lower()
        if kind == "linear":
            tau = linear_tau(timesteps, sub_timesteps)
        elif kind == "quadratic":
            tau = quadratic_tau(timesteps, sub_timesteps)
        else:
            raise NotImplementedError
        self.tau_schedule = kind
        self.register_buffer("tau", tau, persistent=False)
        ab = self.alpha_bar.reshape(-1).to(torch.float32).cpu()
        self._tau_host = [int(v) for v in tau]
        self._s1 = torch.sqrt(1 - ab).tolist()  # sqrt(1 - abar_t), indexed by t
        self._s2 = torch.sqrt(ab).tolist()      # sqrt(abar_t)
        self._tau_dev: Optional[Tensor] = None

    def _ddim_update(self, x: Tensor, eps: Tensor, i: int) -> Tensor:
        ti, tp = self._tau_host[i], self._tau_host[i - 1]
        _lib.check(_lib.lib().dmme_ddim_step(_lib.ptr(x), _lib.ptr(eps), self._s1[ti], self._s2[tp], x.numel(), _lib.stream_ptr()), "dmme_ddim_step")
        return x

    def sampling_step(self, x_tau_i: Tensor, i: Tensor) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i} (reference: diffusion_models/ddim.py:55-77); i has shape (1,)."""
        idx = _scalar_index(i, "an index")
        eps = self._eps(x_tau_i, self.tau[idx].reshape(1))
        x = x_tau_i.detach().to(torch.float32).clone()
        return self._ddim_update(x, eps, idx)

    _chain_kind = _lib.CHAIN_DDIM

    def _chain_tables(self):
        S, tau = self.sub_timesteps, self._tau_host
        rows = [(0.0, 1.0, 0.0, 0.0)] + [(self._s1[tau[i]], self._s2[tau[i - 1]], 0.0, 0.0) for i in range(1, S + 1)]
        return S, rows, list(tau)

    def denoise_once(self, x: Tensor, i: int) -> Tensor:
        i = int(i)
        done = self._once_via_runner(x, i)
        if done is not None:
            return done
        eps = self._eps(x, self.tau_tensor(i, x.device))
        out = x.detach().to(torch.float32).clone()
        return self._ddim_update(out, eps, i)

    def tau_tensor(self, i: int, device) -> Tensor:
        if self._tau_dev is None or self._tau_dev.device != torch.device(device):
            self._tau_dev = self.tau.to(device).unsqueeze(1)
        return self._tau_dev[i]

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """S-step strided chain (reference: diffusion_models/ddim.py:79-99); `history`: a HistoryRecorder for its frames"""
        return self._decode_chain(gaussian(img_size, device=self.beta.device), self.sub_timesteps, history)

    def _decode_chain(self, x: Tensor, start: int, history=None) -> Tensor:
        """`start` reverse steps from loop index `start`, in place on x or through the captured step"""
        runner = self._buffered_runner("_runner", x.shape, x.device)
        return self._run_chain(runner, x, start, start, lambda i: self._ddim_update(x, self._eps(x, self.tau_tensor(i, x.device)), i), history)

    # ------------------------------------------------------------------ argument checks of the samplers with `decode` (GeneralizedDDIM, DPMSolverPP)
    def _last_index(self) -> int:
        """the loop index a full chain starts from"""
        return self.sub_timesteps

    def _index(self, i, what: str) -> int:
        i, n = int(i), self._last_index()
        if not 1 <= i <= n:
            raise ValueError(f"{what}: index {i} outside 1..{n}")
        return i

    def _decode(self, x: Tensor, start: Optional[int], history) -> Tensor:
        n = self._last_index()
        start = n if start is None else int(start)
        if not 0 <= start <= n:
            raise ValueError(f"decode: start {start} outside 0..{n}")
        x = x.detach().to(device=self.beta.device, dtype=torch.float32).contiguous().clone()
        if start == 0 and history is not None:
            raise ValueError("decode: start = 0 runs no chain to record")
        return x if start == 0 else self._decode_chain(x, start, history)


class GeneralizedDDIM(DDIM):
    r"""DDIM as published (Song, Meng & Ermon 2021, eq. 12), next to `DDIM`, which keeps the reference's collapsed update
    (x - sqrt(1 - abar_tau_i) eps: no term pointing back to x_t, so its chain shrinks towards zero even with a perfect network).

    Every step, in either direction and for every eta, is  x' = (k0 x + k1 eps) + k2 z  with the three scalars folded on the host in
    float64 and rounded to fp32 (include/dmme_hip.h: dmme_gddim_step).  eta = 0 is the deterministic sampler, eta = 1 has DDPM's
    posterior variance.  `encode` runs the eta = 0 step forwards (x_0 -> x_T), `decode` / `generate` backwards, `interpolate`
    slerps two encoded latents and decodes them.  The chains replay one captured step like every other sampler here; the encoding
    chain is the same device loop over reversed tables.  The update runs on a noise prediction (an IDDPM network's learned variance is not
    used); an x0 / v network (`prediction=`) is converted to one behind its forward, as in every process."""

    _chain_kind = _lib.CHAIN_GDDIM

    def __init__(self, model: nn.Module, timesteps: int = 1000, sub_timesteps: int = 50, tau_schedule: str = "quadratic", eta: float = 0.0, *,
                 prediction: str = "eps", loss_weight: str = "uniform", snr_gamma: float = 5.0, threshold: str = "none", threshold_percentile: float = 0.995) -> None:
        super().__init__(model, timesteps, sub_timesteps, tau_schedule, prediction=prediction, loss_weight=loss_weight, snr_gamma=snr_gamma, threshold=threshold,
                         threshold_percentile=threshold_percentile)
        eta = float(eta)
        if not 0.0 <= eta <= 1.0:
            raise ValueError(f"eta must lie in [0, 1], got {eta}")
        self.eta = eta
        ab = self.alpha_bar.reshape(-1).to(torch.float64).cpu().numpy()
        S, tau = self.sub_timesteps, self._tau_host
        f32 = lambda v: float(np.float32(v))
        rev = [(1.0, 0.0, 0.0, 0.0)]  # index 0 is never stepped from
        for i in range(1, S + 1):
            a, p = ab[tau[i]], ab[tau[i - 1]]
            sigma = 0.0 if p == 1.0 or a == 1.0 else eta * np.sqrt((1 - p) / (1 - a)) * np.sqrt(1 - a / p)
            k0 = np.sqrt(p / a)
            k1 = np.sqrt(max(1 - p - sigma * sigma, 0.0)) - k0 * np.sqrt(1 - a)
            rev.append((f32(k0), f32(k1), f32(sigma), 0.0))
        # encoding: the loop index only runs downwards, so index j holds the step tau_{S-j} -> tau_{S-j+1}; the network is evaluated at
        # max(tau_{S-j}, 1) (training never draws t = 0; where tau_i = tau_{i+1} = 0 the step is the identity: k0 = 1, k1 = 0)
        enc, enc_t = [(1.0, 0.0, 0.0, 0.0)], [max(tau[S], 1)]
        for j in range(1, S + 1):
            a, n = ab[tau[S - j]], ab[tau[S - j + 1]]
            k0 = np.sqrt(n / a)
            enc.append((f32(k0), f32(np.sqrt(1 - n) - k0 * np.sqrt(1 - a)), 0.0, 0.0))
            enc_t.append(max(tau[S - j], 1))
        self._rev_rows, self._enc_rows, self._enc_t = rev, enc, enc_t
        self._draws = any(r[2] != 0.0 for r in rev)
        self._enc_t_dev: Optional[Tensor] = None

    def _chain_tables(self):
        return self.sub_timesteps, list(self._rev_rows), list(self._tau_host)

    def _encode_tables(self):
        return self.sub_timesteps, list(self._enc_rows), list(self._enc_t)

    def _gddim_update(self, x: Tensor, eps: Tensor, row, noise: Optional[Tensor] = None, draw: bool = False) -> Tensor:
        """in place on x; `draw`: a step of a chain that draws takes its span of the Philox stream whether or not k2 uses it"""
        if noise is None and draw:
            noise = gaussian_like(x)
        z = None if noise is None else noise.detach().to(device=x.device, dtype=torch.float32).contiguous()
        if z is None and row[2] != 0.0:
            raise ValueError("a step with k2 != 0 needs noise")
        _lib.check(_lib.lib().dmme_gddim_step(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(z), row[0], row[1], row[2], x.numel(), _lib.stream_ptr()), "dmme_gddim_step")
        return x

    def _ddim_update(self, x: Tensor, eps: Tensor, i: int) -> Tensor:
        return self._gddim_update(x, eps, self._rev_rows[i], None, self._draws)

    def sampling_step(self, x_tau_i: Tensor, i: Tensor, noise: Optional[Tensor] = None) -> Tensor:
        r"""x_{tau_{i-1}} from x_{tau_i}; i has shape (1,) as in `DDIM.sampling_step`; `noise` replaces the drawn normals"""
        idx = self._index(_scalar_index(i, "an index"), "sampling_step")
        eps = self._eps(x_tau_i, self.tau[idx].reshape(1))
        x = x_tau_i.detach().to(torch.float32).clone()
        return self._gddim_update(x, eps, self._rev_rows[idx], noise, self._draws)

    def denoise_once(self, x: Tensor, i: int) -> Tensor:
        return super().denoise_once(x, self._index(i, "denoise_once"))

    def _enc_t_tensor(self, j: int, device) -> Tensor:
        if self._enc_t_dev is None or self._enc_t_dev.device != torch.device(device):
            self._enc_t_dev = torch.tensor(self._enc_t, dtype=torch.int64, device=device).unsqueeze(1)
        return self._enc_t_dev[j]

    def _encode_runner(self, shape, dev) -> Optional[ChainRunner]:
        """the encoding direction's runner: one per shape, on a buffer of its own (slot `_runner` is the decoding direction's)"""
        r = self._buffered_runner("_enc_runner", shape, dev, spec=lambda: (_lib.CHAIN_GDDIM, self._encode_tables()), buf="_enc_buf")
        return r if r is None else r.no_threshold()  # (encoding never thresholds: a clipped step has no inverse)

    @torch.no_grad()
    def decode(self, x: Tensor, start: Optional[int] = None, history=None) -> Tensor:
        r"""x_0 from x_{tau_start} (start = S by default): `start` reverse steps; draws noise where eta > 0"""
        return self._decode(x, start, history)

    @torch.no_grad()
    def encode(self, x0: Tensor, upto: Optional[int] = None) -> Tensor:
        r"""x_{tau_upto} from x_0 (upto = S by default: the latent x_T): the deterministic (eta = 0) step run forwards"""
        S = self.sub_timesteps
        upto = S if upto is None else int(upto)
        if not 0 <= upto <= S:
            raise ValueError(f"encode: upto {upto} outside 0..{S}")
        x = x0.detach().to(device=self.beta.device, dtype=torch.float32).contiguous().clone()
        if upto == 0:
            return x
        step = lambda j: self._gddim_update(x, self._eps(x, self._enc_t_tensor(j, x.device), _threshold=False), self._enc_rows[j])
        return self._run_chain(self._encode_runner(x.shape, x.device), x, S, upto, step)

    @torch.no_grad()
    def generate(self, img_size: Tuple[int, int, int, int], history=None) -> Tensor:
        """S-step chain from pure noise; with eta = 0 nothing but x_T is drawn, with eta > 0 one span of normals per step"""
        return self.decode(gaussian(img_size, device=self.beta.device), history=history)

    @torch.no_grad()
    def interpolate(self, xa: Tensor, xb: Tensor, weights) -> Tensor:
        r"""images between xa and xb: both encoded to x_T, spherically interpolated there at each of the n `weights` (0: xa, 1: xb),
        all n x B latents decoded in one chain; returns (n, B, C, H, W)"""
        if xa.shape != xb.shape or xa.dim() != 4:
            raise ValueError(f"interpolate: two image batches of one shape, got {tuple(xa.shape)} and {tuple(xb.shape)}")
        la, lb = self.encode(xa), self.encode(xb)
        w = torch.as_tensor(weights, dtype=torch.float32).reshape(-1).to(la.device).contiguous()
        n, B = w.numel(), la.shape[0]
        lat = torch.empty((n,) + tuple(la.shape), dtype=torch.float32, device=la.device)
        _lib.check(_lib.lib().dmme_slerp(_lib.ptr(la), _lib.ptr(lb), _lib.ptr(w), n, B, la[0].numel(), _lib.ptr(lat), _lib.stream_ptr()), "dmme_slerp")
        return self.decode(lat.reshape((n * B,) + tuple(la.shape[1:]))).reshape(lat.shape)
