"""Host-only checks of the paper-form DDIM sampler (dmme_amd.GeneralizedDDIM): its coefficient tables against the float64 restatement
(tests/ddim_ref.py), the DDPM limit at eta = 1, why the class exists (the shipped update collapses under a perfect network, the
published one does not), and the argument checks of the new C entry points (no GPU touched)."""

import ctypes as C

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from oracle import diffusion as D

from . import ddim_ref as R

CASES = [(100, 5, "quadratic"), (100, 5, "linear"), (1000, 50, "quadratic")]


@pytest.mark.parametrize("T,S,schedule", CASES)
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_chain_tables_equal_the_float64_tables_rounded_to_fp32(T, S, schedule, eta):
    proc = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), T, S, schedule, eta=eta)
    abar, tau = R.alpha_bar(T), R.tau(T, S, schedule)
    assert np.array_equal(proc.alpha_bar.reshape(-1).double().numpy(), abar) and proc._tau_host == tau
    n, rows, ttab = proc._chain_tables()
    assert n == S and ttab == tau and len(rows) == S + 1
    want = R.reverse_rows(abar, tau, eta).astype(np.float32)
    got = np.array([r[:3] for r in rows], dtype=np.float64)
    assert np.array_equal(got, want.astype(np.float64))  # fp32 values held exactly in python floats
    assert all(r[3] == 0.0 for r in rows)
    # sigma is exactly zero wherever the step lands on tau = 0 (abar = 1), whatever eta
    for i in range(1, S + 1):
        if tau[i - 1] == 0:
            assert rows[i][2] == 0.0, i
        elif eta > 0 and tau[i] != tau[i - 1]:
            assert rows[i][2] > 0.0, i
    # the encoding direction: reversed tables (loop index j holds the step tau_{S-j} -> tau_{S-j+1}), network at max(tau, 1)
    n, erows, ett = proc._encode_tables()
    ewant, ets = R.encode_rows(abar, tau)
    assert n == S
    for j in range(1, S + 1):
        assert tuple(erows[j][:3]) == tuple(float(v) for v in ewant[S - j].astype(np.float32)), j
        assert erows[j][2] == 0.0 and ett[j] == ets[S - j] == max(tau[S - j], 1)
    if (T, S, schedule) == (1000, 50, "quadratic"):
        assert tau[0] == tau[1] == 0 and tuple(erows[S][:3]) == (1.0, 0.0, 0.0)  # tau_0 = tau_1 = 0: the first encoding step is the identity


def test_eta_one_over_every_timestep_is_the_ddpm_posterior():
    """eta = 1, S = T, linear tau, float64 schedule: k0 = 1/sqrt(alpha_t), k1 = -beta_t / (sqrt(alpha_t) sqrt(1 - abar_t)),
    sigma = sqrt(beta~_t) - DDPM's reverse mean with the posterior variance - to 1e-12 relative (largest gaps measured: k0 2e-16, k1 6e-13, sigma 2e-13)."""
    T = 1000
    beta = np.concatenate([[0.0], np.linspace(1e-4, 0.02, T)])
    alpha = 1 - beta
    abar = np.cumprod(alpha)
    rows = R.reverse_rows(abar, list(range(T + 1)), 1.0)
    t = np.arange(1, T + 1)
    k0 = 1 / np.sqrt(alpha[t])
    k1 = -beta[t] / (np.sqrt(alpha[t]) * np.sqrt(1 - abar[t]))
    sig = np.sqrt((1 - abar[t - 1]) / (1 - abar[t]) * beta[t])
    gaps = [float(np.max(np.abs(rows[1:, c] - w) / np.maximum(np.abs(w), 1e-300))) for c, w in ((0, k0), (1, k1))]
    gaps.append(float(np.max(np.abs(rows[2:, 2] - sig[1:]) / sig[1:])))
    print("eta = 1 vs DDPM, largest relative gaps (k0, k1, sigma):", gaps)
    assert max(gaps) <= 1e-12
    assert rows[1, 2] == 0.0 and sig[0] == 0.0  # t = 1: no noise either way


def test_the_shipped_update_collapses_under_a_perfect_network_and_the_paper_update_does_not():
    """Gaussian data of std 0.5 has an exact noise predictor.  T = 1000, S = 50, quadratic tau, float64: the published update ends
    within 5 % of std 0.5 (0.481 over these 65536 draws: the discretisation error of 50 steps), the shipped one (oracle.diffusion.ddim_step) below 1e-6."""
    T, S, std = 1000, 50, 0.5
    abar, tau = R.alpha_bar(T), R.tau(T, S)
    eps_model = R.gaussian_predictor(abar, std)
    x_T = torch.from_numpy(np.random.RandomState(0).standard_normal(1 << 16))
    paper = float(R.generate(eps_model, x_T, abar, tau, 0.0)[0].std())
    x, ab = x_T.clone(), torch.from_numpy(abar)
    for i in range(S, 0, -1):
        x = D.ddim_step(x, tau[i], tau[i - 1], eps_model(x, torch.tensor([tau[i]])), ab)
    shipped = float(x.std())
    print(f"final std under the exact predictor: paper update {paper:.4f}, shipped update {shipped:.3e}")
    assert abs(paper - std) <= 0.05 * std
    assert shipped < 1e-6


def test_python_surface():
    assert "GeneralizedDDIM" in dmme_amd.__all__ and issubclass(dmme_amd.GeneralizedDDIM, dmme_amd.DDIM)
    for eta in (-0.1, 1.5):
        with pytest.raises(ValueError, match="eta"):
            dmme_amd.GeneralizedDDIM(torch.nn.Identity(), eta=eta)
    proc = dmme_amd.GeneralizedDDIM(torch.nn.Identity(), 100, 5, "linear", eta=0.25)
    assert proc.eta == 0.25 and proc._chain_kind == _lib.CHAIN_GDDIM == 5
    lit = dmme_amd.LitDDIM(diffusion_model=proc)
    assert lit.diffusion_model is proc
    for bad in (0, 6):
        with pytest.raises(ValueError):
            proc.sampling_step(torch.zeros(1, 3, 8, 8), torch.tensor([bad]))
    with pytest.raises(ValueError):
        proc.encode(torch.zeros(1, 3, 8, 8), upto=6)
    with pytest.raises(ValueError):
        proc.decode(torch.zeros(1, 3, 8, 8), start=-1)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    assert lib.dmme_version() >= 108
    p = C.c_void_p(16)
    assert lib.dmme_chain_update(6, p, p, p, p, p, 1, 4, None) == -1 and b"kind 6" in lib.dmme_last_error()
    assert lib.dmme_chain_update(-1, p, p, p, p, p, 1, 4, None) == -1
    assert lib.dmme_chain_update_guided(_lib.CHAIN_GDDIM, p, p, p, None, p, p, p, 1, 4, None) == -1  # not a guided kind
    assert lib.dmme_chain_update_gddim(None, p, None, p, p, p, 1, 4, None) == -1 and b"chain_update_gddim" in lib.dmme_last_error()
    assert lib.dmme_chain_update_gddim(p, p, None, p, p, p, 0, 4, None) == -1
    assert lib.dmme_chain_update_gddim(p, p, None, p, p, p, 1, 6, None) != 0 and b"multiple of 4" in lib.dmme_last_error()
    assert lib.dmme_gddim_step(p, p, None, 1.0, 0.0, 0.5, 16, None) == -1 and b"gddim_step" in lib.dmme_last_error()  # k2 != 0 needs z
    assert lib.dmme_gddim_step(None, p, None, 1.0, 0.0, 0.0, 16, None) == -1
    assert lib.dmme_slerp(p, p, p, 0, 1, 16, p, None) == -1 and b"slerp" in lib.dmme_last_error()
    assert lib.dmme_slerp(p, p, p, 2, 0, 16, p, None) == -1
    assert lib.dmme_slerp(p, p, p, 2, 1, 18, p, None) == -1 and b"multiple of 4" in lib.dmme_last_error()
    assert lib.dmme_slerp(None, p, p, 2, 1, 16, p, None) == -1
