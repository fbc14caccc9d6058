"""Host-only checks of classifier guidance: the DMME_ARCH_CLASSIFIER plan's parameter table (device -1: no GPU touched), the Python
module's state_dict, the refused precisions, and the guided-update coefficient tables against a float64 restatement."""

import ctypes as C

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.models.ddpm import _cfg_struct

from . import classifier_ref as R


def _host_plan(cfg, num_classes, dtype=_lib.F32):
    c = _cfg_struct(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                    cfg.attention_depths, _lib.ARCH_CLASSIFIER, 1, num_classes)
    h = C.c_void_p()
    rc = _lib.lib().dmme_unet_plan_create(C.byref(c), 2, 32, 32, dtype, -1, C.byref(h))
    return rc, h


@pytest.mark.parametrize("cfg,K", [(R.DEFAULT, 10), (R.TINY, 7)], ids=["default", "tiny"])
def test_plan_param_table_matches_restatement(cfg, K):
    rc, h = _host_plan(cfg, K)
    assert rc == 0, _lib.lib().dmme_last_error()
    lib = _lib.lib()
    try:
        n = lib.dmme_unet_plan_num_params(h)
        ref = R.param_table(cfg, K)
        assert n == len(ref)
        name = C.create_string_buffer(256)
        ndim, off, isb = C.c_int(), C.c_int64(), C.c_int()
        shape = (C.c_int64 * 4)()
        total = 0
        for i, (key, shp, _) in enumerate(ref):
            assert lib.dmme_unet_plan_param_info(h, i, name, 256, C.byref(ndim), shape, C.byref(off), C.byref(isb)) == 0
            assert name.value.decode() == key
            assert tuple(shape[k] for k in range(ndim.value)) == shp
            assert off.value == total
            total += int(np.prod(shp))
        assert lib.dmme_unet_plan_ref_numel(h) == total
        assert lib.dmme_unet_plan_out_channels(h) == K
    finally:
        lib.dmme_unet_plan_destroy(h)


def test_state_dict_keys_and_shared_layout():
    clf = dmme_amd.EncoderClassifier()
    sd = clf.state_dict()
    ref = R.param_table(R.DEFAULT, 10)
    assert list(sd.keys()) == [k for k, _, _ in ref]
    assert all(tuple(sd[k].shape) == s for k, s, _ in ref)
    unet = dmme_amd.UNet(dropout=0.0).state_dict()
    shared = [k for k in sd if not k.startswith("out.")]
    assert all(k in unet and unet[k].shape == sd[k].shape for k in shared)
    clf.load_state_dict({**sd, **{k: unet[k] for k in shared}})  # encoder weights copy over from a UNet


@pytest.mark.parametrize("dtype", [_lib.BF16X3, _lib.F16R32], ids=["bf16x3", "fp16r32"])
def test_refused_precisions(dtype):
    rc, h = _host_plan(R.TINY, 4, dtype)
    assert rc == -2  # DMME_ERR_UNSUPPORTED
    assert not h.value
    with pytest.raises(_lib.DmmeError):
        dmme_amd.EncoderClassifier(precision="bf16x3" if dtype == _lib.BF16X3 else "fp16r32")


def test_guided_update_formulas_float64():
    unet = dmme_amd.UNet(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    clf = dmme_amd.EncoderClassifier(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    s = 2.5
    T = 50
    ddpm = dmme_amd.ClassifierGuidedDDPM(unet, clf, timesteps=T, guidance_scale=s)
    ddim = dmme_amd.ClassifierGuidedDDIM(unet, clf, timesteps=T, sub_timesteps=10, guidance_scale=s)
    rs = np.random.RandomState(3)
    x, e, g, z = (rs.standard_normal(64) for _ in range(4))
    beta = ddpm.beta.reshape(-1).double().numpy()
    abar = np.cumprod(1 - beta)
    _, rows, _ = ddpm._chain_tables()
    for t in (T, T // 2, 1):
        c0, c1, c2, c3 = (np.float64(np.float32(v)) for v in rows[t])
        got = c0 * (x - c1 * e) + c3 * g + (c2 * z if t != 1 else 0.0)
        mu = (x - beta[t] / np.sqrt(1 - abar[t]) * e) / np.sqrt(1 - beta[t])
        want = mu + s * beta[t] * g + (np.sqrt(beta[t]) * z if t != 1 else 0.0)  # Algorithm 1: the mean shift stays at t = 1
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    _, rows, ttab = ddim._chain_tables()
    ab = ddim.alpha_bar.reshape(-1).double().numpy()
    for i in (10, 5, 1):
        c0, c1, c2, _ = (np.float64(np.float32(v)) for v in rows[i])
        got = c1 * ((x - c0 * (e - c2 * g)) / c1)
        ti, tp = ttab[i], ttab[i - 1]
        eh = e - s * np.sqrt(1 - ab[ti]) * g  # Algorithm 2
        want = np.sqrt(ab[tp]) * ((x - np.sqrt(1 - ab[ti]) * eh) / np.sqrt(ab[tp]))
        np.testing.assert_allclose(got, want, rtol=2e-6, atol=2e-6)
    # zero scale: the guided tables carry exact zeros in the guidance slot and the unguided coefficients elsewhere
    z0 = dmme_amd.ClassifierGuidedDDPM(unet, clf, timesteps=T, guidance_scale=0.0)
    plain = dmme_amd.DDPM(unet, timesteps=T)
    assert [r[:3] for r in z0._chain_tables()[1]] == [r[:3] for r in plain._chain_tables()[1]]
    assert all(r[3] == 0.0 for r in z0._chain_tables()[1])


def test_guided_kinds_are_refused_by_the_unguided_update():
    assert _lib.lib().dmme_chain_update(_lib.CHAIN_DDPM_GUIDED, C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), C.c_void_p(16), 1, 4, None) == -1
