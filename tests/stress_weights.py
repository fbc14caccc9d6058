"""Deterministic transforms of an oracle state dict that move the network out of the regime the default synthetic weights
(oracle.*.make_state_dict: torch's default init magnitudes) keep it in: an almost uniform softmax in every attention block and almost
centred GroupNorm inputs.  Plain helpers for the tests that import them; the transforms return a new dict and leave `sd` unchanged.

peaked: the q and the k rows of every attention's qkv conv times `a` (logits times a^2): a sharp softmax.
offset: a per-group constant added to the bias of every conv a GroupNorm reads: |group mean| / std of several units, the normalised
        values unchanged (all channels of a group move together).

The two are kept apart: the offsets pile up along the residual stream and flatten the softmax again.
"""

import numpy as np
import torch


def _is_iddpm(cfg):
    return hasattr(cfg, "num_heads")


def peaked(sd, cfg, a=3.0):
    """q and k rows of every *.qkv_proj.weight / .bias times `a`.  DDPM: q | k | v are the three thirds of the output rows; IDDPM: head h
    owns rows [h * 3d, (h + 1) * 3d) as q | k | v (include/dmme_hip.h: dmme_attention_heads), so rows [h * 3d, h * 3d + 2d) of every head."""
    out = {k: v.clone() for k, v in sd.items()}
    heads = cfg.num_heads if _is_iddpm(cfg) else 1
    n = 0
    for k, v in out.items():
        if ".qkv_proj." not in k:
            continue
        d = v.shape[0] // (3 * heads)
        assert 3 * heads * d == v.shape[0], (k, tuple(v.shape), heads)
        for h in range(heads):
            v[h * 3 * d : h * 3 * d + 2 * d] *= a
        n += 1
    assert n > 0 and n % 2 == 0, n
    return out


def offset(sd, cfg, off=1.0, seed=5):
    """bias of every conv whose output a GroupNorm reads (every 4-D-weight conv except qkv_proj and the network's last conv) plus
    off * s_g, s_g = +-1 per group of cfg.num_groups, drawn from a frozen numpy stream in sorted key order"""
    out = {k: v.clone() for k, v in sd.items()}
    rs = np.random.RandomState(seed)
    G = cfg.num_groups
    for k in sorted(out):
        if not k.endswith(".weight") or out[k].dim() != 4 or ".qkv_proj." in k or k.startswith("output_conv."):
            continue
        co = out[k].shape[0]
        assert co % G == 0, (k, co, G)
        s = rs.randint(0, 2, size=G).astype(np.float32) * 2 - 1
        out[k[: -len("weight")] + "bias"] += off * torch.from_numpy(np.repeat(s, co // G))
    return out


def peaked_a(cfg):
    """the factor that puts the logits' standard deviation near 3 (mean top probability >= 0.2: tests/test_stress_regime.py asserts it).
    One head: a = 3.  The IDDPM block divides the scores by sqrt(C) as well (models/iddpm.py:32,40) although a head's q and k rows are
    C / heads wide, so its logits are sqrt(heads) smaller (default weights: standard deviation 0.16-0.21 against 0.32-0.36; with a = 3
    the mean top probability stays at 0.07-0.18).  a^2 grows by sqrt(heads): a = 3 heads^(1/4) (4 heads: 3 sqrt 2, logits x 18)."""
    heads = cfg.num_heads if _is_iddpm(cfg) else 1
    return 3.0 * heads**0.25


FIXTURES = {"default": lambda sd, cfg: sd, "peaked": lambda sd, cfg: peaked(sd, cfg, peaked_a(cfg)), "offset": offset}
