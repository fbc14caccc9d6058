"""Host-only checks of what the conditioned chain samplers share (dmme_amd.diffusion_models.conditioned, chain.ROW_DRAWS): the tables each
grid sampler hands to its runner against its own `*_rows` function rounded to fp32, the per-kind noise rule against `chain_draws` on every
table a class builds, and the one mask checker against the three it replaced, message for message.  No GPU is touched."""

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from dmme_amd.diffusion_models import ddnm, dps, ilvr, repaint
from dmme_amd.diffusion_models.chain import chain_draws

T, LEVELS = 100, 6

# the kernels' noise rule per kind, restated: does a step over this row read normals?
DRAWS = {
    _lib.CHAIN_REPAINT: lambda r: r[2] != 0.0 or r[4] != 0.0 or r[6] != 0.0,     # c2 z0, ks z1, r1 z2
    _lib.CHAIN_ILVR: lambda r: r[2] != 0.0 or (r[5] != 0.0 and r[4] != 0.0),    # c2 z0, ks z1 of a conditioned row
    _lib.CHAIN_DDNM: lambda r: r[2] != 0.0 or r[7] != 0.0,                      # cz z0, r1 z1
    _lib.CHAIN_DPS: lambda r: r[2] != 0.0,                                      # c2 z
}


def _f32(rows, ttab):
    return len(ttab) - 1, [tuple(float(np.float32(v)) for v in r) for r in rows], list(ttab)


def _schedule(proc):
    assert proc.n_levels == LEVELS or proc.sub_timesteps == 1
    return proc.alpha_bar.reshape(-1).double().numpy(), [int(t) for t in proc.tau.tolist()]


def _cases():
    """(kind, (n, rows, ttab) as the class holds it, the same from the module's rows function) for every table the four classes build"""
    net, out = torch.nn.Identity(), []
    p = dmme_amd.RePaint(net, T, LEVELS, jump_length=2, resamples=2)
    ab, g = _schedule(p)
    out.append((_lib.CHAIN_REPAINT, p._chain_tables(), _f32(*repaint.repaint_rows(ab, g, repaint.repaint_levels(LEVELS, 2, 2)))))
    out.append((_lib.CHAIN_REPAINT, p._plain_tables, _f32(*repaint.repaint_rows(ab, g, list(range(LEVELS, -1, -1))))))
    p = dmme_amd.ILVR(net, T, LEVELS, down_factor=2, range_level=2)
    ab, g = _schedule(p)
    out.append((_lib.CHAIN_ILVR, p._chain_tables(), _f32(*ilvr.ilvr_rows(ab, g, 2))))
    out.append((_lib.CHAIN_ILVR, p._free_tables, _f32(*ilvr.ilvr_rows(ab, g, LEVELS + 1))))
    for sigma_y in (0.0, 0.1):
        p = dmme_amd.DDNM(net, T, LEVELS, scale=2, sigma_y=sigma_y, travel_length=2, travel_repeat=2)
        ab, g = _schedule(p)
        out.append((_lib.CHAIN_DDNM, p._chain_tables(), _f32(*ddnm.ddnm_rows(ab, g, repaint.repaint_levels(LEVELS, 2, 2), sigma_y))))
    for levels in (LEVELS, 1):
        p = dmme_amd.DPS(net, T, levels, zeta=0.5)
        ab, g = _schedule(p)
        out.append((_lib.CHAIN_DPS, p._chain_tables(), _f32(*dps.dps_rows(ab, g, 0.5))))
    return out


CASES = _cases()


def test_chain_tables_are_the_rows_functions_rounded_to_fp32():
    for kind, (n, rows, ttab), want in CASES:
        assert (n, [tuple(r) for r in rows], list(ttab)) == want and len(rows) == n + 1 and all(len(r) == 8 for r in rows)
    walk_steps = LEVELS + 2 * ((LEVELS - 1) // 2)  # n + (r - 1) j floor((n - 1) / j)
    assert [c[1][0] for c in CASES] == [walk_steps, LEVELS, LEVELS, LEVELS, walk_steps, walk_steps, LEVELS, 1]


def test_chain_draws_is_the_per_row_rule_over_the_table():
    got = []
    for kind, (n, rows, ttab), _ in CASES:
        got.append(chain_draws(kind, rows))
        assert got[-1] == any(DRAWS[kind](r) for r in rows)
    # every kind draws on its grid of six levels, DDNM with and without measurement noise (sigma_y = 0 leaves the posterior's own
    # variance in cz); DPS with one level has the last row only, c2 = 0: noiseless
    assert got == [True] * 7 + [False]
    assert CASES[-1][1][1][1][2] == 0.0 and all(r[2] != 0.0 for r in CASES[4][1][1][2:])


def test_the_modules_rule_is_the_one_restated_here():
    """chain.ROW_DRAWS, which the eager loops and `chain_draws` read, row by row on every table and on rows with a single term"""
    from dmme_amd.diffusion_models.chain import ROW_DRAWS

    single = [tuple(1.0 if j == k else 0.0 for j in range(8)) for k in range(8)] + [(0.0,) * 8, (0.0, 0.0, 0.0, 0.0, 0.7, 1.0, 0.0, 0.0)]
    for kind, rule in DRAWS.items():
        rows = single + [r for k, (_, rows, _), _ in CASES if k == kind for r in rows]
        assert [bool(ROW_DRAWS[kind](r)) for r in rows] == [bool(rule(r)) for r in rows]


def test_one_mask_checker_keeps_the_three_behaviours():
    from dmme_amd.diffusion_models.conditioned import check_mask

    shape, dev = (2, 3, 4, 4), torch.device("cpu")
    forms = {
        "repaint": (lambda m: dmme_amd.RePaint._mask(m, torch.zeros(shape)), 0.0),
        "ddnm": (lambda m: dmme_amd.DDNM._mask(m, shape, dev, 1.0), 1.0),
        "dps": (lambda m: dmme_amd.DPS._mask(m, shape, dev, 1.0), 1.0),
    }
    small = torch.tensor([0.0, 1.0, 1.0, 0.0]).repeat(4).reshape(1, 1, 4, 4)
    for name, (form, none_value) in forms.items():
        m = form(None)  # binary: None means ones; [0, 1]: None means zeros
        assert m.shape == shape and m.dtype == torch.float32 and m.is_contiguous() and bool((m == none_value).all())
        m = form(small)  # broadcasting from (1, 1, h, w)
        assert m.shape == shape and m.is_contiguous() and torch.equal(m, small.expand(shape))
        with pytest.raises(ValueError, match="does not broadcast"):
            form(torch.zeros(2, 3, 4, 2))
    assert bool((check_mask(None, shape, dev, 0.0) == 0).all())  # (`generate`'s nothing-measured mask is the caller's zeros, not None)
    half = torch.full(shape, 0.5)
    assert torch.equal(forms["repaint"][0](half), half)
    messages = {
        "repaint": ("mask: shape (2, 3, 4, 2) does not broadcast from (B|1, C|1, H, W) to (2, 3, 4, 4)",
                    "mask: values must lie in [0, 1] (1: known pixel, 0: generate)", torch.full(shape, 1.5)),
        "ddnm": ("mask: shape (2, 3, 4, 2) does not broadcast from (B|1, Cm|1, h, w) to the measurement's (2, 3, 4, 4)",
                 "mask: values must be 0 or 1 (1: measured): a fractional mask has no pseudo-inverse of this form", half),
        "dps": ("mask: shape (2, 3, 4, 2) does not broadcast from (B|1, C|1, h, w) to the measurement's (2, 3, 4, 4)",
                "mask: values must be 0 or 1 (1: measured)", half),
    }
    for name, (shape_msg, value_msg, bad) in messages.items():
        with pytest.raises(ValueError) as e:
            forms[name][0](torch.zeros(2, 3, 4, 2))
        assert str(e.value) == shape_msg
        with pytest.raises(ValueError) as e:
            forms[name][0](bad)
        assert str(e.value) == value_msg
