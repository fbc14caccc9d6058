"""CPU: the float64 restatement of the optimiser tail (tests/optim_ref.py) against torch - torch.optim.Adam on float64 parameters,
clip_grad_norm_, the `mul_` / `add_` EMA of the reference's callback, and torch.amp.GradScaler's state machine; that the restatement
can SEE a misplaced eps in the regime tests/test_gpu_optim.py uses for it; what the C ABI refuses before any launch; and the host half of
the device-move order (model and optimiser state loaded on the CPU, moved afterwards): nothing here launches a kernel."""

import ctypes as C
import math

import pytest
import torch

from oracle import unet as O

from . import optim_ref as R

LR, B1, B2, EPS, DECAY = 2e-4, 0.9, 0.999, 1e-8, 0.9999  # configs/ddpm/cifar10.yaml


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def test_restatement_matches_torch_adam_clip_and_ema_over_20_mixed_steps():
    """unrounded scalars; gradient norms on both sides of max_norm = 1; agreement to 1e-12 relative on p, m, v and the EMA"""
    n = 997
    gen = torch.Generator().manual_seed(0)
    p0 = torch.randn(n, dtype=torch.float64, generator=gen) * 0.05
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    ema_t = p0.clone()
    p, m, v, ema = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64), p0.clone()
    clipped = 0
    for t in range(1, 21):
        target = 3.0 if t % 3 else 0.25  # the gradient's norm: above 1 on two steps of three, below on the third
        g = torch.randn(n, dtype=torch.float64, generator=gen)
        g = g * (target / float(g.norm()))
        ref.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_([ref], 1.0)
        assert abs(R.grad_norm(g) - float(total)) <= 1e-12 * float(total)
        clipped += float(total) > 1.0
        opt.step()
        ema_t.mul_(DECAY).add_(ref.detach(), alpha=1.0 - DECAY)
        p, m, v, ema = R.adam_step(p, g, m, v, ema, LR, B1, B2, EPS, t, R.grad_norm(g), 1.0, DECAY, 1.0)
        st = opt.state[ref]
        assert _rel(p, ref.detach()) <= 1e-12 and _rel(m, st["exp_avg"]) <= 1e-12 and _rel(v, st["exp_avg_sq"]) <= 1e-12 and _rel(ema, ema_t) <= 1e-12, t
    assert 0 < clipped < 20
    # grad_scale: sums of 8 ranks with grad_scale = 1/8 are the mean; norm = None and max_norm = 0 both switch the clip off
    g = torch.randn(n, dtype=torch.float64, generator=gen) * 3
    a = R.adam_step(p, g * 8, m, v, ema, LR, B1, B2, EPS, 21, R.grad_norm(g * 8), 1.0, DECAY, 1.0 / 8)
    b = R.adam_step(p, g, m, v, ema, LR, B1, B2, EPS, 21, R.grad_norm(g), 1.0, DECAY, 1.0)
    assert all(_rel(x, y) <= 1e-12 for x, y in zip(a, b))
    c = R.adam_step(p, g, m, v, None, LR, B1, B2, EPS, 21, None, 1.0, DECAY, 1.0)
    d = R.adam_step(p, g, m, v, None, LR, B1, B2, EPS, 21, R.grad_norm(g), 0.0, DECAY, 1.0)
    assert c[3] is None and torch.equal(c[0], d[0]) and not torch.equal(c[0], b[0])


@pytest.mark.parametrize("interval", [1, 3])
def test_amp_state_machine_matches_torch_gradscaler(interval):
    """scale trajectory and parameters against torch.amp.GradScaler("cpu") around torch.optim.Adam: inf gradients at chosen steps (two
    in a row, one right after a growth), growth after `interval` finite steps, skipped steps not counted by the bias correction"""
    n, S0 = 257, 1024.0
    bad_steps = {2, 3, 7, 11}
    gen = torch.Generator().manual_seed(1)
    p0 = torch.randn(n, dtype=torch.float64, generator=gen) * 0.05
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=LR, betas=(B1, B2), eps=EPS, foreach=False)
    scaler = torch.amp.GradScaler("cpu", init_scale=S0, growth_factor=2.0, backoff_factor=0.5, growth_interval=interval)
    scaler.scale(torch.zeros((), dtype=torch.float64))  # (creates the scaler's lazily made state)
    p, m, v = p0.clone(), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    state = R.amp_init(S0)
    taken = 0
    for k in range(14):
        g = torch.randn(n, dtype=torch.float64, generator=gen) * (0.2 if k % 2 else 0.01)
        S = scaler.get_scale()
        assert S == state[R.SCALE], (k, S, state)
        gs = g * S
        if k in bad_steps:
            gs[n - 1] = math.inf if k != 7 else math.nan
        ref.grad = gs.clone()
        scaler.unscale_(opt)
        torch.nn.utils.clip_grad_norm_([ref], 1.0)
        scaler.step(opt)
        scaler.update()
        before = (p, m, v)
        p, m, v, _, state = R.amp_step(p, gs, m, v, None, LR, B1, B2, EPS, R.grad_norm(gs), 1.0, 0.0, 1.0, state, 2.0, 0.5, interval)
        if k in bad_steps:
            assert all(a is b for a, b in zip(before, (p, m, v))) and state[R.FOUND_INF] == 1.0 and state[R.TRACKER] == 0.0
        else:
            taken += 1
        assert state[R.STEPS] == taken and state[R.SKIPPED] == k + 1 - taken
        assert scaler.get_scale() == state[R.SCALE], (k, scaler.get_scale(), state)
        assert _rel(p, ref.detach()) <= 1e-12, k
    assert taken == 10 and float(opt.state[ref]["step"]) == 10.0
    # what GradScaler does not have: the back-off stops at 2^-14, and a scale whose reciprocal is not finite skips the step
    st = R.amp_init(2.0**-14)
    *_, st = R.amp_step(p, g, m, v, None, LR, B1, B2, EPS, math.inf, 1.0, 0.0, 1.0, st, 2.0, 0.5, interval)
    assert st[R.SCALE] == 2.0**-14 and st[R.SKIPPED] == 1.0
    st = R.amp_init(65536.0)
    st[R.SCALE] = 0.0
    q, *_, st = R.amp_step(p, g * 0, m, v, None, LR, B1, B2, EPS, 0.0, 1.0, 0.0, 1.0, st, 2.0, 0.5, interval, round_scalars=True)
    assert q is p and st[R.SCALE] == 2.0**-14 and st[R.STEPS] == 0.0


def small_gradient_case(t, n=4099, seed=0):
    """the regime in which eps decides the update: |g| log-uniform in [1e-10, 1e-6] against eps = 1e-8, no clipping, p = 0, moments
    preloaded with what t - 1 such steps leave (rounded to float32, as a device buffer holds them).  Shared with the GPU module."""
    gen = torch.Generator().manual_seed(seed)
    m, v = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    p = torch.zeros(n, dtype=torch.float64)

    def draw():
        mag = 10.0 ** (-10.0 + 4.0 * torch.rand(n, dtype=torch.float64, generator=gen))
        sign = torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0).double()
        return (mag * sign).float()

    for k in range(1, t):
        _, m, v, _ = R.adam_step(p, draw(), m, v, None, LR, B1, B2, EPS, k, None, 0.0, 0.0, 1.0, round_scalars=True)
    return torch.zeros(n), draw(), m.float(), v.float()


@pytest.mark.parametrize("t", [1, 2, 3])
def test_both_eps_mutants_sit_ten_bounds_away_in_the_small_gradient_regime(t):
    p, g, m, v = small_gradient_case(t)
    args = (p, g, m, v, None, LR, B1, B2, EPS, t, None, 0.0, 0.0, 1.0)
    want = R.adam_step(*args, round_scalars=True)[0]
    bound = R.adam_step_bounds(*args)["p"]
    assert float(bound.min()) > 0
    for mutant in (R.adam_step_eps_inside_sqrt, R.adam_step_eps_before_bias_correction):
        got = mutant(*args, round_scalars=True)[0]
        ratio = (got - want).abs() / bound
        print(f"t = {t}, {mutant.__name__}: off by {float(ratio.median()):.3g} bounds (median), {float(ratio.min()):.3g} (least), {float(ratio.max()):.3g} (most)")
        assert float(ratio.min()) >= 10.0  # every element, not just the worst
    # the moments do not depend on eps: the mutants must NOT differ there (the check above is about eps and nothing else)
    assert torch.equal(R.adam_step_eps_inside_sqrt(*args, round_scalars=True)[1], R.adam_step(*args, round_scalars=True)[1])


def test_bf16_exchange_restatement_rounds_ties_to_even_and_sums_in_rank_order():
    bits = torch.tensor([0x3F808000, 0x3F818000, 0x3F808001, 0x7F7F7FFF, 0x7F7F8000, 0x00008000, 0x00018000], dtype=torch.int64).to(torch.int32)
    got = R.pack_bf16(bits.view(torch.float32), 8).view(torch.int16).tolist()
    assert got == [0x3F80, 0x3F82, 0x3F81, 0x7F7F, 0x7F80, 0x0000, 0x0002, 0]
    recv = torch.tensor([[256.0, 1.0], [1.0, 256.0], [1.0, 1.0]]).to(torch.bfloat16)
    assert R.shard_reduce_bf16(recv, 1.0).tolist() == [258.0, 258.0]  # one rounding, after the fp32 sum
    assert R.unpack_bf16(recv.reshape(-1), 3).tolist() == [256.0, 1.0, 1.0]


# ---------------------------------------------------------------- what the C ABI refuses before any launch
def _lib():
    from dmme_amd import _lib

    return _lib, _lib.lib()


def test_optimiser_entry_points_refuse_bad_arguments_before_any_launch():
    """null pointers, numel <= 0, step < 1, grad_scale <= 0, bad scaler constants: -1 and the function's name in dmme_last_error().
    Every call returns before its launch, so the (host) pointers are never read."""
    _l, lib = _lib()
    buf = torch.zeros(16)
    ok, null = C.c_void_p(buf.data_ptr()), C.c_void_p(0)

    def refused(rc, name):
        assert rc == -1, (name, rc)
        assert name in lib.dmme_last_error().decode(), (name, lib.dmme_last_error())

    for numel, ptrs in ((0, (ok, ok, ok)), (-1, (ok, ok, ok)), (4, (null, ok, ok)), (4, (ok, null, ok)), (4, (ok, ok, null))):
        refused(lib.dmme_grad_norm(ptrs[0], numel, ptrs[1], ptrs[2], null), "grad_norm")

    def adam(p=ok, g=ok, m=ok, v=ok, numel=4, step=1, grad_scale=1.0):
        return lib.dmme_adam_step(p, g, m, v, null, numel, LR, B1, B2, EPS, step, null, 1.0, DECAY, grad_scale, null)

    for kw in (dict(p=null), dict(g=null), dict(m=null), dict(v=null), dict(numel=0), dict(numel=-5), dict(step=0), dict(step=-1), dict(grad_scale=0.0),
               dict(grad_scale=-1.0), dict(grad_scale=math.nan)):
        refused(adam(**kw), "adam_step")

    def adam_amp(p=ok, g=ok, m=ok, v=ok, norm=ok, amp=ok, numel=4, grad_scale=1.0, growth=2.0, backoff=0.5, interval=2000):
        return lib.dmme_adam_step_amp(p, g, m, v, null, numel, LR, B1, B2, EPS, norm, 1.0, DECAY, grad_scale, amp, growth, backoff, interval, null)

    for kw in (dict(p=null), dict(g=null), dict(m=null), dict(v=null), dict(norm=null), dict(amp=null), dict(numel=0), dict(numel=-1), dict(grad_scale=0.0),
               dict(grad_scale=-0.5), dict(grad_scale=math.nan), dict(growth=0.5), dict(backoff=0.0), dict(backoff=1.5), dict(interval=0), dict(growth=math.nan),
               dict(backoff=math.nan)):
        refused(adam_amp(**kw), "adam_step_amp")
    refused(lib.dmme_amp_init(null, 65536.0, null), "amp_init")
    refused(lib.dmme_amp_init(ok, 0.0, null), "amp_init")
    refused(lib.dmme_amp_init(ok, -1.0, null), "amp_init")
    refused(lib.dmme_amp_scale(null, 4, ok, null), "amp_scale")
    refused(lib.dmme_amp_scale(ok, 4, null, null), "amp_scale")
    refused(lib.dmme_amp_scale(ok, -1, ok, null), "amp_scale")
    for args in ((null, 4, ok, 4), (ok, 4, null, 4), (ok, 0, ok, 4), (ok, 5, ok, 4)):
        refused(lib.dmme_grad_pack_bf16(*args, null), "grad_pack_bf16")
    for args in ((null, 2, 4, 0.5, ok), (ok, 2, 4, 0.5, null), (ok, 0, 4, 0.5, ok), (ok, 2, 0, 0.5, ok)):
        refused(lib.dmme_shard_reduce_bf16(*args, null), "shard_reduce_bf16")
    for args in ((null, 4, ok), (ok, 4, null), (ok, 0, ok)):
        refused(lib.dmme_grad_unpack_bf16(*args, null), "grad_unpack_bf16")


# ---------------------------------------------------------------- device move, host half
LAUNCHING = ("dmme_amp_init", "dmme_amp_scale", "dmme_grad_norm", "dmme_adam_step", "dmme_adam_step_amp", "dmme_unet_pack_params")


class _NoLaunch:
    """the library with its launching optimiser entry points replaced by an assertion"""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        if name in LAUNCHING:
            raise AssertionError(f"{name} called on a CPU-resident model: a kernel launch on a host pointer")
        return getattr(self._real, name)


def _tiny(precision):
    import dmme_amd

    cfg = O.TINY
    torch.manual_seed(2)
    return dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks, cfg.attention_depths,
                         precision=precision)


def make_checkpoint(opt, step=3, amp=None, seed=5):
    """an optimiser state dict in the package's layout with recognisable moments, EMA weights and (optionally) scaler state"""
    sd = opt.state_dict()
    gen = torch.Generator().manual_seed(seed)
    for i, e in enumerate(sd["ema"]):
        sd["opt"]["state"][i] = {"step": torch.tensor(float(step)), "exp_avg": torch.randn(e.shape, generator=gen) * 1e-3,
                                 "exp_avg_sq": torch.rand(e.shape, generator=gen) * 1e-6}
    sd["ema"] = tuple(torch.randn(e.shape, generator=gen) * 0.05 for e in sd["ema"])
    sd["current_step"] = step
    if amp is not None:
        sd["amp_state"] = [list(amp)]
    return sd


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_state_loads_into_a_cpu_resident_model_without_a_launch(precision, monkeypatch):
    """build on the CPU, load_state_dict, (then .cuda(): tests/test_gpu_optim.py) - the host half: the moments, the EMA copy and the
    loss-scaling state land in host tensors with the checkpoint's values and no kernel is launched; for fp16 that includes the scaler
    state, which used to be made by dmme_amp_init whatever the device - a launch on a host pointer"""
    from dmme_amd import _lib
    from dmme_amd.optim import FusedAdam

    net = _tiny(precision)
    opt = FusedAdam(net.parameters(), lr=LR, max_grad_norm=1.0, ema_decay=DECAY)
    real = _lib.lib()
    monkeypatch.setattr(_lib, "lib", lambda: _NoLaunch(real))
    amp = [1024.0, 1.0, 2.0, 0.0, 1.0, 0.0, 0.0, 0.0] if precision == "fp16" else None
    if precision == "fp16":  # first use on the CPU: a host tensor holding the initial scale
        fresh = net.amp_state()
        assert fresh.device.type == "cpu" and fresh.tolist() == [65536.0] + [0.0] * 7
    else:
        assert net.amp_state() is None
    sd = make_checkpoint(opt, amp=amp)
    opt.load_state_dict(sd)
    st = opt._flat_state[id(net)]
    assert all(st[k].device.type == "cpu" for k in ("m", "v", "ema"))
    assert opt._step_count == 3
    for i, (_, off, n) in enumerate(opt._param_slices(net)):
        assert torch.equal(st["m"][off : off + n], sd["opt"]["state"][i]["exp_avg"].reshape(-1))
        assert torch.equal(st["v"][off : off + n], sd["opt"]["state"][i]["exp_avg_sq"].reshape(-1))
        assert torch.equal(st["ema"][off : off + n], sd["ema"][i].reshape(-1))
    if precision == "fp16":
        assert net.amp_state().tolist() == amp and net.amp_state().device.type == "cpu"
        assert opt.state_dict()["amp_state"] == [amp]
        assert opt.loss_scale() == 1024.0
    # the fused pass itself has no CPU form: a step on the CPU-resident model is an error, not a launch
    net.flat_grad()
    with pytest.raises(_lib.DmmeError, match="GPU"):
        opt.step()
