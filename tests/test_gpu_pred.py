"""-m gpu: x0- and v-prediction networks on the MI355X - the adapter kernel dmme_pred_to_eps, the targets of dmme_q_sample_pred and the
weighted loss dmme_mse_loss_rows against the numpy restatement tests/pred_ref.py (bit for bit where both sides are float32), the eager
sampling steps, every captured chain entry point against its eager loop, two processes of different prediction over one plan, a
training step and the trainer.

The networks are the tiny golden UNets of the other chain tests (tests/test_gpu_chain.py, test_gpu_cond.py, test_gpu_guidance.py) with
their seeded weights read as x0 / v predictors: what is held here is the arithmetic around the network, not sample quality."""

import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import classifier_ref as CLR
from . import cond_ref as CR
from . import pred_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SHAPE = (2, 3, 32, 32)
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
PREDS = [R.X0, R.V]
LOSS_RTOL = 1e-5          # tests/test_gpu_unet.py:232 - dmme_mse_loss against the float64 mean, the same two-stage reduction
GRAD_RTOL = 4 * 2.0**-24  # three fp32 roundings per element: the difference, the row scalar, the product


def _tiny(seed=11):
    import dmme_amd

    net = dmme_amd.UNet(dropout=0.0, **TINY_KW)
    net.load_state_dict(O.make_state_dict(dataclasses.replace(O.TINY, dropout=0.0), seed), strict=True)
    return net.to(DEV).eval()


def _cond(seed=51, K=3):
    import dmme_amd

    net = dmme_amd.ConditionalUNet(num_classes=K, dropout=0.0, **TINY_KW)
    net.load_state_dict(CR.make_state_dict(CR.TINY, K, seed), strict=True)
    return net.to(DEV).eval()


def _classifier(seed=22, K=10):
    import dmme_amd

    clf = dmme_amd.EncoderClassifier(num_classes=K, **TINY_KW)
    clf.load_state_dict(CLR.make_state_dict(CLR.TINY, K, seed))
    return clf.to(DEV).eval()


def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def tables():
    """the linear T = 1000 schedule as a process holds it: float64 alpha_bar (the fp32 buffer, widened), the fp32 adapter tables of
    pred_ref, and the process's own fp32 sqrt tables (host copies and device tensors); computed once and left unchanged"""
    import dmme_amd

    p = dmme_amd.DDPM(torch.nn.Identity(), 1000)
    ab = p.alpha_bar.reshape(-1).double().numpy()
    out = {"T": 1000, "ab64": ab, "sa": p._sqrt_alpha_bar.numpy().copy(), "sd": p._sqrt_one_minus_alpha_bar.numpy().copy()}
    for pred in PREDS:
        out[pred] = R.ab_table(ab, pred).astype(np.float32)
        out[pred, "dev"] = torch.from_numpy(out[pred]).reshape(-1).contiguous().to(DEV)
    out["sa_dev"], out["sd_dev"] = p._sqrt_alpha_bar.to(DEV), p._sqrt_one_minus_alpha_bar.to(DEV)
    return out


def _pred_to_eps(code, out, x, tab_dev, T, t):
    from dmme_amd import _lib

    B = out.shape[0]
    return _lib.lib().dmme_pred_to_eps(code, _lib.ptr(out), _lib.ptr(x), _lib.ptr(tab_dev), T, _lib.ptr(t), t.numel(), B, out[0].numel(), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------ 1. the adapter kernel
# chw = 5: the element-by-element form; 192: quads, one block; 3 * 512 * 512 at B = 3: 2.36 M elements = 589824 quads, more than one sweep of
# the grid's 2048 x 256 threads, so the stride loop runs
@pytest.mark.parametrize("B,chw", [(2, 5), (2, 192), (3, 3 * 512 * 512)])
@pytest.mark.parametrize("rows", [True, False], ids=["t_len=B", "t_len=1"])
@pytest.mark.parametrize("pred", PREDS)
def test_pred_to_eps_bit_exact(tables, pred, rows, B, chw):
    from dmme_amd import _lib

    T, code = tables["T"], _lib.PREDICTIONS[pred]
    out, x = synth.normal(1, (B, chw)), synth.normal(2, (B, chw))
    cases = [[1, T, 417][:B]] if rows else [[1], [T]]  # (rows at t = 1 and t = T either way)
    for t in cases:
        got = out.clone().to(DEV)
        td = torch.tensor(t, dtype=torch.int64, device=DEV)
        assert _pred_to_eps(code, got, x.to(DEV), tables[pred, "dev"], T, td) == 0
        want = R.to_eps(tables[pred], out.numpy(), x.numpy(), t)
        assert want.dtype == np.float32 and np.isfinite(want).all()
        assert _same_bits(got, want), (pred, t)


def test_pred_to_eps_refusals_and_loud_misuse(tables):
    from dmme_amd import _lib

    T = tables["T"]
    out, x = synth.normal(3, (2, 192)).to(DEV), synth.normal(4, (2, 192)).to(DEV)
    t = torch.tensor([5], dtype=torch.int64, device=DEV)
    keep = out.clone()
    assert _pred_to_eps(_lib.PRED_EPS, out, x, tables[R.V, "dev"], T, t) == -1  # DMME_ERR_INVALID: the caller simply does not launch
    assert b"pred_to_eps" in _lib.lib().dmme_last_error()
    assert _pred_to_eps(_lib.PRED_V, out, x, tables[R.V, "dev"], T, torch.tensor([1, 2, 3], dtype=torch.int64, device=DEV)) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, keep)
    # index 0 of an x0 table and a timestep outside the table: NaN, never a read outside it
    for pred, tt in ((R.X0, [0, 7]), (R.V, [T + 1, 7]), (R.V, [-1, 7])):
        got = keep.clone()
        assert _pred_to_eps(_lib.PREDICTIONS[pred], got, x, tables[pred, "dev"], T, torch.tensor(tt, dtype=torch.int64, device=DEV)) == 0
        assert bool(torch.isnan(got[0]).all()) and _same_bits(got[1], R.to_eps(tables[pred], keep[1:].cpu().numpy(), x[1:].cpu().numpy(), [7])[0])


# ------------------------------------------------------------------------------------------ 2. forward noising with a target
def test_q_sample_pred_targets(tables):
    from dmme_amd import _lib

    lib, B, chw = _lib.lib(), 3, 192
    x0, z = synth.uniform(5, (B, chw)), synth.normal(6, (B, chw))
    t = [1, 500, 1000]
    td = torch.tensor(t, dtype=torch.int64, device=DEV)
    x0d, zd = x0.to(DEV), z.to(DEV)
    xt_ref, tg_ref = torch.empty_like(x0d), torch.empty_like(x0d)
    _lib.check(lib.dmme_q_sample(_lib.ptr(x0d), _lib.ptr(zd), _lib.ptr(tables["sa_dev"]), _lib.ptr(tables["sd_dev"]), _lib.ptr(td), B, chw, _lib.ptr(xt_ref), _lib.ptr(tg_ref),
                                 _lib.stream_ptr()))
    for pred in ("eps", R.X0, R.V):
        x_t, tg = torch.full_like(x0d, float("nan")), torch.full_like(x0d, float("nan"))
        _lib.check(lib.dmme_q_sample_pred(_lib.PREDICTIONS[pred], _lib.ptr(x0d), _lib.ptr(zd), _lib.ptr(tables["sa_dev"]), _lib.ptr(tables["sd_dev"]), _lib.ptr(td), B, chw,
                                          _lib.ptr(x_t), _lib.ptr(tg), _lib.stream_ptr()))
        assert _same_bits(x_t, xt_ref), pred
        assert _same_bits(x_t, R.q_sample(tables["sa"], tables["sd"], x0.numpy(), z.numpy(), t)), pred
        want = tg_ref if pred == "eps" else x0 if pred == R.X0 else R.target(R.V, tables["sa"], tables["sd"], x0.numpy(), z.numpy(), t)
        assert _same_bits(tg, want), pred
        only_x = torch.empty_like(x0d)  # target is optional
        _lib.check(lib.dmme_q_sample_pred(_lib.PREDICTIONS[pred], _lib.ptr(x0d), _lib.ptr(zd), _lib.ptr(tables["sa_dev"]), _lib.ptr(tables["sd_dev"]), _lib.ptr(td), B, chw,
                                          _lib.ptr(only_x), None, _lib.stream_ptr()))
        assert _same_bits(only_x, xt_ref)
    assert lib.dmme_q_sample_pred(3, _lib.ptr(x0d), _lib.ptr(zd), _lib.ptr(tables["sa_dev"]), _lib.ptr(tables["sd_dev"]), _lib.ptr(td), B, chw, _lib.ptr(xt_ref), None,
                                  _lib.stream_ptr()) == -1


# ------------------------------------------------------------------------------------------ 3. the weighted loss
# chw = 5: one partial block per image; 3072: three blocks per image; 70000: the 64-block cap, a stride loop inside the image
@pytest.mark.parametrize("chw", [5, 3 * 32 * 32, 70000])
def test_weighted_mse_loss_and_gradient(tables, chw):
    from dmme_amd import _lib
    from dmme_amd.autograd import weighted_mse_loss_apply

    B, t = 3, [1, 300, 1000]
    w32 = R.weight_table(tables["ab64"], R.V, 5.0).astype(np.float32)
    out, tg = synth.normal(7, (B, chw)), synth.normal(8, (B, chw))
    want_loss, want_grad = R.weighted_loss(out.numpy(), tg.numpy(), w32, t)
    o = out.to(DEV).requires_grad_(True)
    loss = weighted_mse_loss_apply(o, tg.to(DEV), torch.from_numpy(w32), torch.tensor(t))
    loss.backward()
    err = np.abs(o.grad.double().cpu().numpy() - want_grad)
    print(f"chw {chw}: loss {loss.item():.8e} vs float64 {want_loss:.8e} (rel {abs(loss.item() / want_loss - 1):.2e}, bound {LOSS_RTOL:.0e}); "
          f"worst gradient error {float((err / np.abs(want_grad).clip(1e-300)).max()):.3e} relative (bound {GRAD_RTOL:.3e})")
    np.testing.assert_allclose(loss.item(), want_loss, rtol=LOSS_RTOL)
    assert (err <= GRAD_RTOL * np.abs(want_grad)).all()
    # the entry point itself with a loss scale: the gradient scales, the loss does not; without d_out only the loss
    lib = _lib.lib()
    l2, d2 = torch.empty(1, device=DEV), torch.empty((B, chw), device=DEV)
    scratch = torch.empty(64 * B, device=DEV)
    wd, td, od, tgd = torch.from_numpy(w32).to(DEV), torch.tensor(t, device=DEV), out.to(DEV), tg.to(DEV)
    _lib.check(lib.dmme_mse_loss_rows(_lib.ptr(od), _lib.ptr(tgd), _lib.ptr(wd), _lib.ptr(td), B, chw, _lib.ptr(l2), _lib.ptr(d2), 1024.0, _lib.ptr(scratch), _lib.stream_ptr()))
    assert l2.item() == loss.item()
    _, want_scaled = R.weighted_loss(out.numpy(), tg.numpy(), w32, t, 1024.0)
    assert (np.abs(d2.double().cpu().numpy() - want_scaled) <= GRAD_RTOL * np.abs(want_scaled)).all()
    l3 = torch.empty(1, device=DEV)
    _lib.check(lib.dmme_mse_loss_rows(_lib.ptr(od), _lib.ptr(tgd), _lib.ptr(wd), _lib.ptr(td), B, chw, _lib.ptr(l3), None, 1.0, _lib.ptr(scratch), _lib.stream_ptr()))
    assert l3.item() == loss.item()
    with pytest.raises(ValueError):
        weighted_mse_loss_apply(o, tg.to(DEV), torch.from_numpy(w32), torch.tensor([1, 2, 1001]))


# ------------------------------------------------------------------------------------------ 4. the eager step
@pytest.mark.parametrize("pred", PREDS)
def test_eager_sampling_step_is_the_eps_update_on_the_converted_output(pred):
    """P(prediction=p).sampling_step against: the shared network's raw output, converted on the host by pred_ref, through the eps
    process's own update - bit for bit, for DDPM and for the paper-form DDIM at eta = 0.5"""
    import dmme_amd

    net = _tiny()
    x, z = synth.normal(9, SHAPE).to(DEV), synth.normal(10, SHAPE).to(DEV)

    def converted(proc, t):
        with torch.no_grad():
            raw = net(x, torch.tensor([t], device=DEV)).float()
        tab = R.ab_table(proc.alpha_bar.reshape(-1).double().cpu().numpy(), pred).astype(np.float32)
        return raw, torch.from_numpy(R.to_eps(tab, raw.cpu().numpy(), x.cpu().numpy(), [t])).to(DEV)

    T = 100
    proc, plain = dmme_amd.DDPM(net, T, prediction=pred).to(DEV), dmme_amd.DDPM(net, T).to(DEV)
    for t in (T, 17, 1):
        got = proc.sampling_step(x, torch.tensor([t], device=DEV), z)
        raw, e = converted(plain, t)
        with torch.no_grad():
            assert torch.equal(proc(x, torch.tensor([t], device=DEV)).float(), raw)  # forward stays the raw output
        want = plain._reverse_update(x.clone(), e, t, z)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (pred, t)
        assert not torch.equal(got, plain.sampling_step(x, torch.tensor([t], device=DEV), z))
    S = 10
    proc, plain = dmme_amd.GeneralizedDDIM(net, T, S, eta=0.5, prediction=pred).to(DEV), dmme_amd.GeneralizedDDIM(net, T, S, eta=0.5).to(DEV)
    for i in (S, 2, 1):
        got = proc.sampling_step(x, torch.tensor([i], device=DEV), z)
        _, e = converted(plain, int(plain.tau[i]))
        want = plain._gddim_update(x.clone(), e, plain._rev_rows[i], z, plain._draws)
        assert torch.equal(got, want) and bool(torch.isfinite(got).all()), (pred, i)


# ------------------------------------------------------------------------------------------ 5. captured chains against eager loops
def _graph_ran(runner):
    assert runner.capture_error is None and runner.graph is not None


def _chain_ddpm(pred):
    import dmme_amd

    net, T = _tiny(), 8
    proc = dmme_amd.DDPM(net, T, prediction=pred).to(DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE)
    _graph_ran(proc._runner)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    with torch.no_grad():
        for t in range(T, 0, -1):
            proc._reverse_update(x, proc._eps(x, proc.timestep_tensor(t, DEV)), t, None)
    torch.manual_seed(7)
    assert not torch.equal(got, dmme_amd.DDPM(net, T).to(DEV).generate(SHAPE))
    return got, x


def _chain_cfg_ddpm(pred, s=2.5):
    import dmme_amd

    proc = dmme_amd.ClassifierFreeDDPM(_cond(), 8, guidance_scale=s, prediction=pred).to(DEV)
    y = torch.tensor([2, 0])
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._cfg_runner)
    assert proc._cfg_runner.plan.B == (2 if s == 1.0 else 4)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    for t in range(8, 0, -1):
        x = proc.sampling_step(x, torch.tensor([t], device=DEV), y)
    return got, x


def _chain_dpmpp(pred):
    import dmme_amd

    proc = dmme_amd.DPMSolverPP(_tiny(), 100, 5, prediction=pred).to(DEV)
    xT = synth.normal(12, SHAPE).to(DEV)
    got = proc.decode(xT)
    _graph_ran(proc._runner)
    with torch.no_grad():
        return got, proc._eager_chain(xT.clone(), proc.n_steps)


def _chain_cfg_dpmpp(pred):
    import dmme_amd

    proc = dmme_amd.ClassifierFreeDPMSolver(_cond(), 100, 5, guidance_scale=2.5, prediction=pred).to(DEV)
    y = torch.tensor([1, 2])
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._cfg_runner)
    torch.manual_seed(7)
    return got, proc._eager_generate(dmme_amd.gaussian(SHAPE, device=DEV), y)


def _chain_repaint(pred):
    import dmme_amd

    proc = dmme_amd.RePaint(_tiny(), 100, 4, 2, 2, prediction=pred).to(DEV)
    assert proc.n_rows == 6
    x0 = synth.uniform(13, SHAPE).to(DEV)
    m = torch.zeros(SHAPE, device=DEV)
    m[..., :16] = 1.0
    torch.manual_seed(7)
    got = proc.inpaint(x0, m)
    _graph_ran(proc._runner)
    assert torch.equal(got[m.bool()], x0[m.bool()])
    torch.manual_seed(7)
    with torch.no_grad():
        return got, proc._eager_chain(dmme_amd.gaussian(SHAPE, device=DEV), x0, m)


def _chain_guided_ddim(pred):
    import dmme_amd

    proc = dmme_amd.ClassifierGuidedDDIM(_tiny(21), _classifier(), 100, 6, guidance_scale=3.0, prediction=pred).to(DEV)
    y = torch.tensor([9, 3], device=DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._grunner)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    for i in range(6, 0, -1):
        x = proc.sampling_step(x, torch.tensor([i], device=DEV), y)
    return got, x


CHAINS = {"ddpm": _chain_ddpm, "cfg-ddpm": _chain_cfg_ddpm, "cfg-ddpm-s1": lambda p: _chain_cfg_ddpm(p, 1.0), "dpm++": _chain_dpmpp, "cfg-dpm++": _chain_cfg_dpmpp,
          "repaint": _chain_repaint, "guided-ddim": _chain_guided_ddim}


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("chain", list(CHAINS))
def test_captured_chain_equals_eager_loop(chain, pred):
    """one case per chain entry point (dmme_chain_step, dmme_cfg_chain_step, dmme_dpmpp_chain_step, dmme_cfg_dpmpp_chain_step,
    dmme_repaint_chain_step, dmme_guided_chain_step) and the classifier-free s = 1 path, which launches the adapter from the runner: the
    replayed graph, with the adapter inside the step, against the host loop through `_eps` under one seed - the same bits; 8 steps at most"""
    got, want = CHAINS[chain](pred)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


# ------------------------------------------------------------------------------------------ 6. one plan, two predictions
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager-launches"])
def test_processes_of_different_prediction_share_a_plan(use_graph):
    """a v process and an eps process over ONE network (one plan): chains run alternately v, eps, v.  The eps chain equals that of an eps
    process over a fresh copy of the network, and the two v chains under one seed equal each other - as replayed graphs, and as per-step
    launches, where only the runner's set-prediction call in front of every step keeps them apart"""
    import dmme_amd

    T, net = 6, _tiny()
    pv, pe = dmme_amd.DDPM(net, T, prediction="v").to(DEV), dmme_amd.DDPM(net, T).to(DEV)
    fresh = dmme_amd.DDPM(_tiny(), T).to(DEV)
    xT = synth.normal(14, SHAPE).to(DEV)
    runners = {}

    def chain(proc):
        r = runners.get(proc)
        if r is None:
            r = runners[proc] = proc.chain_runner(torch.empty(SHAPE, device=DEV), use_graph=use_graph)
        r.x.copy_(xT)
        torch.manual_seed(5)
        out = r.run(T, T).clone()
        assert (r.graph is not None and r.capture_error is None) == use_graph
        return out

    a, b, c = chain(pv), chain(pe), chain(pv)
    assert runners[pv].plan is runners[pe].plan
    assert torch.equal(b, chain(fresh)) and torch.equal(a, c) and not torch.equal(a, b)
    assert bool(torch.isfinite(a).all())


def test_plan_refuses_a_prediction_it_cannot_convert():
    """an x0 / v process over a network with two output planes (an Improved DDPM UNet): DMME_ERR_UNSUPPORTED from the plan, not a chain"""
    import dmme_amd
    from dmme_amd import _lib
    from dmme_amd.models import iddpm as iddpm_models

    inet = iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,)).to(DEV).eval()
    plan = inet._plan_for(2, 32, 32, DEV)
    tab = torch.zeros(2 * 11, device=DEV)
    assert _lib.lib().dmme_unet_plan_set_prediction(plan.h, _lib.PRED_V, _lib.ptr(tab), 10) == -2
    assert _lib.lib().dmme_unet_plan_set_prediction(plan.h, 3, _lib.ptr(tab), 10) == -1
    assert _lib.lib().dmme_unet_plan_set_prediction(plan.h, _lib.PRED_EPS, None, 0) == 0
    proc = dmme_amd.RePaint(inet, 10, 4, 2, 2, prediction="v").to(DEV)
    with pytest.raises(NotImplementedError):
        proc.generate(SHAPE)


# ------------------------------------------------------------------------------------------ 7. a training step
def test_training_step_v_prediction_min_snr():
    import dmme_amd

    B, T, net = 3, 1000, _tiny()
    proc = dmme_amd.DDPM(net, T, prediction="v", loss_weight="min-snr").to(DEV)
    shape = (B,) + SHAPE[1:]
    x0, z = synth.uniform(15, shape), synth.normal(16, shape)
    t = [1, 412, 999]
    loss = proc.training_step(x0.to(DEV), t=torch.tensor(t, device=DEV), noise=z.to(DEV))
    loss.backward()
    g = net.flat_grad()
    assert bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0
    # the reference from the raw network output at the same x_t
    ab = proc.alpha_bar.reshape(-1).double().cpu().numpy()
    sa, sd = proc._sqrt_alpha_bar.cpu().numpy(), proc._sqrt_one_minus_alpha_bar.cpu().numpy()
    x_t = R.q_sample(sa, sd, x0.numpy(), z.numpy(), t)
    with torch.no_grad():
        raw = net(torch.from_numpy(x_t).to(DEV), torch.tensor(t, device=DEV)).float().cpu().numpy()
    want, _ = R.weighted_loss(raw, R.target(R.V, sa, sd, x0.numpy(), z.numpy(), t), R.weight_table(ab, R.V, 5.0).astype(np.float32), t)
    print(f"training_step v / min-snr: loss {loss.item():.8e} vs float64 {want:.8e} (rel {abs(loss.item() / want - 1):.2e}, bound {LOSS_RTOL:.0e})")
    np.testing.assert_allclose(loss.item(), want, rtol=LOSS_RTOL)
    # uniform weights over the same target: the unweighted mean
    flat = dmme_amd.DDPM(net, T, prediction="v").to(DEV)
    with torch.no_grad():
        l1 = flat.training_step(x0.to(DEV), t=torch.tensor(t, device=DEV), noise=z.to(DEV))
    want1, _ = R.weighted_loss(raw, R.target(R.V, sa, sd, x0.numpy(), z.numpy(), t), np.ones(T + 1), t)
    np.testing.assert_allclose(l1.item(), want1, rtol=LOSS_RTOL)


# ------------------------------------------------------------------------------------------ 8. the trainer
def test_trainer_samples_the_v_config_with_dpm_solver(tmp_path, capsys):
    import json

    from dmme_amd import trainer

    outs = {}
    for name, extra in (("v", []), ("eps", ["--prediction", "eps"])):
        path = str(tmp_path / f"{name}.npy")
        rc = trainer.main(["sample", "--config", os.path.join(ROOT, "configs", "vpred", "cifar10.yaml"), "--sampler", "dpm++", "--sample-steps", "4", "--num-images", "2",
                           "--save", path] + extra)
        line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
        assert rc == 0 and line["images"] == [2, 3, 32, 32] and line["finite"] is True
        outs[name] = np.load(path)
        assert outs[name].shape == (2, 3, 32, 32) and np.isfinite(outs[name]).all()
    assert not np.array_equal(outs["v"], outs["eps"])
