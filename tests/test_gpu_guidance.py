"""Classifier guidance on the MI355X: the classifier's logits and input gradient against the CPU restatement (tests/classifier_ref.py),
the input-only backward, one training step, the guided DDPM / DDIM updates, and the captured guided chain."""

import dataclasses

import numpy as np
import pytest
import torch

import dmme_amd
from dmme_amd import _lib
from oracle import synth
from oracle import unet as O

from . import classifier_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
DEF_KW = {}


def _kw(cfg):
    return TINY_KW if cfg == R.TINY else DEF_KW


def _classifier(cfg, K, seed, precision="fp32"):
    sd = R.make_state_dict(cfg, K, seed)
    clf = dmme_amd.EncoderClassifier(precision=precision, num_classes=K, **_kw(cfg))
    clf.load_state_dict(sd)
    return clf.to(DEV).eval(), sd


def _inputs(B, seed, tmax=1000):
    x = synth.normal(seed, (B, 3, 32, 32))
    t = torch.from_numpy(np.random.RandomState(seed).randint(1, tmax, size=B)).to(torch.int64)
    return x, t


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max() / b.double().abs().max().clamp_min(1e-30))


@pytest.mark.parametrize("cfg,tol", [(R.TINY, 2e-5), (R.DEFAULT, 2e-4)], ids=["tiny", "default"])
def test_logits_fp32(cfg, tol):
    clf, sd = _classifier(cfg, 10, 11)
    x, t = _inputs(4, 5)
    with torch.no_grad():
        got = clf(x.to(DEV), t.to(DEV))
    ref = R.classifier_forward(sd, cfg, x, t.float())
    assert got.shape == (4, 10)
    err = _rel(got, ref)
    print(f"classifier logits fp32 rel err {err:.3e}")
    assert err <= tol


@pytest.mark.parametrize("precision,bound", [("bf16", 6e-2), ("fp16", 1e-2)])
def test_logits_16bit(precision, bound):
    clf, sd = _classifier(R.DEFAULT, 10, 12, precision)
    x, t = _inputs(8, 6)
    with torch.no_grad():
        got = clf(x.to(DEV), t.to(DEV))
    err = _rel(got, R.classifier_forward(sd, R.DEFAULT, x, t.float()))
    print(f"classifier logits {precision} rel err {err:.3e} (bound {bound})")
    assert err <= bound


def _ref_input_grad(sd, cfg, x, t, y):
    xr = x.clone().requires_grad_(True)
    R.log_prob_sum(R.classifier_forward(sd, cfg, xr, t.float()), y).backward()
    return xr.grad


@pytest.mark.parametrize("cfg,precision,tol", [(R.TINY, "fp32", 2e-5), (R.DEFAULT, "fp32", 2e-4), (R.DEFAULT, "bf16", 3e-2)],
                         ids=["tiny-fp32", "default-fp32", "default-bf16"])
def test_input_gradient(cfg, precision, tol):
    """tolerances of tests/test_gpu_chain.py's input-gradient test (relative to the gradient's max); bf16 measured 2.9e-2 here"""
    K = 10
    clf, sd = _classifier(cfg, K, 13, precision)
    x, t = _inputs(6, 7)
    y = torch.tensor([3, 0, 9, 5, 1, 7])  # distinct labels: any mixing across the batch shows
    got = clf.input_grad(x.to(DEV), t.to(DEV), y.to(DEV))
    ref = _ref_input_grad(sd, cfg, x, t, y)
    err = _rel(got, ref)
    print(f"classifier input gradient {precision} rel err {err:.3e}")
    assert err <= tol
    # the B x B mixing of the reference sketch (every label's gradient summed into every image) differs from the row-wise one
    xr = x.clone().requires_grad_(True)
    torch.log_softmax(R.classifier_forward(sd, cfg, xr, t.float()), 1)[:, y].sum().backward()
    assert _rel(xr.grad, ref) > 10 * tol


def test_input_only_backward():
    clf, sd = _classifier(R.TINY, 10, 14)
    x, t = _inputs(4, 8)
    xd, td = x.to(DEV), t.to(DEV)
    dlog = torch.randn(4, 10, generator=torch.Generator().manual_seed(0)).to(DEV)
    g = clf.flat_grad()
    g.copy_(torch.randn(g.numel(), generator=torch.Generator().manual_seed(1)).to(DEV))
    before = g.clone()
    _, saved = clf._forward_impl(xd, td, want_ctx=True)
    dx_in = clf._backward_input_impl(saved, dlog)
    torch.cuda.synchronize()
    assert torch.equal(g, before)  # grad_flat bit-untouched
    _, saved = clf._forward_impl(xd, td, want_ctx=True)
    dx_full = clf._backward_impl(saved, dlog, want_dx=True)
    assert not torch.equal(g, before)
    torch.testing.assert_close(dx_in, dx_full, rtol=1e-5, atol=1e-7 * float(dx_full.abs().max()))


def test_classifier_training_step():
    cfg, K = R.TINY, 10
    clf, sd = _classifier(cfg, K, 15)
    clf.train()
    ddpm = dmme_amd.DDPM(dmme_amd.UNet(**TINY_KW), timesteps=1000).to(DEV)
    x0, _ = _inputs(8, 9)
    noise = synth.normal(10, (8, 3, 32, 32))
    t = torch.tensor([1, 50, 200, 400, 600, 800, 950, 999])
    y = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7])
    clf.zero_grad(set_to_none=True)
    loss = dmme_amd.classifier_loss(clf, ddpm, x0.to(DEV), y.to(DEV), t=t.to(DEV), noise=noise.to(DEV))
    loss.backward()
    # restatement: the same noising and the same network in torch autograd
    ab = ddpm.alpha_bar.reshape(-1).cpu().float()
    x_t = ab.sqrt()[t].view(-1, 1, 1, 1) * x0 + (1 - ab).sqrt()[t].view(-1, 1, 1, 1) * noise
    sdr = {k: v.clone().requires_grad_(not k.endswith("embeddings")) for k, v in sd.items()}
    ref_loss = torch.nn.functional.cross_entropy(R.classifier_forward(sdr, cfg, x_t, t.float()), y)
    ref_loss.backward()
    assert abs(float(loss.detach()) - float(ref_loss)) <= 1e-4 * abs(float(ref_loss))
    params = dict(clf.named_parameters())
    for k, v in sdr.items():
        if v.grad is None:
            continue
        got = params[k].grad.detach().cpu()
        scale = float(v.grad.abs().max())
        torch.testing.assert_close(got, v.grad, rtol=1e-4, atol=1e-4 * scale + 1e-12, msg=lambda m, k=k: f"{k}: {m}")
    # a few FusedAdam steps on the fixed noisy batch lower the loss
    from dmme_amd.optim import FusedAdam

    opt = FusedAdam(clf.parameters(), lr=1e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad()
        l = dmme_amd.classifier_loss(clf, ddpm, x0.to(DEV), y.to(DEV), t=t.to(DEV), noise=noise.to(DEV))
        l.backward()
        opt.step()
        losses.append(float(l.detach()))
    print("classifier loss over FusedAdam steps", losses)
    assert losses[-1] < losses[0]


def _tiny_pair(seed=21, K=10):
    unet = dmme_amd.UNet(dropout=0.0, **TINY_KW)
    unet.load_state_dict(O.make_state_dict(dataclasses.replace(O.TINY, dropout=0.0), seed))
    clf, _ = _classifier(R.TINY, K, seed + 1)
    return unet.to(DEV).eval(), clf


def test_guided_steps_match_float64():
    unet, clf = _tiny_pair()
    B = 4
    x, _ = _inputs(B, 30)
    x = x.to(DEV)
    y = torch.tensor([1, 4, 7, 2], device=DEV)
    s = 3.0
    ddpm = dmme_amd.ClassifierGuidedDDPM(unet, clf, timesteps=100, guidance_scale=s).to(DEV)
    z = synth.normal(31, (B, 3, 32, 32)).to(DEV)
    for step in (57, 1):
        t = torch.tensor([step], device=DEV)
        got = ddpm.sampling_step(x, t, y, noise=z)
        with torch.no_grad():
            eps = unet(x, t).double()
        g = clf.input_grad(x, t, y).double()
        beta = float(ddpm.beta.reshape(-1)[step])
        ab = float(ddpm.alpha_bar.reshape(-1)[step])
        mu = (x.double() - beta / np.sqrt(1 - ab) * eps) / np.sqrt(1 - beta)
        want = mu + s * beta * g + (np.sqrt(beta) * z.double() if step != 1 else 0.0)
        assert _rel(got, want) <= 1e-5, step
    ddim = dmme_amd.ClassifierGuidedDDIM(unet, clf, timesteps=100, sub_timesteps=10, guidance_scale=s).to(DEV)
    i = 6
    ti, tp = int(ddim.tau[i]), int(ddim.tau[i - 1])
    got = ddim.sampling_step(x, torch.tensor([i]), y)
    tt = torch.tensor([ti], device=DEV)
    with torch.no_grad():
        eps = unet(x, tt).double()
    g = clf.input_grad(x, tt, y).double()
    ab = ddim.alpha_bar.reshape(-1).double()
    eh = eps - s * float((1 - ab[ti]).sqrt()) * g
    want = float(ab[tp].sqrt()) * ((x.double() - float((1 - ab[ti]).sqrt()) * eh) / float(ab[tp].sqrt()))
    assert _rel(got, want) <= 1e-5


def test_zero_scale_equals_unguided():
    unet, clf = _tiny_pair()
    y = torch.arange(8, device=DEV) % 10
    for guided, plain, n in (
        (dmme_amd.ClassifierGuidedDDPM(unet, clf, timesteps=12, guidance_scale=0.0), dmme_amd.DDPM(unet, timesteps=12), 12),
        (dmme_amd.ClassifierGuidedDDIM(unet, clf, timesteps=100, sub_timesteps=6, guidance_scale=0.0), dmme_amd.DDIM(unet, timesteps=100, sub_timesteps=6), 6),
    ):
        guided, plain = guided.to(DEV), plain.to(DEV)
        torch.manual_seed(123)
        a = guided.generate((8, 3, 32, 32), y)
        torch.manual_seed(123)
        b = plain.generate((8, 3, 32, 32))
        assert torch.equal(a, b), type(guided).__name__


def test_eager_loop_equals_captured_chain():
    unet, clf = _tiny_pair()
    y = torch.tensor([9, 3, 3, 0, 5, 1, 8, 2], device=DEV)
    T = 8
    ddpm = dmme_amd.ClassifierGuidedDDPM(unet, clf, timesteps=T, guidance_scale=5.0).to(DEV)
    torch.manual_seed(7)
    chain = ddpm.generate((8, 3, 32, 32), y)
    torch.manual_seed(7)
    x = dmme_amd.gaussian((8, 3, 32, 32), device=DEV)
    for t in range(T, 0, -1):
        x = ddpm.sampling_step(x, torch.tensor([t], device=DEV), y)
    assert torch.equal(chain, x)


def test_captured_chain_b128_repeatable():
    unet = dmme_amd.UNet(dropout=0.0, precision="bf16")
    unet.load_state_dict(O.make_state_dict(O.UNetConfig(dropout=0.0), 3))
    clf, _ = _classifier(R.DEFAULT, 10, 4, "bf16")
    ddpm = dmme_amd.ClassifierGuidedDDPM(unet.to(DEV).eval(), clf, timesteps=6, guidance_scale=2.0).to(DEV)
    y = torch.arange(128, device=DEV) % 10
    torch.manual_seed(99)
    a = ddpm.generate((128, 3, 32, 32), y)
    torch.manual_seed(99)
    b = ddpm.generate((128, 3, 32, 32), y)
    assert torch.isfinite(a).all()
    assert torch.equal(a, b)
    assert ddpm._grunner.capture_error is None  # the step really was replayed from a graph


def test_refusals():
    for p in ("fp16r32", "bf16x3"):
        with pytest.raises(_lib.DmmeError):
            dmme_amd.EncoderClassifier(precision=p, **TINY_KW)
    clf, _ = _classifier(R.TINY, 10, 16)
    x, t = _inputs(2, 3)
    with pytest.raises(ValueError):
        clf.input_grad(x.to(DEV), t.to(DEV), torch.tensor([0, 10], device=DEV))
    # the kernel itself never indexes with a bad label: NaN row and the status word, no fault
    logits = torch.randn(3, 10, device=DEV)
    y = torch.tensor([2, -1, 11], device=DEV)
    d = torch.empty_like(logits)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().dmme_log_softmax_grad(_lib.ptr(logits), _lib.ptr(y), 3, 10, 1, 1.0, None, _lib.ptr(d), _lib.ptr(status), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert int(status.item()) == 1
    assert torch.isfinite(d[0]).all() and torch.isnan(d[1:]).all()
