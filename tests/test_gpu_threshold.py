"""GPU: x0 thresholding (csrc/threshold.hip) - the stage against its float32 numpy restatement bit for bit (static, dynamic; the LDS
form, the streaming form and the boundary between them; two planes; two classifier-free halves), the two forms against each other, the
refusals, every captured chain entry point against its eager loop with thresholding on, off meaning off, the effect on a DDPM chain,
and the trainer's flag."""

import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import classifier_ref as CLR
from . import cond_ref as CR
from . import threshold_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
SHAPE = (2, 3, 32, 32)
TINY_KW = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
T = 1000
PERCENTILES = (0.5, 0.995, 1.0)


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


def _same(got, want):
    """the same bits, NaN standing for NaN"""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    got, want = np.ascontiguousarray(got, dtype=np.float32).reshape(-1), np.ascontiguousarray(want, dtype=np.float32).reshape(-1)
    ng, nw = np.isnan(got), np.isnan(want)
    return got.shape == want.shape and np.array_equal(ng, nw) and np.array_equal(got.view(np.uint32)[~ng], want.view(np.uint32)[~nw])


@pytest.fixture(scope="module")
def tables():
    """the linear T = 1000 schedule's thresholding table as a process holds it; computed once and left unchanged"""
    import dmme_amd
    from dmme_amd import _lib

    p = dmme_amd.DDPM(torch.nn.Identity(), T, threshold="static")
    ab = p.alpha_bar.reshape(-1).double().numpy()
    t32 = R.table32(ab)
    assert np.array_equal(p._thr_tab.numpy().reshape(-1, 4), t32, equal_nan=True)
    cap = int(_lib.lib().dmme_x0_threshold_lds_capacity())
    assert cap >= 3 * 64 * 64 and cap % 4 == 0
    return {"ab64": ab, "t64": R.table64(ab), "t32": t32, "dev": torch.from_numpy(t32).reshape(-1).contiguous().to(DEV), "cap": cap}


def _threshold(mode, out, x, tab_dev, t, p=None, planes=1, halves=1, sg=1.0, k=None, frac=None, scratch="auto"):
    from dmme_amd import _lib

    lib = _lib.lib()
    B, chw = x.shape[0], x[0].numel()
    if k is None:
        k, frac = R.rank(p, chw) if mode == R.DYNAMIC and p is not None else (0, 0.0)
    if isinstance(scratch, str):
        scratch = torch.empty(max(1, int(lib.dmme_x0_threshold_scratch_bytes(B, chw)) // 4), dtype=torch.int32, device=DEV)
    return lib.dmme_x0_threshold(mode, _lib.ptr(out), _lib.ptr(x), _lib.ptr(tab_dev), T, _lib.ptr(t), t.numel(), B, chw, planes, halves, float(sg), int(k), float(frac),
                                 _lib.ptr(scratch), _lib.stream_ptr())


# ------------------------------------------------------------------------------------------ the inputs: one image per hazard
HAZARDS = [("below", "above", "mixed"), ("ties", "equal", "zeros"), ("nan", "mixed", "above"), ("zeros", "nan", "ties")]  # (B = 2 takes the first two of each)


def _image(kind, chw, row64, rng):
    """(x, e) of one image whose x0 = A x - B e shows the hazard `kind`; x is solved in float64 for the wanted x0 and rounded"""
    A, Bc = row64[0], row64[1]
    e = rng.standard_normal(chw)
    want = {"below": rng.uniform(-0.9, 0.9, chw), "above": 3.0 * rng.standard_normal(chw)}.get(kind, 0.8 * rng.standard_normal(chw))
    x = (want + Bc * e) / A
    if kind == "ties":  # x on a grid of 1/8 and no noise: x0 = fl(A x) takes a few dozen values
        x, e = np.round(rng.standard_normal(chw) * 8.0) / 8.0, np.zeros(chw)
    elif kind == "equal":
        x, e = np.full(chw, 0.5), np.full(chw, 0.25)
    elif kind == "zeros":  # the first half: x = +0, -0, +0 ... and e = +0, so x0 = +0 and -0
        h = max(1, chw // 2)
        x[:h] = np.where(np.arange(h) % 2 == 0, 0.0, -0.0)
        e[:h] = 0.0
    x, e = x.astype(np.float32), e.astype(np.float32)
    if kind == "nan":
        e[chw // 2] = np.nan
    return x, e


_INPUTS = {}


def _inputs(tables, B, chw, group, t):
    key = (B, chw, group, tuple(t))
    if key not in _INPUTS:
        rng = np.random.RandomState(B * 131 + chw % 9973 + group * 17 + len(t))
        kinds = HAZARDS[group][:B]
        xs, es = zip(*[_image(kind, chw, tables["t64"][t[0 if len(t) == 1 else b]], rng) for b, kind in enumerate(kinds)])
        _INPUTS[key] = (kinds, np.stack(xs), np.stack(es))
    return _INPUTS[key]


def _assert_hazards(kinds, info, mode, p, chw, e_in, got):
    """each image shows what it was built for, read off the restatement"""
    big = chw >= 192
    for b, kind in enumerate(kinds):
        x0, s, n = info["x0"][b], info["s"][b], info["touched"][b]
        if kind == "nan":
            assert info["nonfinite"][b] and n >= 1 and (mode == R.STATIC or (n == chw and np.isnan(got[b]).all()))
            continue
        assert not info["nonfinite"][b] and np.isfinite(got[b]).all(), kind  # (a NaN elsewhere in the batch does not spread)
        if kind == "below":
            assert s == 1 and n == 0 and np.array_equal(got[b].view(np.uint32), e_in[b].view(np.uint32))
        elif kind == "above" and big:
            assert n > 0 and (mode == R.STATIC or s > 1)
        elif kind == "mixed" and big and (mode == R.STATIC or p == 0.5):
            assert s == 1 and 0 < n < chw
        elif kind == "ties" and big and mode == R.DYNAMIC and p == 0.5:
            srt = np.sort(np.abs(x0))
            k, frac = R.rank(p, chw)
            assert frac != 0 and srt[k] == srt[k + 1] and len(np.unique(srt)) < chw // 4
        elif kind == "equal":
            assert len(np.unique(np.abs(x0))) == 1
        elif kind == "zeros":
            bits = x0.view(np.uint32)
            assert (bits == 0).any() and (bits == 0x80000000).any()


# ------------------------------------------------------------------------------------------ 1. the kernel against the restatement
def _shapes(cap):
    return [(2, 5), (2, 192), (3, 3072), (2, cap), (2, cap + 4), (2, 3 * 256 * 256)]


@pytest.mark.parametrize("shape", range(6), ids=["elem", "one-block", "cifar", "lds-last", "stream-first", "stream-256x256"])
@pytest.mark.parametrize("rows", [True, False], ids=["t_len=B", "t_len=1"])
@pytest.mark.parametrize("mode", [R.STATIC, R.DYNAMIC], ids=["static", "dynamic"])
def test_threshold_bit_exact(tables, mode, rows, shape):
    B, chw = _shapes(tables["cap"])[shape]
    cases = [[1, T, 417][:B]] if rows else [[1], [T]]  # (rows at t = 1 and t = T either way)
    for t in cases:
        td = torch.tensor(t, dtype=torch.int64, device=DEV)
        for group in range(len(HAZARDS)):
            kinds, x, e = _inputs(tables, B, chw, group, t)
            xd = torch.from_numpy(x).to(DEV)
            for p in PERCENTILES if mode == R.DYNAMIC else (None,):
                got = torch.from_numpy(e).to(DEV)
                assert _threshold(mode, got, xd, tables["dev"], td, p) == 0
                want, info = R.threshold(mode, e, x, tables["t32"], t, p)
                got = got.cpu().numpy()
                assert _same(got, want), (kinds, t, p, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
                _assert_hazards(kinds, info, mode, p, chw, e, got)


@pytest.mark.parametrize("B,chw", [(2, 192), (3, 3072), (2, 7)])
@pytest.mark.parametrize("mode", [R.STATIC, R.DYNAMIC], ids=["static", "dynamic"])
def test_two_planes_leave_the_variance_plane_alone(tables, mode, B, chw):
    """an IDDPM network's [B][2][chw]: the eps plane is the one-plane result, the v plane keeps its bits (chw = 7: unaligned planes)"""
    t = [T, 1, 417][:B]
    td = torch.tensor(t, dtype=torch.int64, device=DEV)
    kinds, x, e = _inputs(tables, B, chw, 0, t)
    v = synth.normal(31, (B, chw)).numpy()
    both = np.concatenate([e, v], axis=1)
    got = torch.from_numpy(both).to(DEV)
    assert _threshold(mode, got, torch.from_numpy(x).to(DEV), tables["dev"], td, 0.995, planes=2) == 0
    want, info = R.threshold(mode, both, x, tables["t32"], t, 0.995, planes=2)
    one, _ = R.threshold(mode, e, x, tables["t32"], t, 0.995)
    got = got.cpu().numpy()
    assert info["touched"].sum() > 0 and _same(got, want) and _same(got[:, :chw], one)
    assert np.array_equal(got[:, chw:].view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("sg", [1.0, 2.5, 0.0])
@pytest.mark.parametrize("B,chw", [(2, 192), (2, 3072), (2, 5)])
@pytest.mark.parametrize("mode", [R.STATIC, R.DYNAMIC], ids=["static", "dynamic"])
def test_two_halves_get_the_thresholded_mix(tables, mode, B, chw, sg):
    """[2B][chw], conditional then unconditional: the x0 of the update's own mix e_u + s_g (e_c - e_u) is what is clipped, e' goes to
    both halves - the update's mix of them returns e' exactly - and an untouched element stays as it was in both"""
    t = [417]
    td = torch.tensor(t, dtype=torch.int64, device=DEV)
    kinds, x, ec = _inputs(tables, B, chw, 0, t)  # ("below", "above"); the median as the percentile: the first image keeps s = 1
    eu = (ec + 0.3 * synth.normal(32, (B, chw)).numpy()).astype(np.float32)
    e = np.concatenate([ec, eu], axis=0)
    got = torch.from_numpy(e).to(DEV)
    assert _threshold(mode, got, torch.from_numpy(x).to(DEV), tables["dev"], td, 0.5, halves=2, sg=sg) == 0
    want, info = R.threshold(mode, e, x, tables["t32"], t, 0.5, halves=2, sg=sg)
    got = got.cpu().numpy()
    assert _same(got, want)
    m = info["mask"]
    assert 0 < m.sum() and (~m).sum() > 0
    assert _same(got[:B][m], got[B:][m]) and np.array_equal(got[:B][~m].view(np.uint32), ec[~m].view(np.uint32))
    assert np.array_equal(got[B:][~m].view(np.uint32), eu[~m].view(np.uint32))
    s = np.float32(sg)
    with np.errstate(all="ignore"):
        mix = (got[B:] + (s * (got[:B] - got[B:]).astype(np.float32)).astype(np.float32)).astype(np.float32)
    assert _same(mix[m], got[:B][m])


# ------------------------------------------------------------------------------------------ 2. the two forms of the select
class _Route:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("DMME_DEBUG_ROUTE")
        os.environ["DMME_DEBUG_ROUTE"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("DMME_DEBUG_ROUTE", None)
        else:
            os.environ["DMME_DEBUG_ROUTE"] = self.old


@pytest.mark.parametrize("shape", [2, 3], ids=["cifar", "lds-last"])
def test_lds_and_streaming_forms_agree(tables, shape):
    """the same images through the one-workgroup form and, under DMME_DEBUG_ROUTE=thr_stream, through the streaming form (which leaves
    its scratch in any state: it is filled with ones first): the same bits, and the restatement's"""
    B, chw = _shapes(tables["cap"])[shape]
    t = [T, 1, 417][:B]
    td = torch.tensor(t, dtype=torch.int64, device=DEV)
    from dmme_amd import _lib

    dirty = torch.full((int(_lib.lib().dmme_x0_threshold_scratch_bytes(B, chw)) // 4,), -1, dtype=torch.int32, device=DEV)
    for group in range(len(HAZARDS)):
        kinds, x, e = _inputs(tables, B, chw, group, t)
        xd = torch.from_numpy(x).to(DEV)
        for p in PERCENTILES:
            a, b = torch.from_numpy(e).to(DEV), torch.from_numpy(e).to(DEV)
            assert _threshold(R.DYNAMIC, a, xd, tables["dev"], td, p, scratch=None) == 0
            with _Route("thr_stream"):
                assert _threshold(R.DYNAMIC, b, xd, tables["dev"], td, p, scratch=dirty) == 0
                assert _threshold(R.DYNAMIC, b.clone(), xd, tables["dev"], td, p, scratch=None) == -1  # (the streaming form needs its scratch)
            want, _ = R.threshold(R.DYNAMIC, e, x, tables["t32"], t, p)
            assert _same(a, b.cpu().numpy()) and _same(a, want), (kinds, p)


# ------------------------------------------------------------------------------------------ 3. refusals
def test_refusals_launch_nothing(tables):
    import dmme_amd
    from dmme_amd import _lib

    lib = _lib.lib()
    B, chw = 2, 192
    x, e = synth.normal(3, (B, chw)).to(DEV), (3.0 * synth.normal(4, (B, chw))).to(DEV)
    keep = e.clone()
    t = torch.tensor([5], dtype=torch.int64, device=DEV)
    bad = [dict(mode=0), dict(mode=3), dict(mode=-1), dict(mode=R.DYNAMIC, k=chw, frac=0.0), dict(mode=R.DYNAMIC, k=-1, frac=0.0), dict(mode=R.DYNAMIC, k=3, frac=1.5),
           dict(mode=R.DYNAMIC, k=3, frac=-0.25), dict(mode=R.DYNAMIC, k=chw - 1, frac=0.5), dict(mode=R.STATIC, planes=3), dict(mode=R.STATIC, halves=2, planes=2)]
    for kw in bad:
        mode = kw.pop("mode")
        assert _threshold(mode, e, x, tables["dev"], t, **kw) == -1, kw  # DMME_ERR_INVALID
        assert b"x0_threshold" in lib.dmme_last_error()
    assert lib.dmme_x0_threshold(R.STATIC, _lib.ptr(e), _lib.ptr(x), None, T, _lib.ptr(t), 1, B, chw, 1, 1, 1.0, 0, 0.0, None, _lib.stream_ptr()) == -1
    assert b"null table" in lib.dmme_last_error()
    assert _threshold(R.STATIC, e, x, tables["dev"], torch.tensor([1, 2, 3], dtype=torch.int64, device=DEV)) == -1
    torch.cuda.synchronize()
    assert torch.equal(e, keep)
    # a percentile outside [0, 1] never becomes a (k, frac): the host refuses it
    from dmme_amd.diffusion_models.ddpm import threshold_rank

    for p in (1.5, -0.1):
        with pytest.raises(ValueError):
            threshold_rank(p, chw)
        with pytest.raises(ValueError):
            dmme_amd.DDPM(_tiny(), 8).set_threshold("dynamic", p)
    # the plan's setter: a classifier plan, a null table, a mode out of range, (k, frac) out of the plan's range
    tab = tables["dev"]
    cplan = _classifier()._plan_for(2, 32, 32, DEV)
    assert lib.dmme_unet_plan_set_threshold(cplan.h, R.STATIC, _lib.ptr(tab), T, 0, 0.0, None) == -1
    assert b"classifier" in lib.dmme_last_error()
    plan = _tiny()._plan_for(2, 32, 32, DEV)
    assert lib.dmme_unet_plan_set_threshold(plan.h, R.STATIC, None, T, 0, 0.0, None) == -1
    assert lib.dmme_unet_plan_set_threshold(plan.h, 3, _lib.ptr(tab), T, 0, 0.0, None) == -1
    assert lib.dmme_unet_plan_set_threshold(plan.h, R.DYNAMIC, _lib.ptr(tab), T, 3072, 0.0, None) == -1
    assert lib.dmme_unet_plan_set_threshold(plan.h, R.DYNAMIC, _lib.ptr(tab), T, 5, 1.5, None) == -1
    assert b"plan_set_threshold" in lib.dmme_last_error()
    assert lib.dmme_unet_plan_set_threshold(plan.h, R.DYNAMIC, _lib.ptr(tab), T, 3055, 0.5, None) == 0
    assert lib.dmme_unet_plan_set_threshold(plan.h, 0, None, 0, 0, 0.0, None) == 0
    # loud misuse: t = 0 (the NaN row) and a timestep outside the table give NaN, never a read outside it
    for mode in (R.STATIC, R.DYNAMIC):
        for tt in ([0, 7], [T + 1, 7], [-1, 7]):
            got = keep.clone()
            assert _threshold(mode, got, x, tab, torch.tensor(tt, dtype=torch.int64, device=DEV), 0.995) == 0
            assert bool(torch.isnan(got[0]).all()) and bool(torch.isfinite(got[1]).all())


# ------------------------------------------------------------------------------------------ 4. captured chains against eager loops
def _graph_ran(runner):
    assert runner.capture_error is None and runner.graph is not None


def _spy(proc):
    """records every eager call of the stage on `proc`: (eps before, x, t, halves, scale, eps after)"""
    calls, real = [], proc._threshold_eps

    def wrapped(e, x, t, halves=1, guidance_scale=1.0):
        before = e.detach().clone().cpu().numpy()
        out = real(e, x, t, halves=halves, guidance_scale=guidance_scale)
        calls.append((before, x.detach().float().cpu().numpy(), t.detach().reshape(-1).cpu().numpy(), halves, guidance_scale, out.detach().cpu().numpy().copy()))
        return out

    proc._threshold_eps = wrapped
    return calls


def _assert_clipped(proc, calls, n_steps):
    """the eager loop's stage calls are the restatement's, bit for bit, on the chain's real inputs - and at least one step clipped
    something, so the comparison of the two chains is not one of two chains that never threshold"""
    assert len(calls) == n_steps
    tab = R.table32(proc.alpha_bar.reshape(-1).double().cpu().numpy())
    touched = 0
    for before, x, t, halves, sg, after in calls:
        B = x.shape[0]
        x = x.reshape(B, -1)
        want, info = R.threshold(proc._thr, before.reshape(B * halves, -1), x, tab, t, proc.threshold_percentile, planes=before[0].size // x[0].size, halves=halves, sg=sg)
        assert _same(after, want)
        touched += int(info["touched"].sum())
    assert touched > 0


def _chain_ddpm(mode):
    import dmme_amd

    n = 8
    proc = dmme_amd.DDPM(_tiny(), n, threshold=mode).to(DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE)
    _graph_ran(proc._runner)
    calls = _spy(proc)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    with torch.no_grad():
        for t in range(n, 0, -1):
            proc._reverse_update(x, proc._eps(x, proc.timestep_tensor(t, DEV)), t, None)
    return got, x, proc, calls, n


def _chain_strided(cls, mode, **kw):
    import dmme_amd

    proc = cls(_tiny(), 100, 6, threshold=mode, **kw).to(DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE)
    _graph_ran(proc._runner)
    calls = _spy(proc)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    with torch.no_grad():
        for i in range(6, 0, -1):
            proc._ddim_update(x, proc._eps(x, proc.tau_tensor(i, DEV)), i)
    return got, x, proc, calls, 6


def _chain_ddim(mode):
    import dmme_amd

    return _chain_strided(dmme_amd.DDIM, mode)


def _chain_gddim(mode):
    import dmme_amd

    return _chain_strided(dmme_amd.GeneralizedDDIM, mode, eta=0.5)


def _chain_iddpm(mode):
    """the two-plane network, on its cosine schedule (abar_T = 1.9e-15: the first x0 is of the order 1e7)"""
    import dmme_amd
    from dmme_amd.models import iddpm as iddpm_models

    torch.manual_seed(3)
    inet = iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,)).to(DEV).eval()
    n = 6
    proc = dmme_amd.IDDPM(inet, n).to(DEV).set_threshold(mode)
    torch.manual_seed(7)
    got = proc.generate(SHAPE)
    _graph_ran(proc._runner)
    calls = _spy(proc)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    with torch.no_grad():
        for t in range(n, 0, -1):
            proc._reverse_update(x, proc._eps(x, proc.timestep_tensor(t, DEV)), t, None)
    assert calls[0][0][0].size == 2 * x[0].numel()
    return got, x, proc, calls, n


def _chain_cfg_ddpm(mode, s=2.5):
    import dmme_amd

    proc = dmme_amd.ClassifierFreeDDPM(_cond(), 8, guidance_scale=s, threshold=mode).to(DEV)
    y = torch.tensor([2, 0])
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._cfg_runner)
    assert proc._cfg_runner.plan.B == (2 if s == 1.0 else 4)
    calls = _spy(proc)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    for t in range(8, 0, -1):
        x = proc.sampling_step(x, torch.tensor([t], device=DEV), y)
    assert all(c[3] == (1 if s == 1.0 else 2) for c in calls)
    return got, x, proc, calls, 8


def _chain_dpmpp(mode):
    import dmme_amd

    proc = dmme_amd.DPMSolverPP(_tiny(), 100, 5, threshold=mode).to(DEV)
    xT = synth.normal(12, SHAPE).to(DEV)
    got = proc.decode(xT)
    _graph_ran(proc._runner)
    calls = _spy(proc)
    with torch.no_grad():
        return got, proc._eager_chain(xT.clone(), proc.n_steps), proc, calls, proc.n_steps


def _chain_cfg_dpmpp(mode):
    import dmme_amd

    proc = dmme_amd.ClassifierFreeDPMSolver(_cond(), 100, 5, guidance_scale=2.5, threshold=mode).to(DEV)
    y = torch.tensor([1, 2])
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._cfg_runner)
    calls = _spy(proc)
    torch.manual_seed(7)
    return got, proc._eager_generate(dmme_amd.gaussian(SHAPE, device=DEV), y), proc, calls, proc.n_steps


def _chain_repaint(mode):
    import dmme_amd

    proc = dmme_amd.RePaint(_tiny(), 100, 4, 2, 2, threshold=mode).to(DEV)
    assert proc.n_rows == 6
    x0 = synth.uniform(13, SHAPE).to(DEV)
    m = torch.zeros(SHAPE, device=DEV)
    m[..., :16] = 1.0
    torch.manual_seed(7)
    got = proc.inpaint(x0, m)
    _graph_ran(proc._runner)
    assert torch.equal(got[m.bool()], x0[m.bool()])
    calls = _spy(proc)
    torch.manual_seed(7)
    with torch.no_grad():
        return got, proc._eager_chain(dmme_amd.gaussian(SHAPE, device=DEV), x0, m), proc, calls, 6


def _chain_guided_ddim(mode):
    import dmme_amd

    proc = dmme_amd.ClassifierGuidedDDIM(_tiny(21), _classifier(), 100, 6, guidance_scale=3.0, threshold=mode).to(DEV)
    y = torch.tensor([9, 3], device=DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE, y)
    _graph_ran(proc._grunner)
    calls = _spy(proc)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    for i in range(6, 0, -1):
        x = proc.sampling_step(x, torch.tensor([i], device=DEV), y)
    return got, x, proc, calls, 6


CHAINS = {"ddpm": _chain_ddpm, "ddim": _chain_ddim, "gddim": _chain_gddim, "iddpm": _chain_iddpm, "cfg-ddpm": _chain_cfg_ddpm,
          "cfg-ddpm-s1": lambda m: _chain_cfg_ddpm(m, 1.0), "dpm++": _chain_dpmpp, "cfg-dpm++": _chain_cfg_dpmpp, "repaint": _chain_repaint,
          "guided-ddim": _chain_guided_ddim}


@pytest.mark.parametrize("mode", ["static", "dynamic"])
@pytest.mark.parametrize("chain", list(CHAINS))
def test_captured_chain_equals_eager_loop(chain, mode):
    """one case per chain entry point (dmme_chain_step for the DDPM, DDIM, paper-DDIM and IDDPM kinds, dmme_cfg_chain_step,
    dmme_dpmpp_chain_step, dmme_cfg_dpmpp_chain_step, dmme_repaint_chain_step, dmme_guided_chain_step) and the classifier-free s = 1
    path, which launches the stage from the runner: the replayed graph, with the stage inside the step, against the host loop through
    `_eps` under one seed - the same bits; 8 steps at most, from the top of the schedule"""
    got, want, proc, calls, n = CHAINS[chain](mode)
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    _assert_clipped(proc, calls, n)


def test_encode_never_thresholds():
    """GeneralizedDDIM.encode with thresholding on is the encode of a process without it (graph and eager); decode differs"""
    import dmme_amd

    x0 = (2.0 * synth.uniform(17, SHAPE) - 1.0).to(DEV)
    plain, thr = dmme_amd.GeneralizedDDIM(_tiny(), 100, 6).to(DEV), dmme_amd.GeneralizedDDIM(_tiny(), 100, 6, threshold="static").to(DEV)
    a, b = plain.encode(x0), thr.encode(x0)
    _graph_ran(thr._enc_runner)
    assert torch.equal(a, b)
    with torch.no_grad():
        x = x0.clone()
        for j in range(6, 0, -1):
            thr._gddim_update(x, thr._eps(x, thr._enc_t_tensor(j, DEV), _threshold=False), thr._enc_rows[j])
    assert torch.equal(x, b)
    big = 3.0 * a
    assert not torch.equal(plain.decode(big), thr.decode(big))


# ------------------------------------------------------------------------------------------ 5. off means off
def test_off_after_on_is_a_process_that_never_had_it():
    import dmme_amd
    from dmme_amd import _lib

    proc, fresh = dmme_amd.DDPM(_tiny(), 8, threshold="dynamic").to(DEV), dmme_amd.DDPM(_tiny(), 8).to(DEV)
    torch.manual_seed(7)
    on = proc.generate(SHAPE)
    plan = proc._runner.plan
    n_on = (_lib.lib().dmme_unet_plan_num_launches(plan.h), _lib.lib().dmme_unet_plan_num_launches_nograd(plan.h))
    proc.set_threshold("none")
    torch.manual_seed(7)
    off = proc.generate(SHAPE)
    _graph_ran(proc._runner)
    assert proc._runner.plan is plan and proc._runner.thr == _lib.THRESHOLD_NONE
    torch.manual_seed(7)
    want = fresh.generate(SHAPE)
    fplan = fresh._runner.plan
    assert torch.equal(off, want) and not torch.equal(on, off)
    assert n_on == (_lib.lib().dmme_unet_plan_num_launches(fplan.h), _lib.lib().dmme_unet_plan_num_launches_nograd(fplan.h))
    # eager: `_eps` hands back the network's own output again
    with torch.no_grad():
        x = synth.normal(5, SHAPE).to(DEV)
        assert torch.equal(proc._eps(x, proc.timestep_tensor(8, DEV)), fresh._eps(x, fresh.timestep_tensor(8, DEV)))


# ------------------------------------------------------------------------------------------ 6. the effect
def test_static_thresholding_bounds_the_final_images():
    """A DDPM chain's final images with threshold="static": max |x| <= 1 + delta.  The last step (t = 1, no noise) returns the mean
    c0 (x - c1 e'), which is the clipped x0 up to rounding; delta is twice the largest excess over 1 of that step's float32
    restatement on the chain's own inputs (x_1 and the network's eps at t = 1 from the eager loop, which test 4 holds equal to the
    captured chain).  On this network and seed the restatement's largest excess is 3.588e-05, so delta = 7.176e-05 (the rewrite
    e' = C x - D x0c cancels at t = 1, where C = D = 100: an ulp of C x is 1e-5 of x0); the chain's max |x| is 1.00003588.  The same
    chain without thresholding reaches 4.7064 > 1.5 (it ends near N(0, 1): 8 steps of the linear schedule remove little), so the
    bound is not vacuous."""
    import dmme_amd

    n, net = 8, _tiny()
    proc, plain = dmme_amd.DDPM(net, n, threshold="static").to(DEV), dmme_amd.DDPM(net, n).to(DEV)
    torch.manual_seed(7)
    got = proc.generate(SHAPE)
    torch.manual_seed(7)
    loose = plain.generate(SHAPE)
    torch.manual_seed(7)
    x = dmme_amd.gaussian(SHAPE, device=DEV)
    with torch.no_grad():
        for t in range(n, 1, -1):
            proc._reverse_update(x, proc._eps(x, proc.timestep_tensor(t, DEV)), t, None)
        e_raw = proc._eps(x, proc.timestep_tensor(1, DEV), _threshold=False).float().cpu().numpy().reshape(SHAPE[0], -1)
    x1 = x.cpu().numpy().reshape(SHAPE[0], -1)
    tab = R.table32(proc.alpha_bar.reshape(-1).double().cpu().numpy())
    e, info = R.threshold(R.STATIC, e_raw, x1, tab, [1], None)
    c0, c1 = np.float32(proc._c1[1]), np.float32(proc._c2[1])
    mean = (c0 * (x1 - (c1 * e).astype(np.float32)).astype(np.float32)).astype(np.float32)
    excess = max(0.0, float(np.abs(mean).max()) - 1.0)
    delta = 2.0 * excess
    print(f"static thresholding, last step restated: largest excess over 1 = {excess:.3e}, delta = {delta:.3e}; chain max |x| = {float(got.abs().max()):.8f}, "
          f"unthresholded {float(loose.abs().max()):.4f}, clipped at t = 1: {int(info['touched'].sum())} of {e.size}")
    assert info["touched"].sum() > 0
    assert float(loose.abs().max()) > 1.5
    assert float(got.abs().max()) <= 1.0 + delta
    assert _same(got, mean)


# ------------------------------------------------------------------------------------------ 7. the trainer
def _sample(capsys, argv):
    from dmme_amd import trainer

    rc = trainer.main(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    return rc, line


def test_trainer_samples_the_cfg_config_with_dynamic_thresholding(tmp_path, capsys):
    path = str(tmp_path / "cfg.npy")
    rc, line = _sample(capsys, ["sample", "--config", os.path.join(ROOT, "configs", "cfg", "cifar10.yaml"), "--labels", "3", "--guidance-scale", "2.5", "--threshold", "dynamic",
                                "--num-images", "2", "--save", path])
    assert rc == 0 and line["images"] == [2, 3, 32, 32] and line["finite"] is True
    out = np.load(path)
    assert out.shape == (2, 3, 32, 32) and np.isfinite(out).all()


def test_trainer_samples_the_iddpm_config_with_dynamic_thresholding(tmp_path, capsys):
    """the cosine schedule and the two-plane network through the trainer.  (`--sampler ddim-paper` is refused for this config, with or
    without thresholding: the paper-form DDIM kind takes one output plane; the config's own strided sampler stands in, and the
    refusal is asserted as it stands.)"""
    from dmme_amd import trainer

    cfg = os.path.join(ROOT, "configs", "iddpm", "cifar10.yaml")
    with pytest.raises(SystemExit, match="needs a DDIM config"):
        trainer.main(["sample", "--config", cfg, "--sampler", "ddim-paper", "--threshold", "dynamic", "--num-images", "2"])
    capsys.readouterr()
    path = str(tmp_path / "iddpm.npy")
    rc, line = _sample(capsys, ["sample", "--config", cfg, "--sample-steps", "8", "--threshold", "dynamic", "--threshold-percentile", "0.99", "--num-images", "2", "--save", path])
    assert rc == 0 and line["images"] == [2, 3, 32, 32] and line["finite"] is True
    out = np.load(path)
    assert out.shape == (2, 3, 32, 32) and np.isfinite(out).all()
    # the paper-form sampler on the config it takes, thresholded: the first steps of its chain (the config's quadratic schedule ends with a
    # step from tau_1 = 0, where abar = 1 and the table's row is NaN by design: see README)
    rc, line = _sample(capsys, ["sample", "--config", os.path.join(ROOT, "configs", "ddim", "cifar10.yaml"), "--sampler", "ddim-paper", "--threshold", "dynamic", "--num-images", "2",
                                "--steps", "3"])
    assert rc == 0 and line["images"] == [2, 3, 32, 32] and line["finite"] is True
