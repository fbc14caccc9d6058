"""-m gpu: denoising-history grids - dmme_grid_tile, HistoryRecorder and make_history against the numpy float32 restatement
(tests/vis_ref.py), recorded chains against unrecorded ones and against the eager loop's frames, the GenerateImage callback's two
paths, and the trainer's PNG output.  Every comparison is bit for bit (torch.equal / np.array_equal): no tolerance anywhere.

Chains run on the tiny UNet of tests/test_gpu_chain.py at 32 x 32, the size at which the suite runs that network's chains (smaller
inputs would take its four levels down to 2 x 2 and 1 x 1 maps, which no UNet test covers and which is not this feature's ground)."""

import json
import os

import numpy as np
import pytest
import torch

from oracle import synth
from oracle import unet as O

from . import vis_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (2, 3, 32, 32)
T, VIS = 12, 5


def _tiny(seed=11):
    import dmme_amd

    cfg = O.TINY
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision="fp32")
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _frames(shape, n, seed):
    """n image batches spread over [-3, 3], with exact -1, 1, +0 and -0 in every one"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        x = (torch.rand(shape, generator=g) * 6.0 - 3.0).to(torch.float32)
        flat = x.reshape(-1)
        flat[0], flat[1], flat[2], flat[3] = -1.0, 1.0, 0.0, -0.0
        flat[-1], flat[-2] = 1.0, -1.0
        out.append(x.contiguous())
    return out


def _np(t):
    return t.detach().cpu().numpy()


def _recorder(shape, n_frames, out_kind=0):
    import dmme_amd

    return dmme_amd.HistoryRecorder(shape[0], *shape[1:], range(n_frames), out_kind)


# ------------------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("shape,n_frames", [((3, 3, 8, 12), 4),   # 864 values per frame: four blocks
                                            ((2, 1, 6, 10), 3),   # one channel shown as three; rows of 10 and a canvas 38 wide: nothing aligned
                                            ((5, 3, 4, 4), 2),
                                            ((1, 3, 5, 7), 1)])   # a single image: unpadded, as make_grid returns it
def test_recorder_float_canvas_vs_restatement(shape, n_frames):
    frames = _frames(shape, n_frames, 3)
    rec = _recorder(shape, n_frames)
    B, C, H, W = shape
    if B * n_frames == 1:
        assert tuple(rec.canvas.shape) == (3 if C == 1 else C, H, W)
    elif n_frames > 1:
        assert tuple(rec.canvas.shape) == (3 if C == 1 else C, B * (H + 2) + 2, n_frames * (W + 2) + 2)
    assert rec.canvas.dtype == torch.float32 and not bool(rec.canvas.any())
    for k, x in enumerate(frames):
        rec.at(k, x.cuda())
    torch.cuda.synchronize()
    want = R.make_history([R.denorm(_np(x)) for x in frames])
    got = _np(rec.canvas)
    assert got.shape == want.shape and np.array_equal(got, want)
    assert got.min() == 0.0 and got.max() == 1.0
    if B * n_frames > 1:  # the padding: where a grid of all-ones images is 0
        padding = R.make_history([np.ones(shape, np.float32)] * n_frames) == 0
        assert padding.any() and not got[padding].any()
    # a second recording into the same recorder: every cell overwritten, the padding still 0
    again = _frames(shape, n_frames, 4)
    for k, x in enumerate(again):
        rec.at(k, x.cuda())
    torch.cuda.synchronize()
    assert np.array_equal(_np(rec.canvas), R.make_history([R.denorm(_np(x)) for x in again]))
    assert rec.recorded == 2 * n_frames


def test_grid_stride_loop_and_a_wide_canvas():
    """(17, 1, 500, 500): 4 250 000 values for the 4 194 304 threads of the largest grid, so some threads take a second trip"""
    import dmme_amd

    x = _frames((17, 1, 500, 500), 1, 5)[0]
    got = dmme_amd.make_history([x.cuda()])
    torch.cuda.synchronize()
    want = R.make_history([_np(x)])
    assert tuple(got.shape) == (3, 17 * 502 + 2, 504) and np.array_equal(_np(got), want)


# ------------------------------------------------------------------------------------------ 2. the uint8 rule
def _byte_inputs():
    k = np.arange(256, dtype=np.float32)
    exact = k / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
    half = (k + np.float32(0.5)) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
    outside = np.float32([-3.0, 5.0, -1.0001, 1.0001])
    return np.concatenate([exact, half, outside]).astype(np.float32)  # 516 values


def test_uint8_rule_vs_restatement():
    import dmme_amd

    vals = _byte_inputs()
    x = np.stack([vals.reshape(3, 4, 43), vals[::-1].reshape(3, 4, 43)])  # (2, 3, 4, 43)
    want = R.make_history([R.to_uint8(R.denorm(x))])
    assert want.dtype == np.uint8 and want.min() == 0 and want.max() == 255 and len(np.unique(want)) == 256
    rec = dmme_amd.HistoryRecorder(2, 3, 4, 43, [0], out_kind=1)
    assert rec.canvas.dtype == torch.uint8
    rec.at(0, torch.from_numpy(x).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(_np(rec.canvas), want)
    # frames denormed already take the same bytes through make_history's path (no second denorm)
    den = torch.from_numpy(R.denorm(x)).cuda()
    assert np.array_equal(_np(dmme_amd.make_history([den], out_kind=1)), want)
    # and the byte grid is the float grid under the same rule
    assert np.array_equal(R.to_uint8(_np(dmme_amd.make_history([den]))), want)


# ------------------------------------------------------------------------------------------ 3. make_history
@pytest.mark.parametrize("N,nrow", [(1, 1), (8, 1), (12, 4), (16, 4)])
def test_make_history_single_history(N, nrow):
    import dmme_amd

    x = _frames((N, 3, 6, 10), 1, 10 + N)[0]
    got = dmme_amd.make_history([x.cuda()])
    torch.cuda.synchronize()
    if N == 1:
        assert tuple(got.shape) == (3, 6, 10)
    else:
        assert tuple(got.shape) == (3, (N // nrow) * 8 + 2, nrow * 12 + 2)
    assert np.array_equal(_np(got), R.make_history([_np(x)]))  # values outside [0, 1] pass through: no denorm here


@pytest.mark.parametrize("shape,L", [((3, 3, 8, 12), 4), ((2, 1, 6, 10), 2)])
def test_make_history_several_histories(shape, L):
    import dmme_amd

    frames = _frames(shape, L, 21)
    got = dmme_amd.make_history([x.cuda() for x in frames])
    torch.cuda.synchronize()
    assert np.array_equal(_np(got), R.make_history([_np(x) for x in frames]))
    with pytest.raises(ValueError):
        dmme_amd.make_history([frames[0].cuda(), frames[1][:1].cuda()])
    with pytest.raises(ValueError):
        dmme_amd.make_history([frames[0]])  # CPU tensors: the grid is built on the device


# ------------------------------------------------------------------------------------------ 4. recording does not disturb a chain
def _eager_frames(step, x, count, ordinals):
    """the denormed frames an eager loop keeps: `step(x, k)` is the k-th step (k = 0 first) as a new tensor"""
    import dmme_amd

    keep = []
    with torch.no_grad():
        for k in range(count):
            if k in ordinals:
                keep.append(dmme_amd.denorm(x.clone()))
            x = step(x, k)
        if count in ordinals:
            keep.append(dmme_amd.denorm(x.clone()))
    return keep, x


def _check_canvas(rec, frames):
    import dmme_amd

    assert rec.recorded == len(frames) == len(rec.ordinals)
    assert torch.equal(rec.canvas, dmme_amd.make_history(frames))
    assert np.array_equal(_np(rec.canvas), R.make_history([_np(f) for f in frames]))


def test_recorded_ddpm_chain_equals_the_unrecorded_one_and_the_eager_frames():
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.DDPM(net, T).cuda()
    ords = dmme_amd.history_ordinals(T, VIS)
    assert ords == [0, 3, 6, 9, 12]
    torch.manual_seed(77)
    plain = proc.generate(SHAPE).clone()
    state_plain = torch.cuda.get_rng_state()
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(77)
    got = proc.generate(SHAPE, history=rec)
    assert torch.equal(got, plain) and torch.equal(torch.cuda.get_rng_state(), state_plain)
    assert proc._runner.capture_error is None and proc._runner.graph is not None
    torch.manual_seed(77)
    x = dmme_amd.gaussian(SHAPE, device="cuda")
    frames, last = _eager_frames(lambda x, k: proc.sampling_step(x, torch.tensor([T - k], device="cuda")), x, T, ords)
    assert torch.equal(last, plain)
    _check_canvas(rec, frames)
    # the uint8 recorder of the same chain: the float canvas under the byte rule; the positional call is what it was
    rec8 = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords, out_kind=1)
    torch.manual_seed(77)
    assert torch.equal(proc.generate(SHAPE, rec8), plain)
    assert np.array_equal(_np(rec8.canvas), R.to_uint8(_np(rec.canvas)))
    # a recorder that does not fit the chain is refused before anything is drawn
    before = torch.cuda.get_rng_state()
    for bad in (dmme_amd.HistoryRecorder(2, 3, 32, 32, [0, T + 1]), dmme_amd.HistoryRecorder(3, 3, 32, 32, ords), dmme_amd.HistoryRecorder(2, 3, 16, 32, ords)):
        with pytest.raises(ValueError):
            proc._runner.run(T, T, bad)
    assert torch.equal(torch.cuda.get_rng_state(), before)


def test_recorded_ddim_and_dpm_solver_chains_equal_the_eager_frames():
    import dmme_amd

    net = _tiny()
    ddim = dmme_amd.DDIM(net, T, 5).cuda()  # the deterministic 5-of-12 chain
    ords = dmme_amd.history_ordinals(5, VIS)
    assert ords == [0, 2, 3, 4, 5]
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(5)
    got = ddim.generate(SHAPE, history=rec)
    torch.manual_seed(5)
    assert torch.equal(ddim.generate(SHAPE), got)
    torch.manual_seed(5)
    x = dmme_amd.gaussian(SHAPE, device="cuda")
    frames, last = _eager_frames(lambda x, k: ddim.sampling_step(x, torch.tensor([5 - k], device="cuda")), x, 5, ords)
    assert torch.equal(last, got)
    _check_canvas(rec, frames)

    dpm = dmme_amd.DPMSolverPP(net, 100, 4).cuda()
    ords = dmme_amd.history_ordinals(4, VIS)
    assert ords == [0, 1, 2, 3, 4]
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(6)
    got = dpm.generate(SHAPE, history=rec)
    torch.manual_seed(6)
    assert torch.equal(dpm.generate(SHAPE), got)
    torch.manual_seed(6)
    x = dmme_amd.gaussian(SHAPE, device="cuda")
    hist = torch.empty_like(x)
    frames, last = _eager_frames(lambda x, k: dpm.sampling_step(x, torch.tensor([4 - k], device="cuda"), history=hist, history_valid=k > 0), x, 4, ords)
    assert torch.equal(last, got)
    _check_canvas(rec, frames)


def test_recorded_repaint_chain():
    """a walk with jumps (8 levels, jump length 3, 2 resamples: 14 steps): the recorded chain returns the unrecorded one's images and
    keeps one frame per ordinal; the last column is the denormed result"""
    import dmme_amd

    net = _tiny()
    proc = dmme_amd.RePaint(net, 100, 8, 3, 2).cuda()
    count = proc.chain_length()
    assert count == proc.n_rows == 14
    x0 = (0.5 * synth.normal(42, SHAPE)).clamp(-1, 1).cuda()
    m = torch.zeros((1, 1, 32, 32))
    m[..., :16] = 1.0
    ords = dmme_amd.history_ordinals(count, VIS)
    rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
    torch.manual_seed(9)
    plain = proc.inpaint(x0, m)
    state = torch.cuda.get_rng_state()
    torch.manual_seed(9)
    got = proc.inpaint(x0, m, history=rec)
    assert torch.equal(got, plain) and torch.equal(torch.cuda.get_rng_state(), state)
    assert rec.recorded == len(ords) == len(dmme_amd.history_ordinals(count, VIS)) == 5
    canvas, L = _np(rec.canvas), len(ords)
    want_last = R.denorm(_np(got))
    for b in range(SHAPE[0]):
        y0, c0 = b * 34 + 2, (L - 1) * 34 + 2
        assert np.array_equal(canvas[:, y0:y0 + 32, c0:c0 + 32], want_last[b])
    # SDEdit: the frames of the edit_level(strength) steps
    k = proc.edit_level(0.5)
    rec2 = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], dmme_amd.history_ordinals(k, 3))
    torch.manual_seed(10)
    plain = proc.edit(x0, 0.5)
    torch.manual_seed(10)
    assert torch.equal(proc.edit(x0, 0.5, history=rec2), plain) and rec2.recorded == 3


@pytest.mark.parametrize("case", ["ddpm", "iddpm-strided", "dpm-solver", "repaint"])
def test_recorded_host_walk_equals_the_recorded_captured_chain(case):
    """the host walk (diffusion_models/chain.py: walk) with a recorder - what a process runs where its step cannot be replayed - keeps
    the frames of the captured chain and returns its images, bit for bit: DDPM's and the strided IDDPM's `_run_chain`, DPMSolverPP's
    and RePaint's `_eager_chain` (a walk with a jump: 4 levels, jump length 2, 2 resamples, 6 steps).  Chains of 4 to 8 steps."""
    import dmme_amd
    from dmme_amd.models import iddpm as iddpm_models

    if case == "ddpm":
        proc = dmme_amd.DDPM(_tiny(), 8).cuda()
        count, run = 8, lambda rec: proc.generate(SHAPE, history=rec)
    elif case == "iddpm-strided":
        proc = dmme_amd.IDDPM(iddpm_models.UNet(3, 4, 8, 2, 0.0, (4, 8), 1, (2,)).cuda().eval(), 20).cuda()
        count, run = proc._respaced_tables(5)[0], lambda rec: proc.generate(SHAPE, sample_steps=5, history=rec)
        assert count == 5
    elif case == "dpm-solver":
        proc = dmme_amd.DPMSolverPP(_tiny(), 100, 4).cuda()
        count, run = 4, lambda rec: proc.generate(SHAPE, history=rec)
    else:
        proc = dmme_amd.RePaint(_tiny(), 100, 4, 2, 2).cuda()
        x0 = (0.5 * synth.normal(42, SHAPE)).clamp(-1, 1).cuda()
        m = torch.zeros((1, 1, 32, 32))
        m[..., :16] = 1.0
        count, run = 6, lambda rec: proc.inpaint(x0, m, history=rec)
        assert proc.chain_length() == 6
    ords = dmme_amd.history_ordinals(count, 3)
    captured, hosted = (dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords) for _ in range(2))
    torch.manual_seed(23)
    want = run(captured).clone()
    asked = []

    def never(x):
        asked.append(tuple(x.shape))
        return False

    proc._replayable = never  # no runner: the process walks on the host
    torch.manual_seed(23)
    got = run(hosted)
    assert asked == [SHAPE] and torch.equal(got, want)
    assert hosted.recorded == captured.recorded == len(ords) == 3 and torch.equal(hosted.canvas, captured.canvas)
    assert bool(captured.canvas.any())
    torch.manual_seed(23)
    assert torch.equal(run(None), want) and len(asked) == 2  # the same walk with nobody watching


def _column(canvas, k, b):
    return canvas[:, b * 34 + 2:b * 34 + 34, k * 34 + 2:k * 34 + 34]


def test_recorded_cfg_and_guided_chains():
    """the runners that hold more than they return: the classifier-free chain steps a buffer of 2B images and the recorder keeps the
    first B; the classifier-guided chain carries a classifier beside the UNet.  Recording changes neither the images nor the generator;
    column 0 is the denormed x_T, the last column the denormed result."""
    import dmme_amd

    from . import classifier_ref as CR
    from . import cond_ref as KR

    kw = dict(pos_dim=4, emb_dim=8, num_groups=2, channels_per_depth=(4, 8, 16, 32), num_blocks=3)
    K, n = 10, 6
    cnet = dmme_amd.ConditionalUNet(precision="fp32", num_classes=K, dropout=0.0, **kw)
    cnet.load_state_dict(KR.make_state_dict(KR.TINY, K, 11), strict=True)
    clf = dmme_amd.EncoderClassifier(precision="fp32", num_classes=K, **kw)
    clf.load_state_dict(CR.make_state_dict(CR.TINY, K, 22))
    y = [3, K]
    cases = [dmme_amd.ClassifierFreeDDPM(cnet.cuda().eval(), n, guidance_scale=2.0), dmme_amd.ClassifierGuidedDDPM(_tiny(), clf.cuda().eval(), timesteps=n, guidance_scale=2.0)]
    for proc in cases:
        proc = proc.cuda()
        labels = y if isinstance(proc, dmme_amd.ClassifierFreeDDPM) else [3, 7]
        ords = dmme_amd.history_ordinals(proc.chain_length(), 3)
        assert ords == [0, 3, 6]
        rec = dmme_amd.HistoryRecorder(SHAPE[0], *SHAPE[1:], ords)
        torch.manual_seed(41)
        plain = proc.generate(SHAPE, labels)
        state = torch.cuda.get_rng_state()
        torch.manual_seed(41)
        got = proc.generate(SHAPE, labels, history=rec)
        assert torch.equal(got, plain) and torch.equal(torch.cuda.get_rng_state(), state), type(proc).__name__
        assert rec.recorded == 3
        torch.manual_seed(41)
        x_T = dmme_amd.gaussian(SHAPE, device="cuda")
        canvas, first, last = _np(rec.canvas), R.denorm(_np(x_T)), R.denorm(_np(got))
        for b in range(SHAPE[0]):
            assert np.array_equal(_column(canvas, 0, b), first[b]) and np.array_equal(_column(canvas, 2, b), last[b]), type(proc).__name__
    assert cases[0]._cfg_runner.x.shape[0] == 2 * SHAPE[0]


# ------------------------------------------------------------------------------------------ 5. the callback's two paths
def test_generate_image_grid_equals_make_history_of_generate_img():
    """the per-step path (LitDDPM.forward -> denoise_once: one replayed step per call, one span of the Philox stream reserved per call)
    consumes the stream as the chain does (one reservation of `count` spans at the same offsets), so the two grids are equal bits"""
    import dmme_amd

    net = _tiny()
    lit = dmme_amd.LitDDPM(model=net, timesteps=T).cuda()
    lit.train()
    cb = dmme_amd.GenerateImage((3, 32, 32), T, batch_size=2, vis_length=VIS)
    torch.manual_seed(31)
    fast = cb.grid(lit).clone()
    assert lit.training and net.training
    torch.manual_seed(31)
    history = cb.generate_img(lit)
    assert lit.training and len(history) == VIS and all(tuple(h.shape) == SHAPE for h in history)
    assert float(torch.stack(history).min()) >= 0.0 and float(torch.stack(history).max()) <= 1.0
    slow = dmme_amd.make_history(history)
    assert tuple(fast.shape) == (3, 2 * 34 + 2, VIS * 34 + 2) and torch.equal(fast, slow)
    assert np.array_equal(_np(slow), R.make_history([_np(h) for h in history]))
    torch.manual_seed(31)
    again = cb.grid(lit, out_kind=1)
    assert again.dtype == torch.uint8 and np.array_equal(_np(again), R.to_uint8(_np(fast)))


# ------------------------------------------------------------------------------------------ 6. the trainer
def _tiny_yaml(tmp_path):
    import yaml

    cfg = {
        "seed_everything": 7,
        "trainer": {"max_steps": 2, "precision": 32, "log_every_n_steps": 1,
                    "callbacks": [{"class_path": "dmme.callbacks.GenerateImage", "init_args": {"imgsize": [3, 32, 32], "timesteps": T, "batch_size": 2, "vis_length": 3}}]},
        "model": {"class_path": "dmme.LitDDPM", "init_args": {"lr": 2e-4, "warmup": 10, "decay": 0.99, "timesteps": T,
                  "model": {"class_path": "dmme.UNet", "init_args": {"pos_dim": 8, "emb_dim": 16, "num_groups": 2, "channels_per_depth": [8, 16], "num_blocks": 1, "attention_depths": [2]}}}},
        "data": {"class_path": "dmme.CIFAR10", "init_args": {"data_dir": str(tmp_path), "batch_size": 4}},
    }
    path = tmp_path / "cfg.yaml"
    path.write_text(yaml.safe_dump(cfg))
    return str(path)


def test_trainer_sample_grid_writes_the_canvas(tmp_path, capsys):
    import dmme_amd
    from dmme_amd import trainer

    cfg = _tiny_yaml(tmp_path)
    png, npy = str(tmp_path / "hist.png"), str(tmp_path / "imgs.npy")
    assert trainer.main(["sample", "--config", cfg, "--num-images", "3", "--vis-length", "4", "--grid", png, "--save", npy]) == 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["finite"]
    pixels = R.read_png(png)
    assert pixels.shape == (3, 3 * 34 + 2, 4 * 34 + 2)
    # the same chain again, as the command sets it up: the YAML's seed, the module built under it, the recorder's uint8 canvas
    conf = trainer.parse_config(cfg)
    torch.manual_seed(conf["seed"])
    module = trainer.build_module(conf).cuda().eval()
    rec = dmme_amd.HistoryRecorder(3, 3, 32, 32, dmme_amd.history_ordinals(T, 4), out_kind=1)
    imgs = module.diffusion_model.generate((3, 3, 32, 32), history=rec)
    assert np.array_equal(np.load(npy), _np(imgs))
    assert np.array_equal(pixels, _np(rec.canvas))
    last = R.to_uint8(R.denorm(_np(imgs)))
    assert np.array_equal(pixels[:, 2:34, 3 * 34 + 2:4 * 34], last[0])
    # --vis-length 1 (the default): the final images in the single-history layout, 12 images in rows of 4
    png1 = str(tmp_path / "final.png")
    assert trainer.main(["sample", "--config", cfg, "--num-images", "12", "--grid", png1, "--save", npy]) == 0
    capsys.readouterr()
    assert np.array_equal(R.read_png(png1), R.make_history([R.to_uint8(R.denorm(np.load(npy)))]))
    assert R.read_png(png1).shape == (3, 3 * 34 + 2, 4 * 34 + 2)


def test_trainer_fit_writes_previews(tmp_path, capsys):
    from dmme_amd import trainer

    cfg = _tiny_yaml(tmp_path)
    out = tmp_path / "previews"
    assert trainer.main(["fit", "--config", cfg, "--preview-dir", str(out), "--preview-every", "1"]) == 0
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert [l["preview"] for l in lines if "preview" in l] == [str(out / "step_1.png"), str(out / "step_2.png")]
    assert all(np.isfinite(l["train/loss"]) for l in lines if "train/loss" in l)
    for n in (1, 2):  # the YAML's GenerateImage entry: 2 images, 3 frames of 32 x 32
        assert R.read_png(str(out / f"step_{n}.png")).shape == (3, 2 * 34 + 2, 3 * 34 + 2)
    assert sorted(os.listdir(out)) == ["step_1.png", "step_2.png"]
