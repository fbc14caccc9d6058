"""CPU: the host side of the denoising-history grids - history_ordinals against the reference callback's save_t, save_png through
the restatement's reader (tests/vis_ref.py), dmme_grid_tile's argument checks, and the YAML entry of dmme.callbacks.GenerateImage."""

import ctypes as C
import os

import numpy as np
import pytest

import dmme_amd
from dmme_amd import _lib

from . import vis_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------ history_ordinals
def test_history_ordinals_are_the_reference_frames_of_a_full_chain():
    """(1000, 20): the callback keeps x_t in front of the step from every t of save_t, i.e. after 1000 - t steps, then the final x_0"""
    save_t = R.reference_save_t(1000, 20)
    # (1000 / 19 * 19 rounds below 1000 in float64: the reference's first frame is x_999, one step into the chain, and that is kept)
    assert save_t[0] == 999 and save_t[1] == 947 and len(save_t) == 19 and save_t[-1] == 52
    want = sorted({1000 - t for t in save_t} | {1000})
    got = dmme_amd.history_ordinals(1000, 20)
    assert got == want and len(got) == 20 and got[0] == 1 and got[-1] == 1000 and got[1] == 1000 - 947
    # the frames of the host loop itself: walk t = T .. 1 as the callback does
    walked = [1000 - t for t in range(1000, 0, -1) if t in save_t] + [1000]
    assert got == walked


@pytest.mark.parametrize("count,L", [(50, 20), (5, 20), (12, 1), (12, 5), (1, 2), (7, 8)])
def test_history_ordinals_short_chains(count, L):
    got = dmme_amd.history_ordinals(count, L)
    assert got == R.history_ordinals(count, L)
    assert got == sorted(set(got)) and got[-1] == count and all(0 <= s <= count for s in got) and len(got) <= L
    if L == 1:
        assert got == [count]
    if (count, L) == (50, 20):  # 50 / 19 * 19 is 50 exactly: the first frame is x_T
        assert len(got) == 20 and got[:3] == [0, 3, 6] and got[-2:] == [48, 50]
    if (count, L) == (5, 20):  # more frames asked for than the chain has states: duplicates collapse
        assert got == [0, 1, 2, 3, 4, 5]
    if (count, L) == (12, 5):
        assert got == [0, 3, 6, 9, 12]


def test_history_ordinals_reject_nonsense():
    for bad in ((-1, 5), (10, 0)):
        with pytest.raises(ValueError):
            dmme_amd.history_ordinals(*bad)


def test_history_nrow_keeps_the_reference_quirk():
    from dmme_amd.common import vis

    assert [vis.history_nrow(n) for n in (1, 8, 9, 12, 16, 64)] == [1, 1, 3, 4, 4, 8]
    assert [R.history_nrow(n) for n in (1, 8, 9, 12, 16, 64)] == [1, 1, 3, 4, 4, 8]


# ------------------------------------------------------------------------------------------ PNG
def _image(C_, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(C_, H, W), dtype=np.uint8)


@pytest.mark.parametrize("shape", [(3, 5, 7), (1, 4, 9), (3, 1, 1), (3, 70, 130)])
def test_save_png_round_trip(tmp_path, shape):
    img = _image(*shape, seed=3)
    path = str(tmp_path / "a.png")
    dmme_amd.save_png(path, img)
    back = R.read_png(path)  # (checks the signature and every CRC)
    assert back.dtype == np.uint8 and np.array_equal(back, img)
    try:
        from PIL import Image
    except ImportError:
        return
    with Image.open(path) as im:
        im.load()
        assert im.size == (shape[2], shape[1]) and im.mode == ("RGB" if shape[0] == 3 else "L")
        pil = np.asarray(im)
    assert np.array_equal(pil if shape[0] == 3 else pil[:, :, None], img.transpose(1, 2, 0))


def test_save_png_converts_floats_by_the_uint8_rule_and_accepts_tensors(tmp_path):
    import torch

    k = np.arange(256, dtype=np.float32)
    vals = np.concatenate([k / np.float32(255.0), (k + np.float32(0.5)) / np.float32(255.0), np.float32([-0.25, 1.5, 0.0, 1.0])])
    img = np.resize(vals, (3, 12, 43)).astype(np.float32)
    path = str(tmp_path / "f.png")
    dmme_amd.save_png(path, torch.from_numpy(img))
    assert np.array_equal(R.read_png(path), R.to_uint8(img))
    grey = str(tmp_path / "g.png")
    dmme_amd.save_png(grey, img[0])  # (H, W): greyscale
    assert np.array_equal(R.read_png(grey), R.to_uint8(img[:1]))
    for bad in (np.zeros((2, 4, 4), np.uint8), np.zeros((3, 4), np.int32), np.zeros((4, 3, 4, 4), np.uint8)):
        with pytest.raises(ValueError):
            dmme_amd.save_png(str(tmp_path / "bad.png"), bad)


def test_restated_uint8_rule_truncates_after_the_half():
    assert R.to_uint8(np.float32([0.0, 1.0, 0.5, -3.0, 7.0])).tolist() == [0, 255, 128, 0, 255]
    k = np.arange(256, dtype=np.float32)
    assert np.array_equal(R.to_uint8(k / np.float32(255.0)), np.arange(256, dtype=np.uint8))


def test_restated_make_grid_layout():
    x = np.arange(5 * 1 * 2 * 3, dtype=np.float32).reshape(5, 1, 2, 3) + 1
    g = R.make_grid(x, 2)
    assert g.shape == (3, 3 * 4 + 2, 2 * 5 + 2) and np.array_equal(g[0], g[2])
    assert np.array_equal(g[1, 2 + 4:2 + 4 + 2, 2 + 5:2 + 5 + 3], x[3, 0])  # image 3: row 1, column 1
    assert g[:, :2].sum() == 0 and g[:, :, :2].sum() == 0 and g[:, 10:, 7:].sum() == 0  # padding and the empty sixth cell
    assert R.make_grid(x[:1], 4).shape == (3, 2, 3)
    h = R.make_history([x[:2], x[2:4]])
    assert h.shape == (3, 2 * 4 + 2, 2 * 5 + 2) and np.array_equal(h[0, 2:4, 7:10], x[2, 0]) and np.array_equal(h[0, 6:8, 2:5], x[1, 0])


# ------------------------------------------------------------------------------------------ ABI
def test_grid_tile_rejects_bad_arguments_without_a_gpu():
    lib = _lib.lib()
    assert lib.dmme_version() >= 113
    p = C.c_void_p(16)
    good = dict(x=p, B=2, C=3, H=4, W=6, cell0=1, cell_stride=3, xmaps=3, ymaps=2, pad=2, out_kind=0, raw=0, canvas=p, stream=None)

    def call(**kw):
        return lib.dmme_grid_tile(*{**good, **kw}.values())

    for kw in (dict(x=None), dict(canvas=None), dict(B=0), dict(C=0), dict(H=-1), dict(W=0), dict(xmaps=0), dict(ymaps=0), dict(pad=-1),
               dict(cell0=-1), dict(cell0=3), dict(cell_stride=0), dict(cell_stride=5), dict(B=3), dict(out_kind=2), dict(out_kind=-1),
               dict(raw=2)):
        assert call(**kw) == -1, kw
        assert b"grid_tile" in lib.dmme_last_error(), kw
    with pytest.raises(ValueError, match="grid_tile"):
        _lib.check(call(out_kind=7), "dmme_grid_tile")


def test_package_exports_the_history_surface():
    for name in ("make_history", "save_png", "HistoryRecorder", "history_ordinals", "GenerateImage"):
        assert name in dmme_amd.__all__ and hasattr(dmme_amd, name)
    assert dmme_amd.callbacks.GenerateImage is dmme_amd.GenerateImage
    import inspect

    for cls, meth in ((dmme_amd.DDPM, "generate"), (dmme_amd.DDIM, "generate"), (dmme_amd.GeneralizedDDIM, "generate"), (dmme_amd.IDDPM, "generate"),
                      (dmme_amd.DPMSolverPP, "generate"), (dmme_amd.ClassifierFreeDDPM, "generate"), (dmme_amd.ClassifierFreeDDIM, "generate"),
                      (dmme_amd.ClassifierFreeDPMSolver, "generate"), (dmme_amd.ClassifierGuidedDDPM, "generate"), (dmme_amd.ClassifierGuidedDDIM, "generate"),
                      (dmme_amd.RePaint, "inpaint"), (dmme_amd.RePaint, "edit"), (dmme_amd.RePaint, "generate")):
        par = inspect.signature(getattr(cls, meth)).parameters
        assert "history" in par and par["history"].default is None, (cls.__name__, meth)
    run = inspect.signature(dmme_amd.diffusion_models.ddpm.ChainRunner.run).parameters
    assert list(run)[:3] == ["self", "first", "count"] and run["recorder"].default is None


# ------------------------------------------------------------------------------------------ YAML
_CALLBACKS_YAML = """
seed_everything: true
trainer:
  callbacks:
    - class_path: pytorch_lightning.callbacks.ModelCheckpoint
      init_args:
        save_last: true
    - class_path: pytorch_lightning.callbacks.LearningRateMonitor
    - class_path: dmme.callbacks.GenerateImage
      init_args:
        imgsize:
          - 1
          - 28
          - 28
        timesteps: 1_000
        vis_length: 7
        batch_size: 4
  max_steps: 10
model:
  class_path: dmme.LitDDPM
"""


def _generate_image_of(conf):
    got = [cb for cb in conf["callbacks"] if isinstance(cb, dmme_amd.GenerateImage)]
    assert len(got) == 1 and len(conf["callbacks"]) == 1  # (Lightning's own callbacks are not instantiated)
    return got[0]


def test_yaml_generate_image_entry_is_parsed(tmp_path):
    from dmme_amd import trainer

    cb = _generate_image_of(trainer.parse_config(os.path.join(ROOT, "configs", "ddpm", "cifar10.yaml")))
    assert cb.imgsize == (3, 32, 32) and cb.timesteps == 1000 and cb.vis_length == 20 and cb.batch_size == 8 and cb.every_n_epochs == 5
    path = tmp_path / "cb.yaml"
    path.write_text(_CALLBACKS_YAML)
    cb = _generate_image_of(trainer.parse_config(str(path)))
    assert cb.imgsize == (1, 28, 28) and cb.timesteps == 1000 and isinstance(cb.timesteps, int) and cb.vis_length == 7 and cb.batch_size == 4
    assert trainer._resolve("dmme.callbacks.GenerateImage") is dmme_amd.GenerateImage
    assert trainer.parse_config(os.path.join(ROOT, "configs", "ddim", "cifar10.yaml"))["callbacks"] == []


@pytest.mark.skipif(not os.path.isdir("/root/reference/configs"), reason="reference checkout absent (GPU box)")
def test_reference_ddpm_yaml_yields_its_generate_image():
    """build container only: the reference's own configs/ddpm/cifar10.yaml, read in place"""
    from dmme_amd import trainer

    cb = _generate_image_of(trainer.parse_config("/root/reference/configs/ddpm/cifar10.yaml"))
    assert cb.imgsize == (3, 32, 32) and cb.timesteps == 1000 and cb.vis_length == 20


def test_trainer_refuses_grid_flags_in_the_wrong_place():
    from dmme_amd import trainer

    cfg = os.path.join(ROOT, "configs", "ddpm", "cifar10.yaml")
    for argv in (["fit", "--config", cfg, "--grid", "x.png"], ["sample", "--config", cfg, "--vis-length", "4"],
                 ["sample", "--config", cfg, "--grid", "x.png", "--vis-length", "0"], ["sample", "--config", cfg, "--grid", "x.png", "--steps", "3"],
                 ["fit", "--config", cfg, "--preview-dir", "d"], ["fit", "--config", cfg, "--preview-every", "5"],
                 ["sample", "--config", cfg, "--preview-dir", "d", "--preview-every", "5"],
                 ["fit", "--config", cfg, "--preview-dir", "d", "--preview-every", "0"]):
        with pytest.raises(SystemExit) as exc:
            trainer.main(argv)
        assert isinstance(exc.value.code, str), argv  # a message, not argparse's usage error
