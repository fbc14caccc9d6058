"""Minimal runner for the reference's LightningCLI YAML files
(`dmme.trainer fit --config configs/ddpm/cifar10.yaml`, reference src/dmme/trainer.py:4-9).

pytorch_lightning / jsonargparse are not part of this image, so the runner parses the
same YAML with PyYAML and applies jsonargparse's rule itself: every `init_args` value is
converted to the type its constructor parameter is annotated with (`lr: 2e-4` is a string
to YAML 1.1 and a float to `LitDDPM.__init__(lr: float)`; `800_000` an int; an
`Optional[nn.Module]` parameter takes a nested `class_path` / `init_args` block).  It
honours the keys that affect the hot path and ignores the Lightning-only ones (loggers,
checkpoint callbacks, ...):

  model.class_path / init_args[.model.init_args]   -> dmme_amd.LitDDPM / LitDDIM (+ UNet overrides)
  data.init_args.batch_size                         -> synthetic batches of that size (default), or with `--data config`
                                                       the YAML's data module (dmme.CIFAR10: HBM-resident uint8 set, GPU flip + norm)
  trainer.max_steps, gradient_clip_val, precision, log_every_n_steps, devices
  trainer.callbacks: dmme.callbacks.GenerateImage   -> dmme_amd.GenerateImage (what `fit --preview-dir` samples)
  seed_everything

  python -m dmme_amd.trainer fit    --config configs/ddpm/cifar10.yaml [--max-steps N] [--batch-size B]
  python -m dmme_amd.trainer sample --config configs/ddim/cifar10.yaml [--num-images N] [--steps K] [--sampler ddim-paper --eta E]
  python -m dmme_amd.trainer sample --config configs/iddpm/cifar10.yaml --sample-steps K    (Improved DDPM: K << T strided steps)
  python -m dmme_amd.trainer sample --config configs/cfg/cifar10.yaml --labels 3,5 --guidance-scale 2.5   (classifier-free guidance)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler dpm++ --sample-steps 20   (DPM-Solver++(2M); any of the four configs)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler repaint --image X.npy --mask M.npy --save OUT.npy   (RePaint inpainting)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler ilvr --image X.npy --down-factor 8 --save OUT.npy   (ILVR: samples that share X's coarse content)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler ddnm --measurement Y.npy --sr-scale 4 --save OUT.npy   (DDNM: 4x super-resolution of Y; --gray colourises, --mask inpaints)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler dps --operator blur --blur-size 9 --blur-sigma 2 --zeta 1 --sigma-y 0.05 --image X.npy --save OUT.npy   (DPS: deblurring a noisy measurement; --operator identity | blur | bicubic | average [--down-scale s], --measurement Y.npy, --mask inpaints)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler heun --sample-steps 30 [--tau-schedule logsnr]   (the Heun walk on the probability-flow ODE: two network evaluations per node)
  python -m dmme_amd.trainer evaluate --config configs/ddpm/cifar10.yaml --ckpt-path OUT.ckpt --nodes 100 --image X.npy [--dequantize] [--num-images K]   (bits/dim under the probability-flow ODE, mean and per image; --data config: the YAML's data module)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler analytic --sample-steps 20 [--eta 1] [--tau-schedule linear] [--moments G.npy | --data config [--moment-images 64]] [--save-checkpoint OUT.ckpt]
                                    (Analytic-DPM: the optimal reverse variance on a K-step grid; the moments come from G.npy, from the checkpoint, or are estimated first on the YAML's data module)
  python -m dmme_amd.trainer evaluate --config configs/ddpm/cifar10.yaml --ckpt-path OUT.ckpt --sampler analytic --variance analytic --sample-steps 100 --image X.npy
                                    (bits/dim by the K-step variational bound, with its prior, KL sum and decoder parts; --variance analytic | beta | beta-tilde)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --sampler sdedit--image X.npy --strength 0.5 --save OUT.npy   (SDEdit editing)
  python -m dmme_amd.trainer sample --config configs/ddpm/cifar10.yaml --num-images 8 --vis-length 20 --grid OUT.png   (the denoising history as a PNG; any sampler)
  python -m dmme_amd.trainer sample --config configs/cfg/cifar10.yaml --labels 3 --guidance-scale 2.5 --threshold dynamic   (x0 thresholding in front of the update: none | static | dynamic [--threshold-percentile P]; any sampler)
  python -m dmme_amd.trainer fit    --config configs/vpred/cifar10.yaml   (a v-prediction network under min-SNR weights; --prediction / --loss-weight / --snr-gamma override any YAML)
  python -m dmme_amd.trainer fit    --config configs/ddpm/cifar10.yaml --preview-dir DIR --preview-every N   (a history grid DIR/step_<n>.png every N optimiser steps)
  python -m dmme_amd.trainer distill --config configs/vpred/cifar10.yaml --ckpt-path TEACHER.ckpt --distill-from 1024 --distill-to 4 --stage-steps 50000 --save-checkpoint OUT.ckpt
                                    (progressive distillation: a teacher sampled in 1024 DDIM steps becomes a 4-step student, one halving per stage; [--clip-x0] [--data config])
  python -m dmme_amd.trainer sample --config configs/vpred/cifar10.yaml --ckpt-path OUT.ckpt   (a distilled checkpoint samples with the steps and the grid it was trained for)
  python -m dmme_amd.trainer consistency --config configs/vpred/cifar10.yaml --ckpt-path TEACHER.ckpt --consistency-steps 50 --max-steps M --save-checkpoint OUT.ckpt
                                    (consistency distillation: one run, then 1-, 2- or 4-step samples; [--metric l2] [--huber-c C] [--target-decay 0.95] [--clip-x0] [--data config])
  python -m dmme_amd.trainer sample --config configs/vpred/cifar10.yaml --ckpt-path OUT.ckpt --sample-steps 2   (a consistency checkpoint samples in K steps, K a divisor of its grid; default 1)
"""

from __future__ import annotations

import argparse
import importlib
import json
import sys
import time
import inspect
import typing
from typing import Any, Dict

import torch
import yaml


def _resolve(class_path: str):
    """`dmme.X` in a reference YAML means this package's drop-in X."""
    mod, _, name = class_path.rpartition(".")
    if class_path == "torchvision.transforms.RandomHorizontalFlip":  # the flip runs on the GPU inside dmme_image_batch
        mod = "dmme_amd.data_modules"
    if mod == "dmme" or mod.startswith("dmme."):
        mod = "dmme_amd" + mod[4:]
    return getattr(importlib.import_module(mod), name)


def _number(text: str, kind):
    """YAML 1.1 scalars jsonargparse reads as numbers: `2e-4` (no dot: a string to PyYAML), `800_000`"""
    cleaned = text.strip().replace("_", "")
    if kind is int:
        try:
            return int(cleaned, 0)
        except ValueError:
            as_float = float(cleaned)
            if as_float != int(as_float):
                raise
            return int(as_float)
    return float(cleaned)


def _coerce(value: Any, annotation: Any) -> Any:
    """Convert a parsed YAML value to the annotated parameter type (the subset of jsonargparse's typing rules the
    reference's configs exercise: float / int / bool / str, Optional and Union, Sequence / List / Tuple of those,
    sub-class specs as `class_path` + `init_args`)."""
    if isinstance(value, dict) and "class_path" in value:
        return _instantiate(value)
    if annotation is inspect.Parameter.empty or annotation is Any or annotation is None:
        return _instantiate(value) if isinstance(value, list) else value
    origin = typing.get_origin(annotation)
    args = typing.get_args(annotation)
    if origin is typing.Union:
        if value is None and type(None) in args:
            return None
        last = None
        for cand in args:
            if cand is type(None):
                continue
            try:
                return _coerce(value, cand)
            except (TypeError, ValueError) as exc:
                last = exc
        raise last if last else TypeError(f"{value!r} matches no member of {annotation}")
    if origin in (list, tuple, typing.Sequence) or (isinstance(origin, type) and issubclass(origin, (list, tuple, typing.Sequence))) \
            or origin is __import__("collections").abc.Sequence:
        if not isinstance(value, (list, tuple)):
            raise TypeError(f"expected a sequence for {annotation}, got {value!r}")
        if origin is tuple and args and not (len(args) == 2 and args[1] is Ellipsis):
            items = [_coerce(v, a) for v, a in zip(value, args)]
        else:
            inner = args[0] if args else Any
            items = [_coerce(v, inner) for v in value]
        return tuple(items) if origin is tuple else items
    if annotation is float:
        if isinstance(value, bool):
            raise TypeError(f"expected a float, got {value!r}")
        if isinstance(value, (int, float)):
            return float(value)
        if isinstance(value, str):
            return _number(value, float)
        raise TypeError(f"expected a float, got {value!r}")
    if annotation is int:
        if isinstance(value, bool):
            raise TypeError(f"expected an int, got {value!r}")
        if isinstance(value, int):
            return value
        if isinstance(value, float) and value == int(value):
            return int(value)
        if isinstance(value, str):
            return _number(value, int)
        raise TypeError(f"expected an int, got {value!r}")
    if annotation is bool:
        if isinstance(value, bool):
            return value
        if isinstance(value, str) and value.lower() in ("true", "false"):
            return value.lower() == "true"
        raise TypeError(f"expected a bool, got {value!r}")
    if annotation is str:
        if isinstance(value, str):
            return value
        raise TypeError(f"expected a str, got {value!r}")
    if isinstance(value, list):
        return [_instantiate(v) for v in value]
    return value


def _init_annotations(cls) -> Dict[str, Any]:
    """parameter name -> annotation over the class and its bases (a subclass that forwards **kwargs inherits its parent's)"""
    out: Dict[str, Any] = {}
    for klass in reversed(inspect.getmro(cls)):
        init = klass.__dict__.get("__init__")
        if init is None:
            continue
        try:
            hints = typing.get_type_hints(init)
        except Exception:  # noqa: BLE001 - unresolved forward references: fall back to the raw annotations
            hints = getattr(init, "__annotations__", {})
        for name, par in inspect.signature(init).parameters.items():
            if name == "self":
                continue
            ann = hints.get(name, par.annotation)
            if isinstance(ann, str):
                ann = inspect.Parameter.empty
            out[name] = ann
    return out


def _instantiate(spec: Any):
    if isinstance(spec, dict) and "class_path" in spec:
        cls = _resolve(spec["class_path"])
        hints = _init_annotations(cls)
        kwargs = {}
        for k, v in (spec.get("init_args") or {}).items():
            try:
                kwargs[k] = _coerce(v, hints.get(k, inspect.Parameter.empty))
            except (TypeError, ValueError) as exc:
                raise TypeError(f"{spec['class_path']}: init_args.{k} = {v!r} does not fit the parameter's type {hints.get(k)}: {exc}") from exc
        return cls(**kwargs)
    if isinstance(spec, list):
        return [_instantiate(v) for v in spec]
    return spec


def _callbacks(specs) -> list:
    """the entries of trainer.callbacks this package has a counterpart for (`dmme.callbacks.GenerateImage`), instantiated; Lightning's
    own (ModelCheckpoint: --save-checkpoint, LearningRateMonitor) are not"""
    return [_instantiate(s) for s in specs or [] if isinstance(s, dict) and str(s.get("class_path", "")).startswith("dmme.")]


def preview_callback(conf: Dict[str, Any], module, image_size=None):
    """the GenerateImage the previews of `fit` come from: the YAML's entry when there is one, else one built from the model (its
    channels, the data module's image size, the process's timesteps) and the callback's defaults"""
    from .callbacks import GenerateImage

    for cb in conf.get("callbacks") or []:
        if isinstance(cb, GenerateImage):
            return cb
    dm = module.diffusion_model
    hw = image_size or conf["image_size"]
    return GenerateImage((dm.model.in_channels, hw, hw), dm.timesteps)


def parse_config(path: str) -> Dict[str, Any]:
    with open(path) as f:
        cfg = yaml.safe_load(f)
    trainer = cfg.get("trainer") or {}
    data_args = ((cfg.get("data") or {}).get("init_args")) or {}
    precision = trainer.get("precision", 32)
    p16 = str(precision) in ("16", "16-mixed")
    pbf = str(precision) in ("bf16", "bf16-mixed")
    return {
        "model_spec": cfg["model"],
        "data_spec": cfg.get("data"),
        "batch_size": _coerce(data_args.get("batch_size", 128), int),
        "max_steps": _coerce(trainer.get("max_steps") if trainer.get("max_steps") is not None else -1, int),
        "gradient_clip_val": _coerce(trainer.get("gradient_clip_val"), typing.Optional[float]),
        # `precision: 16` (configs/ddpm/cifar10.yaml:53) is fp16 autocast under a GradScaler in the reference: here IEEE-half tensors and
        # MFMA operands with fp32 accumulation and master weights, under the device-resident dynamic loss scaling of the fused optimiser
        # pass (optim.FusedAdam(amp=True), include/dmme_hip.h: dmme_amp_*) - for `fit` and for sampling alike
        "precision": "fp16" if p16 else "bf16" if pbf else "fp32",
        "sample_precision": "fp16" if p16 else "bf16" if pbf else "fp32",
        # images the YAML's data module yields (dmme.CIFAR10: 32 x 32; dmme.LSUN: init_args.imgsize, configs/ddpm/lsun_church.yaml:94)
        "image_size": _coerce(data_args.get("imgsize", 32), int),
        "log_every_n_steps": _coerce(trainer.get("log_every_n_steps") or 50, int),
        "devices": trainer.get("devices", 1),
        "seed": cfg.get("seed_everything", 1337),
        "ckpt_path": cfg.get("ckpt_path"),
        "callbacks": _callbacks(trainer.get("callbacks")),
    }


PREDICTION_FLAGS = ("prediction", "loss_weight", "snr_gamma")


def override_prediction(conf: Dict[str, Any], **overrides) -> None:
    """--prediction / --loss-weight / --snr-gamma over the YAML: written into the init_args of the block that builds the process (a nested
    `diffusion_model` where the YAML has one, else the Lit module's own); exits where that class takes no such argument (Improved DDPM)"""
    given = {k: v for k, v in overrides.items() if v is not None}
    if not given:
        return
    spec = conf["model_spec"] = dict(conf["model_spec"])
    args = spec["init_args"] = dict(spec.get("init_args") or {})
    inner = args.get("diffusion_model")
    if isinstance(inner, dict) and "class_path" in inner:
        spec = args["diffusion_model"] = dict(inner)
        args = spec["init_args"] = dict(spec.get("init_args") or {})
    cls = _resolve(spec["class_path"])
    missing = [k for k in given if k not in inspect.signature(cls.__init__).parameters]
    if missing:
        raise SystemExit(f"{spec['class_path']} takes no {', '.join('--' + k.replace('_', '-') for k in missing)}: it is written for eps prediction and its own loss")
    args.update(given)


def build_module(conf: Dict[str, Any]):
    module = _instantiate(conf["model_spec"])
    unet = module.diffusion_model.model
    if hasattr(unet, "set_precision"):
        unet.set_precision(conf["precision"])
    return module


def _check_solver_args(args) -> None:
    """what goes with --sampler dpm++ and what does not; exits with a message (before anything touches the GPU)"""
    # (--tau-schedule linear / quadratic also goes with --sampler ddim-paper: the grid of GeneralizedDDIM; --clip-x0 also with `distill`)
    paper_tau = args.sampler == "ddim-paper" and args.tau_schedule in ("linear", "quadratic")
    paper_tau = paper_tau or args.sampler == "heun" or args.command == "evaluate"  # (the probability-flow ODE's grid takes all three)
    paper_tau = paper_tau or args.sampler == "analytic"  # (`_check_analytic_args`: linear | quadratic)
    solver_flags = [f for f, given in (("--solver-order", args.solver_order is not None), ("--tau-schedule", args.tau_schedule is not None and not paper_tau),
                                       ("--clip-x0", args.clip_x0 and args.command not in ("distill", "consistency"))) if given]
    if args.sampler != "dpm++":
        if solver_flags:
            raise SystemExit(f"{', '.join(solver_flags)} belong{'s' if len(solver_flags) == 1 else ''} to --sampler dpm++")
        return
    if args.command != "sample":
        raise SystemExit("--sampler dpm++ belongs to `sample`: DPM-Solver++ is a sampler, training is the config's own")
    if args.eta is not None:
        raise SystemExit("--eta belongs to --sampler ddim-paper: DPM-Solver++(2M) is deterministic")
    if args.steps is not None:
        raise SystemExit("--sampler dpm++ runs whole chains: --sample-steps K sets their length, --steps does not apply")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")


def _check_threshold_args(args) -> None:
    """what goes with --threshold and what does not; exits with a message (before anything touches the GPU)"""
    if args.threshold is None and args.threshold_percentile is None:
        return
    if args.command != "sample":
        raise SystemExit("--threshold / --threshold-percentile belong to `sample`: x0 thresholding is a sampler's, training does not clip")
    if args.threshold_percentile is not None:
        if args.threshold != "dynamic":
            raise SystemExit("--threshold-percentile belongs to --threshold dynamic")
        if not 0.0 <= args.threshold_percentile <= 1.0:
            raise SystemExit(f"--threshold-percentile {args.threshold_percentile} outside [0, 1]")


DISTILL_FLAGS = (("--distill-from", "distill_from"), ("--distill-to", "distill_to"), ("--stage-steps", "stage_steps"))


def _check_distill_args(args) -> None:
    """what goes with `distill` and what does not; exits with a message (before anything touches the GPU)"""
    given = [f for f, name in DISTILL_FLAGS if getattr(args, name) is not None]
    if args.command != "distill":
        if given:
            raise SystemExit(f"{', '.join(given)} belong{'s' if len(given) == 1 else ''} to `distill`")
        return
    missing = [f for f, name in DISTILL_FLAGS if getattr(args, name) is None]
    if missing:
        raise SystemExit(f"distill needs {', '.join(missing)}")
    if args.ckpt_path is None:
        raise SystemExit("distill needs --ckpt-path TEACHER.ckpt: the trained network whose sampler is distilled")
    if args.save_checkpoint is None:
        raise SystemExit("distill needs --save-checkpoint OUT.ckpt: the student is its only result")
    if args.sampler != "config" or args.max_steps is not None:
        raise SystemExit("--sampler / --max-steps do not go with `distill`: --stage-steps K sets the length of every stage")
    n0, n1 = args.distill_from, args.distill_to
    if n1 < 1 or n0 <= n1:
        raise SystemExit(f"--distill-from {n0} --distill-to {n1}: the teacher's steps must exceed the last student's, which are at least 1")
    ratio = n0 // n1
    if n0 % n1 != 0 or ratio & (ratio - 1) != 0:
        raise SystemExit(f"--distill-from {n0} --distill-to {n1}: every stage halves the steps, so the first must be the last times a power of two")
    if args.stage_steps < 1:
        raise SystemExit("--stage-steps must be at least 1")


CONSISTENCY_FLAGS = (("--consistency-steps", "consistency_steps"), ("--metric", "metric"), ("--huber-c", "huber_c"), ("--target-decay", "target_decay"))


def _check_consistency_args(args) -> None:
    """what goes with `consistency` and what does not; exits with a message (before anything touches the GPU)"""
    given = [f for f, name in CONSISTENCY_FLAGS if getattr(args, name) is not None]
    if args.command != "consistency":
        if given:
            raise SystemExit(f"{', '.join(given)} belong{'s' if len(given) == 1 else ''} to `consistency`")
        return
    if args.consistency_steps is None or args.max_steps is None:
        raise SystemExit("consistency needs --consistency-steps N (the training grid) and --max-steps M (the optimiser steps of its one run)")
    if args.ckpt_path is None:
        raise SystemExit("consistency needs --ckpt-path TEACHER.ckpt: the trained network that is distilled")
    if args.save_checkpoint is None:
        raise SystemExit("consistency needs --save-checkpoint OUT.ckpt: the student is its only result")
    if args.sampler != "config" or args.sample_steps is not None:
        raise SystemExit("--sampler / --sample-steps do not go with `consistency`: `sample --ckpt-path OUT.ckpt --sample-steps K` samples its student")
    if args.consistency_steps < 1 or args.max_steps < 1:
        raise SystemExit("--consistency-steps and --max-steps must be at least 1")
    if args.huber_c is not None and (args.metric == "l2" or not args.huber_c > 0.0):
        raise SystemExit("--huber-c C > 0 belongs to the pseudo-Huber metric")
    if args.target_decay is not None and not 0.0 <= args.target_decay <= 1.0:
        raise SystemExit(f"--target-decay {args.target_decay} outside [0, 1]")


def _consistency(args, conf, B, rank_seed=None) -> int:
    """`consistency`: the YAML's network twice (teacher and student, both from --ckpt-path), then one run of train_loop.fit"""
    from .checkpoint import load_checkpoint
    from .diffusion_models import ConsistencyDistillation
    from .lit_modules import LitConsistency
    from .train_loop import fit

    if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
        raise SystemExit("consistency needs an unconditional config: guided consistency distillation is out of scope")
    built = []
    for _ in range(2):
        module = build_module(conf).cuda()
        load_checkpoint(args.ckpt_path, module, strict=False)
        built.append(module)
    if rank_seed is not None:
        torch.manual_seed(rank_seed)
    old = built[0].diffusion_model
    try:
        process = ConsistencyDistillation(built[1].diffusion_model.model, old.model, old.timesteps, args.consistency_steps, prediction=old.prediction,
                                          clip_x0=args.clip_x0, metric=args.metric or "pseudo-huber", huber_c=args.huber_c,
                                          target_decay=args.target_decay or 0.0).cuda()
    except (NotImplementedError, ValueError) as exc:
        raise SystemExit(str(exc))
    lit = LitConsistency(process, lr=built[0].lr).cuda()
    loader = None
    if args.data == "config" and conf["data_spec"]:
        data = _instantiate(conf["data_spec"])
        data.batch_size = B
        try:
            data.prepare_data()
        except FileNotFoundError as e:
            print(json.dumps({"data": "random bytes (dataset files absent)", "reason": str(e)[:160]}), flush=True)
            data.synthetic = True
        data.setup("fit")
        loader = data.train_dataloader()
    fit(lit, batch_size=B, max_steps=args.max_steps, clip=conf["gradient_clip_val"], log_every=conf["log_every_n_steps"], loader=loader,
        save_path=args.save_checkpoint)
    return 0


def _distill(args, conf, B, rank_seed=None) -> int:
    """`distill`: the YAML's network twice (teacher and student, both from --ckpt-path), then the stages of train_loop.fit_distill"""
    from .checkpoint import load_checkpoint
    from .diffusion_models import ProgressiveDistillation
    from .lit_modules import LitDistill
    from .train_loop import fit_distill

    if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
        raise SystemExit("distill needs an unconditional config: classifier-free distillation is out of scope")
    built = []
    for _ in range(2):
        module = build_module(conf).cuda()
        load_checkpoint(args.ckpt_path, module, strict=False)
        built.append(module)
    if rank_seed is not None:
        torch.manual_seed(rank_seed)
    old = built[0].diffusion_model
    if args.distill_from > old.timesteps:
        raise SystemExit(f"--distill-from {args.distill_from}: the process has {old.timesteps} timesteps")
    try:
        process = ProgressiveDistillation(built[1].diffusion_model.model, old.model, old.timesteps, args.distill_from // 2, prediction=old.prediction,
                                          clip_x0=args.clip_x0).cuda()
    except NotImplementedError as exc:
        raise SystemExit(str(exc))
    lit = LitDistill(process, lr=built[0].lr, stage_steps=args.stage_steps).cuda()
    loader = None
    if args.data == "config" and conf["data_spec"]:
        data = _instantiate(conf["data_spec"])
        data.batch_size = B
        try:
            data.prepare_data()
        except FileNotFoundError as e:
            print(json.dumps({"data": "random bytes (dataset files absent)", "reason": str(e)[:160]}), flush=True)
            data.synthetic = True
        data.setup("fit")
        loader = data.train_dataloader()
    fit_distill(lit, args.distill_from // 2, args.distill_to, args.stage_steps, batch_size=B, clip=conf["gradient_clip_val"], log_every=conf["log_every_n_steps"],
                loader=loader, save_path=args.save_checkpoint)
    return 0


def _consistency_entry(args, conf):
    """the "consistency" entry of the checkpoint `sample` is given, or None (read on the host, before anything touches the GPU)"""
    path = args.ckpt_path or conf.get("ckpt_path")
    if not path:
        return None
    try:
        return torch.load(path, map_location="cpu", weights_only=False).get("consistency")
    except (OSError, RuntimeError, AttributeError):
        return None


def _dpm_solver(module, args):
    """DPM-Solver++(2M) over the network and the noise schedule of the process the YAML built (classifier-free where that one is)"""
    from .diffusion_models import DPMSolverPP

    old = module.diffusion_model
    kw = dict(sub_timesteps=20 if args.sample_steps is None else args.sample_steps, tau_schedule=args.tau_schedule or "logsnr",
              order=args.solver_order or 2, clip_x0=args.clip_x0)
    if getattr(module, "conditional", False):
        from .guidance.cfg import ClassifierFreeDPMSolver

        return ClassifierFreeDPMSolver.from_process(old, guidance_scale=old.guidance_scale, p_uncond=old.p_uncond, **kw)
    return DPMSolverPP.from_process(old, **kw)


def _check_flow_args(args) -> None:
    """what goes with --sampler heun and with `evaluate` (the probability-flow ODE: diffusion_models/pfode.py) and what does not; exits
    with a message (before anything touches the GPU)"""
    own = [f for f, given in (("--nodes", args.nodes is not None), ("--dequantize", args.dequantize)) if given]
    if args.command == "evaluate" and args.sampler == "analytic":
        if own:
            raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to the probability-flow likelihood, not to --sampler analytic (--sample-steps K sets its grid)")
        return  # (`_check_analytic_args` has looked at the rest)
    if args.command != "evaluate":
        if own:
            raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to `evaluate`")
        if args.sampler != "heun":
            return
        name = "--sampler heun"
        if args.command != "sample":
            raise SystemExit(f"{name} belongs to `sample`: the Heun walk is a sampler, training is the config's own")
        for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale)):
            if v is not None:
                raise SystemExit(f"{flag} does not go with {name}: it runs whole deterministic walks of an unconditional network (--sample-steps N sets the nodes)")
        if args.sample_steps is not None and args.sample_steps < 1:
            raise SystemExit("--sample-steps must be at least 1")
        return
    name = "`evaluate`"
    if args.sampler != "config":
        raise SystemExit(f"--sampler does not go with {name}: the likelihood is the probability-flow ODE's (--nodes N, --tau-schedule S)")
    for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--sample-steps", args.sample_steps), ("--labels", args.labels),
                    ("--guidance-scale", args.guidance_scale), ("--max-steps", args.max_steps)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: --nodes N sets the grid of the likelihood's walk")
    if args.prediction not in (None, "eps"):
        raise SystemExit(f"--prediction {args.prediction} does not go with {name}: the derivative of the x0 / v adapter is not built (an eps network only)")
    if args.nodes is not None and args.nodes < 1:
        raise SystemExit("--nodes must be at least 1")
    if args.num_images < 1:
        raise SystemExit("--num-images must be at least 1")
    if (args.image is not None) == (args.data == "config"):
        raise SystemExit(f"{name} needs exactly one of --image X.npy (float32 in [-1, 1]) and --data config (the YAML's data module)")
    if (args.precision or "").lower() == "fp16r32":
        raise SystemExit(f"--precision fp16r32 does not go with {name}: an inference mode without a backward")


def _flow_process(module, args, nodes_default: int):
    """ProbabilityFlow over the network, the noise schedule, the prediction and the thresholding of the process the YAML built"""
    from .diffusion_models import ProbabilityFlow

    old = module.diffusion_model
    nodes = args.sample_steps if args.command == "sample" else args.nodes
    try:
        return ProbabilityFlow.from_process(old, nodes=min(nodes_default, old.timesteps) if nodes is None else nodes, schedule=args.tau_schedule or "linear")
    except (ValueError, NotImplementedError) as exc:
        raise SystemExit(f"{'--sampler heun' if args.command == 'sample' else 'evaluate'}: {exc}")


def _data_loader(conf, batch_size: int):
    """the train loader of the YAML's data module at this batch size (random bytes where the dataset files are absent)"""
    dm = _instantiate(conf["data_spec"])
    dm.batch_size = batch_size
    try:
        dm.prepare_data()
    except FileNotFoundError as e:
        print(json.dumps({"data": "random bytes (dataset files absent)", "reason": str(e)[:160]}), flush=True)
        dm.synthetic = True
    dm.setup("fit")
    return dm.train_dataloader()


def _evaluate_images(args, conf) -> torch.Tensor:
    """the images `evaluate` scores: --image X.npy, or the first batch of the YAML's data module"""
    if args.image is not None:
        return _load_npy(args.image, "--image")[: args.num_images]
    return next(iter(_data_loader(conf, args.num_images)))[0][: args.num_images]


def _check_analytic_args(args) -> None:
    """what goes with --sampler analytic (Analytic-DPM: diffusion_models/analytic.py) and what does not; exits with a message (before
    anything touches the GPU)"""
    own = [f for f, v in (("--variance", args.variance), ("--moments", args.moments), ("--moment-images", args.moment_images)) if v is not None]
    if args.sampler != "analytic":
        if own:
            raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to --sampler analytic")
        return
    name = "--sampler analytic"
    if args.command not in ("sample", "evaluate"):
        raise SystemExit(f"{name} belongs to `sample` and `evaluate`: it needs no training, the network is the config's own")
    for flag, v in (("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale), ("--max-steps", args.max_steps)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: it runs whole chains of an unconditional network (--sample-steps K sets the grid)")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")
    if args.tau_schedule == "logsnr":
        raise SystemExit(f"--tau-schedule logsnr does not go with {name}: its grid is GeneralizedDDIM's (linear | quadratic)")
    if args.eta is not None and not 0.0 <= args.eta <= 1.0:
        raise SystemExit(f"--eta {args.eta} outside [0, 1]")
    if args.moments is not None and args.moment_images is not None:
        raise SystemExit("--moments G.npy installs a table, --moment-images M estimates one: give one of them")
    if args.moment_images is not None and args.moment_images < 1:
        raise SystemExit("--moment-images must be at least 1")
    if args.moment_images is not None and args.data != "config":
        raise SystemExit("--moment-images estimates the moments on data: it needs --data config (the YAML's data module)")
    if args.command == "sample":
        if args.variance is not None:
            raise SystemExit("--variance belongs to `evaluate`: sampling uses the analytic variance")
        return
    if args.eta not in (None, 1.0):
        raise SystemExit(f"--eta {args.eta} does not go with `evaluate`: the bound needs eta = 1 (the KL against a narrower posterior grows without limit)")
    if args.num_images < 1:
        raise SystemExit("--num-images must be at least 1")
    if args.image is None and args.data != "config":
        raise SystemExit("`evaluate` needs --image X.npy (float32 in [-1, 1]) or --data config (the YAML's data module)")


def _analytic_process(module, args, conf, B: int, ckpt):
    """AnalyticDPM over the network, the prediction and the thresholding of the process the YAML built, with its moments: --moments G.npy,
    else the checkpoint's where they cover the grid, else estimated here on the YAML's data module (--data config; --moment-images M per
    timestep, default 64).  Nothing is estimated on made-up images: such moments would travel in a checkpoint looking like any others.
    The module goes into eval mode first: the statistic is that of the network that samples, not of one that draws dropout masks."""
    import numpy as np

    from .diffusion_models import AnalyticDPM

    module.eval()
    old = module.diffusion_model
    K = min(50, old.timesteps) if args.sample_steps is None else args.sample_steps
    try:
        proc = AnalyticDPM(old.model, old.timesteps, K, args.tau_schedule or "linear", 1.0 if args.eta is None else args.eta, prediction=getattr(old, "prediction", "eps"),
                           threshold=getattr(old, "threshold", "none"), threshold_percentile=getattr(old, "threshold_percentile", 0.995))
    except ValueError as exc:
        raise SystemExit(f"--sampler analytic: {exc}")
    if not torch.equal(proc.alpha_bar.reshape(-1).cpu(), old.alpha_bar.reshape(-1).to(torch.float32).cpu()):
        raise SystemExit("--sampler analytic runs on the linear noise schedule of the DDPM / DDIM configs; this config's process has another one")
    proc = proc.cuda()
    tau = proc._tau_host[1:]
    state = (ckpt or {}).get("state_dict") or {}
    g_sum, g_count = state.get("diffusion_model._g_sum"), state.get("diffusion_model._g_count")
    source = None
    if args.moments is not None:
        try:
            proc.set_moments(np.load(args.moments, allow_pickle=False))
        except (OSError, ValueError) as exc:
            raise SystemExit(f"--moments {args.moments}: {exc}")
        source = "file"
    elif args.moment_images is None and g_sum is not None and g_count is not None and tuple(g_sum.shape) == tuple(proc._g_sum.shape) and bool((g_count[tau] > 0).all()):
        proc._g_sum.copy_(g_sum)
        proc._g_count.copy_(g_count)
        proc._moments_changed()
        source = "checkpoint"
    else:
        if args.data != "config" or not conf["data_spec"]:
            raise SystemExit("--sampler analytic: no moments for this grid in the checkpoint; give --moments G.npy, or --data config to estimate them on the YAML's data module")
        proc.estimate_moments(_data_loader(conf, B), images_per_timestep=args.moment_images or 64, batch_size=B, seed=None)
        source = "estimated on the data module"
    return proc, source


def _evaluate_analytic(module, args, conf, B: int, ckpt) -> int:
    """`evaluate --sampler analytic`: bits/dim by the K-step variational bound under --variance, with its three parts, as one JSON line"""
    module.eval()
    proc, source = _analytic_process(module, args, conf, B, ckpt)
    images = _evaluate_images(args, conf)
    t0 = time.perf_counter()
    parts = [proc.bits_per_dim(images[k:k + B].cuda(), variance=args.variance or "analytic") for k in range(0, images.shape[0], B)]
    torch.cuda.synchronize()
    total = torch.cat([p.total for p in parts]).cpu()
    prior = torch.cat([p.prior for p in parts]).cpu()
    terms = torch.cat([p.terms for p in parts]).cpu()
    mean = lambda v: round(float(v.mean()), 6)
    print(json.dumps({"images": list(images.shape), "precision": conf["precision"], "sample_steps": proc.sub_timesteps, "tau_schedule": proc.tau_schedule,
                      "variance": args.variance or "analytic", "moments": source, "bits_per_dim": mean(total), "prior": mean(prior), "kl_sum": mean(terms[:, 1:].sum(dim=1)),
                      "decoder": mean(terms[:, 0]), "per_image": [round(float(v), 6) for v in total], "seconds": round(time.perf_counter() - t0, 3)}))
    return 0


def _evaluate(module, args, conf, B: int) -> int:
    """`evaluate`: bits/dim of images under the probability-flow ODE of the checkpoint's network, mean and per image, as one JSON line"""
    module.eval()
    flow = _flow_process(module, args, 100).cuda()
    images = _evaluate_images(args, conf)
    t0 = time.perf_counter()
    try:
        bpd = torch.cat([flow.bits_per_dim(images[k:k + B].cuda(), dequantize=args.dequantize) for k in range(0, images.shape[0], B)])
    except NotImplementedError as exc:
        raise SystemExit(f"evaluate: {exc}")
    torch.cuda.synchronize()
    vals = [float(v) for v in bpd.cpu()]
    print(json.dumps({"images": list(images.shape), "precision": conf["precision"], "nodes": flow.nodes, "tau_schedule": flow.schedule, "dequantize": bool(args.dequantize),
                      "bits_per_dim": round(sum(vals) / len(vals), 6), "per_image": [round(v, 6) for v in vals], "seconds": round(time.perf_counter() - t0, 3)}))
    return 0


PAINT_SAMPLERS = ("repaint", "sdedit")


def _check_paint_args(args) -> None:
    """what goes with --sampler repaint / sdedit and what does not; exits with a message (before anything touches the GPU)"""
    given = [f for f, v in (("--image", args.image), ("--mask", args.mask), ("--strength", args.strength), ("--jump-length", args.jump_length),
                            ("--resamples", args.resamples)) if v is not None]
    if args.sampler in ("ilvr", "ddnm", "dps"):
        return  # (`_check_ilvr_args` / `_check_ddnm_args` / `_check_dps_args` have looked at all of these)
    if args.command == "evaluate":
        given = [f for f in given if f != "--image"]  # (`_check_flow_args`: the images whose likelihood is asked for)
    if args.sampler not in PAINT_SAMPLERS:
        if given:
            raise SystemExit(f"{', '.join(given)} belong{'s' if len(given) == 1 else ''} to --sampler repaint / sdedit")
        return
    name = f"--sampler {args.sampler}"
    if args.command != "sample":
        raise SystemExit(f"{name} belongs to `sample`: it conditions a trained network on pixels, training is the config's own")
    for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: it runs whole chains of an unconditional network (--sample-steps K sets the grid)")
    if args.image is None:
        raise SystemExit(f"{name} needs --image X.npy (float32 in [-1, 1], (B, C, H, W) or (C, H, W))")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")
    if args.sampler == "repaint":
        if args.mask is None:
            raise SystemExit("--sampler repaint needs --mask M.npy (1: keep the image's pixel, 0: generate it)")
        if args.strength is not None:
            raise SystemExit("--strength belongs to --sampler sdedit")
        for flag, v in (("--jump-length", args.jump_length), ("--resamples", args.resamples)):
            if v is not None and v < 1:
                raise SystemExit(f"{flag} must be at least 1")
    else:
        walk = [f for f, v in (("--jump-length", args.jump_length), ("--resamples", args.resamples)) if v is not None]
        if walk:
            raise SystemExit(f"{', '.join(walk)} belong{'s' if len(walk) == 1 else ''} to --sampler repaint: SDEdit walks straight down")
        if args.strength is None or not 0.0 < args.strength <= 1.0:
            raise SystemExit("--sampler sdedit needs --strength S in (0, 1]: the share of the noise levels the guide is pushed up")


def _check_ilvr_args(args):
    """what goes with --sampler ilvr and what does not; exits with a message (before anything touches the GPU).  Returns the reference
    image (--sampler ilvr) or None."""
    own = [f for f, v in (("--down-factor", args.down_factor), ("--range-level", args.range_level)) if v is not None]
    if args.sampler != "ilvr":
        if own:
            raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to --sampler ilvr")
        return None
    name = "--sampler ilvr"
    if args.command != "sample":
        raise SystemExit(f"{name} belongs to `sample`: it conditions a trained network on a reference image, training is the config's own")
    other = [f for f, v in (("--mask", args.mask), ("--strength", args.strength), ("--jump-length", args.jump_length), ("--resamples", args.resamples))
             if v is not None]
    if other:
        raise SystemExit(f"{', '.join(other)} belong{'s' if len(other) == 1 else ''} to --sampler repaint / sdedit, not to {name}")
    for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: it runs whole chains of an unconditional network (--sample-steps K sets the grid)")
    if args.image is None:
        raise SystemExit(f"{name} needs --image X.npy, the reference (float32 in [-1, 1], (B, C, H, W) or (C, H, W))")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")
    N = 4 if args.down_factor is None else args.down_factor
    if N < 2:
        raise SystemExit("--down-factor must be at least 2")
    if args.range_level is not None and args.range_level < 0:
        raise SystemExit("--range-level must be at least 0")
    image = _load_npy(args.image, "--image")
    H, W = image.shape[2:]
    if H % N != 0 or W % N != 0:
        raise SystemExit(f"--image {args.image}: the image size {H} x {W} is not divisible by --down-factor {N}")
    return image


def _ilvr_process(module, args):
    """ILVR over the network and the noise schedule of the process the YAML built"""
    from .diffusion_models import ILVR

    old = module.diffusion_model
    sub = min(250, old.timesteps) if args.sample_steps is None else args.sample_steps
    r = args.range_level or 0
    if r > sub:
        raise SystemExit(f"--range-level {r} lies above the grid's {sub} levels")
    return ILVR.from_process(old, sub_timesteps=sub, down_factor=args.down_factor or 4, range_level=r)


def _check_ddnm_flags(args) -> None:
    """the flags that only --sampler ddnm takes, in front of every check that opens a file"""
    own = [f for f, v in (("--sr-scale", args.sr_scale), ("--gray", args.gray or None), ("--sigma-y", args.sigma_y), ("--measurement", args.measurement))
           if v is not None]
    if args.sampler == "dps":  # (shares --sigma-y and --measurement; the operator has flags of its own)
        own = [f for f in own if f in ("--sr-scale", "--gray")]
    if args.sampler != "ddnm" and own:
        raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to --sampler ddnm")


def _check_ddnm_args(args):
    """what goes with --sampler ddnm and what does not; exits with a message (before anything touches the GPU).  Returns
    (measurement or None, image or None, mask or None) for --sampler ddnm, else None."""
    if args.sampler != "ddnm":
        return None
    name = "--sampler ddnm"
    if args.command != "sample":
        raise SystemExit(f"{name} belongs to `sample`: it restores images from a measurement with a trained network, training is the config's own")
    for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale),
                    ("--strength", args.strength)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: it runs whole chains of an unconditional network (--sample-steps K sets the grid)")
    if (args.measurement is None) == (args.image is None):
        raise SystemExit(f"{name} needs exactly one of --measurement Y.npy (the degraded input) and --image X.npy (degraded here first: the demo path)")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")
    S = 1 if args.sr_scale is None else args.sr_scale
    if S < 1:
        raise SystemExit("--sr-scale must be at least 1")
    if args.sigma_y is not None and not args.sigma_y >= 0.0:
        raise SystemExit("--sigma-y must be at least 0")
    for flag, v in (("--jump-length", args.jump_length), ("--resamples", args.resamples)):
        if v is not None and v < 1:
            raise SystemExit(f"{flag} must be at least 1")
    meas = image = None
    if args.image is not None:
        image = _load_npy(args.image, "--image")
        H, W = image.shape[2:]
        if H % S != 0 or W % S != 0:
            raise SystemExit(f"--image {args.image}: the image size {H} x {W} is not divisible by --sr-scale {S}")
        shape = (image.shape[0], 1 if args.gray else image.shape[1], H // S, W // S)
    else:
        meas = _load_npy(args.measurement, "--measurement")
        if args.gray and meas.shape[1] != 1:
            raise SystemExit(f"--measurement {args.measurement}: a --gray measurement has one channel, got {meas.shape[1]}")
        shape = tuple(meas.shape)
    mask = None if args.mask is None else _load_npy(args.mask, "--mask")
    if mask is not None and (mask.shape[0] not in (1, shape[0]) or mask.shape[1] not in (1, shape[1]) or tuple(mask.shape[2:]) != shape[2:]):
        raise SystemExit(f"--mask {args.mask}: shape {tuple(mask.shape)} does not broadcast to the measurement's {shape} (the mask is at measurement resolution)")
    if mask is not None and not bool(((mask == 0) | (mask == 1)).all()):
        raise SystemExit(f"--mask {args.mask}: values must be 0 or 1 (1: measured)")
    return meas, image, mask


def _ddnm_process(module, args):
    """DDNM over the network and the noise schedule of the process the YAML built"""
    from .diffusion_models import DDNM

    old = module.diffusion_model
    sub = min(100, old.timesteps) if args.sample_steps is None else args.sample_steps
    return DDNM.from_process(old, sub_timesteps=sub, scale=args.sr_scale or 1, gray=bool(args.gray), sigma_y=args.sigma_y or 0.0,
                             travel_length=args.jump_length or 1, travel_repeat=args.resamples or 1)


DPS_OPERATORS = ("identity", "blur", "bicubic", "average")


def _check_dps_flags(args) -> None:
    """the flags that only --sampler dps takes, in front of every check that opens a file"""
    own = [f for f, v in (("--operator", args.operator), ("--blur-size", args.blur_size), ("--blur-sigma", args.blur_sigma), ("--down-scale", args.down_scale),
                          ("--zeta", args.zeta)) if v is not None]
    if args.sampler != "dps" and own:
        raise SystemExit(f"{', '.join(own)} belong{'s' if len(own) == 1 else ''} to --sampler dps")


def _check_dps_args(args):
    """what goes with --sampler dps and what does not; exits with a message (before anything touches the GPU).  Returns
    (measurement or None, image or None, mask or None) for --sampler dps, else None."""
    if args.sampler != "dps":
        return None
    name = "--sampler dps"
    if args.command != "sample":
        raise SystemExit(f"{name} belongs to `sample`: it restores images from a measurement with a trained network, training is the config's own")
    for flag, v in (("--eta", args.eta), ("--steps", args.steps), ("--labels", args.labels), ("--guidance-scale", args.guidance_scale),
                    ("--strength", args.strength), ("--jump-length", args.jump_length), ("--resamples", args.resamples)):
        if v is not None:
            raise SystemExit(f"{flag} does not go with {name}: it runs whole chains of an unconditional network (--sample-steps K sets the grid)")
    if args.prediction not in (None, "eps"):
        raise SystemExit(f"--prediction {args.prediction} does not go with {name}: the derivative of the x0 / v adapter is not built (an eps network only)")
    if args.threshold not in (None, "none"):
        raise SystemExit(f"--threshold {args.threshold} does not go with {name}: the derivative of the clip is not built")
    if (args.measurement is None) == (args.image is None):
        raise SystemExit(f"{name} needs exactly one of --measurement Y.npy (the degraded input) and --image X.npy (degraded here first: the demo path)")
    if args.sample_steps is not None and args.sample_steps < 1:
        raise SystemExit("--sample-steps must be at least 1")
    op = args.operator or "identity"
    if op != "blur" and (args.blur_size is not None or args.blur_sigma is not None):
        raise SystemExit("--blur-size / --blur-sigma belong to --operator blur")
    if op not in ("bicubic", "average") and args.down_scale is not None:
        raise SystemExit("--down-scale belongs to --operator bicubic / average")
    if args.blur_size is not None and (args.blur_size < 1 or args.blur_size % 2 != 1):
        raise SystemExit("--blur-size must be an odd number of taps, at least 1")
    if args.blur_sigma is not None and not args.blur_sigma > 0.0:
        raise SystemExit("--blur-sigma must be positive")
    s = _dps_scale(args)
    if s < 1:
        raise SystemExit("--down-scale must be at least 1")
    if args.zeta is not None and not args.zeta >= 0.0:
        raise SystemExit("--zeta must be at least 0")
    if args.sigma_y is not None and not args.sigma_y >= 0.0:
        raise SystemExit("--sigma-y must be at least 0")
    meas = image = None
    if args.image is not None:
        image = _load_npy(args.image, "--image")
        H, W = image.shape[2:]
        if H % s != 0 or W % s != 0:
            raise SystemExit(f"--image {args.image}: the image size {H} x {W} is not divisible by --down-scale {s}")
        shape = (image.shape[0], image.shape[1], H // s, W // s)
    else:
        meas = _load_npy(args.measurement, "--measurement")
        shape = tuple(meas.shape)
    mask = None if args.mask is None else _load_npy(args.mask, "--mask")
    if mask is not None and (mask.shape[0] not in (1, shape[0]) or mask.shape[1] not in (1, shape[1]) or tuple(mask.shape[2:]) != shape[2:]):
        raise SystemExit(f"--mask {args.mask}: shape {tuple(mask.shape)} does not broadcast to the measurement's {shape} (the mask is at measurement resolution)")
    if mask is not None and not bool(((mask == 0) | (mask == 1)).all()):
        raise SystemExit(f"--mask {args.mask}: values must be 0 or 1 (1: measured)")
    return meas, image, mask


def _dps_scale(args) -> int:
    """s of the down-sampling operators (default 4), 1 for the ones that keep the size"""
    return (4 if args.down_scale is None else args.down_scale) if (args.operator or "identity") in ("bicubic", "average") else 1


def _dps_process(module, args, H: int, W: int):
    """DPS over the network and the noise schedule of the process the YAML built, with the operator for images of H x W"""
    from .diffusion_models import DPS, SeparableOperator

    old = module.diffusion_model
    sub = min(100, old.timesteps) if args.sample_steps is None else args.sample_steps
    try:
        op = SeparableOperator.preset(args.operator or "identity", H, W, blur_size=args.blur_size or 9, blur_sigma=args.blur_sigma or 2.0, scale=_dps_scale(args))
        return DPS.from_process(old, sub_timesteps=sub, operator=op, zeta=1.0 if args.zeta is None else args.zeta, sigma_y=args.sigma_y or 0.0)
    except (ValueError, NotImplementedError) as exc:
        raise SystemExit(f"--sampler dps: {exc}")


def _load_npy(path: str, what: str) -> torch.Tensor:
    """a float image array (B, C, H, W) or (C, H, W) from a .npy file, as a 4-D fp32 tensor"""
    import numpy as np

    try:
        arr = np.load(path, allow_pickle=False)
    except (OSError, ValueError) as exc:
        raise SystemExit(f"{what} {path}: {exc}")
    if arr.ndim == 3:
        arr = arr[None]
    if arr.ndim != 4 or not np.issubdtype(arr.dtype, np.floating):
        raise SystemExit(f"{what} {path}: a float array shaped (B, C, H, W) or (C, H, W), got {arr.dtype} {arr.shape}")
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32))


def _paint_process(module, args):
    """RePaint / SDEdit over the network and the noise schedule of the process the YAML built"""
    from .diffusion_models import RePaint

    old = module.diffusion_model
    sub = min(250, old.timesteps) if args.sample_steps is None else args.sample_steps
    return RePaint.from_process(old, sub_timesteps=sub, jump_length=args.jump_length or 10, resamples=args.resamples or 10)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="dmme_amd.trainer")
    ap.add_argument("command", choices=["fit", "sample", "distill", "consistency", "evaluate"])
    ap.add_argument("--config", required=True)
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None)
    ap.add_argument("--data", default="synthetic", choices=["synthetic", "config"],
                    help="fit: 'config' instantiates the YAML's data module (falls back to a random byte set when the CIFAR10 files are absent)")
    ap.add_argument("--ckpt-path", default=None, help="resume / sample from a Lightning-layout checkpoint (the YAML's ckpt_path key)")
    ap.add_argument("--save-checkpoint", default=None, help="fit: write a Lightning-layout checkpoint (weights, Adam moments, EMA copy) at the end")
    ap.add_argument("--num-images", type=int, default=16)
    ap.add_argument("--image-size", type=int, default=None, help="sample: image height = width (default: what the YAML's data module yields)")
    ap.add_argument("--precision", default=None, help="override the YAML's trainer.precision (fp32 | bf16 | fp16 | bf16x3)")
    ap.add_argument("--steps", type=int, default=None, help="sample: stop after this many denoising steps")
    ap.add_argument("--sampler", default="config", choices=["config", "ddim-paper", "dpm++", "repaint", "sdedit", "ilvr", "ddnm", "dps", "heun", "analytic"],
                    help="sample: 'ddim-paper' swaps the YAML's DDIM for GeneralizedDDIM (the published update) over the same network and tau table; "
                         "'dpm++' samples the YAML's network and noise schedule with DPM-Solver++(2M) in --sample-steps steps (default 20); "
                         "'repaint' inpaints --image where --mask is 0, 'sdedit' edits --image at --strength (any unconditional config; --sample-steps: grid levels, default 250); "
                         "'ilvr' samples images that share the low frequencies of --image (any unconditional config; --down-factor N, --range-level R, --sample-steps); "
                         "'ddnm' restores images from --measurement (or from --image, degraded first): super-resolution --sr-scale S, colourisation --gray, "
                         "inpainting --mask, a noisy measurement --sigma-y (any unconditional config; --sample-steps, default 100; --jump-length / --resamples: time travel); "
                         "'dps' restores images from a noisy --measurement (or from --image, degraded first) by posterior sampling: --operator identity | blur | bicubic | "
                         "average, step size --zeta, inpainting --mask, noise level --sigma-y (any unconditional eps config; --sample-steps, default 100); "
                         "'heun' samples with the second-order Heun walk on the probability-flow ODE (any unconditional config; --sample-steps N nodes, default 50, two "
                         "network evaluations per node; --tau-schedule linear (default) | quadratic | logsnr); "
                         "'analytic' samples with Analytic-DPM's optimal reverse variance on GeneralizedDDIM's grid (any unconditional config on the linear noise schedule; "
                         "--sample-steps K, default 50; --eta, default 1; --tau-schedule linear (default) | quadratic; the moments: --moments G.npy, the checkpoint's, or "
                         "with --data config estimated first, --moment-images M per timestep); evaluate --sampler analytic: bits/dim by the K-step variational bound under --variance")
    ap.add_argument("--variance", default=None, choices=["analytic", "beta", "beta-tilde"], help="evaluate --sampler analytic: the reverse variance of the bound (default analytic)")
    ap.add_argument("--moments", default=None, help="--sampler analytic: .npy, float64[T+1], the table G_t = E mean eps_theta^2 (entry 0 unused)")
    ap.add_argument("--moment-images", type=int, default=None, help="--sampler analytic --data config: estimate the moments on this many images per timestep, whatever the checkpoint holds (default 64 where none are at hand)")
    ap.add_argument("--nodes", type=int, default=None, help="evaluate: nodes of the likelihood's grid (default 100; two network evaluations and two input gradients per node)")
    ap.add_argument("--dequantize", action="store_true", help="evaluate: add uniform noise of one pixel step (2/255) to the images first, as published bits/dim figures do")
    ap.add_argument("--image", default=None, help="sample --sampler repaint / sdedit: .npy, float32 in [-1, 1], (B, C, H, W) or (C, H, W)")
    ap.add_argument("--mask", default=None, help="sample --sampler repaint (needed) / sdedit (optional): .npy broadcastable to the image, 1 = keep the pixel, 0 = generate")
    ap.add_argument("--strength", type=float, default=None, help="sample --sampler sdedit: in (0, 1], the share of the noise levels the guide is pushed up before it is denoised")
    ap.add_argument("--jump-length", type=int, default=None, help="sample --sampler repaint: levels a resampling jump climbs (default 10)")
    ap.add_argument("--resamples", type=int, default=None, help="sample --sampler repaint: times each stretch of --jump-length levels is walked (default 10)")
    ap.add_argument("--down-factor", type=int, default=None, help="sample --sampler ilvr: N of the low-pass filter, at least 2 and a divisor of the image size (default 4); small N stays close to --image")
    ap.add_argument("--range-level", type=int, default=None, help="sample --sampler ilvr: steps that end below this grid level are not conditioned (default 0: every step is)")
    ap.add_argument("--measurement", default=None, help="sample --sampler ddnm: .npy, the degraded input (B, Cm, h, w) or (Cm, h, w), float32 in [-1, 1]")
    ap.add_argument("--sr-scale", type=int, default=None, help="sample --sampler ddnm: s of the s x s average pooling the measurement went through (default 1: none); a divisor of the image size")
    ap.add_argument("--gray", action="store_true", help="sample --sampler ddnm: the measurement is the mean of the channels (colourisation)")
    ap.add_argument("--sigma-y", type=float, default=None, help="sample --sampler ddnm: the noise level of the measurement (default 0); with --image, noise of this level is added to the degraded image")
    ap.add_argument("--operator", default=None, choices=list(DPS_OPERATORS), help="sample --sampler dps: the measurement operator per channel plane (default identity)")
    ap.add_argument("--blur-size", type=int, default=None, help="sample --sampler dps --operator blur: taps of the Gaussian kernel, odd (default 9)")
    ap.add_argument("--blur-sigma", type=float, default=None, help="sample --sampler dps --operator blur: standard deviation of the Gaussian kernel in pixels (default 2)")
    ap.add_argument("--down-scale", type=int, default=None, help="sample --sampler dps --operator bicubic / average: the down-sampling factor, a divisor of the image size (default 4)")
    ap.add_argument("--zeta", type=float, default=None, help="sample --sampler dps: the step size of the gradient step on the measurement's residual (default 1; 0: the unconditioned chain)")
    ap.add_argument("--save", default=None, help="sample: write the images to this .npy file (float32, (B, C, H, W))")
    ap.add_argument("--grid", default=None, help="sample: write the images to this PNG file as a grid (every sampler; goes with --save)")
    ap.add_argument("--vis-length", type=int, default=1,
                    help="sample --grid: 1 (default) the final images in rows; L > 1 the denoising history, one row per image and up to L frames of its chain per row")
    ap.add_argument("--preview-dir", default=None, help="fit: write history grids of freshly sampled images to DIR/step_<n>.png (rank 0; the samples draw from the run's random stream)")
    ap.add_argument("--preview-every", type=int, default=None,
                    help="fit --preview-dir: every N optimiser steps - steps, not the epochs of the YAML's GenerateImage entry: synthetic-data runs have no epochs")
    ap.add_argument("--eta", type=float, default=None, help="sample --sampler ddim-paper: 0 (default) deterministic ... 1 DDPM's posterior variance")
    ap.add_argument("--solver-order", type=int, default=None, choices=[1, 2], help="sample --sampler dpm++: 2 (default) multistep second order, 1 first order")
    ap.add_argument("--tau-schedule", default=None, choices=["linear", "quadratic", "logsnr"], help="sample --sampler dpm++: the timestep grid (default logsnr); --sampler ddim-paper: linear | quadratic, over the YAML's")
    ap.add_argument("--clip-x0", action="store_true", help="sample --sampler dpm++: clamp every x0 prediction to [-1, 1] (wanted with the cosine schedule of the iddpm config, "
                         "whose abar_T = 1.9e-15 scales the first x0 prediction by 2.3e7); distill: clamp the teacher's two x0 estimates")
    ap.add_argument("--labels", default=None, help="sample, class-conditional configs: comma-separated class labels, one per image or one for all (e.g. 3,5,7)")
    ap.add_argument("--guidance-scale", type=float, default=None, help="sample, class-conditional configs: s of e_u + s (e_c - e_u); 1 = conditional, 0 = unconditional")
    ap.add_argument("--sample-steps", type=int, default=None,
                    help="sample, Improved DDPM configs: a strided chain over this many of the T timesteps, with the learned variance; "
                         "sample --sampler dpm++: the solver's steps")
    ap.add_argument("--prediction", default=None, choices=["eps", "x0", "v"], help="what the network predicts, over the YAML's `prediction` (default eps)")
    ap.add_argument("--loss-weight", default=None, choices=["uniform", "min-snr", "truncated-snr"], help="fit: the loss's weight per timestep, over the YAML's `loss_weight`")
    ap.add_argument("--snr-gamma", type=float, default=None, help="fit --loss-weight min-snr: the SNR the weight is clipped at (default 5)")
    ap.add_argument("--distill-from", type=int, default=None, help="distill: the DDIM steps the teacher is sampled in (the first student takes half)")
    ap.add_argument("--distill-to", type=int, default=None, help="distill: the steps of the last student; --distill-from is this times a power of two")
    ap.add_argument("--stage-steps", type=int, default=None, help="distill: optimiser steps of every halving stage (the rate falls linearly to zero within each)")
    ap.add_argument("--consistency-steps", type=int, default=None, help="consistency: N of the training grid linear_tau(T, N); the student samples in any K that divides it")
    ap.add_argument("--metric", default=None, choices=["pseudo-huber", "l2"], help="consistency: the loss's metric per image (default pseudo-huber)")
    ap.add_argument("--huber-c", type=float, default=None, help="consistency: c of the pseudo-Huber metric (default 0.00054 sqrt(C H W))")
    ap.add_argument("--target-decay", type=float, default=None,
                    help="consistency: 0 (default) the target network is the student itself; in (0, 1] a third network that follows the student at this moving-average rate")
    ap.add_argument("--threshold", default=None, choices=["none", "static", "dynamic"],
                    help="sample, every sampler: clip the x0 each noise prediction implies, in front of the update - static: to [-1, 1] (clip_denoised); "
                         "dynamic: to the image's --threshold-percentile quantile of |x0| where above 1, rescaled (wanted with --guidance-scale above 1)")
    ap.add_argument("--threshold-percentile", type=float, default=None, help="sample --threshold dynamic: the quantile, in [0, 1] (default 0.995)")
    args = ap.parse_args(argv)
    _check_solver_args(args)
    _check_distill_args(args)
    _check_consistency_args(args)
    _check_threshold_args(args)
    _check_ddnm_flags(args)
    _check_dps_flags(args)
    ilvr_image = _check_ilvr_args(args)
    ddnm_inputs = _check_ddnm_args(args)
    dps_inputs = _check_dps_args(args)
    _check_paint_args(args)
    _check_analytic_args(args)
    _check_flow_args(args)
    if args.save is not None and args.command != "sample":
        raise SystemExit("--save belongs to `sample` (fit: --save-checkpoint)")
    if args.command != "sample" and (args.grid is not None or args.vis_length != 1):
        raise SystemExit("--grid / --vis-length belong to `sample` (fit: --preview-dir)")
    if args.vis_length < 1 or (args.vis_length != 1 and args.grid is None):
        raise SystemExit("--vis-length L >= 1 goes with --grid OUT.png")
    if args.grid is not None and args.steps is not None:
        raise SystemExit("--grid records whole chains: --steps does not go with it")
    if (args.preview_dir is None) != (args.preview_every is None) or (args.preview_dir is not None and args.command != "fit"):
        raise SystemExit("fit --preview-dir DIR --preview-every N go together")
    if args.preview_every is not None and args.preview_every < 1:
        raise SystemExit("--preview-every must be at least 1")

    from . import _lib
    from . import distributed as D

    conf = parse_config(args.config)
    override_prediction(conf, prediction=args.prediction, loss_weight=args.loss_weight, snr_gamma=args.snr_gamma)
    if args.sampler in PAINT_SAMPLERS:
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit(f"--sampler {args.sampler} needs an unconditional config: guided inpainting / editing is not implemented")
        image = _load_npy(args.image, "--image")
        mask = None if args.mask is None else _load_npy(args.mask, "--mask")
    elif args.sampler == "ilvr":
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit("--sampler ilvr needs an unconditional config: guided ILVR is not implemented")
        image = ilvr_image
    elif args.sampler == "ddnm":
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit("--sampler ddnm needs an unconditional config: guided DDNM is not implemented")
        measurement, image, mask = ddnm_inputs
    elif args.sampler == "dps":
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit("--sampler dps needs an unconditional config: guided DPS is not implemented")
        measurement, image, mask = dps_inputs
    elif args.sampler == "analytic":
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit("--sampler analytic needs an unconditional config: guided Analytic-DPM is not implemented")
    elif args.sample_steps is not None and args.sampler == "config" and args.command == "sample" and args.steps is None and _consistency_entry(args, conf) is not None:
        pass  # (a consistency checkpoint: --sample-steps K is the K of its sampler)
    elif args.sampler == "heun" or args.command == "evaluate":
        if getattr(_resolve(conf["model_spec"]["class_path"]), "conditional", False):
            raise SystemExit(f"{'--sampler heun' if args.command == 'sample' else 'evaluate'} needs an unconditional config: the guided probability-flow ODE is not implemented")
    elif args.sample_steps is not None and args.sampler != "dpm++":
        from .lit_modules import LitIDDPM

        cls = _resolve(conf["model_spec"]["class_path"])
        if not (isinstance(cls, type) and issubclass(cls, LitIDDPM)):
            raise SystemExit("--sample-steps needs an Improved DDPM config (LitIDDPM: the strided chain uses the learned variance)")
        if args.command != "sample" or args.steps is not None or args.sampler != "config":
            raise SystemExit("--sample-steps belongs to `sample` and replaces --steps / --sampler")
    if args.precision:
        conf["precision"] = conf["sample_precision"] = args.precision
    if args.command in ("sample", "evaluate"):
        conf["precision"] = conf["sample_precision"]
    _lib.require_gpu()  # the product path is the HIP denoiser: no CPU fallback (the CPU plumbing run of BASELINE configs[0] is bench.py --mode cpu-plumbing)
    # one process per GPU under `python -m torch.distributed.run` (the reference reaches DDP through trainer.devices / strategy)
    rank, local, world = D.init_from_env()
    torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    seed = conf["seed"] if isinstance(conf["seed"], int) and not isinstance(conf["seed"], bool) else 1337
    torch.manual_seed(seed)  # identical initial weights on every rank ...
    if args.command == "consistency":
        return _consistency(args, conf, args.batch_size or conf["batch_size"], D.rank_seed(seed, rank) if world > 1 else None)
    if args.command == "distill":
        # (builds the YAML's network twice, teacher and student; several ranks: each draws from its own stream afterwards, as below)
        return _distill(args, conf, args.batch_size or conf["batch_size"], D.rank_seed(seed, rank) if world > 1 else None)
    module = build_module(conf).cuda()
    if world > 1:
        torch.manual_seed(D.rank_seed(seed, rank))  # ... then each rank's own stream for timesteps, noise and dropout masks
    B = args.batch_size or conf["batch_size"]

    ckpt_path = args.ckpt_path or conf.get("ckpt_path")
    distilled = consistency = None
    if args.command == "evaluate":
        ckpt = None
        if ckpt_path:
            from .checkpoint import load_checkpoint

            ckpt = load_checkpoint(ckpt_path, module, strict=False)
        if args.sampler == "analytic":
            return _evaluate_analytic(module, args, conf, B, ckpt)
        return _evaluate(module, args, conf, B)
    if args.command == "sample":
        ckpt = None
        if ckpt_path:
            from .checkpoint import load_checkpoint

            ckpt = load_checkpoint(ckpt_path, module, strict=False)
            distilled, consistency = ckpt.get("distill"), ckpt.get("consistency")
        if args.sampler != "config" or args.sample_steps is not None:
            distilled = None  # (an explicit sampler wins over the checkpoint's)
        if args.sampler != "config":
            consistency = None
        if consistency is not None:
            from .diffusion_models import ConsistencySampler

            old = module.diffusion_model
            try:
                module.diffusion_model = ConsistencySampler(old.model, old.timesteps, args.sample_steps or 1, int(consistency["steps"]),
                                                            prediction=consistency.get("prediction", old.prediction), sigma_data=consistency.get("sigma_data", 0.5),
                                                            timestep_scaling=consistency.get("timestep_scaling", 10.0)).cuda()
            except ValueError as exc:
                raise SystemExit(str(exc))
        if distilled is not None:
            from .diffusion_models import GeneralizedDDIM

            old = module.diffusion_model
            module.diffusion_model = GeneralizedDDIM(old.model, old.timesteps, int(distilled["steps"]), distilled.get("tau_schedule", "linear"), eta=0.0,
                                                     prediction=distilled.get("prediction", old.prediction)).cuda()
        if args.sampler == "ddim-paper":
            from .diffusion_models import DDIM, GeneralizedDDIM

            old = module.diffusion_model
            if not isinstance(old, DDIM):
                raise SystemExit("--sampler ddim-paper needs a DDIM config (sub_timesteps and a tau schedule)")
            module.diffusion_model = GeneralizedDDIM(old.model, old.timesteps, old.sub_timesteps, args.tau_schedule or old.tau_schedule, eta=args.eta or 0.0,
                                                     prediction=old.prediction).cuda()
        elif args.sampler == "dpm++":
            module.diffusion_model = _dpm_solver(module, args).cuda()
        elif args.sampler in PAINT_SAMPLERS:
            module.diffusion_model = _paint_process(module, args).cuda()
        elif args.sampler == "ilvr":
            module.diffusion_model = _ilvr_process(module, args).cuda()
        elif args.sampler == "ddnm":
            module.diffusion_model = _ddnm_process(module, args).cuda()
        elif args.sampler == "heun":
            module.diffusion_model = _flow_process(module, args, 50).cuda()
        elif args.sampler == "analytic":
            module.diffusion_model, moment_source = _analytic_process(module, args, conf, B, ckpt)
            if args.save_checkpoint is not None:  # (the moments travel in the state_dict: the next run finds them)
                from .checkpoint import save_checkpoint

                save_checkpoint(args.save_checkpoint, module)
        elif args.sampler == "dps":
            s = _dps_scale(args)
            H, W = tuple(image.shape[2:]) if image is not None else (measurement.shape[2] * s, measurement.shape[3] * s)
            module.diffusion_model = _dps_process(module, args, H, W).cuda()
        module.eval()
        dm = module.diffusion_model
        if args.threshold is not None:
            dm.set_threshold(args.threshold, args.threshold_percentile)  # (whatever process the sampler flags built: every kind reads one eps buffer)
        t0 = time.perf_counter()
        hw = args.image_size or conf["image_size"]
        shape = (args.num_images, dm.model.in_channels, hw, hw)
        rec = None
        if args.sampler == "ddnm":
            if image is not None:  # (the demo path: the measurement is made here, with noise of the level the sampler is told)
                import dmme_amd

                measurement = dm.degrade(image, mask)
                if dm.sigma_y > 0.0:
                    measurement = measurement + dm.sigma_y * dmme_amd.gaussian(tuple(measurement.shape), device=measurement.device)
            restored_shape = (measurement.shape[0], dm._channels(measurement.shape[1]), measurement.shape[2] * dm.scale, measurement.shape[3] * dm.scale)
        if args.sampler == "dps":
            if image is not None:  # (the demo path: the measurement is made here, with noise of the level the sampler is told)
                measurement = dm.degrade(image, mask)
            restored_shape = (measurement.shape[0], measurement.shape[1], dm.operator.H, dm.operator.W)
        if args.grid is not None:
            from .diffusion_models import HistoryRecorder, history_ordinals

            if args.sampler == "sdedit":
                count = dm.edit_level(args.strength)
            elif args.sample_steps is not None and args.sampler == "config" and consistency is None:
                count = dm._respaced_tables(args.sample_steps)[0]  # (Improved DDPM's strided chain)
            else:
                count = dm.chain_length()
            rec_shape = restored_shape if args.sampler in ("ddnm", "dps") else tuple(image.shape) if args.sampler in PAINT_SAMPLERS + ("ilvr",) else shape
            rec = HistoryRecorder(rec_shape[0], *rec_shape[1:], history_ordinals(count, args.vis_length), out_kind=1)
        if args.sampler == "repaint":
            imgs = dm.inpaint(image, mask, history=rec)
        elif args.sampler == "sdedit":
            imgs = dm.edit(image, args.strength, mask, history=rec)
        elif args.sampler == "ilvr":
            imgs = dm.sample_like(image, history=rec)
        elif args.sampler in ("ddnm", "dps"):
            imgs = dm.restore(measurement, mask, history=rec)
        elif getattr(module, "conditional", False):
            if args.steps is not None or args.sampler == "ddim-paper" or (args.sample_steps is not None and args.sampler != "dpm++"):
                raise SystemExit("class-conditional configs sample whole chains: --labels / --guidance-scale only")
            if args.guidance_scale is not None:
                dm.set_guidance_scale(args.guidance_scale)  # (the process stays what the YAML built: schedule, sampler, p_uncond)
            labels = [int(v) for v in args.labels.split(",")] if args.labels else [dm.model.null_label]
            if len(labels) == 1:
                labels = labels * args.num_images
            imgs = dm.generate(shape, labels, history=rec)
        elif args.labels is not None or args.guidance_scale is not None:
            raise SystemExit("--labels / --guidance-scale need a class-conditional config (LitClassifierFreeDDPM)")
        elif args.sampler in ("dpm++", "heun", "analytic"):
            imgs = dm.generate(shape, history=rec)
        elif args.sample_steps is not None and consistency is None:
            imgs = dm.generate(shape, sample_steps=args.sample_steps, history=rec)
        elif args.steps is None:
            imgs = dm.generate(shape, history=rec)
        else:
            import dmme_amd

            imgs = dmme_amd.gaussian(shape, device="cuda")
            first = dm.sub_timesteps if args.sampler == "ddim-paper" or distilled is not None or consistency is not None else dm.timesteps  # (the paper sampler's loop index counts sub-steps)
            for k in range(args.steps):
                imgs = module(imgs, first - k)
        torch.cuda.synchronize()
        if args.save is not None:
            import numpy as np

            np.save(args.save, imgs.detach().to(torch.float32).cpu().numpy())
        if rec is not None:
            from .common.vis import save_png

            save_png(args.grid, rec.canvas)
        line = {"images": list(imgs.shape), "precision": conf["precision"], "seconds": round(time.perf_counter() - t0, 3), "finite": bool(torch.isfinite(imgs).all())}
        if args.sampler == "analytic":
            line["analytic"] = {"sample_steps": int(dm.sub_timesteps), "eta": dm.eta, "tau_schedule": dm.tau_schedule, "moments": moment_source}
        if distilled is not None:
            line["distill"] = {"steps": int(distilled["steps"]), "tau_schedule": distilled.get("tau_schedule", "linear")}
        if consistency is not None:
            line["consistency"] = {"steps": int(consistency["steps"]), "sample_steps": int(dm.sub_timesteps)}
        print(json.dumps(line))
        return 0

    from .train_loop import fit

    steps = args.max_steps if args.max_steps is not None else conf["max_steps"]
    loader = None
    if args.data == "config" and conf["data_spec"]:
        dm = _instantiate(conf["data_spec"])
        dm.batch_size = B
        try:
            dm.prepare_data()
        except FileNotFoundError as e:
            print(json.dumps({"data": "random bytes (dataset files absent)", "reason": str(e)[:160]}), flush=True)
            dm.synthetic = True
        dm.setup("fit")
        loader = dm.train_dataloader()
    preview = None
    if args.preview_dir is not None:
        preview = (preview_callback(conf, module, args.image_size), args.preview_dir, args.preview_every)
    fit(module, batch_size=B, max_steps=steps, clip=conf["gradient_clip_val"], log_every=conf["log_every_n_steps"], loader=loader,
        ckpt_path=ckpt_path, save_path=args.save_checkpoint, preview=preview)
    return 0


if __name__ == "__main__":
    sys.exit(main())
