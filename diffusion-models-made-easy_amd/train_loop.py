"""Plain training loop behind `python -m dmme_amd.trainer fit` (stands in for pl.Trainer.fit on
the keys of configs/ddpm/cifar10.yaml that touch the hot path).  Synthetic CIFAR10-shaped data:
x_0 = 2 U[0,1) - 1 (there is no dataset in the image; the input pipeline is out of scope)."""

from __future__ import annotations

import json
import os
import time

import torch

from . import distributed as D
from .common.noise import gaussian


def synthetic_batch(batch_size: int, device, shape=(3, 32, 32)):
    return torch.rand((batch_size, *shape), device=device) * 2 - 1


def train_step(module, optimizer, scheduler, x0, clip=None, reduce=True, exchange=None, y=None):
    """one optimisation step: loss -> HIP backward (data parallel: the gradient exchange of the first bucket runs on a side
    stream under the rest of backward) -> clip+Adam(+EMA) -> LR step.  `reduce=False` leaves the gradient exchange out
    (bench.py times the step without its collective to tell exposed from hidden exchange time).  `exchange`: wire format of
    the gradient mean (distributed.make_reducer: "fp32-allreduce" | "bf16-rs-ag"; default DMME_EXCHANGE or fp32).  `y`: the batch's class
    labels, handed to a conditional module (lit_modules.LitClassifierFreeDDPM) next to the images."""
    model = module.diffusion_model.model
    reducer = getattr(model, "_grad_reducer", None)
    multi = reduce and D.dist.is_available() and D.dist.is_initialized() and D.dist.get_world_size() > 1
    if multi and not getattr(model, "_dp_synced", False):  # first data-parallel step: identical replicas (rank 0's weights)
        D.sync_parameters(model, optimizer)
        model._dp_synced = True
    if multi and not os.environ.get("DMME_NO_OVERLAP"):
        want = D.run_exchange(model, int(x0.shape[0]), exchange)  # decided once per run, rank 0's choice (16-bit models at <= 32 images per rank: bf16)
        if reducer is not None and reducer.exchange != want:
            reducer.detach()
            reducer = None
        if reducer is None:
            reducer = model._grad_reducer = D.make_reducer(model, want)
        reducer.attach()
    elif reducer is not None:
        # no exchange in this step: the hook must be gone BEFORE backward runs, or that backward would issue all-reduces (and divide
        # the gradients) on the side stream with nobody waiting for them
        reducer.detach()
    loss = module.training_step((x0,) if y is None else (x0, y), 0)
    loss.backward()
    if multi:
        if reducer is not None and getattr(model, "_bucket_hook", None) is not None and reducer.finish():
            if hasattr(optimizer, "grad_scale"):
                optimizer.grad_scale = reducer.grad_scale()
            elif reducer.grad_scale() != 1.0:
                model.flat_grad().mul_(reducer.grad_scale())
        else:
            D.allreduce_mean_flat(model.flat_grad())
    optimizer.step()
    if scheduler is not None:
        scheduler.step()
    optimizer.zero_grad()
    return loss


def write_preview(module, callback, directory: str, step: int) -> str:
    """`directory`/step_<step>.png: the callback's history grid (callbacks.GenerateImage.grid: one recorded chain of the module's
    current weights, uint8 on the device, one copy to the host at the end)"""
    from .common.vis import save_png

    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"step_{step}.png")
    save_png(path, callback.grid(module, out_kind=1))
    return path


def fit(module, batch_size=128, max_steps=100, clip=None, log_every=50, loader=None, ckpt_path=None, save_path=None, preview=None):
    """`preview`: (GenerateImage, directory, N) - rank 0 writes a history grid every N optimiser steps (steps, not the callback's
    epochs: synthetic-data runs have no epochs); None: nothing changes"""
    dev = next(module.parameters()).device
    module.train()
    opts, scheds = module.configure_optimizers()
    opt = opts[0]
    if clip:
        for g in opt.param_groups:
            g["max_grad_norm"] = float(clip)
    sched = scheds[0]["scheduler"] if scheds else None
    first = 0
    if ckpt_path:
        from .checkpoint import load_checkpoint

        first = int(load_checkpoint(ckpt_path, module, opt, sched).get("global_step", 0))
        if hasattr(module.diffusion_model, "reset_target"):
            module.diffusion_model.reset_target()  # (consistency distillation: the target network is not in a checkpoint and restarts from the student)
    model = module.diffusion_model.model
    after_step = getattr(module.diffusion_model, "after_step", None)  # (consistency distillation: the target network's moving average)
    if D.sync_parameters(model, opt):  # several ranks: start from rank 0's weights (after a resume too)
        model._dp_synced = True
    t0 = time.perf_counter()
    batches = None
    conditional = bool(getattr(module, "conditional", False))  # the module's training_step takes (images, labels)
    for step in range(first, max_steps):
        y = None
        if loader is None:
            x0 = synthetic_batch(batch_size, dev)
            if conditional:
                y = torch.randint(0, model.num_classes, (batch_size,), device=dev)
        else:  # epochs over the HBM-resident set: a fresh permutation each time the loader is exhausted
            try:
                batch = next(batches)
            except (StopIteration, TypeError):
                batches = iter(loader)
                batch = next(batches)
            x0 = batch[0]
            if conditional:
                y = batch[1]
        loss = train_step(module, opt, sched, x0, clip, y=y)
        if after_step is not None:
            after_step()
        if preview is not None and (step + 1) % preview[2] == 0 and D.env_rank_world()[0] == 0:
            print(json.dumps({"step": step + 1, "preview": write_preview(module, preview[0], preview[1], step + 1)}), flush=True)
        if (step + 1) % log_every == 0 or step + 1 == max_steps:
            torch.cuda.synchronize()
            if hasattr(model, "check_engine"):
                model.check_engine()  # a level-engine hand-off that timed out since the last log line: stop, do not train on it
            if conditional:
                model.check_labels()  # a label outside [0, num_classes] that reached the device since the last log line
            if after_step is not None:
                module.diffusion_model.check_indices()  # a grid index outside 1..N that reached the device since the last log line
            dt = time.perf_counter() - t0
            print(json.dumps({"step": step + 1, "train/loss": round(float(loss.detach()), 5), "images_per_s": round((step + 1 - first) * batch_size / dt, 1)}), flush=True)
    if save_path and D.env_rank_world()[0] == 0:
        from .checkpoint import save_checkpoint

        save_checkpoint(save_path, module, opt, sched, global_step=max(max_steps, first))
    return module


def _batches(loader, batch_size, dev):
    """endless (x0,) stream: synthetic batches, or epochs over the loader"""
    while True:
        if loader is None:
            yield synthetic_batch(batch_size, dev)
        else:
            for batch in loader:
                yield batch[0]


def fit_distill(module, steps_from: int, steps_to: int, stage_steps: int, batch_size=128, clip=None, log_every=50, loader=None, save_path=None):
    """progressive distillation behind `python -m dmme_amd.trainer distill`: stages N = steps_from, steps_from / 2, ..., steps_to of
    `stage_steps` optimiser steps each, `halve()` between them, the optimiser and its schedule built fresh for every stage (`module`: a
    lit_modules.LitDistill whose process stands at steps_from).  One JSON line per log interval: stage N, step, loss, images/s."""
    dm = module.diffusion_model
    if dm.steps != steps_from:
        raise ValueError(f"fit_distill: the process stands at {dm.steps} steps, the first stage is {steps_from}")
    dev = next(module.parameters()).device
    model = dm.model
    module.stage_steps = int(stage_steps)
    stream = _batches(loader, batch_size, dev)
    total = 0
    while True:
        module.train()
        opts, scheds = module.configure_optimizers()
        opt, sched = opts[0], scheds[0]["scheduler"]
        if clip:
            for g in opt.param_groups:
                g["max_grad_norm"] = float(clip)
        if D.sync_parameters(model, opt):
            model._dp_synced = True
        t0 = time.perf_counter()
        for step in range(stage_steps):
            loss = train_step(module, opt, sched, next(stream), clip)
            if (step + 1) % log_every == 0 or step + 1 == stage_steps:
                torch.cuda.synchronize()
                if hasattr(model, "check_engine"):
                    model.check_engine()
                dm.check_indices()
                dt = time.perf_counter() - t0
                print(json.dumps({"stage": dm.steps, "step": step + 1, "train/loss": round(float(loss.detach()), 5),
                                  "images_per_s": round((step + 1) * batch_size / dt, 1)}), flush=True)
        total += stage_steps
        if dm.steps <= steps_to:
            break
        dm.halve()
    if save_path and D.env_rank_world()[0] == 0:
        from .checkpoint import save_checkpoint

        save_checkpoint(save_path, module, opt, sched, global_step=total)
    return module
