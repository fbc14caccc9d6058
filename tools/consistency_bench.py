"""Cost of a consistency-distillation step on the GPU (run on the MI355X; DESIGN's section on consistency distillation quotes its output).

  step      one optimisation step of dmme_amd.LitConsistency (noise launch, teacher forward, mid launch, target-network forward, target
            launch, the student's training step under the consistency loss, the target network's moving average) on bench.py's flagship
            network at the CIFAR10 shape, at target_decay 0 (the student is its own target) and 0.95 (a third network), against its parts
            measured in the same process: the plain training step of the same network, and one no-grad forward with a timestep per
            image.  The yardstick is that sum of parts - one training step plus two forwards; the legs run in alternating blocks, timed by
            events on the launch stream, and every figure comes with its spread over the blocks.
  launches  the three new launches alone, in microseconds per call.

usage: python tools/consistency_bench.py [--batch 128] [--precision bf16] [--steps 20] [--warmup 10] [--blocks 3] [--grid-steps 50]
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload definitions of the benchmark)
import dmme_amd  # noqa: E402
from dmme_amd import _lib  # noqa: E402
from dmme_amd.optim import FusedAdam  # noqa: E402
from dmme_amd.train_loop import synthetic_batch, train_step  # noqa: E402

from distill_bench import _figure, _median, _timed_blocks  # noqa: E402  (tools/ is the script's directory)


def step_legs(args, dev):
    torch.manual_seed(1337)
    student, side, T, _, _, label = bench.workload(dmme_amd, "ddpm", args.precision)
    teacher = bench.workload(dmme_amd, "ddpm", args.precision)[0]
    student.to(dev)
    teacher.to(dev)
    teacher.load_state_dict(student.state_dict())
    B, N = args.batch, args.grid_steps
    procs = {name: dmme_amd.ConsistencyDistillation(student, teacher, T, N, prediction="v", target_decay=decay).to(dev) for name, decay in (("cd_decay0", 0.0), ("cd_decay095", 0.95))}
    lits = {name: dmme_amd.LitConsistency(p).train() for name, p in procs.items()}
    plain = dmme_amd.LitDDPM(diffusion_model=dmme_amd.DDPM(student, T, prediction="v").to(dev)).train()
    opts = {name: lit.configure_optimizers()[0][0] for name, lit in lits.items()}
    opts["train"] = FusedAdam(student.parameters(), lr=1e-4)
    x0 = synthetic_batch(B, dev, (3, side, side))
    z = dmme_amd.gaussian(x0.shape, device=dev)
    t = torch.randint(1, T + 1, (B,), device=dev)

    def forward():
        with torch.no_grad():
            teacher(z, t)

    def cd(name):
        def one():
            train_step(lits[name], opts[name], None, x0, 1.0)
            procs[name].after_step()
        return one

    legs = {"cd_decay0": cd("cd_decay0"), "cd_decay095": cd("cd_decay095"), "train": lambda: train_step(plain, opts["train"], None, x0, 1.0), "forward": forward}
    for g in opts.values():
        for group in g.param_groups:
            group["max_grad_norm"] = 1.0
    for one in legs.values():
        for _ in range(args.warmup):
            one()
    ms = _timed_blocks(legs, args.steps, args.blocks)
    student.check_engine()
    teacher.check_engine()
    for p in procs.values():
        p.check_indices()
    parts = [a + 2.0 * b for a, b in zip(ms["train"], ms["forward"])]
    out = {"workload": label, "batch": B, "grid_steps": N, "timed_steps_per_leg": args.steps * args.blocks, "train_step": _figure(ms["train"]),
           "forward_nograd_per_image_t": _figure(ms["forward"]), "train_plus_two_forwards": _figure(parts)}
    for name in ("cd_decay0", "cd_decay095"):
        out[name] = {"step": _figure(ms[name]), "minus_parts": _figure([a - b for a, b in zip(ms[name], parts)]),
                     "over_parts": round(_median(ms[name]) / _median(parts), 4), "images_per_s": round(1e3 * B / _median(ms[name]), 1)}
    return out


def launch_legs(args, dev):
    lib = _lib.lib()
    B, chw, N, T = args.batch, 3 * 32 * 32, args.grid_steps, 1000
    p = dmme_amd.ConsistencyDistillation(torch.nn.Linear(1, 1), torch.nn.Linear(1, 1), T, N, prediction="v").to(dev)
    z_t, z_m, o_m, out = (dmme_amd.gaussian((B, chw), device=dev) for _ in range(4))
    idx = torch.randint(1, N + 1, (B,), device=dev)
    ft, d_out = torch.empty_like(z_t), torch.empty_like(z_t)
    loss, scratch = torch.empty(1, device=dev), torch.empty(65 * B, device=dev)
    numel = 32_416_643  # the flagship network's parameters
    dst, src = torch.zeros(numel, device=dev), torch.ones(numel, device=dev)
    s, c = _lib.stream_ptr(), p.huber_constant(chw)
    legs = {
        "cm_target": lambda: _lib.check(lib.dmme_cm_target(0, _lib.ptr(z_m), _lib.ptr(o_m), _lib.ptr(p._rows), _lib.ptr(idx), N, B, chw, _lib.ptr(ft), s)),
        "cm_loss": lambda: _lib.check(lib.dmme_cm_loss(0, _lib.ptr(z_t), _lib.ptr(out), _lib.ptr(ft), _lib.ptr(p._rows), _lib.ptr(idx), N, B, chw, c, _lib.ptr(loss),
                                                       _lib.ptr(None), _lib.ptr(d_out), 1.0, _lib.ptr(scratch), s)),
        "ema_lerp": lambda: _lib.check(lib.dmme_ema_lerp(_lib.ptr(dst), _lib.ptr(src), numel, 0.95, s)),
    }
    for one in legs.values():
        for _ in range(args.warmup):
            one()
    ms = _timed_blocks(legs, args.launch_calls, args.blocks)
    moved = {"cm_target": 3 * 4 * B * chw, "cm_loss": 7 * 4 * B * chw, "ema_lerp": 3 * 4 * numel}
    return {k: {"us": round(1e3 * _median(v), 2), "spread_us": round(1e3 * (max(v) - min(v)), 2), "bytes_moved": moved[k]} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--grid-steps", type=int, default=50, help="N of the training grid")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and block")
    ap.add_argument("--launch-calls", type=int, default=200, help="timed calls of each new launch per block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3, help="alternated repetitions")
    ap.add_argument("--only", default=None, choices=["step", "launches"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "consistency_bench", "precision": args.precision}
    if args.only in (None, "launches"):
        out["launches"] = launch_legs(args, dev)
    if args.only in (None, "step"):
        out["step"] = step_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
