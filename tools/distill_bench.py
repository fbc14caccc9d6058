"""Cost of a progressive-distillation step on the GPU (run on the MI355X; DESIGN's section on distillation quotes its output).

  step      one optimisation step of dmme_amd.LitDistill (noise launch, teacher forward, mid launch, teacher forward, target launch, the
            student's training step) on bench.py's flagship network at the CIFAR10 shape, against its parts measured in the same process:
            the plain training step of the same network under the same loss weights, and one no-grad forward with a timestep per image.
            The yardstick is that sum of parts - one training step plus two forwards; the legs run in alternating blocks, timed by events
            on the launch stream, and every figure comes with its spread over the blocks.
  launches  the three new launches alone, in microseconds per call.

usage: python tools/distill_bench.py [--batch 128] [--precision bf16] [--steps 20] [--warmup 10] [--blocks 3] [--student-steps 256]
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


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _timed_blocks(legs, per_block, blocks):
    """legs: {name: callable doing one step}.  `blocks` rounds; in each, every leg runs `per_block` steps between two events.
    Returns {name: [ms per step of each block]}."""
    out = {k: [] for k in legs}
    for _ in range(blocks):
        for name, one in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(per_block):
                one()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / per_block)
    return out


def _figure(ms):
    return {"ms": round(_median(ms), 4), "spread_ms": round(max(ms) - min(ms), 4), "blocks_ms": [round(v, 4) for v in ms]}


def step_legs(args, dev):
    torch.manual_seed(1337)
    student, side, T, _, _, label = bench.workload(dmme_amd, "ddpm", args.precision)
    teacher = bench.workload(dmme_amd, "ddpm", args.precision)[0]
    student.to(dev)
    teacher.to(dev)
    teacher.load_state_dict(student.state_dict())
    B, N = args.batch, args.student_steps
    process = dmme_amd.ProgressiveDistillation(student, teacher, T, N, prediction="v").to(dev)
    lit = dmme_amd.LitDistill(process, stage_steps=10 ** 6).train()
    plain = dmme_amd.LitDDPM(diffusion_model=dmme_amd.DDPM(student, T, prediction="v", loss_weight="truncated-snr").to(dev)).train()
    opts = {"distill": lit.configure_optimizers()[0][0], "train": FusedAdam(student.parameters(), lr=1e-4)}
    x0 = synthetic_batch(B, dev, (3, side, side))
    z = dmme_amd.gaussian(x0.shape, device=dev)
    t = torch.randint(1, T + 1, (B,), device=dev)

    def forward():
        with torch.no_grad():
            teacher(z, t)

    legs = {"distill": lambda: train_step(lit, opts["distill"], None, x0, 1.0), "train": lambda: train_step(plain, opts["train"], None, x0, 1.0), "forward": forward}
    for g in opts.values():
        for group in g.param_groups:
            group["max_grad_norm"] = 1.0
    for one in legs.values():
        for _ in range(args.warmup):
            one()
    ms = _timed_blocks(legs, args.steps, args.blocks)
    student.check_engine()
    teacher.check_engine()
    process.check_indices()
    parts = [a + 2.0 * b for a, b in zip(ms["train"], ms["forward"])]
    diff = [a - b for a, b in zip(ms["distill"], parts)]
    out = {"workload": label, "batch": B, "student_steps": N, "timed_steps_per_leg": args.steps * args.blocks, "distill_step": _figure(ms["distill"]),
           "train_step": _figure(ms["train"]), "forward_nograd_per_image_t": _figure(ms["forward"]), "train_plus_two_forwards": _figure(parts),
           "distill_minus_parts": _figure(diff), "distill_over_parts": round(_median(ms["distill"]) / _median(parts), 4),
           "images_per_s": round(1e3 * B / _median(ms["distill"]), 1)}
    return out


def launch_legs(args, dev):
    lib = _lib.lib()
    B, chw, N, T = args.batch, 3 * 32 * 32, args.student_steps, 1000
    p = dmme_amd.ProgressiveDistillation(torch.nn.Identity(), torch.nn.Identity(), T, N, prediction="v").to(dev)
    x0, z, o1, o2 = (dmme_amd.gaussian((B, chw), device=dev) for _ in range(4))
    idx = torch.randint(1, N + 1, (B,), device=dev)
    z_t, z_m, tgt = torch.empty_like(x0), torch.empty_like(x0), torch.empty_like(x0)
    t, m = torch.empty(B, dtype=torch.int64, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    s = _lib.stream_ptr()
    legs = {
        "noise": lambda: _lib.check(lib.dmme_distill_noise(_lib.ptr(x0), _lib.ptr(z), _lib.ptr(idx), _lib.ptr(p._tt), _lib.ptr(p._sqrt_alpha_bar),
                                                           _lib.ptr(p._sqrt_one_minus_alpha_bar), N, B, chw, _lib.ptr(z_t), _lib.ptr(t), _lib.ptr(m), _lib.ptr(p._status), s)),
        "mid": lambda: _lib.check(lib.dmme_distill_mid(p._pred, 0, _lib.ptr(z_t), _lib.ptr(o1), _lib.ptr(p._rows), _lib.ptr(idx), N, B, chw, _lib.ptr(z_m), s)),
        "target": lambda: _lib.check(lib.dmme_distill_target(p._pred, 0, _lib.ptr(z_t), _lib.ptr(o1), _lib.ptr(z_m), _lib.ptr(o2), _lib.ptr(p._rows), _lib.ptr(idx), N, B, chw,
                                                             _lib.ptr(tgt), s)),
    }
    for one in legs.values():
        for _ in range(args.warmup):
            one()
    ms = _timed_blocks(legs, args.launch_calls, args.blocks)
    p.check_indices()
    moved = {"noise": 3, "mid": 3, "target": 5}
    return {k: {"us": round(1e3 * _median(v), 2), "spread_us": round(1e3 * (max(v) - min(v)), 2), "bytes_moved": moved[k] * 4 * B * chw} for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--student-steps", type=int, default=256, help="N of the student (the teacher samples in 2N)")
    ap.add_argument("--steps", type=int, default=20, help="timed steps per leg and block")
    ap.add_argument("--launch-calls", type=int, default=200, help="timed calls of each new launch per block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3, help="alternated repetitions")
    ap.add_argument("--only", default=None, choices=["step", "launches"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "distill_bench", "precision": args.precision}
    if args.only in (None, "launches"):
        out["launches"] = launch_legs(args, dev)
    if args.only in (None, "step"):
        out["step"] = step_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
