"""Cost of x0 thresholding on the GPU (run on the MI355X; DESIGN's section on the stage quotes its output).

  chains  the replayed DDPM sampling step of bench.py's flagship workload (default UNet, CIFAR10 shape) with threshold "none", "static"
          and "dynamic": three processes over one network, one runner each, timed in alternating blocks by events on the launch stream.
  stage   the stand-alone stage (dmme_x0_threshold) on a batch of LSUN-shaped 3 x 256 x 256 images: static, and dynamic through the
          streaming form (seven launches), in microseconds per call; and on the CIFAR10 batch through the one-workgroup form.

usage: python tools/threshold_bench.py [--batch 128] [--precision bf16] [--chain-steps 400] [--warmup 20] [--blocks 4] [--big-batch 8]
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload definitions and the box calibration of the benchmark)
import dmme_amd  # noqa: E402
from dmme_amd import _lib  # noqa: E402
from dmme_amd.common.noise import philox_reserve  # noqa: E402
from dmme_amd.diffusion_models.ddpm import threshold_rank  # noqa: E402

MODES = ("none", "static", "dynamic")


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


def chain_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, proc_cls, _, _ = bench.workload(dmme_amd, "ddpm", args.precision)
    net.to(dev).eval()
    shape = (args.batch, 3, side, side)
    runners = {}
    for mode in MODES:
        proc = proc_cls(net, T, threshold=mode).to(dev)
        runners[mode] = proc.chain_runner(dmme_amd.gaussian(shape, device=dev))
    left = {k: 0 for k in runners}

    def stepper(name):
        runner = runners[name]

        def one():
            if left[name] == 0:  # a fresh chain from the top: a random network's chain does not stay in range for T steps
                runner.x.copy_(dmme_amd.gaussian(shape, device=dev))
                seed, off = philox_reserve(dev, runner.x.numel() * args.restart)
                runner.set(T, seed, off)
                left[name] = args.restart
            runner.step()
            left[name] -= 1
        return one

    legs = {k: stepper(k) for k in runners}
    with torch.no_grad():
        for one in legs.values():
            for _ in range(args.warmup):
                one()
        per_block = max(1, -(-args.chain_steps // args.blocks))
        ms = _timed_blocks(legs, per_block, args.blocks)
    for runner in runners.values():
        runner.plan.check()
    base = _median(ms["none"])
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, r in runners.items()},
           "image_bytes_per_step": 3 * 4 * runners["none"].x.numel()}
    for k in runners:
        m = _median(ms[k])
        out[k] = {"ms_per_step": round(m, 4), "steps_per_s": round(1e3 / m, 1), "over_none": round(m / base, 4), "added_us": round(1e3 * (m - base), 2),
                  "blocks_ms": [round(v, 4) for v in ms[k]]}
    return out


def stage_legs(args, dev):
    """the stage alone, eps restored in front of every call by a device copy that is timed on its own and subtracted"""
    lib = _lib.lib()
    proc = dmme_amd.DDPM(torch.nn.Identity(), 1000, threshold="dynamic").to(dev)
    tab = proc._thr_table(dev)
    t = torch.tensor([900], dtype=torch.int64, device=dev)
    out = {"lds_capacity": int(lib.dmme_x0_threshold_lds_capacity())}
    for name, (B, chw) in (("cifar", (args.batch, 3 * 32 * 32)), ("lsun256", (args.big_batch, 3 * 256 * 256))):
        x = dmme_amd.gaussian((B, chw), device=dev)
        e0 = dmme_amd.gaussian((B, chw), device=dev)
        e = e0.clone()
        k, frac = threshold_rank(0.995, chw)
        scratch = torch.empty(int(lib.dmme_x0_threshold_scratch_bytes(B, chw)) // 4, dtype=torch.int32, device=dev)

        def call(mode):
            e.copy_(e0)
            _lib.check(lib.dmme_x0_threshold(mode, _lib.ptr(e), _lib.ptr(x), _lib.ptr(tab), 1000, _lib.ptr(t), 1, B, chw, 1, 1, 1.0, k, frac, _lib.ptr(scratch),
                                             _lib.stream_ptr()), "dmme_x0_threshold")

        legs = {"copy": lambda: e.copy_(e0), "static": lambda: call(_lib.THRESHOLD_STATIC), "dynamic": lambda: call(_lib.THRESHOLD_DYNAMIC)}
        for one in legs.values():
            for _ in range(args.warmup):
                one()
        ms = _timed_blocks(legs, args.stage_calls, args.blocks)
        copy = _median(ms["copy"])
        out[name] = {"batch": B, "chw": chw, "form": "lds" if chw <= out["lds_capacity"] else "streaming", "copy_us": round(1e3 * copy, 2),
                     "static_us": round(1e3 * (_median(ms["static"]) - copy), 2), "dynamic_us": round(1e3 * (_median(ms["dynamic"]) - copy), 2),
                     "bytes_moved": 3 * 4 * B * chw, "finite": bool(torch.isfinite(e).all())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--big-batch", type=int, default=8, help="images of 3 x 256 x 256 in the stage's streaming leg")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--chain-steps", type=int, default=400, help="timed denoising steps per leg")
    ap.add_argument("--restart", type=int, default=50, help="steps after which a leg starts a fresh chain from x_T")
    ap.add_argument("--stage-calls", type=int, default=200, help="timed calls of the stage per block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["chains", "stage"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "threshold_bench", "precision": args.precision}
    if args.only in (None, "stage"):
        out["stage"] = stage_legs(args, dev)
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
