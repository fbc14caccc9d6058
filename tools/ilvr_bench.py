"""Cost of ILVR's low-pass refinement on the GPU (run on the MI355X; DESIGN's section on ILVR quotes its output).

  chains  the replayed sampling step of bench.py's flagship workload (default UNet, CIFAR10 shape): DDPM's step against the ILVR step
          (the same forward, then the fused update in place of DDPM's) for each --down-factor, one runner each over one network, timed
          in alternating blocks by events on the launch stream.  The ILVR process runs on the full grid, so its rows are DDPM's.
  filter  the stand-alone filter (dmme_lowpass) on batch x 3 planes of 32 x 32 through the fused form and on big-batch x 3 planes of
          256 x 256 through the streaming form, in microseconds per call, with the bytes each call has to move.

usage: python tools/ilvr_bench.py [--batch 128] [--precision bf16] [--chain-steps 400] [--warmup 20] [--blocks 4] [--big-batch 8]
Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workload definitions and the box calibration of the benchmark)
import dmme_amd  # noqa: E402
from dmme_amd import _lib  # noqa: E402
from dmme_amd.common.noise import philox_reserve  # noqa: E402


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
    ref = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    runners = {"ddpm": proc_cls(net, T).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev))}
    for N in args.down_factors:
        runners[f"ilvr{N}"] = dmme_amd.ILVR(net, T, T, N).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev))
        runners[f"ilvr{N}"].ref.copy_(ref)
    left = {k: 0 for k in runners}

    def stepper(name):
        runner = runners[name]

        def one():
            if left[name] == 0:  # a fresh chain from the top: a random network's chain does not stay in range for T steps
                runner.x.copy_(dmme_amd.gaussian(shape, device=dev))
                seed, off = philox_reserve(dev, runner.noise_numel * args.restart)
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
    base = _median(ms["ddpm"])
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, r in runners.items()},
           "update_bytes_floor": 4 * 4 * runners["ddpm"].x.numel()}  # x, e, y read, x written
    for k in runners:
        m = _median(ms[k])
        out[k] = {"ms_per_step": round(m, 4), "steps_per_s": round(1e3 / m, 1), "over_ddpm": round(m / base, 4), "added_us": round(1e3 * (m - base), 2),
                  "added_share_of_step": round((m - base) / m, 4), "blocks_ms": [round(v, 4) for v in ms[k]]}
    return out


def filter_legs(args, dev):
    lib = _lib.lib()
    out = {"lds_capacity": int(lib.dmme_lowpass_lds_capacity())}
    for name, (B, side, N) in (("cifar", (args.batch, 32, 4)), ("lsun256", (args.big_batch, 256, 32))):
        planes = 3 * B
        P = torch.from_numpy(dmme_amd.lowpass_matrix(side, N).astype(np.float32)).to(dev)
        src = dmme_amd.gaussian((planes, side, side), device=dev)
        dst = torch.empty_like(src)
        scratch = torch.empty(int(lib.dmme_lowpass_scratch_bytes(planes, side, side)) // 4, dtype=torch.float32, device=dev)

        def call():
            _lib.check(lib.dmme_lowpass(_lib.ptr(src), _lib.ptr(dst), planes, side, side, _lib.ptr(P), _lib.ptr(P), _lib.ptr(scratch), 0, _lib.stream_ptr()), "dmme_lowpass")

        for _ in range(args.warmup):
            call()
        ms = _timed_blocks({"lowpass": call}, args.filter_calls, args.blocks)
        fused = side * side <= out["lds_capacity"]
        out[name] = {"planes": planes, "side": side, "down_factor": N, "form": "fused" if fused else "streaming", "us": round(1e3 * _median(ms["lowpass"]), 2),
                     "bytes_floor": (2 if fused else 4) * 4 * src.numel(), "flop": 2 * 2 * side * src.numel(), "finite": bool(torch.isfinite(dst).all())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--big-batch", type=int, default=8, help="images of 3 x 256 x 256 in the filter's streaming leg")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--down-factors", type=int, nargs="+", default=[4, 8])
    ap.add_argument("--chain-steps", type=int, default=400, help="timed denoising steps per leg")
    ap.add_argument("--restart", type=int, default=50, help="steps after which a leg starts a fresh chain from x_T")
    ap.add_argument("--filter-calls", type=int, default=200, help="timed calls of the filter per block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["chains", "filter"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "ilvr_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "filter"):
        out["filter"] = filter_legs(args, dev)
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
