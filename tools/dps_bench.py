"""Cost of a DPS step on the GPU (run on the MI355X; DESIGN's section on DPS quotes its output).

  chains    the replayed sampling step of bench.py's flagship workload (default UNet, CIFAR10 shape): DDPM's step (one no-grad forward and
            the update) against the DPS step (keep-forward, adjoint kernel, input-only backward, update) for each --cases operator, one
            runner each over one network, timed in alternating blocks by events on the launch stream.  Both run on the full grid.
  launches  the two launches of csrc/dps.hip alone on the same shape in fp32 (dmme_chain_adjoint_dps, and dmme_chain_update_dps drawing
            its own normals), and dmme_dps_measure, in microseconds per call, with the bytes each call has to move.

usage: python tools/dps_bench.py [--batch 128] [--precision bf16] [--chain-steps 200] [--warmup 10] [--blocks 4] [--cases blur bicubic]
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


def _operator(name, side):
    return dmme_amd.SeparableOperator.preset(name, side, side, blur_size=9, blur_sigma=2.0, scale=4)


def chain_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, proc_cls, _, _ = bench.workload(dmme_amd, "ddpm", args.precision)
    net.to(dev).eval()
    shape = (args.batch, 3, side, side)
    image = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    runners = {"ddpm": proc_cls(net, T).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev))}
    for name in args.cases:
        proc = dmme_amd.DPS(net, T, T, operator=_operator(name, side), zeta=1.0).to(dev)
        r = runners[f"dps_{name}"] = proc.chain_runner(dmme_amd.gaussian(shape, device=dev))
        r.y.copy_(proc.degrade(image))
        r.mask.fill_(1.0)
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
    lib = _lib.lib()
    plan = runners["ddpm"].plan
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, r in runners.items()},
           "forward_launches_nograd": int(lib.dmme_unet_plan_num_launches_nograd(plan.h)), "forward_launches_keep": int(lib.dmme_unet_plan_num_launches(plan.h)),
           "finite": {k: bool(torch.isfinite(r.x).all()) for k, r in runners.items()}}
    for k in runners:
        m = _median(ms[k])
        out[k] = {"ms_per_step": round(m, 4), "steps_per_s": round(1e3 / m, 1), "over_ddpm": round(m / base, 4), "blocks_ms": [round(v, 4) for v in ms[k]]}
    return out


def launch_legs(args, dev):
    """the adjoint kernel, the update and the measurement alone, on the chains' shape in fp32"""
    lib = _lib.lib()
    B, Cc, side = args.batch, 3, 32
    shape = (B, Cc, side, side)
    out = {"capacity": int(lib.dmme_dps_capacity())}
    x, e, image, dx = (dmme_amd.gaussian(shape, device=dev) for _ in range(4))
    g, d_out = torch.empty_like(x), torch.empty_like(x)
    ss = torch.empty((B, Cc), dtype=torch.float32, device=dev)
    for name in args.cases:
        op = _operator(name, side)
        proc = dmme_amd.DPS(torch.nn.Identity(), 1000, 1000, operator=op).to(dev)
        n, rows, ttab = proc._chain_tables()
        Kh, Kw = op.device(dev)
        y = proc.degrade(image)
        coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).to(dev)
        tt = torch.tensor(ttab, dtype=torch.int64).to(dev)
        state = torch.zeros(8, dtype=torch.int64, device=dev)

        def only_set():
            _lib.check(lib.dmme_chain_set(_lib.ptr(state), 500, _lib.ptr(tt), 7, 0, _lib.stream_ptr()), "dmme_chain_set")

        def adjoint():
            only_set()
            _lib.check(lib.dmme_chain_adjoint_dps(_lib.ptr(x), _lib.ptr(e), 1, _lib.ptr(coef), _lib.ptr(state), _lib.ptr(y), None, _lib.ptr(Kh), _lib.ptr(Kw), _lib.ptr(g),
                                                  _lib.ptr(d_out), _lib.ptr(ss), B, Cc, side, side, op.h, op.w, _lib.stream_ptr()), "dmme_chain_adjoint_dps")

        def update():
            only_set()
            _lib.check(lib.dmme_chain_update_dps(_lib.ptr(x), _lib.ptr(e), _lib.ptr(g), _lib.ptr(dx), _lib.ptr(ss), None, _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), B, Cc,
                                                 side, side, 1, _lib.stream_ptr()), "dmme_chain_update_dps")

        def measure():
            _lib.check(lib.dmme_dps_measure(_lib.ptr(image), _lib.ptr(Kh), _lib.ptr(Kw), None, _lib.ptr(y), B, Cc, side, side, op.h, op.w, _lib.stream_ptr()),
                       "dmme_dps_measure")

        legs = {"adjoint": adjoint, "update": update, "set": only_set, "measure": measure}
        for f in legs.values():
            for _ in range(args.warmup):
                f()
            x.copy_(image)  # (the update works in place: keep x in range)
        ms = _timed_blocks(legs, args.launch_calls, args.blocks)
        base = _median(ms["set"])
        flops = 2 * B * Cc * (side * side * op.w + op.h * side * op.w) * 2  # the four products of one plane, all planes
        out[f"dps_{name}"] = {"h": op.h, "w": op.w, "adjoint_us": round(1e3 * (_median(ms["adjoint"]) - base), 2), "adjoint_flops": flops,
                              "adjoint_bytes_floor": 4 * (4 * x.numel() + 2 * y.numel()), "update_us": round(1e3 * (_median(ms["update"]) - base), 2),
                              "update_bytes_floor": 5 * 4 * x.numel(), "measure_us": round(1e3 * _median(ms["measure"]), 2),
                              "measure_bytes_floor": 4 * (x.numel() + y.numel()), "finite": bool(torch.isfinite(g).all())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--cases", nargs="+", default=["blur", "bicubic"], choices=["identity", "blur", "bicubic", "average"])
    ap.add_argument("--chain-steps", type=int, default=200, help="timed denoising steps per leg")
    ap.add_argument("--restart", type=int, default=50, help="steps after which a leg starts a fresh chain from x_T")
    ap.add_argument("--launch-calls", type=int, default=200, help="timed calls of the stand-alone launches per block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["chains", "launches"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "dps_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "launches"):
        out["launches"] = launch_legs(args, dev)
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
