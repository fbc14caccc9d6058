"""Cost of DDNM's cell-wise update on the GPU (run on the MI355X; DESIGN's section on DDNM quotes its output).

  chains  the replayed sampling step of bench.py's flagship workload (default UNet, CIFAR10 shape): DDPM's step against the DDNM step
          (the same forward, then the band update in place of DDPM's) for each --cases entry "s" or "sg" (g: grey), one runner each over
          one network, timed in alternating blocks by events on the launch stream.  The DDNM process runs on the full grid.
  update  the stand-alone update (dmme_chain_update_ddnm with in-kernel draws) and the measurement (dmme_ddnm_measure) on the same
          shape, in microseconds per call, with the bytes each call has to move.

usage: python tools/ddnm_bench.py [--batch 128] [--precision bf16] [--chain-steps 400] [--warmup 20] [--blocks 4] [--cases 4 4g]
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


def _case(text):
    return int(text.rstrip("g")), text.endswith("g")


def chain_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, proc_cls, _, _ = bench.workload(dmme_amd, "ddpm", args.precision)
    net.to(dev).eval()
    shape = (args.batch, 3, side, side)
    image = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    runners = {"ddpm": proc_cls(net, T).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev))}
    for text in args.cases:
        s, gray = _case(text)
        proc = dmme_amd.DDNM(net, T, T, scale=s, gray=gray).to(dev)
        r = runners[f"ddnm{text}"] = proc.chain_runner(dmme_amd.gaussian(shape, device=dev))
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
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, r in runners.items()},
           "update_bytes_floor": 3 * 4 * runners["ddpm"].x.numel()}  # x, e read, x written (y and m are 1 / n of that)
    for k in runners:
        m = _median(ms[k])
        out[k] = {"ms_per_step": round(m, 4), "steps_per_s": round(1e3 / m, 1), "over_ddpm": round(m / base, 4), "added_us": round(1e3 * (m - base), 2),
                  "added_share_of_step": round((m - base) / m, 4), "blocks_ms": [round(v, 4) for v in ms[k]]}
    return out


def update_legs(args, dev):
    """the update and the measurement alone, on the chains' shape in fp32"""
    lib = _lib.lib()
    B, Cc, side = args.batch, 3, 32
    shape = (B, Cc, side, side)
    out = {"band_capacity": int(lib.dmme_ddnm_band_capacity())}
    x, e, image = (dmme_amd.gaussian(shape, device=dev) for _ in range(3))
    for text in args.cases:
        s, gray = _case(text)
        proc = dmme_amd.DDNM(torch.nn.Identity(), 1000, 1000, scale=s, gray=gray).to(dev)
        n, rows, ttab = proc._chain_tables()
        y = proc.degrade(image)
        m = torch.ones_like(y)
        coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).to(dev)
        tt = torch.tensor(ttab, dtype=torch.int64).to(dev)
        state = torch.zeros(8, dtype=torch.int64, device=dev)

        def update():
            _lib.check(lib.dmme_chain_set(_lib.ptr(state), 500, _lib.ptr(tt), 7, 0, _lib.stream_ptr()), "dmme_chain_set")
            _lib.check(lib.dmme_chain_update_ddnm(_lib.ptr(x), _lib.ptr(e), _lib.ptr(y), _lib.ptr(m), None, _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), B, Cc, side, side,
                                                  s, int(gray), 1, _lib.stream_ptr()), "dmme_chain_update_ddnm")

        def only_set():
            _lib.check(lib.dmme_chain_set(_lib.ptr(state), 500, _lib.ptr(tt), 7, 0, _lib.stream_ptr()), "dmme_chain_set")

        def measure():
            _lib.check(lib.dmme_ddnm_measure(_lib.ptr(image), None, _lib.ptr(y), B, Cc, side, side, s, int(gray), _lib.stream_ptr()), "dmme_ddnm_measure")

        for f in (update, only_set, measure):
            for _ in range(args.warmup):
                f()
        ms = _timed_blocks({"update": update, "set": only_set, "measure": measure}, args.update_calls, args.blocks)
        out[f"ddnm{text}"] = {"cell": (Cc if gray else 1) * s * s, "update_us": round(1e3 * (_median(ms["update"]) - _median(ms["set"])), 2),
                              "update_bytes_floor": 3 * 4 * x.numel() + 2 * 4 * y.numel(), "measure_us": round(1e3 * _median(ms["measure"]), 2),
                              "measure_bytes_floor": 4 * (x.numel() + y.numel()), "finite": bool(torch.isfinite(y).all())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--cases", nargs="+", default=["4", "4g"], help="scale of the pooling, with a trailing g for a grey measurement")
    ap.add_argument("--chain-steps", type=int, default=400, help="timed denoising steps per leg")
    ap.add_argument("--restart", type=int, default=50, help="steps after which a leg starts a fresh chain from x_T")
    ap.add_argument("--update-calls", type=int, default=200, help="timed calls of the stand-alone update per block")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["chains", "update"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "ddnm_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "update"):
        out["update"] = update_legs(args, dev)
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
