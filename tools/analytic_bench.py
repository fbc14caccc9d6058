"""Cost of Analytic-DPM's device work on the GPU (run on the MI355X; nothing in the repository quotes a number from it yet).

  launches  the two entry points of csrc/analytic.hip alone on the flagship workload's shape in fp32, in microseconds per call, with the
            bytes each call has to move: the statistics pass (dmme_analytic_moment) on a one- and a two-plane network output, the rows of
            the bound (dmme_analytic_vlb_rows) at a KL index and at the decoder index.
  passes    a sweep of `estimate_moments` over one image per timestep (per pass: Philox span, dmme_q_sample, the no-grad forward of bench.py's
            default UNet, the statistics pass; the status word read once per sweep) next to as many forwards alone, timed in alternating
            blocks by events on the launch stream, in ONE run on one box.

usage: python tools/analytic_bench.py [--batch 128] [--precision bf16] [--calls 8] [--warmup 2] [--blocks 4]
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

from dps_bench import _median, _timed_blocks  # noqa: E402  (the same timing loop: the tools' figures stand beside each other)


def launch_legs(args, dev):
    lib = _lib.lib()
    B, chw, T, S = args.batch, 3 * 32 * 32, 1000, 50
    shape = (B, 3, 32, 32)
    x0 = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    x_t, e1 = dmme_amd.gaussian(shape, device=dev), dmme_amd.gaussian(shape, device=dev)
    e2 = torch.cat([e1.reshape(B, -1), torch.zeros(B, chw, device=dev)], dim=1).contiguous()
    proc = dmme_amd.AnalyticDPM(torch.nn.Identity(), T, S).set_moments(np.full(T + 1, 0.9))
    coef = torch.from_numpy(proc._vlb_table("analytic")).reshape(-1).to(dev)
    t = 1 + (torch.arange(B, device=dev, dtype=torch.int64) % T)
    sums, counts = torch.zeros(T + 1, dtype=torch.float64, device=dev), torch.zeros(T + 1, dtype=torch.int64, device=dev)
    rows = torch.zeros(B, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.zeros(32 * B, dtype=torch.float32, device=dev)
    idx = {"kl": torch.full((B,), S // 2, dtype=torch.int64, device=dev), "nll": torch.ones(B, dtype=torch.int64, device=dev)}

    def moment(out, stride):
        def run():
            _lib.check(lib.dmme_analytic_moment(_lib.ptr(out), stride, _lib.ptr(t), T, B, chw, _lib.ptr(sums), _lib.ptr(counts), _lib.ptr(rows), _lib.ptr(status),
                                                _lib.ptr(scratch), _lib.stream_ptr()), "dmme_analytic_moment")
        return run

    def vlb(which):
        def run():
            _lib.check(lib.dmme_analytic_vlb_rows(_lib.ptr(e1), chw, _lib.ptr(x_t), _lib.ptr(x0), _lib.ptr(idx[which]), _lib.ptr(coef), S, B, chw, _lib.ptr(rows),
                                                  _lib.ptr(status), _lib.ptr(scratch), _lib.stream_ptr()), "dmme_analytic_vlb_rows")
        return run

    legs = {"moment_1plane": moment(e1, chw), "moment_2plane": moment(e2, 2 * chw), "vlb_kl": vlb("kl"), "vlb_nll": vlb("nll")}
    for f in legs.values():
        for _ in range(args.warmup):
            f()
    ms = _timed_blocks(legs, args.launch_calls, args.blocks)
    nb = 4 * x0.numel()
    out = {k + "_us": round(1e3 * _median(v), 2) for k, v in ms.items()}
    out.update({"moment_bytes_floor": nb, "vlb_bytes_floor": 3 * nb, "status": int(status.item())})
    return out


def pass_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, _, _, _ = bench.workload(dmme_amd, "ddpm", args.precision)
    net.to(dev).eval()
    shape = (args.batch, 3, side, side)
    data = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    proc = dmme_amd.AnalyticDPM(net, T, 50).to(dev)
    passes = len(dmme_amd.moment_schedule(T, args.batch, 1))
    t = 1 + (torch.arange(args.batch, device=dev, dtype=torch.int64) % T)
    noisy = dmme_amd.gaussian(shape, device=dev)

    def estimate():  # one image per timestep: `passes` passes, the last one cut
        proc.estimate_moments(data, images_per_timestep=1, batch_size=args.batch, seed=None)

    def forward():
        for _ in range(passes):
            net(noisy, t)

    legs = {"estimate": estimate, "forward": forward}
    with torch.no_grad():
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        per_block = max(1, -(-args.calls // args.blocks))
        ms = _timed_blocks(legs, per_block, args.blocks)
    med = {k: _median(v) for k, v in ms.items()}
    return {"batch": args.batch, "passes_per_call": passes, "estimate_ms_per_pass": round(med["estimate"] / passes, 4), "forward_ms_per_pass": round(med["forward"] / passes, 4),
            "blocks_ms": {k: [round(v, 4) for v in ms[k]] for k in ms}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--calls", type=int, default=8, help="timed calls per leg of the estimation comparison (each a sweep of one image per timestep)")
    ap.add_argument("--launch-calls", type=int, default=200, help="timed calls of the stand-alone launches per block")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["passes", "launches"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "analytic_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "launches"):
        out["launches"] = launch_legs(args, dev)
    if args.only in (None, "passes"):
        out["passes"] = pass_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
