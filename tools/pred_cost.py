"""What the x0 / v adapter costs a sampling step: the captured DDPM step of the benchmark workload (default UNet, batch 128, bf16) for an
eps process and for a v process over the SAME network and plan, timed alternately with HIP events over blocks of replays.

  python tools/pred_cost.py [--batch 128] [--precision bf16] [--replays 100] [--rounds 3]

Prints one JSON line: ms per step of each process per round, the medians, their difference (the adapter's launch) and the box's
dense bf16 MFMA rate (bench.py: mfma_calibration), which says what kind of board the figures were taken on."""

import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import dmme_amd

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    torch.manual_seed(1337)
    model, side, T, _, _, label = bench.workload(dmme_amd, "ddpm", args.precision)
    model = model.to(dev).eval()
    legs = {}
    for pred in ("eps", "v"):
        proc = dmme_amd.DDPM(model, T, prediction=pred).to(dev)
        x = dmme_amd.gaussian((args.batch, 3, side, side), device=dev)
        runner = proc.chain_runner(x)
        bench.chain_leg(proc, runner, T, args.warmup, [], None, dev, back_to_back=True)  # capture + warm-up
        legs[pred] = (proc, runner)
    assert legs["eps"][1].plan is legs["v"][1].plan
    ms = {"eps": [], "v": []}
    for _ in range(args.rounds):
        for pred, (proc, runner) in legs.items():
            t = bench.chain_leg(proc, runner, T, 0, [args.replays], None, dev, back_to_back=True)[0]
            ms[pred].append(round(1e3 * t / args.replays, 4))
    for pred, (_, runner) in legs.items():
        assert runner.graph is not None and torch.isfinite(runner.x).all(), pred
    med = {k: bench._median(v) for k, v in ms.items()}
    print(json.dumps({"workload": f"DDPM T={T} captured step, {label}, batch {args.batch}, {args.precision}", "replays_per_block": args.replays,
                      "ms_per_step": ms, "ms_per_step_median": med, "adapter_ms": round(med["v"] - med["eps"], 4),
                      "adapter_share_of_step": round((med["v"] - med["eps"]) / med["eps"], 5), "box_mfma_tfps": bench.mfma_calibration(dev)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
