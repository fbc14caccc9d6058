"""Cost of the Improved-DDPM-as-published additions on the GPU (run on the MI355X; DESIGN 1b quotes its output).

  train   the IDDPM ImageNet-64 training step (bench.py's --model iddpm64 --mode train leg: q_sample, UNet forward in train mode, loss,
          HIP backward, fused clip + Adam + EMA) at batch 32 with t_sampler="uniform" and with "loss-second-moment", two modules in one
          process, timed in alternating blocks by events on the launch stream.  The resampler is measured warm (a filled history: its
          full path - scan, bisection, weighted loss) unless --cold.
  chains  the replayed step of the full T = 4000 chain and of the strided K = 50 / 100 chains (IDDPM.generate(sample_steps=K)), in
          steps/s, alternating likewise, and what a whole chain of each costs.

usage: python tools/iddpm_paper_bench.py [--batch 32] [--precision bf16] [--steps 60] [--warmup 10] [--blocks 4] [--cold]
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


def train_legs(args, dev):
    legs, mods = {}, {}
    x0 = None
    for mode in ("uniform", "loss-second-moment"):
        torch.manual_seed(1337)
        net, side, T, _, lit_cls, _ = bench.workload(dmme_amd, "iddpm64", args.precision)
        lit = lit_cls(model=net, timesteps=T, loss_type=args.loss_type, t_sampler=mode).to(dev)
        lit.train()
        opts, scheds = lit.configure_optimizers()
        opt, sched = opts[0], scheds[0]["scheduler"]
        for g in opt.param_groups:
            g["max_grad_norm"] = 1.0
        if x0 is None:
            x0 = synthetic_batch(args.batch, dev, (3, side, side))
        idd = lit.diffusion_model
        if mode != "uniform" and not args.cold:  # a filled history, so that the weighted path is what gets timed
            idd._ts_hist.copy_(torch.exp(1.5 * torch.randn(idd._ts_hist.shape, device=dev)))
            idd._ts_count.fill_(idd._ts_hist.shape[1])
        mods[mode] = (lit, opt, sched)
        legs[mode] = (lambda l=lit, o=opt, s=sched: train_step(l, o, s, x0))
    for _ in range(args.warmup):
        for one in legs.values():
            one()
    per_block = max(1, -(-args.steps // args.blocks))
    ms = _timed_blocks(legs, per_block, args.blocks)
    losses = {}
    for mode, (lit, opt, sched) in mods.items():
        losses[mode] = float(train_step(lit, opt, sched, x0).detach())
        assert losses[mode] == losses[mode], f"{mode}: non-finite loss"
    idd = mods["loss-second-moment"][0].diffusion_model
    idd.check_t_sampler()
    a, b = _median(ms["uniform"]), _median(ms["loss-second-moment"])
    return {"batch": args.batch, "loss_type": args.loss_type, "timed_steps_per_leg": per_block * args.blocks, "resampler_warm": not args.cold,
            "uniform_ms_per_step": round(a, 3), "resampled_ms_per_step": round(b, 3), "resampled_over_uniform": round(b / a, 4),
            "uniform_blocks_ms": [round(v, 3) for v in ms["uniform"]], "resampled_blocks_ms": [round(v, 3) for v in ms["loss-second-moment"]],
            "last_loss": losses}


def chain_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, proc_cls, _, _ = bench.workload(dmme_amd, "iddpm64", args.precision)
    net.to(dev).eval()
    idd = proc_cls(net, T).to(dev)
    shape = (args.batch, 3, side, side)
    runners = {"full": (idd.chain_runner(dmme_amd.gaussian(shape, device=dev)), T)}
    for K in (50, 100):
        runners[f"k{K}"] = (idd.respaced_runner(dmme_amd.gaussian(shape, device=dev), K), K)
    left = {k: 0 for k in runners}

    def stepper(name):
        runner, n = runners[name]

        def one():
            if left[name] == 0:
                seed, off = philox_reserve(dev, runner.x.numel() * n)
                runner.set(n, seed, off)
                left[name] = n
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
    for runner, _ in runners.values():
        runner.plan.check()
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, (r, _) in runners.items()}}
    for k, (_, n) in runners.items():
        m = _median(ms[k])
        out[k] = {"steps_in_chain": n, "ms_per_step": round(m, 3), "steps_per_s": round(1e3 / m, 1), "chain_seconds": round(n * m * 1e-3, 3),
                  "blocks_ms": [round(v, 3) for v in ms[k]]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--loss-type", default="hybrid", choices=["hybrid", "vlb"])
    ap.add_argument("--steps", type=int, default=60, help="timed training steps per leg (>= 50)")
    ap.add_argument("--chain-steps", type=int, default=400, help="timed denoising steps per leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--cold", action="store_true", help="time the resampler before its history is full (uniform draws, unit weights)")
    ap.add_argument("--only", default=None, choices=["train", "chains"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "iddpm_paper_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "train"):
        out["train"] = train_legs(args, dev)
        torch.cuda.empty_cache()
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
