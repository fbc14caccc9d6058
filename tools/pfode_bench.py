"""Cost of a probability-flow ODE stage on the GPU (run on the MI355X; DESIGN section 20 quotes its output).

  chains    the replayed steps of bench.py's flagship workload (default UNet, CIFAR10 shape), one runner each over one network, timed in
            alternating blocks by events on the launch stream, in ONE run on one box: DDPM's step and DDIM's step (one no-grad forward and
            the update), the Heun sampling stage (the same forward and the four-term stage update), the DPS step (keep-forward, adjoint kernel,
            input-only backward, update) and the likelihood stage (keep-forward, Rademacher probe, input-only backward, probe dot, stage update).
  launches  the launches of csrc/pfode.hip alone on the same shape in fp32 (probe, dot with its finish, stage update, prior), in microseconds
            per call, with the bytes each call has to move.

usage: python tools/pfode_bench.py [--batch 128] [--precision bf16] [--chain-steps 200] [--warmup 10] [--blocks 4]
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

from dps_bench import _median, _timed_blocks  # noqa: E402  (the same timing loop: the two tools' figures stand beside each other)


def chain_legs(args, dev):
    torch.manual_seed(1337)
    net, side, T, proc_cls, _, _ = bench.workload(dmme_amd, "ddpm", args.precision)
    net.to(dev).eval()
    shape = (args.batch, 3, side, side)
    image = dmme_amd.gaussian(shape, device=dev).clamp_(-1.0, 1.0)
    flow = dmme_amd.ProbabilityFlow(net, T, nodes=T).to(dev)
    dps = dmme_amd.DPS(net, T, T, operator=dmme_amd.SeparableOperator.gaussian_blur(side, side, 9, 2.0), zeta=1.0).to(dev)
    runners = {
        "ddpm": proc_cls(net, T).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev)),
        "ddim": dmme_amd.DDIM(net, T, 50).to(dev).chain_runner(dmme_amd.gaussian(shape, device=dev)),
        "heun_stage": flow._flow_runner("decode", shape, dev),
        "dps_blur": dps.chain_runner(dmme_amd.gaussian(shape, device=dev)),
        "likelihood_stage": flow._flow_runner("likelihood", shape, dev, dmme_amd.LikelihoodChainRunner),
    }
    runners["dps_blur"].y.copy_(dps.degrade(image))
    runners["dps_blur"].mask.fill_(1.0)
    left = {k: 0 for k in runners}

    def stepper(name):
        runner = runners[name]

        def one():
            if left[name] == 0:  # a fresh walk from its first index: a random network's chain does not stay in range for long
                up = name == "likelihood_stage"
                runner.x.copy_(image if up else dmme_amd.gaussian(shape, device=dev))
                if up:
                    runner.acc.zero_()
                seed, off = philox_reserve(dev, runner.noise_numel * args.restart) if runner.draws else (0, 0)
                runner.set(runner.n_steps, seed, off)
                left[name] = min(args.restart, runner.n_steps)
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
    lib = _lib.lib()
    plan = runners["ddpm"].plan
    out = {"batch": args.batch, "timed_steps_per_leg": per_block * args.blocks, "graph": {k: r.graph is not None for k, r in runners.items()},
           "forward_launches_nograd": int(lib.dmme_unet_plan_num_launches_nograd(plan.h)), "forward_launches_keep": int(lib.dmme_unet_plan_num_launches(plan.h)),
           "finite": {k: bool(torch.isfinite(r.x).all()) for k, r in runners.items()}}
    med = {k: _median(ms[k]) for k in runners}
    for k in runners:
        out[k] = {"ms_per_step": round(med[k], 4), "steps_per_s": round(1e3 / med[k], 1), "blocks_ms": [round(v, 4) for v in ms[k]]}
    out["likelihood_over_dps"] = round(med["likelihood_stage"] / med["dps_blur"], 4)
    out["heun_over_ddim"] = round(med["heun_stage"] / med["ddim"], 4)
    return out


def launch_legs(args, dev):
    """the probe, the dot, the stage update and the prior alone, on the chains' shape in fp32"""
    lib = _lib.lib()
    B, chw = args.batch, 3 * 32 * 32
    shape = (B, 3, 32, 32)
    x, e, dx = (dmme_amd.gaussian(shape, device=dev) for _ in range(3))
    xs, es, d_out = torch.zeros_like(x), torch.zeros_like(x), torch.zeros_like(x)
    scratch = torch.zeros(int(lib.dmme_pf_scratch_floats(B, chw)), dtype=torch.float32, device=dev)
    s = torch.zeros(B, dtype=torch.float32, device=dev)
    acc = torch.zeros(B, dtype=torch.float64, device=dev)
    n, rows, ttab = dmme_amd.ProbabilityFlow(torch.nn.Identity(), 1000, nodes=1000)._tables["likelihood"]
    coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).to(dev)
    tt = torch.tensor(ttab, dtype=torch.int64).to(dev)
    state = torch.zeros(8, dtype=torch.int64, device=dev)
    index = {"a": n - 500, "b": n - 501}  # (an A stage and the B stage behind it, mid-walk)

    def only_set(i=index["a"]):
        _lib.check(lib.dmme_chain_set(_lib.ptr(state), i, _lib.ptr(tt), 7, 0, _lib.stream_ptr()), "dmme_chain_set")

    def probe():
        only_set()
        _lib.check(lib.dmme_chain_probe_pf(_lib.ptr(d_out), _lib.ptr(state), B, chw, 1, _lib.stream_ptr()), "dmme_chain_probe_pf")

    def dot():
        only_set()
        _lib.check(lib.dmme_chain_dot_pf(_lib.ptr(d_out), 1, _lib.ptr(dx), _lib.ptr(coef), _lib.ptr(state), B, chw, _lib.ptr(scratch), _lib.ptr(s), _lib.ptr(acc),
                                         _lib.stream_ptr()), "dmme_chain_dot_pf")

    def stage(which):
        def run():
            only_set(index[which])
            _lib.check(lib.dmme_chain_stage_pf(_lib.ptr(x), _lib.ptr(e), 1, _lib.ptr(xs), _lib.ptr(es), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), 1, B, chw,
                                               _lib.stream_ptr()), "dmme_chain_stage_pf")
        return run

    def prior():
        _lib.check(lib.dmme_pf_prior(_lib.ptr(x), B, chw, _lib.ptr(scratch), _lib.ptr(acc), _lib.stream_ptr()), "dmme_pf_prior")

    legs = {"probe": probe, "dot": dot, "stage_a": stage("a"), "stage_b": stage("b"), "set": only_set, "prior": prior}
    for f in legs.values():
        for _ in range(args.warmup):
            f()
        x.copy_(dx)  # (the update works in place: keep x in range)
    ms = _timed_blocks(legs, args.launch_calls, args.blocks)
    base = _median(ms["set"])
    nb = 4 * x.numel()
    return {"probe_us": round(1e3 * (_median(ms["probe"]) - base), 2), "probe_bytes_floor": nb, "dot_us": round(1e3 * (_median(ms["dot"]) - base), 2),
            "dot_bytes_floor": 2 * nb, "stage_a_us": round(1e3 * (_median(ms["stage_a"]) - base), 2), "stage_a_bytes_floor": 5 * nb,
            "stage_b_us": round(1e3 * (_median(ms["stage_b"]) - base), 2), "stage_b_bytes_floor": 5 * nb, "prior_us": round(1e3 * _median(ms["prior"]), 2),
            "prior_bytes_floor": nb, "finite": bool(torch.isfinite(x).all())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--chain-steps", type=int, default=200, help="timed steps per leg")
    ap.add_argument("--restart", type=int, default=50, help="steps after which a leg starts a fresh walk")
    ap.add_argument("--launch-calls", type=int, default=200, help="timed calls of the stand-alone launches per block")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["chains", "launches"])
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "pfode_bench", "precision": args.precision, "box_mfma_tfps": bench.mfma_calibration(dev)}
    if args.only in (None, "launches"):
        out["launches"] = launch_legs(args, dev)
    if args.only in (None, "chains"):
        out["chains"] = chain_legs(args, dev)
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
