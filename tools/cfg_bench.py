"""Cost of classifier-free guidance on the GPU (run on the MI355X; DESIGN 9 quotes its output).

For each batch B (default 128, 32, 1), default net, three replayed steps timed in alternating blocks by events on the launch stream:

  cfg        the captured guided step (dmme_cfg_chain_step): ONE conditional forward at batch 2B + the mixing update, s = 2
  uncond_2B  the yardstick: the unconditional captured step (dmme_chain_step, plain UNet) at batch 2B
  two_cond   what batching the halves replaces: two conditional forwards at batch B one after the other (two replays of the
             s = 1 step: forward at batch B + the base update)

and whether the kernel labels of the 2B conditional plan equal those of the 2B DDPM plan apart from the label op (a conditional route
that fell off a fast path shows here).

The cross-build yardstick is `python bench.py --batch 2B` run from a checkout of the parent commit, alternating with this tool in one
GPU session, three repeats each.  `--fold` (no GPU needed) puts the two sets of lines together: per batch the medians and spreads of
the guided step and of the parent's step at 2B, their ratio, the bound max(spread of the yardstick's repeats, 4 %) and the speed-up
over two conditional forwards - what profiles/cfg_bench_<date>.json holds.

usage: python tools/cfg_bench.py [--batches 128,32,1] [--precision bf16] [--steps 60] [--warmup 10] [--blocks 3] [--scale 2.0]
       python tools/cfg_bench.py --fold CFG_LINES PARENT_BENCH_LINES        (files of JSON lines; other lines are skipped)
Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the box calibration of the benchmark)
import dmme_amd  # noqa: E402
from dmme_amd import _lib  # noqa: E402
from dmme_amd.common.noise import philox_reserve  # noqa: E402


def _median(v):
    v = sorted(v)
    return v[len(v) // 2] if len(v) % 2 else 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def _timed_blocks(legs, blocks):
    """legs: {name: (callable doing one step, steps per block)}; every leg runs its steps between two events, `blocks` rounds in turn"""
    out = {k: [] for k in legs}
    for _ in range(blocks):
        for name, (one, per_block) in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(per_block):
                one()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / per_block)
    return out


def _labels(plan):
    lib, buf, f, b = _lib.lib(), C.create_string_buffer(160), C.c_double(), C.c_double()
    out = []
    for i in range(lib.dmme_unet_plan_num_ops(plan.h)):
        _lib.check(lib.dmme_unet_plan_op_info(plan.h, i, buf, 160, C.byref(f), C.byref(b)))
        out.append(buf.value.decode())
    return out


def _stepper(runner, n, dev):
    left = [0]

    def one():
        if left[0] == 0:
            seed, off = philox_reserve(dev, runner.noise_numel * n)
            runner.set(n, seed, off)
            left[0] = n
        runner.step()
        left[0] -= 1

    return one


def one_batch(B, args, dev):
    torch.manual_seed(1337)
    T, K = 1000, 10
    cond = dmme_amd.ConditionalUNet(precision=args.precision, num_classes=K).to(dev).eval()
    unet = dmme_amd.UNet(precision=args.precision).to(dev).eval()
    guided = dmme_amd.ClassifierFreeDDPM(cond, T, guidance_scale=args.scale).to(dev)
    single = dmme_amd.ClassifierFreeDDPM(cond, T, guidance_scale=1.0).to(dev)
    plain = dmme_amd.DDPM(unet, T).to(dev)
    y = torch.arange(B, device=dev) % K
    r_cfg = guided._buffered_runner("_cfg_runner", (2 * B, 3, 32, 32), dev, buf="_cfg_buf")
    r_one = single._buffered_runner("_cfg_runner", (B, 3, 32, 32), dev, buf="_cfg_buf")
    r_unc = plain._buffered_runner("_runner", (2 * B, 3, 32, 32), dev)
    x = dmme_amd.gaussian((B, 3, 32, 32), device=dev)
    r_cfg.x[:B].copy_(x), r_cfg.x[B:].copy_(x), r_cfg.y[:B].copy_(y), r_cfg.y[B:].fill_(K)
    r_one.x.copy_(x), r_one.y.copy_(y)
    r_unc.x.copy_(torch.cat([x, x]))
    cfg_step, one_step, unc_step = _stepper(r_cfg, T, dev), _stepper(r_one, T, dev), _stepper(r_unc, T, dev)

    def two():
        one_step()
        one_step()

    per_block = max(1, -(-args.steps // args.blocks))
    legs = {"cfg": (cfg_step, per_block), "uncond_2B": (unc_step, per_block), "two_cond": (two, per_block)}
    with torch.no_grad():
        for one, _ in legs.values():
            for _ in range(args.warmup):
                one()
        ms = _timed_blocks(legs, args.blocks)
    for r in (r_cfg, r_one, r_unc):
        torch.cuda.synchronize()
        r.plan.check()
    cond.check_labels()
    lc, lu = _labels(r_cfg.plan), _labels(r_unc.plan)
    out = {"batch": B, "timed_steps_per_leg": per_block * args.blocks, "graph": {"cfg": r_cfg.graph is not None, "uncond_2B": r_unc.graph is not None, "two_cond": r_one.graph is not None},
           "finite": bool(torch.isfinite(r_cfg.x).all()), "labels_equal_apart_from_label_op": [v for v in lc if v != "label_cond_kernel"] == lu}
    for k, v in ms.items():
        m = _median(v)
        out[k] = {"ms_per_step": round(m, 4), "spread": round((max(v) - min(v)) / m, 4), "blocks_ms": [round(b, 4) for b in v]}
    out["cfg_over_uncond_2B"] = round(out["cfg"]["ms_per_step"] / out["uncond_2B"]["ms_per_step"], 4)
    out["speedup_over_two_cond"] = round(out["two_cond"]["ms_per_step"] / out["cfg"]["ms_per_step"], 4)
    return out


def _json_lines(path):
    out = []
    with open(path) as f:
        for line in f:
            if line.startswith("{"):
                out.append(json.loads(line))
    return out


def fold(cfg_path, parent_path):
    """one record per batch from repeated runs of this tool and of the parent checkout's bench.py at twice the batch"""
    runs = [d for d in _json_lines(cfg_path) if d.get("tool") == "cfg_bench"]
    parent = [d for d in _json_lines(parent_path) if "ms_per_step" in d and d.get("config", {}).get("global_batch")]
    out = {"tool": "cfg_bench --fold", "precision": runs[0]["precision"], "scale": runs[0]["scale"],
           "box_mfma_tfps": [d["box_mfma_tfps"] for d in runs], "protocol": "parent bench.py --batch 2B and this tool alternating in one GPU session", "batches": []}

    def stat(v):
        m = _median(v)
        return {"median_ms": round(m, 4), "spread": round((max(v) - min(v)) / m, 4), "runs_ms": v}

    for B in sorted({b["batch"] for d in runs for b in d["batches"]}, reverse=True):
        mine = [b for d in runs for b in d["batches"] if b["batch"] == B]
        yard = [d["ms_per_step"] for d in parent if d["config"]["global_batch"] == 2 * B and d.get("n_gpus", 1) == 1]
        rec = {"batch": B, "cfg": stat([b["cfg"]["ms_per_step"] for b in mine]), "uncond_2B_same_build": stat([b["uncond_2B"]["ms_per_step"] for b in mine]),
               "two_cond": stat([b["two_cond"]["ms_per_step"] for b in mine]), "labels_equal_apart_from_label_op": all(b["labels_equal_apart_from_label_op"] for b in mine)}
        rec["speedup_over_two_cond"] = round(rec["two_cond"]["median_ms"] / rec["cfg"]["median_ms"], 4)
        if yard:
            rec["parent_uncond_2B"] = stat(yard)
            rec["cfg_over_parent_2B"] = round(rec["cfg"]["median_ms"] / rec["parent_uncond_2B"]["median_ms"], 4)
            rec["bound"] = round(1 + max(rec["parent_uncond_2B"]["spread"], 0.04), 4)
            rec["within_bound"] = rec["cfg_over_parent_2B"] <= rec["bound"]
        out["batches"].append(rec)
    return out


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--fold":
        print(json.dumps(fold(sys.argv[2], sys.argv[3])), flush=True)
        return 0
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="128,32,1")
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--scale", type=float, default=2.0)
    ap.add_argument("--steps", type=int, default=60, help="timed steps per leg")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda:0")
    out = {"tool": "cfg_bench", "precision": args.precision, "scale": args.scale, "box_mfma_tfps": bench.mfma_calibration(dev), "batches": []}
    for B in (int(v) for v in args.batches.split(",")):
        out["batches"].append(one_batch(B, args, dev))
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
