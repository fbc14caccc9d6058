"""DESIGN section 10's throughput figures: one 20-step chain at batch 128, bf16, default UNet, GeneralizedDDIM (eta = 0) against
DPMSolverPP on the same (quadratic) grid, alternating, HIP events around `decode`; and the two update kernels alone.  Prints one JSON line
(sorted per-step / per-launch times of every repeat).

  python tools/dpmpp_bench.py"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import dmme_amd
from dmme_amd import _lib

torch.manual_seed(0)
net = dmme_amd.UNet(precision="bf16").cuda().eval()
shape = (128, 3, 32, 32)
procs = {"gddim": dmme_amd.GeneralizedDDIM(net, 1000, 20, "quadratic").cuda(), "dpmpp": dmme_amd.DPMSolverPP(net, 1000, 20, "quadratic").cuda()}
assert procs["dpmpp"].n_steps == 20
x_T = dmme_amd.gaussian(shape, device="cuda")
for p in procs.values():
    for _ in range(2):
        p.decode(x_T)
times = {k: [] for k in procs}
for rep in range(7):
    for k, p in procs.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = p.decode(x_T)
        b.record()
        torch.cuda.synchronize()
        times[k].append(a.elapsed_time(b) / 20)
        assert bool(torch.isfinite(out).all())
res = {f"{k}_ms_per_step": sorted(v) for k, v in times.items()}
# the update kernels alone
lib = _lib.lib()
x = dmme_amd.gaussian(shape, device="cuda")
eps = dmme_amd.gaussian(shape, device="cuda")
hist = torch.zeros_like(x)
chw = x[0].numel()
for name, p in procs.items():
    n, rows, ttab = p._chain_tables()
    coef = torch.tensor(rows, dtype=torch.float32).reshape(-1).cuda()
    tt = torch.tensor(ttab, dtype=torch.int64).cuda()
    state = torch.zeros(8, dtype=torch.int64, device="cuda")

    def launch():
        if name == "gddim":
            _lib.check(lib.dmme_chain_update(_lib.CHAIN_GDDIM, _lib.ptr(x), _lib.ptr(eps), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), 128, chw, _lib.stream_ptr()))
        else:
            _lib.check(lib.dmme_chain_update_dpmpp(_lib.ptr(x), _lib.ptr(eps), _lib.ptr(hist), _lib.ptr(coef), _lib.ptr(tt), _lib.ptr(state), 128, chw, 1, _lib.stream_ptr()))

    runs = []
    for rep in range(5):
        x.copy_(x_T)
        _lib.check(lib.dmme_chain_set(_lib.ptr(state), 10, _lib.ptr(tt), 0, 0, _lib.stream_ptr()))
        for _ in range(3):
            launch()
        _lib.check(lib.dmme_chain_set(_lib.ptr(state), 10, _lib.ptr(tt), 0, 0, _lib.stream_ptr()))
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(8):  # (indices 10 .. 3: the history is valid from the second launch on)
            launch()
        b.record()
        torch.cuda.synchronize()
        runs.append(a.elapsed_time(b) / 8 * 1e3)
    res[f"{name}_update_us_per_launch"] = sorted(runs)
print(json.dumps(res))
