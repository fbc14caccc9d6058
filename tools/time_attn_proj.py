#!/usr/bin/env python3
"""event-bracketed launch times of the attention block's tail: separate launches vs one, and of the whole block folded (no qkv conv, no
qkv tensor: dmme_attention_block; the norm from partials).  usage: python tools/time_attn_proj.py [C]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from dmme_amd import _lib
C = int(sys.argv[1]) if len(sys.argv) > 1 else 256
N, S = 128, 256
dev = torch.device("cuda:0"); lib = _lib.lib(); dt = _lib.BF16
qkv = torch.randn(N, S, 3 * C, device=dev).bfloat16()
w = (torch.randn(C, C, device=dev) * C**-0.5).bfloat16(); b = torch.randn(C, device=dev)
res = torch.randn(N, S, C, device=dev).bfloat16(); dst = torch.empty_like(res); ctx = torch.empty_like(res)
part = torch.zeros(N, S // 32, 32, 2, device=dev)
st = _lib.stream_ptr()
def t(fn, n=50):
    for _ in range(5): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3
att = lambda: _lib.check(lib.dmme_attention(dt, _lib.ptr(qkv), N, S, C, _lib.ptr(ctx), 0, st))
fused = lambda: _lib.check(lib.dmme_attention_proj(dt, _lib.ptr(qkv), N, S, C, _lib.ptr(w), _lib.ptr(b), _lib.ptr(res), _lib.ptr(dst), None, _lib.ptr(part), C // 32, st))
fused_ctx = lambda: _lib.check(lib.dmme_attention_proj(dt, _lib.ptr(qkv), N, S, C, _lib.ptr(w), _lib.ptr(b), _lib.ptr(res), _lib.ptr(dst), _lib.ptr(ctx), _lib.ptr(part), C // 32, st))
x = (torch.randn(N, S, C, device=dev) + 3.0).bfloat16()
wqkv = (torch.randn(3 * C, C, device=dev) * C**-0.5).bfloat16(); bqkv = torch.randn(3 * C, device=dev) * 0.5
M, wpv = torch.empty_like(w), torch.empty_like(w); cc, b2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
_lib.check(lib.dmme_attention_fold(dt, C, _lib.ptr(wqkv), _lib.ptr(bqkv), _lib.ptr(w), _lib.ptr(b), _lib.ptr(M), _lib.ptr(cc), _lib.ptr(wpv), _lib.ptr(b2), st))
xt = x.float().view(N, S // 32, 32, 32, C // 32); pm = xt.mean(dim=(2, 4)); pm2 = ((xt - pm[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
parts = torch.stack([pm, pm2], dim=-1).contiguous(); gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
sc, sh = torch.empty(N, C, device=dev), torch.empty(N, C, device=dev)
fold = lambda: _lib.check(lib.dmme_attention_block(dt, _lib.ptr(x), N, S, C, _lib.ptr(parts), S // 32, 32 * (C // 32), 32, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, _lib.ptr(sc), _lib.ptr(sh),
                                                    _lib.ptr(M), _lib.ptr(cc), _lib.ptr(wpv), _lib.ptr(b2), _lib.ptr(x), _lib.ptr(dst), _lib.ptr(part), C // 32, st))
print(f"C={C}: the whole block folded (x in, out out) {t(fold):.1f} us")
print(f"C={C} route={os.environ.get('DMME_DEBUG_ROUTE', '')}: attention {t(att):.1f} us; attention+proj {t(fused):.1f} us; with the context tensor {t(fused_ctx):.1f} us")
