"""The folded form of the single-head 16x16 attention blocks (csrc/attn_mfma.hip: AttnFold; csrc/plan.hip: assign_attn_fold): forwards no
backward follows read the block's raw input x and write `res + proj(attention(qkv(norm(x))))` in ONE launch, with matrices folded from
the weights once per weight version (M = C^-0.5 Wk^T Wq, c = C^-0.5 Wk^T bq, Wpv = Wp Wv, b' = Wp bv + bp).

1. dmme_attention_fold against the float64 products of the 16-bit weights;
2. dmme_attention_block against the UNFOLDED block in float64 (from the 16-bit x and weights, nothing rounded in between), inside the
   project's own `res+attention` bounds (tests/test_gpu_block_forward.py), with four mutated references that must fall outside them;
3. the batch-128 network with and without the fold (golden rows, the two routes against each other, launches, training gradients), and
   a re-pack between two no-grad forwards: never the earlier fold.

Inputs of 1 and 2: x with per-group offsets up to 8.7 sigma; q / k rows x sqrt(3) each (logit std ~3; mean top probability asserted >= 0.2
on the CPU); biases of std 0.5; the residual an independent unit normal (with res = x the scores-x-1.05 mutation hides inside the bf16
bound), one case with res = x."""
import functools
import math

import pytest
import torch

from oracle import synth

pytestmark = pytest.mark.gpu

S = 256
EPS = 1e-5
# (max |err| / max |want|, relative RMS): tests/test_gpu_block_forward.py BOUNDS[..]["res+attention"]
BOUNDS = {"bf16": (2.0e-2, 8.2e-3), "fp16": (1.9e-3, 7.7e-4)}
MANT = {"bf16": 7, "fp16": 10}  # explicit mantissa bits


def _td(dtname):
    return torch.bfloat16 if dtname == "bf16" else torch.float16


@functools.lru_cache(maxsize=None)
def _inputs(C, dtname, cg, N):
    """CPU: the 16-bit operands (as float64) of one block and the norm's exact (a, b) rows"""
    td = _td(dtname)
    G = C // cg
    r16 = lambda t: t.to(td).double()  # noqa: E731
    x = synth.normal(101 + C + N, (N, S, C)).double()
    off = synth.uniform(102 + C + N, (N, G), -8.7, 8.7).double()
    off[:, 0], off[:, 1] = 8.7, -8.7
    x = r16(x + off.repeat_interleave(cg, dim=1)[:, None, :])
    res = r16(synth.normal(103 + C + N, (N, S, C)).double())
    wqkv = synth.normal(104 + C, (3 * C, C)).double() * C**-0.5
    wqkv[: 2 * C] *= math.sqrt(3.0)
    wqkv = r16(wqkv)
    bqkv = synth.normal(105 + C, (3 * C,)).double() * 0.5
    wp = r16(synth.normal(106 + C, (C, C)).double() * C**-0.5)
    bp = synth.normal(107 + C, (C,)).double() * 0.5
    gamma = (1.0 + 0.1 * synth.normal(108 + C, (C,))).double()
    beta = (0.1 * synth.normal(109 + C, (C,))).double()
    f32 = lambda t: t.float().double()  # noqa: E731  (the fp32 rows the kernels read)
    bqkv, bp, gamma, beta = f32(bqkv), f32(bp), f32(gamma), f32(beta)
    xg = x.view(N, S, G, cg)
    mean = xg.mean(dim=(1, 3))
    var = xg.var(dim=(1, 3), unbiased=False)
    rstd = (var + EPS).rsqrt()
    a = rstd.repeat_interleave(cg, dim=1) * gamma
    b = beta - mean.repeat_interleave(cg, dim=1) * a
    # the producers' partials: (mean, M2) per (image, 32 pixels, group)
    xt = x.view(N, S // 32, 32, G, cg)
    pm = xt.mean(dim=(2, 4))
    pm2 = ((xt - pm[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    parts = torch.stack([pm, pm2], dim=-1).float().contiguous()
    return dict(x=x, res=res, wqkv=wqkv, bqkv=bqkv, wp=wp, bp=bp, gamma=gamma, beta=beta, a=a, b=b, parts=parts, offsig=float((mean.abs() * rstd).max()))


def _reference(inp, C, res=None, mutate=None, bk=None):
    """float64, the unfolded block: res + Wp softmax(q k^T C^-0.5) v + bp over n = a x + b"""
    x, a, b = inp["x"], inp["a"], inp["b"]
    res = inp["res"] if res is None else res
    n = x * a[:, None, :] + b[:, None, :]
    wq, wk, wv = inp["wqkv"][:C], inp["wqkv"][C : 2 * C], inp["wqkv"][2 * C :]
    bq, bkk, bv = inp["bqkv"][:C], inp["bqkv"][C : 2 * C], inp["bqkv"][2 * C :]
    if bk is not None:
        bkk = bk
    q = n @ wq.t() + (0.0 if mutate == "no_c" else bq)  # (c = s Wk^T bq is all that bq leaves in a softmax over the keys)
    k = n @ wk.t() + bkk
    nv = x * a[:, None, :] if mutate == "no_vb" else n
    v = nv @ wv.t() + bv
    sc = q @ k.transpose(1, 2) * C**-0.5
    if mutate == "scale":
        sc = sc * 1.05
    p = torch.softmax(sc, dim=2)
    topp = float(p.max(dim=2).values.mean())
    if mutate == "uniform":
        p = torch.full_like(p, 1.0 / S)
    return res + (p @ v) @ inp["wp"].t() + inp["bp"], topp


def _err(got, want):
    d = (got.double() - want).abs()
    return float(d.max()) / float(want.abs().max()), float(d.pow(2).sum().sqrt() / want.pow(2).sum().sqrt())


def _fold_gpu(inp, C, dtname, bk=None):
    from dmme_amd import _lib

    dt, td, dev = _lib.dtype_code(dtname), _td(dtname), torch.device("cuda:0")
    wqkv = inp["wqkv"].to(td).to(dev).contiguous()
    bqkv = inp["bqkv"].clone()
    if bk is not None:
        bqkv[C : 2 * C] = bk
    bqkv = bqkv.float().to(dev).contiguous()
    wp, bp = inp["wp"].to(td).to(dev).contiguous(), inp["bp"].float().to(dev).contiguous()
    M, wpv = torch.zeros((C, C), dtype=td, device=dev), torch.zeros((C, C), dtype=td, device=dev)
    c, b2 = torch.zeros(C, device=dev), torch.zeros(C, device=dev)
    _lib.check(_lib.lib().dmme_attention_fold(dt, C, _lib.ptr(wqkv), _lib.ptr(bqkv), _lib.ptr(wp), _lib.ptr(bp), _lib.ptr(M), _lib.ptr(c), _lib.ptr(wpv), _lib.ptr(b2),
                                              _lib.stream_ptr()), "dmme_attention_fold")
    torch.cuda.synchronize()
    return M, c, wpv, b2


def _block_gpu(inp, C, dtname, cg, N, folded, res=None, rows=False, stats=True):
    """dmme_attention_block; rows: the norm as (scale, shift) rows instead of partials"""
    from dmme_amd import _lib

    dt, td, dev = _lib.dtype_code(dtname), _td(dtname), torch.device("cuda:0")
    M, c, wpv, b2 = folded
    x = inp["x"].to(td).to(dev).contiguous()
    r = (inp["res"] if res is None else res).to(td).to(dev).contiguous()
    dst = torch.zeros((N, S, C), dtype=td, device=dev)
    part = torch.zeros((N, S // 32, C // cg, 2), dtype=torch.float32, device=dev) if stats else None
    if rows:
        parts, gamma, beta = None, None, None
        scale, shift = inp["a"].float().to(dev).contiguous(), inp["b"].float().to(dev).contiguous()
    else:
        parts, gamma, beta = inp["parts"].to(dev), inp["gamma"].float().to(dev), inp["beta"].float().to(dev)
        scale, shift = torch.zeros((N, C), device=dev), torch.zeros((N, C), device=dev)
    _lib.check(_lib.lib().dmme_attention_block(dt, _lib.ptr(x), N, S, C, _lib.ptr(parts), S // 32, 32 * cg, C // cg, _lib.ptr(gamma), _lib.ptr(beta), EPS, _lib.ptr(scale),
                                               _lib.ptr(shift), _lib.ptr(M), _lib.ptr(c), _lib.ptr(wpv), _lib.ptr(b2), _lib.ptr(r), _lib.ptr(dst), _lib.ptr(part), cg,
                                               _lib.stream_ptr()), "dmme_attention_block")
    torch.cuda.synchronize()
    return dst.cpu(), None if part is None else part.cpu(), scale.cpu(), shift.cpu()


CASES = [(256, "bf16", 8), (256, "fp16", 8), (128, "bf16", 4), (128, "fp16", 4), (256, "bf16", 4), (128, "fp16", 8)]


@pytest.mark.parametrize("C,dtname", [(256, "bf16"), (256, "fp16"), (128, "bf16"), (128, "fp16")])
def test_fold_entry_vs_float64_products(C, dtname):
    """every matrix element: one rounding of the float64 value - half a unit in the last place of the 16-bit type, plus the a-priori bound
    of an fp32 sum of C products (C 2^-24 sum |terms|); the fp32 rows within 1e-5 of their maximum"""
    inp = _inputs(C, dtname, 8, 3)
    M, c, wpv, b2 = [t.cpu().double() for t in _fold_gpu(inp, C, dtname)]
    s = C**-0.5
    wq, wk, wv = inp["wqkv"][:C], inp["wqkv"][C : 2 * C], inp["wqkv"][2 * C :]
    bq, bv = inp["bqkv"][:C], inp["bqkv"][2 * C :]
    for name, got, want, mag in (("M", M, s * wk.t() @ wq, s * wk.abs().t() @ wq.abs()), ("Wpv", wpv, inp["wp"] @ wv, inp["wp"].abs() @ wv.abs())):
        e = torch.floor(torch.log2(want.abs().clamp_min(2.0**-14 if dtname == "fp16" else 1e-30)))
        ulp = torch.exp2(e - MANT[dtname])
        bound = 0.5 * ulp + C * 2.0**-24 * mag
        excess = float(((got - want).abs() / bound).max())
        print(f"fold C={C} {dtname} {name}: worst |err| / bound {excess:.3f}; rms {float(want.pow(2).mean().sqrt()):.3e}")
        assert excess <= 1.0, name
    for name, got, want in (("c", c, s * wk.t() @ bq), ("b'", b2, inp["wp"] @ bv + inp["bp"])):
        err = float((got - want).abs().max()) / float(want.abs().max())
        print(f"fold C={C} {dtname} {name}: max |err| / max {err:.3e}")
        assert err <= 1e-5, name


@pytest.mark.parametrize("C,dtname,cg", CASES)
@pytest.mark.parametrize("N", [3, 16])  # (odd N, a / b per image; 16: the XCD-ordered index map works in eights)
def test_attention_block_vs_unfolded_float64(C, dtname, cg, N):
    inp = _inputs(C, dtname, cg, N)
    want, topp = _reference(inp, C)
    print(f"\nattention_block C={C} {dtname} cg={cg} N={N}: mean top probability {topp:.3f}, group |mean| / std up to {inp['offsig']:.2f}")
    assert topp >= 0.2 and inp["offsig"] >= 8.0
    folded = _fold_gpu(inp, C, dtname)
    dst, part, scale, shift = _block_gpu(inp, C, dtname, cg, N, folded)
    assert bool(torch.isfinite(dst.float()).all())
    bmx, brms = BOUNDS[dtname]
    mx, rms = _err(dst, want)
    print(f"  fold vs float64: max-abs / max {mx:.3e} (bound {bmx}), relative RMS {rms:.3e} (bound {brms})")
    # the norm's rows, as the workgroup of an image's first tile leaves them for later readers
    ea = float((scale.double() - inp["a"]).abs().max() / inp["a"].abs().max())
    eb = float((shift.double() - inp["b"]).abs().max() / inp["b"].abs().max())
    print(f"  norm rows vs float64: a {ea:.2e}, b {eb:.2e}")
    assert ea <= 1e-5 and eb <= 1e-5
    assert mx <= bmx and rms <= brms
    if N == 3:
        # mutated references must FAIL the bound on the same inputs
        for mode in ("uniform", "scale", "no_c", "no_vb"):
            m_mx, m_rms = _err(dst, _reference(inp, C, mutate=mode)[0])
            print(f"  vs {mode}: max-abs / max {m_mx:.3e}, relative RMS {m_rms:.3e}")
            assert m_mx > bmx or m_rms > brms, mode
        # bk drops out of a softmax over the keys: bit-identical output with large values there
        bk = 50.0 * synth.normal(7, (C,)).double()
        folded_bk = _fold_gpu(inp, C, dtname, bk=bk)
        for t0, t1 in zip(folded, folded_bk):
            assert torch.equal(t0, t1)
        dst_bk, _, _, _ = _block_gpu(inp, C, dtname, cg, N, folded_bk)
        assert torch.equal(dst_bk, dst)
        # the norm as (scale, shift) rows: the same block (rows rounded to fp32 from float64 instead of merged from partials in fp32)
        dst_rows, part_rows, _, _ = _block_gpu(inp, C, dtname, cg, N, folded, rows=True)
        r_mx, r_rms = _err(dst_rows, want)
        print(f"  rows instead of partials: max-abs / max {r_mx:.3e}, relative RMS {r_rms:.3e}")
        assert r_mx <= bmx and r_rms <= brms
        # without statistics: the same outputs
        assert torch.equal(_block_gpu(inp, C, dtname, cg, N, folded, stats=False)[0], dst)
    # the next norm's partials: (mean, M2) of the ROUNDED outputs per (image, 32 tokens, group)
    xo = dst.double().view(N, S // 32, 32, C // cg, cg)
    mean = xo.mean(dim=(2, 4))
    m2 = ((xo - mean[:, :, None, :, None]) ** 2).sum(dim=(2, 4))
    assert (part[..., 0].double() - mean).abs().max().item() <= 1e-5 * max(1.0, mean.abs().max().item())
    assert ((part[..., 1].double() - m2).abs() / m2.clamp_min(1e-6)).max().item() <= 1e-4


@pytest.mark.parametrize("C,dtname,cg", [(256, "bf16", 8), (128, "fp16", 4)])
def test_attention_block_with_its_own_input_as_residual(C, dtname, cg):
    inp = _inputs(C, dtname, cg, 3)
    want, _ = _reference(inp, C, res=inp["x"])
    dst, _, _, _ = _block_gpu(inp, C, dtname, cg, 3, _fold_gpu(inp, C, dtname), res=inp["x"])
    mx, rms = _err(dst, want)
    print(f"attention_block C={C} {dtname} res = x: max-abs / max {mx:.3e}, relative RMS {rms:.3e}")
    assert mx <= BOUNDS[dtname][0] and rms <= BOUNDS[dtname][1]


def test_attention_block_refuses_other_shapes():
    from dmme_amd import _lib

    dev = torch.device("cuda:0")
    dt = _lib.dtype_code("bf16")
    z = lambda *s: torch.zeros(s, dtype=torch.bfloat16, device=dev)  # noqa: E731
    f = lambda *s: torch.zeros(s, device=dev)  # noqa: E731
    for N, S_, C in ((4, 64, 256), (4, 256, 64), (4, 256, 512)):
        rc = _lib.lib().dmme_attention_block(dt, _lib.ptr(z(N, S_, C)), N, S_, C, None, 0, 0, 0, None, None, EPS, _lib.ptr(f(N, C)), _lib.ptr(f(N, C)), _lib.ptr(z(C, C)),
                                             _lib.ptr(f(C)), _lib.ptr(z(C, C)), _lib.ptr(f(C)), _lib.ptr(z(N, S_, C)), _lib.ptr(z(N, S_, C)), None, 0, _lib.stream_ptr())
        assert rc != 0, (N, S_, C)


# ---------------------------------------------------------------------------------------------------------------- the network
def _net(seed, precision):
    import dmme_amd
    from oracle import unet as O

    cfg = O.UNetConfig()
    net = dmme_amd.UNet(cfg.in_channels, cfg.pos_dim, cfg.emb_dim, cfg.num_groups, cfg.dropout, cfg.channels_per_depth, cfg.num_blocks,
                        cfg.attention_depths, precision=precision)
    net.load_state_dict(O.make_state_dict(cfg, seed), strict=True)
    return net.cuda().eval()


def _rel(a, b):
    return float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt())


@pytest.mark.parametrize("precision,atol_ref,rtol_ab", [("bf16", 1.7e-2, 1.0e-2), ("fp16", 2.0e-3, 2.5e-3)])  # (the networks' bounds; tests/test_gpu_switches.py's between routes)
def test_batch128_network_folded_vs_reference_rows_and_vs_the_unfolded_route(golden, precision, atol_ref, rtol_ab):
    from tests.gpu_util import route_env

    g = golden("unet_full")
    seed = int(g["full_seed"])
    base = synth.normal(int(g["full_xseed"]), (2, 3, 32, 32))
    x = base.repeat(64, 1, 1, 1).cuda()
    t = torch.from_numpy(g["full_t_one"]).cuda()

    def run(env):
        with route_env(env):
            net = _net(seed, precision)
            with torch.no_grad():
                y0 = net(x, t).float().cpu()
                # another weight version: the value rows of one 16x16 block's qkv weight doubled - the re-pack ends the fold's validity,
                # the forward folds again; never the earlier matrices
                w = dict(net.named_parameters())["down_layers.3.attention.qkv_proj.weight"]
                w[2 * w.shape[1] :] *= 2.0
                y1 = net(x, t).float().cpu()
            plan = net._last_plan
            return y0, y1, plan.lib.dmme_unet_plan_num_launches(plan.h), plan.lib.dmme_unet_plan_num_launches_nograd(plan.h), plan.lib.dmme_unet_plan_num_folded(plan.h), net

    ya0, ya1, na, na_ng, nf, net_a = run({})
    yb0, yb1, nb, nb_ng, nfb, _ = run({"DMME_NO_ATTN_FOLD": "1"})
    assert na == nb == nb_ng and nb_ng - na_ng == 5 and nf == 5 and nfb == 0, (na, na_ng, nb, nb_ng, nf, nfb)
    rows = ya0.reshape(64, 2, 3, 32, 32)
    assert torch.equal(rows, rows[:1].expand_as(rows))  # every image pair took the same arithmetic
    e_ref = float((rows[0] - torch.from_numpy(g["full_y_one"])).abs().max())
    e_ab = _rel(ya0, yb0)
    print(f"{precision}: no-grad launches {nb_ng} -> {na_ng}; max|err| vs reference {e_ref:.3e} (unfolded: {float((yb0.reshape(64, 2, 3, 32, 32)[0] - torch.from_numpy(g['full_y_one'])).abs().max()):.3e});"
          f" relative rms between the two routes {e_ab:.3e}")
    assert e_ref <= atol_ref
    assert e_ab <= rtol_ab
    # the changed weight moves the output, and by what it moves the unfolded route's
    da, db = ya1 - ya0, yb1 - yb0
    e_d, moved = _rel(da, db), _rel(yb1, yb0)
    print(f"  value rows x 2: the unfolded output moves by {moved:.3e} relative rms, the folded route's change differs from that change by {e_d:.3e} of it;"
          f" routes now {_rel(ya1, yb1):.3e} apart")
    assert moved >= 4 * rtol_ab  # (a property of the inputs: the change stands clear of what the routes may differ by)
    assert _rel(ya1, yb1) <= rtol_ab
    assert e_d <= 0.5  # (each output within rtol_ab of the other route's, the change at least four times that)
    # C ABI: a re-pack alone (no dmme_unet_pack_folded behind it) makes the no-grad forward run the unfolded walk - bit for bit the
    # switch-off plan's result, not a mixture with the earlier matrices
    from dmme_amd import _lib

    plan = net_a._last_plan
    flat = net_a._ensure_flat()
    _lib.check(plan.lib.dmme_unet_pack_params(plan.h, _lib.ptr(flat), _lib.ptr(plan.packed), _lib.stream_ptr()))
    y = torch.empty(128, 3, 32, 32, device="cuda")
    tt = t.to(torch.int64).reshape(-1).contiguous()
    _lib.check(plan.lib.dmme_unet_forward_nograd(plan.h, _lib.ptr(plan.packed), _lib.ptr(x.contiguous()), _lib.ptr(tt), int(tt.numel()), _lib.ptr(y), _lib.ptr(plan.workspace),
                                                 None, _lib.stream_ptr()))
    torch.cuda.synchronize()
    plan.fold_version = None  # (the module's own stamp: this call went behind its back)
    assert torch.equal(y.cpu(), yb1), "a no-grad forward behind a bare re-pack did not run the unfolded walk"


def test_batch128_training_step_is_the_unfolded_one():
    """a forward that a backward follows never folds: loss and gradient of one training step with and without the switch, same seed and
    dropout masks (bound: tests/test_gpu_attn_proj.py's for two runs of one route); a no-grad forward in between does not disturb it"""
    import dmme_amd
    from tests.gpu_util import route_env

    def step(env):
        with route_env(env):
            torch.manual_seed(0)
            net = dmme_amd.UNet(precision="bf16").cuda().train()
            x = torch.randn(128, 3, 32, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
            t = torch.arange(128, device="cuda") * 7 % 1000
            net.eval()
            with torch.no_grad():
                net(x, t)  # (folds, where the plan folds)
            net.train()
            y = net(x, t)
            l = (y.float() ** 2).mean()
            l.backward()
            return float(l.detach()), net.flat_grad().float().clone()

    la, ga = step({})
    lb, gb = step({"DMME_NO_ATTN_FOLD": "1"})
    rel = float((ga - gb).norm() / gb.norm())
    print(f"training step loss {la:.6f} vs {lb:.6f} with the switch; relative gradient difference {rel:.3e}")
    assert abs(la - lb) <= 2e-3 * abs(lb)
    assert rel <= 5e-2
