"""What the block-local parity tests share (tests/test_gpu_block_grads.py: the backward; tests/test_gpu_block_forward.py: the forward
and the GroupNorm statistics): the walk over the layer graph, the rounding conventions of the float64 reference, the attention block
restated so that it runs on picked images and with a mutated softmax, and the float64 forward of every node from its stored inputs.
Plain helpers; CPU only."""

import dataclasses
from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

from oracle import iddpm as OI
from oracle import unet as O

EPS = 1e-5  # nn.GroupNorm's default, the reference's (models/ddpm.py:25-35)


def _storage(precision):
    """the 16-bit type tensors are stored in, None where they stay fp32 (fp32, and bf16x3: three-pass bf16 products of fp32 tensors)"""
    return {"bf16": torch.bfloat16, "fp16": torch.float16}.get(precision)


def _rounder(precision):
    """straight-through rounding to the 16-bit type (identity for fp32): forward value rounded, gradient passed unchanged"""
    dt = _storage(precision)
    if dt is None:
        return lambda t: t

    def q(t):
        return t + (t.to(dt).to(t.dtype) - t).detach()

    return q


def _wround(precision):
    dt = _storage(precision)
    if dt is None:
        return lambda w: w.double()
    return lambda w: w.to(dt).double()


def _walk(g) -> Tuple[List[Tuple[object, List[str]]], str]:
    """(node, names of its input tensors) in forward order, as oracle.unet.unet_forward walks the graph; the last tensor's name"""
    seq, prev, skips = [], "input_conv", ["input_conv"]
    for n in g.down:
        seq.append((n, [prev]))
        prev = n.prefix
        skips.append(prev)
    for n in g.mid:
        seq.append((n, [prev]))
        prev = n.prefix
    for n in g.up:
        seq.append((n, [prev, skips.pop()] if n.kind == "res" else [prev]))
        prev = n.prefix
    return seq, prev


def _shapes(g, B, H):
    """name -> (B, C, H, W) of every named tensor"""
    out = {"input_conv": (B, g.base, H, H)}
    seq, _ = _walk(g)
    for n, ins in seq:
        h = out[ins[0]][2]
        h = h // 2 if n.kind == "down" else 2 * h if n.kind == "up" else h
        out[n.prefix] = (B, n.c_out, h, h)
    return out


# ---- picked images --------------------------------------------------------------------------------------------------------------------
def pick_images(B):
    """the images a float64 reference is computed for: all of a small batch; of a larger one the first and last two (the first and last
    pixel groups of the level engine) and both sides of the middle"""
    if B <= 5:
        return list(range(B))
    return sorted({0, 1, B // 2 - 1, B // 2, B - 2, B - 1})


def attention_sources(pick, B, heads):
    """images whose attention rows the outputs of `pick` read.  One head: the image itself.  The IDDPM merge reads the (b head) rows as
    (head b) (oracle.iddpm.multi_head_attention): output image b', head slot h' is row h' * B + b' = (image (h' B + b') // heads,
    head (h' B + b') % heads)."""
    return sorted(set(pick) | {(h * B + b) // heads for b in pick for h in range(heads)})


# ---- attention, block-local -----------------------------------------------------------------------------------------------------------
def softmax_figures(s):
    """of the logits (..., S, S): their standard deviation, the largest max - min of a row, the mean of the rows' top probability"""
    p = torch.softmax(s, -1)
    return {"logit_std": float(s.std()), "row_range": float((s.amax(-1) - s.amin(-1)).max()), "top_p": float(p.amax(-1).mean()), "keys": s.shape[-1]}


MUTATIONS = ("uniform", "scale")  # softmax of zeros; softmax of 1.05 x the scores


def attention_local(sd, p, x, groups, heads, src, pick, B, q=None, modes=(None,), figures=None, norm_inputs=None):
    """oracle.unet.attention_block / oracle.iddpm.multi_head_attention on the images `src` (global indices, x = their rows) for the
    output images `pick` of a batch of B, with the rounding points of `q`.  modes: None (the block), "uniform" (every key weighted
    1 / S), "scale" (scores x 1.05) - the mutated references a parity bound must tell from the kernel.  Returns {mode: (len(pick), C,
    H, W)}.  figures / norm_inputs: dicts that receive the softmax figures / the norm's input rows of `pick`."""
    rq = q or (lambda t: t)
    n, c, hh, ww = x.shape
    S, d = hh * ww, c // heads
    pos = {g: i for i, g in enumerate(src)}
    own = [pos[b] for b in pick]
    if norm_inputs is not None:
        norm_inputs[p + ".norm"] = x[own]
    h = rq(F.group_norm(x, groups, sd[p + ".norm.weight"], sd[p + ".norm.bias"], eps=EPS))
    qkv = rq(F.conv2d(h, sd[p + ".qkv_proj.weight"], sd[p + ".qkv_proj.bias"])).reshape(n, heads, 3 * d, S)
    Q, K, V = qkv[:, :, :d].transpose(2, 3), qkv[:, :, d : 2 * d] * c**-0.5, qkv[:, :, 2 * d :].transpose(2, 3)
    s = Q @ K  # (n, heads, S, S)
    if figures is not None:
        figures[p] = softmax_figures(s)
    out = {}
    for mode in modes:
        sm = s * 1.05 if mode == "scale" else torch.zeros_like(s) if mode == "uniform" else s
        o = torch.softmax(sm, -1) @ V  # (n, heads, S, d)
        ctx = torch.stack([torch.cat([o[pos[(hs * B + b) // heads], (hs * B + b) % heads].t() for hs in range(heads)], 0) for b in pick])
        ctx = rq(ctx.reshape(len(pick), c, hh, ww))
        out[mode] = F.conv2d(ctx, sd[p + ".proj.weight"], sd[p + ".proj.bias"]) + x[own]
    return out


class _NormTap:
    """records the input of every F.group_norm call made inside the block (the oracle's res_block calls it once per norm, in order)"""

    def __enter__(self):
        self.inputs, self._orig = [], F.group_norm

        def tap(x, *a, **kw):
            self.inputs.append(x)
            return self._orig(x, *a, **kw)

        F.group_norm = tap
        return self

    def __exit__(self, *a):
        F.group_norm = self._orig


def group_stats(x, groups):
    """float64 {mean, rstd} rows (n, groups) of nn.GroupNorm over x (n, C, H, W)"""
    v = x.double().reshape(x.shape[0], groups, -1)
    mean = v.mean(-1)
    var = (v - mean[..., None]).pow(2).mean(-1)
    return mean, (var + EPS).rsqrt()


def images_needed(arch, cfg, pick, B):
    """the images whose stored activations forward_reference reads for the outputs of `pick`"""
    return attention_sources(pick, B, cfg.num_heads if arch == "iddpm" else 1)


def forward_reference(arch, cfg, sd, precision, x_in, acts, masks, pick, B, mutations=(), figures=None, norm_inputs=None, have=None):
    """Block-local float64 forward.  acts: name -> stored activation ("condition" included) of the whole batch, or of the images
    `have` (a sorted list holding at least images_needed) in that order; x_in and masks: the whole batch.  Every node is computed
    for the images `pick` from the stored outputs of its producers (an up ResBlock: the concat), rounding where the kernels round (the
    oracle's `q` hook, 16-bit conv / linear weights).  Returns name -> {mode: (len(pick), C, H, W)}: every named tensor and "output",
    mode None plus, for the blocks with attention, `mutations`.  norm_inputs receives the input rows of every GroupNorm, by the norm's
    state_dict prefix."""
    q, wq = _rounder(precision), _wround(precision)
    M = OI if arch == "iddpm" else O
    g = M.build_graph(cfg)
    heads = cfg.num_heads if arch == "iddpm" else 1
    sdq = {k: (wq(v) if v.dim() >= 2 and k != "condition.0.embeddings" else v.double()) for k, v in sd.items()}
    pos = {b: i for i, b in enumerate(have if have is not None else range(B))}
    rows = lambda idx: [pos[b] for b in idx]  # noqa: E731
    temb = acts["condition"].double()
    second = ".norm" if arch == "iddpm" else ".conv2.0"
    out: Dict[str, Dict] = {}
    with torch.no_grad():
        # input conv: the 3-channel network input stays fp32
        out["input_conv"] = {None: F.conv2d(x_in[pick].double(), sdq["input_conv.weight"], sdq["input_conv.bias"], padding=1)}
        seq, last = _walk(g)
        for n, ins in seq:
            src = attention_sources(pick, B, heads) if n.kind == "res" and n.attn else pick
            x = torch.cat([acts[k][rows(src)].double() for k in ins], 1)
            if n.kind == "res":
                own = [src.index(b) for b in pick]
                m = masks[n.prefix][src].double() if masks is not None else None
                with _NormTap() as tap:
                    h = M.res_block(sdq, cfg, dataclasses.replace(n, attn=False), x, temb[rows(src)], m, q)
                assert len(tap.inputs) == 2, len(tap.inputs)
                if norm_inputs is not None:
                    norm_inputs[n.prefix + ".conv1.0"] = tap.inputs[0][own]
                    norm_inputs[n.prefix + second] = tap.inputs[1][own]
                if n.attn:
                    out[n.prefix] = attention_local(sdq, n.prefix + ".attention", q(h), cfg.num_groups, heads, src, pick, B, q, (None,) + tuple(mutations),
                                                    figures, norm_inputs)
                else:
                    out[n.prefix] = {None: h}
            elif n.kind == "down":
                out[n.prefix] = {None: F.conv2d(x, sdq[n.prefix + ".weight"], sdq[n.prefix + ".bias"], stride=2, padding=1)}
            else:
                out[n.prefix] = {None: F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), sdq[n.prefix + ".conv.weight"], sdq[n.prefix + ".conv.bias"],
                                                padding=1)}
        # output conv: GroupNorm + SiLU, rounded, conv
        xl = acts[last][rows(pick)].double()
        if norm_inputs is not None:
            norm_inputs["output_conv.0"] = xl
        h = q(F.silu(F.group_norm(xl, cfg.num_groups, sdq["output_conv.0.weight"], sdq["output_conv.0.bias"], eps=EPS)))
        out["output"] = {None: F.conv2d(h, sdq["output_conv.2.weight"], sdq["output_conv.2.bias"], padding=1)}
    return out


def node_roles(g):
    """name -> role of every node the forward reference returns"""
    roles = {"input_conv": "in", "output": "out"}
    for n, _ in _walk(g)[0]:
        roles[n.prefix] = ("res+attention" if n.attn else "res") if n.kind == "res" else n.kind
    return roles
