"""Image grids with the reference's names (src/dmme/common/vis.py:7-30): `make_history` lays a list of image batches out as
torchvision's `make_grid(padding=2, pad_value=0)` does, through dmme_grid_tile launches (one per batch; nothing leaves the
device), and `save_png` writes a grid with the standard library alone.  torchvision and PIL are not dependencies."""

from __future__ import annotations

import math
import struct
import zlib

import torch
from torch import Tensor

from .. import _lib

PAD = 2  # make_grid's default padding, which the reference never changes
FLOAT32, UINT8 = 0, 1  # dmme_grid_tile's out_kind


def grid_shape(C: int, H: int, W: int, xmaps: int, ymaps: int, pad: int = PAD):
    """shape of the canvas of xmaps x ymaps cells (a single channel is shown as three, as make_grid does)"""
    return (3 if C == 1 else C, ymaps * (H + pad) + pad, xmaps * (W + pad) + pad)


def new_canvas(C: int, H: int, W: int, xmaps: int, ymaps: int, pad: int = PAD, out_kind: int = FLOAT32, device="cuda") -> Tensor:
    """a zeroed canvas: the padding is never written again"""
    if out_kind not in (FLOAT32, UINT8):
        raise ValueError(f"out_kind {out_kind!r}: 0 (float32) or 1 (uint8)")
    return torch.zeros(grid_shape(C, H, W, xmaps, ymaps, pad), dtype=torch.uint8 if out_kind == UINT8 else torch.float32, device=device)


def grid_tile(x: Tensor, canvas: Tensor, cell0: int, cell_stride: int, xmaps: int, ymaps: int, pad: int = PAD, raw: bool = False) -> Tensor:
    """one dmme_grid_tile launch on the current stream: image b of x into cell cell0 + b*cell_stride of `canvas`, denormed unless `raw`"""
    if not (isinstance(x, Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise ValueError("grid_tile: a contiguous fp32 GPU image batch (B, C, H, W)")
    B, C, H, W = x.shape
    if canvas.dtype not in (torch.float32, torch.uint8) or not canvas.is_contiguous() or canvas.device != x.device \
            or tuple(canvas.shape) != grid_shape(C, H, W, xmaps, ymaps, pad):
        raise ValueError(f"grid_tile: canvas {tuple(canvas.shape)} {canvas.dtype} where {grid_shape(C, H, W, xmaps, ymaps, pad)} float32 / uint8 on {x.device} is due")
    _lib.check(_lib.lib().dmme_grid_tile(_lib.ptr(x), B, C, H, W, int(cell0), int(cell_stride), int(xmaps), int(ymaps), int(pad),
                                         UINT8 if canvas.dtype == torch.uint8 else FLOAT32, int(bool(raw)), _lib.ptr(canvas), _lib.stream_ptr()), "dmme_grid_tile")
    return canvas


def history_nrow(batch_size: int) -> int:
    """images per row of a single history, by the reference's loop (common/vis.py:17-23): the largest divisor i of the batch in
    3..floor(sqrt(batch)) gives batch // i; without one (a batch of 8 included) the grid is one column"""
    for i in range(int(math.sqrt(batch_size)), 2, -1):
        if batch_size % i == 0:
            return batch_size // i
    return 1


def make_history(history, out_kind: int = FLOAT32) -> Tensor:
    r"""the grid of a list of image batches :math:`(N, C, H, W)` (reference: common/vis.py:7-30).  One batch: its images in rows of
    `history_nrow(N)`; several: one row per image, one column per batch.  The values are placed as they are (no denorm, as in the
    reference: `GenerateImage.generate_img` has denormed them); `out_kind=1` gives the uint8 grid `save_png` writes.
    A batch of exactly one image comes back unpadded, as make_grid returns it."""
    history = list(history)
    if not history:
        raise ValueError("make_history: an empty history")
    x0 = history[0]
    for x in history:
        if not isinstance(x, Tensor) or x.dim() != 4 or x.shape != x0.shape:
            raise ValueError("make_history: a list of image batches (N, C, H, W) of one shape")
    frames = [x.detach().to(torch.float32).contiguous() for x in history]
    N, C, H, W = frames[0].shape
    L = len(frames)
    if L == 1:
        xmaps = min(history_nrow(N), N)
        ymaps = -(-N // xmaps)
    else:
        xmaps, ymaps = L, N
    pad = 0 if N * L == 1 else PAD
    canvas = new_canvas(C, H, W, xmaps, ymaps, pad, out_kind, frames[0].device)
    for k, x in enumerate(frames):
        grid_tile(x, canvas, k, L, xmaps, ymaps, pad, raw=True)
    return canvas


def to_uint8(grid):
    """float values in [0, 1] -> bytes by torchvision's save_image rule, (uint8) clamp(v * 255 + 0.5, 0, 255) in float32; uint8 passes"""
    import numpy as np

    a = grid.detach().cpu().numpy() if isinstance(grid, Tensor) else np.asarray(grid)
    if a.dtype == np.uint8:
        return a
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError(f"an image of uint8 or floating-point values, got {a.dtype}")
    v = a.astype(np.float32) * np.float32(255.0) + np.float32(0.5)
    return np.clip(v, np.float32(0.0), np.float32(255.0)).astype(np.uint8)


def _chunk(tag: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def save_png(path, grid) -> None:
    """write `grid`, uint8 (C, H, W) or float in [0, 1] (converted by `to_uint8`), C = 3 (RGB) or 1 (greyscale; (H, W) too), as an
    8-bit non-interlaced PNG with filter type 0 on every row"""
    import numpy as np

    a = to_uint8(grid)
    if a.ndim == 2:
        a = a[None]
    if a.ndim != 3 or a.shape[0] not in (1, 3) or a.shape[1] < 1 or a.shape[2] < 1:
        raise ValueError(f"save_png: an image (C, H, W) with C = 1 or 3, got {a.shape}")
    C, H, W = a.shape
    rows = np.zeros((H, 1 + W * C), dtype=np.uint8)  # a filter byte (0: none) in front of every row
    rows[:, 1:] = np.ascontiguousarray(a.transpose(1, 2, 0)).reshape(H, W * C)
    ihdr = struct.pack(">IIBBBBB", W, H, 8, 2 if C == 3 else 0, 0, 0, 0)
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", zlib.compress(rows.tobytes(), 6)) + _chunk(b"IEND", b""))
