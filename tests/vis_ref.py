"""CPU restatement of the image-grid surface (dmme_amd.common.vis, dmme_grid_tile, history_ordinals) in numpy float32, written from
the descriptions of torchvision's make_grid / save_image and of the reference's make_history, not from their code; plus a reader
for the PNG files save_png writes (filter type 0 only), which checks every chunk's CRC."""

import math
import struct
import zlib

import numpy as np

F = np.float32


def denorm(x):
    """clip((x + 1) / 2, 0, 1), every operation rounded to float32"""
    v = (np.asarray(x, dtype=F) + F(1.0)) * F(0.5)
    return np.clip(v, F(0.0), F(1.0)).astype(F)


def to_uint8(v):
    """(uint8) clamp(v * 255 + 0.5, 0, 255), truncated; the multiply and the add rounded to float32 one by one"""
    s = np.asarray(v, dtype=F) * F(255.0)
    s = s + F(0.5)
    return np.clip(s, F(0.0), F(255.0)).astype(np.uint8)


def make_grid(x, nrow, pad=2):
    """images (B, C, H, W) in rows of `nrow`, `pad` zero pixels around and between them; a single channel is shown three times; a batch
    of exactly one image comes back as (C, H, W), unpadded"""
    x = np.asarray(x)
    if x.shape[1] == 1:
        x = np.concatenate([x, x, x], axis=1)
    B, C, H, W = x.shape
    if B == 1:
        return x[0].copy()
    xmaps = min(nrow, B)
    ymaps = int(math.ceil(B / xmaps))
    out = np.zeros((C, ymaps * (H + pad) + pad, xmaps * (W + pad) + pad), dtype=x.dtype)
    for k in range(B):
        r, c = divmod(k, xmaps)
        y0, x0 = r * (H + pad) + pad, c * (W + pad) + pad
        out[:, y0:y0 + H, x0:x0 + W] = x[k]
    return out


def history_nrow(n):
    for i in range(int(math.sqrt(n)), 2, -1):
        if n % i == 0:
            return n // i
    return 1


def make_history(history):
    """one batch: rows of history_nrow(N); several: image b's frames in row b"""
    history = [np.asarray(h) for h in history]
    if len(history) == 1:
        return make_grid(history[0], history_nrow(history[0].shape[0]))
    st = np.stack(history, axis=1)  # (N, L, C, H, W)
    return make_grid(st.reshape((-1,) + st.shape[2:]), st.shape[1])


def reference_save_t(timesteps, vis_length):
    """the timesteps in front of whose step the reference's callback keeps a frame"""
    return [int(timesteps / (vis_length - 1) * i) for i in range(vis_length - 1, 0, -1)]


def history_ordinals(count, vis_length):
    """a frame in front of the step from t is a frame after count - t steps; the final frame after `count`; t = 0 is never stepped from"""
    kept = {count - t for t in reference_save_t(count, vis_length) if 1 <= t <= count}
    return sorted(kept | {count})


def read_png(path):
    """(C, H, W) uint8 of an 8-bit RGB / greyscale, non-interlaced PNG whose rows all have filter type 0; asserts the signature, the
    chunk order and every CRC"""
    with open(path, "rb") as f:
        data = f.read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "PNG signature"
    pos, chunks = 8, []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert crc == (zlib.crc32(tag + body) & 0xFFFFFFFF), f"CRC of chunk {tag!r}"
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    W, H, depth, colour, comp, filt, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert depth == 8 and colour in (0, 2) and comp == 0 and filt == 0 and interlace == 0
    C = 3 if colour == 2 else 1
    raw = zlib.decompress(b"".join(body for tag, body in chunks if tag == b"IDAT"))
    rows = np.frombuffer(raw, dtype=np.uint8).reshape(H, 1 + W * C)
    assert not rows[:, 0].any(), "filter type 0 on every row"
    return np.ascontiguousarray(rows[:, 1:].reshape(H, W, C).transpose(2, 0, 1))
