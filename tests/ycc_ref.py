"""Plain numpy restatement of libjpeg's planar YCbCr -> RGB output stage, the reference
for the engine's MIPX_OP_YCC (PARITY_ASSUMPTIONS.md row 16).  Not part of the oracle.

Planes are packed as the engine takes them (include/mipx.h): Y (h x w), then Cb and Cr
(ch x cw each), no padding; cw = w, ch = h for 4:4:4 and ceil(w / 2), ceil(h / 2) for 4:2:0.

  4:2:0 upsample (jdsample.c h2v2 fancy, used when cw > 2; plain replication otherwise):
      cy = y >> 1, cx = x >> 1; ny = cy - 1 (even y) / cy + 1 (odd y), nx likewise, clamped;
      s(c) = 3 * C[cy][c] + C[ny][c];  out = (3 * s(cx) + s(nx) + (8 if x even else 7)) >> 4
  conversion (jdcolor.c), int32 with arithmetic shifts, cb = Cb - 128, cr = Cr - 128:
      R = clamp(Y + ((91881 * cr + 32768) >> 16))
      G = clamp(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16))
      B = clamp(Y + ((116130 * cb + 32768) >> 16))
"""
from __future__ import annotations

import numpy as np

YCC_444 = 0
YCC_420 = 1


def chroma_size(w: int, h: int, layout: int):
    return (w, h) if layout == YCC_444 else ((w + 1) // 2, (h + 1) // 2)


def ycc_bytes(w: int, h: int, layout: int) -> int:
    cw, ch = chroma_size(w, h, layout)
    return w * h + 2 * cw * ch


def split(planes: np.ndarray, w: int, h: int, layout: int):
    """(Y, Cb, Cr) views of one image's packed planes."""
    cw, ch = chroma_size(w, h, layout)
    p = np.asarray(planes, dtype=np.uint8).ravel()
    assert p.size == ycc_bytes(w, h, layout), (p.size, w, h, layout)
    y = p[:w * h].reshape(h, w)
    cb = p[w * h:w * h + cw * ch].reshape(ch, cw)
    cr = p[w * h + cw * ch:].reshape(ch, cw)
    return y, cb, cr


def upsample_420(c: np.ndarray, w: int, h: int) -> np.ndarray:
    """One ch x cw chroma plane at h x w, as int32."""
    ch, cw = c.shape
    c = c.astype(np.int32)
    ys, xs = np.arange(h), np.arange(w)
    cy, cx = ys >> 1, xs >> 1
    if cw <= 2:  # libjpeg picks the fancy upsampler only for downsampled_width > 2
        return c[cy][:, cx]
    ny = np.clip(np.where(ys % 2 == 0, cy - 1, cy + 1), 0, ch - 1)
    nx = np.clip(np.where(xs % 2 == 0, cx - 1, cx + 1), 0, cw - 1)
    s = 3 * c[cy] + c[ny]                       # h x cw column sums
    bias = np.where(xs % 2 == 0, 8, 7)
    return (3 * s[:, cx] + s[:, nx] + bias) >> 4


def ycc_ref(planes: np.ndarray, w: int, h: int, layout: int) -> np.ndarray:
    """(h, w, 3) RGB of one image's packed planes, or (n, h, w, 3) of an (n, bytes) batch."""
    p = np.asarray(planes, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([ycc_ref(q, w, h, layout) for q in p])
    y, cb, cr = split(p, w, h, layout)
    y = y.astype(np.int32)
    if layout == YCC_420:
        cb, cr = upsample_420(cb, w, h), upsample_420(cr, w, h)
    cb = cb.astype(np.int32) - 128
    cr = cr.astype(np.int32) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)
