"""libjpeg's shrink-on-load in numpy (PARITY_ASSUMPTIONS.md row 19): the coefficient payload of
tests/jpegd_ref.py decoded at 1/2, 1/4 or 1/8, as jdmaster.c, jddctmgr.c and jidctred.c do it,
made total the way jpegd_ref is.  tests/test_jpegds_cpu.py pins it to libjpeg-turbo inside Pillow
on files an encoder wrote; the GPU tests hold the kernel to it on every input.  Not part of the
oracle.

  output size: ceil(W / s) x ceil(H / s); every component gets an N x N inverse DCT of its
      8 x 8 blocks, which tile its plane at pitch N, and the plane is cropped to the output size:
        Y and 4:4:4 chroma: N = 8 / s;  4:2:0 chroma: N = 16 / s (8 at s = 2: jpegd_ref's pass)
      so there is no upsampling, and the result is three equal planes (ycc_ref's YCC_444)
  dequantise: d = int16(coef * q)
  DS(v, S) = (v + (1 << (S - 1))) >> S on int32 sums that wrap; pass 1 down the columns,
      saturated to int16; pass 2 along the rows; sample = clamp(v + 128, 0, 255)
  N = 4, on i0 i1 i2 i3 i5 i6 i7 (row 4 and column 4 are never read), S = 12 then 19:
      t0 = i0 << 14;  t2 = i2 * 15137 - i6 * 6270;  t10 = t0 + t2;  t12 = t0 - t2
      a0 = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697
      a2 = -i7 * 4176 - i5 * 4926 + i3 * 7373 + i1 * 20995
      out = DS(t10 + a2), DS(t12 + a0), DS(t12 - a0), DS(t10 - a2)
  N = 2, on i0 i1 i3 i5 i7, S = 13 then 20:
      t10 = i0 << 15;  t0 = -i7 * 5906 + i5 * 6967 - i3 * 10426 + i1 * 29692
      out = DS(t10 + t0), DS(t10 - t0)
  N = 1: DS(d00, 3)"""
import numpy as np

from jpegd_ref import YCC_420, YCC_444, idct_blocks, split_payload, wrap16, wrap32  # noqa: F401

SHIFTS = {4: (12, 19), 2: (13, 20)}


def out_size(w, h, s):
    return -(-w // s), -(-h // s)


def idct_sizes(layout, s):
    """N of Y, Cb, Cr at scale 1/s."""
    c = min(8, 16 // s) if layout == YCC_420 else 8 // s
    return [8 // s, c, c]


def _ds(v, shift):
    return wrap32(wrap32(v) + (1 << (shift - 1))) >> shift


def pass4(d, shift):
    """One 4-point pass of jidctred.c over the last axis (8 long) of an int64 array: 4 results."""
    i = [d[..., k] for k in range(8)]
    t0 = i[0] << 14
    t2 = i[2] * 15137 - i[6] * 6270
    t10, t12 = t0 + t2, t0 - t2
    a0 = -i[7] * 1730 + i[5] * 11893 - i[3] * 17799 + i[1] * 8697
    a2 = -i[7] * 4176 - i[5] * 4926 + i[3] * 7373 + i[1] * 20995
    return np.stack([_ds(v, shift) for v in (t10 + a2, t12 + a0, t12 - a0, t10 - a2)], axis=-1)


def pass2(d, shift):
    """... and of its 2-point one: 2 results."""
    i = [d[..., k] for k in range(8)]
    t10 = i[0] << 15
    t0 = -i[7] * 5906 + i[5] * 6967 - i[3] * 10426 + i[1] * 29692
    return np.stack([_ds(v, shift) for v in (t10 + t0, t10 - t0)], axis=-1)


def idct_blocks_scaled(coefs, q, n, trace=None):
    """(hb, wb, 64) quantised coefficients and a 64-entry table -> (n hb, n wb) uint8 samples."""
    if n == 8:
        return idct_blocks(coefs, q, trace)
    hb, wb, _ = coefs.shape
    d = wrap16(coefs * q.reshape(1, 1, 64)).reshape(hb, wb, 8, 8)          # block row, block, row, column
    if n == 1:
        v = _ds(d[:, :, 0, 0], 3)
        return np.clip(v + 128, 0, 255).astype(np.uint8)
    one, (s1, s2) = {4: pass4, 2: pass2}[n], SHIFTS[n]
    p1 = one(d.transpose(0, 1, 3, 2), s1)                                 # (hb, wb, column, n rows)
    ws = np.clip(p1, -32768, 32767).transpose(0, 1, 3, 2)                 # (hb, wb, n rows, 8 columns)
    p2 = one(ws, s2)                                                      # (hb, wb, n rows, n columns)
    if trace is not None:
        trace["saturated"] = trace.get("saturated", 0) + int((ws != p1.transpose(0, 1, 3, 2)).sum())
    return np.clip(p2 + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(n * hb, n * wb)


def jpegds_ref(p, w, h, layout, s, trace=None):
    """The three ceil(w / s) x ceil(h / s) planes, packed (ycc_ref's YCC_444 input), of the payload
    of one w x h file decoded at 1/s, or (n, bytes) of an (n, bytes) batch."""
    assert s in (2, 4, 8)
    p = np.asarray(p, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([jpegds_ref(q, w, h, layout, s, trace) for q in p])
    tables, comps = split_payload(p, w, h, layout)
    ow, oh = out_size(w, h, s)
    planes = []
    for k, (c, n) in enumerate(zip(comps, idct_sizes(layout, s))):
        plane = idct_blocks_scaled(c, tables[k], n, trace)[:oh, :ow]
        assert plane.shape == (oh, ow), (plane.shape, ow, oh)
        planes.append(plane.ravel())
    return np.concatenate(planes)
