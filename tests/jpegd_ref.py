"""The JPEG decoder's middle in numpy (PARITY_ASSUMPTIONS.md row 18): a file's quantisation
tables and quantised DCT coefficients in, the packed sample planes of tests/ycc_ref.py out, as
libjpeg computes them with its default settings (jddctmgr.c, jidctint.c jpeg_idct_islow:
CONST_BITS 13, PASS1_BITS 2), made total so that every input has a defined result.
tests/test_jpegd_cpu.py pins it to libjpeg-turbo inside Pillow on files an encoder wrote; the
GPU tests hold the kernel to it on every input.  Not part of the oracle.

  dequantise: d = int16(coef * q), the low 16 bits as a signed value
  one 8-point pass with descale shift S: sums are int32 and wrap modulo 2^32 (computed here in
      int64 and reduced to signed 32 bits before the shift), the shift is arithmetic
  pass 1 down the columns, S = 11, saturated to int16; pass 2 along the rows, S = 18
  sample = clamp(v + 128, 0, 255)

One image's payload is 384 bytes of tables (Y, Cb, Cr: 64 little-endian uint16 each, natural
order) and then the int16 coefficients in tests/jpegc_ref.py's layout."""
import numpy as np

from jpegc_ref import YCC_420, YCC_444, geometry, jpegc_bytes  # noqa: F401
from ycc_ref import chroma_size

HEADER_BYTES = 384


def jpegd_bytes(w, h, layout):
    return HEADER_BYTES + jpegc_bytes(w, h, layout)


def payload(coefs, tables):
    """One image's payload, uint8, from its int16 coefficients and 1 (all components), 2 (Y,
    chroma) or 3 tables of 64 values in natural order."""
    t = [np.asarray(q).ravel() for q in tables]
    t = {1: [t[0]] * 3, 2: [t[0], t[-1], t[-1]], 3: t}[len(t)]
    assert all(q.size == 64 for q in t)
    head = np.concatenate(t).astype("<u2").view(np.uint8)
    return np.concatenate([head, np.ascontiguousarray(coefs, dtype="<i2").ravel().view(np.uint8)])


def split_payload(p, w, h, layout):
    """(tables (3, 64) int64, [coefficients (hb, wb, 64) int64 per component])."""
    p = np.ascontiguousarray(p, dtype=np.uint8).ravel()
    assert p.size == jpegd_bytes(w, h, layout), (p.size, w, h, layout)
    tables = p[:HEADER_BYTES].view("<u2").astype(np.int64).reshape(3, 64)
    c = p[HEADER_BYTES:].view("<i2").astype(np.int64)
    out, at = [], 0
    for wb, hb in geometry(w, h, layout):
        out.append(c[at:at + 64 * wb * hb].reshape(hb, wb, 64))
        at += 64 * wb * hb
    return tables, out


def wrap32(v):
    """int64 -> the signed value of its low 32 bits."""
    return ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31


def wrap16(v):
    return ((v + 2 ** 15) & 0xFFFF) - 2 ** 15


def idct_pass(d, shift):
    """One 8-point pass of jidctint.c over the last axis of an int64 array."""
    i = [d[..., k] for k in range(8)]
    z1 = (i[2] + i[6]) * 4433
    t2, t3 = z1 - i[6] * 15137, z1 + i[2] * 6270
    t0, t1 = (i[0] + i[4]) << 13, (i[0] - i[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    a0, a1, a2, a3 = i[7], i[5], i[3], i[1]
    z1, z2, z3, z4 = a0 + a3, a1 + a2, a0 + a2, a1 + a3
    z5 = (z3 + z4) * 9633
    a0, a1, a2, a3 = a0 * 2446, a1 * 16819, a2 * 25172, a3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    a0, a1, a2, a3 = a0 + z1 + z3, a1 + z2 + z4, a2 + z2 + z3, a3 + z1 + z4
    out = [t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3]
    return np.stack([wrap32(wrap32(v) + (1 << (shift - 1))) >> shift for v in out], axis=-1)


def idct_blocks(coefs, q, trace=None):
    """(hb, wb, 64) quantised coefficients and a 64-entry table -> (8 hb, 8 wb) uint8 samples.
    trace: a dict that receives what the total rule did ('saturated': pass-1 results outside
    int16, 'pass2': the extreme pass-2 results before the + 128)."""
    hb, wb, _ = coefs.shape
    d = wrap16(coefs * q.reshape(1, 1, 64)).reshape(hb, wb, 8, 8)          # block row, block, row, column
    p1 = idct_pass(d.transpose(0, 1, 3, 2), 11).transpose(0, 1, 3, 2)      # down the columns
    ws = np.clip(p1, -32768, 32767)
    p2 = idct_pass(ws, 18)                                                # along the rows
    if trace is not None:
        trace["saturated"] = trace.get("saturated", 0) + int((ws != p1).sum())
        trace["pass2"] = (min(trace.get("pass2", (0, 0))[0], int(p2.min())),
                          max(trace.get("pass2", (0, 0))[1], int(p2.max())))
    return np.clip(p2 + 128, 0, 255).astype(np.uint8).transpose(0, 2, 1, 3).reshape(8 * hb, 8 * wb)


def jpegd_ref(p, w, h, layout, trace=None):
    """The packed planes (ycc_ref's input) of one payload, or (n, bytes) of an (n, bytes) batch."""
    p = np.asarray(p, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([jpegd_ref(q, w, h, layout, trace) for q in p])
    tables, comps = split_payload(p, w, h, layout)
    cw, ch = chroma_size(w, h, layout)
    sizes = [(w, h), (cw, ch), (cw, ch)]
    return np.concatenate([idct_blocks(c, tables[k], trace)[:sizes[k][1], :sizes[k][0]].ravel()
                           for k, c in enumerate(comps)])
