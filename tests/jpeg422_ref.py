"""Plain numpy restatement of what libjpeg does with a 4:2:2 (h2v1) file, the reference for the
engine's MIPX_YCC_422 input layout (PARITY_ASSUMPTIONS.md row 25).  Not part of the oracle.  Built
on the other restatements' primitives (ycc_ref's conversion, jpegd_ref / jpegds_ref's inverse DCTs,
jpegh_ref's decoder model), none of which it changes.

  geometry: Y is h x w; Cb and Cr are h x cw, cw = ceil(w / 2).  In blocks Y is ceil(w / 8) x
      ceil(h / 8), chroma ceil(cw / 8) x ceil(h / 8).  The MCU is 16 x 8 pixels, four blocks in
      scan order Y left, Y right, Cb, Cr; there are ceil(w / 16) x ceil(h / 8) MCUs.
  upsample (jdsample.c h2v1_fancy_upsample, chosen when cw > 2), cx = x >> 1, no vertical term:
      even x: c = (3 C[cx] + C[max(cx - 1, 0)] + 1) >> 2
      odd x:  c = (3 C[cx] + C[min(cx + 1, cw - 1)] + 2) >> 2
      cw <= 2, or fancy upsampling off: c = C[cx]
  shrink-on-load (jdmaster.c): at 1 / s every component takes the N = 8 / s inverse DCT (chroma's
      vertical ratio is 1, so its IDCT is not enlarged); chroma comes out ceil(h / s) high and
      ceil(w / (2 s)) = ceil(ceil(w / s) / 2) wide, the 4:2:2 planes of the decoded size, and is
      upsampled by the rule above; at 1 / 8 libjpeg turns fancy upsampling off.
"""
from __future__ import annotations

import numpy as np

import jpegh_ref
import ycc_ref
from jpegds_ref import idct_blocks_scaled

YCC_422 = 3
HEADER_BYTES = 384          # MIPX_JPEGD_HEADER_BYTES
SLOT_HEADER_BYTES = 1504    # MIPX_JPEGH_HEADER_BYTES


# ---- geometry ---------------------------------------------------------------------------------
def chroma_size(w, h):
    return (w + 1) // 2, h


def ycc_bytes(w, h):
    return w * h + 2 * ((w + 1) // 2) * h


def block_grid(w, h):
    """(ywb, yhb, cwb, chb): real blocks across and down of Y and of a chroma component."""
    return (w + 7) // 8, (h + 7) // 8, ((w + 1) // 2 + 7) // 8, (h + 7) // 8


def mcus(w, h):
    return (w + 15) // 16, (h + 7) // 8


def scan_blocks(w, h):
    mw, mh = mcus(w, h)
    return 4 * mw * mh


def jpegc_bytes(w, h):
    ywb, yhb, cwb, chb = block_grid(w, h)
    return 128 * (ywb * yhb + 2 * cwb * chb)


def jpegd_bytes(w, h):
    return HEADER_BYTES + jpegc_bytes(w, h)


def jpegh_bytes(w, h):
    return SLOT_HEADER_BYTES + jpegc_bytes(w, h)


def workspace_bytes(n, w, h):
    """jpegh_ref.workspace_bytes with `blocks` the most of the three input layouts."""
    def up(v):
        return (v + 255) // 256 * 256
    old = max(jpegh_ref.scan_blocks(w, h, ycc_ref.YCC_444), jpegh_ref.scan_blocks(w, h, ycc_ref.YCC_420))
    new = max(old, scan_blocks(w, h))
    tiles = lambda b: -(-b // jpegh_ref.SEQ)   # noqa: E731
    return (jpegh_ref.workspace_bytes(n, w, h) + up(4 * n * new) - up(4 * n * old)
            + up(12 * n * tiles(new)) - up(12 * n * tiles(old)) + up(24 * n * tiles(new)) - up(24 * n * tiles(old)))


# ---- planes to RGB ----------------------------------------------------------------------------
def split(planes, w, h):
    """(Y, Cb, Cr) views of one image's packed planes."""
    cw = (w + 1) // 2
    p = np.asarray(planes, dtype=np.uint8).ravel()
    assert p.size == ycc_bytes(w, h), (p.size, w, h)
    return p[:w * h].reshape(h, w), p[w * h:w * h + cw * h].reshape(h, cw), p[w * h + cw * h:].reshape(h, cw)


def upsample_422(c, w, fancy=True):
    """One h x cw chroma plane at h x w, as int32."""
    _, cw = c.shape
    c = c.astype(np.int32)
    xs = np.arange(w)
    cx = xs >> 1
    if cw <= 2 or not fancy:   # libjpeg picks the fancy upsampler only for downsampled_width > 2
        return c[:, cx]
    nx = np.clip(np.where(xs % 2 == 0, cx - 1, cx + 1), 0, cw - 1)
    return (3 * c[:, cx] + c[:, nx] + np.where(xs % 2 == 0, 1, 2)) >> 2


def ycc422_ref(planes, w, h, fancy=True):
    """(h, w, 3) RGB of one image's packed 4:2:2 planes, or (n, h, w, 3) of an (n, bytes) batch."""
    p = np.asarray(planes, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([ycc422_ref(q, w, h, fancy) for q in p])
    y, cb, cr = split(p, w, h)
    full = np.concatenate([y.ravel(), upsample_422(cb, w, fancy).astype(np.uint8).ravel(),
                           upsample_422(cr, w, fancy).astype(np.uint8).ravel()])
    return ycc_ref.ycc_ref(full, w, h, ycc_ref.YCC_444)   # jdcolor.c's conversion, unchanged


# ---- coefficients to planes and RGB -----------------------------------------------------------
def split_payload(p, w, h):
    """(tables (3, 64) int64, [Y, Cb, Cr] coefficients as (hb, wb, 64) int64) of one payload."""
    p = np.ascontiguousarray(p, dtype=np.uint8).ravel()
    assert p.size == jpegd_bytes(w, h), (p.size, w, h)
    tables = p[:HEADER_BYTES].view("<u2").reshape(3, 64).astype(np.int64)
    c = p[HEADER_BYTES:].view("<i2").astype(np.int64)
    ywb, yhb, cwb, chb = block_grid(w, h)
    out, at = [], 0
    for wb, hb in ((ywb, yhb), (cwb, chb), (cwb, chb)):
        out.append(c[at:at + 64 * wb * hb].reshape(hb, wb, 64))
        at += 64 * wb * hb
    return tables, out


def payload(tables, comps):
    """The payload of (3, 64) tables and the three components' (hb, wb, 64) coefficients."""
    head = np.asarray(tables, "<u2").reshape(192).view(np.uint8)
    return np.concatenate([head] + [np.ascontiguousarray(c, dtype="<i2").ravel().view(np.uint8) for c in comps])


def planes_ref(p, w, h, s=1, trace=None):
    """The packed 4:2:2 planes of the decoded size, ceil(w / s) x ceil(h / s), of one payload."""
    assert s in (1, 2, 4, 8)
    tables, comps = split_payload(p, w, h)
    ow, oh = -(-w // s), -(-h // s)
    sizes = [(ow, oh), ((ow + 1) // 2, oh), ((ow + 1) // 2, oh)]
    out = []
    for k, c in enumerate(comps):
        plane = idct_blocks_scaled(c, tables[k], 8 // s, trace)[:sizes[k][1], :sizes[k][0]]
        assert plane.shape == (sizes[k][1], sizes[k][0]), (plane.shape, sizes[k])
        out.append(plane.ravel())
    return np.concatenate(out)


def jpegd422_ref(p, w, h, s=1, trace=None):
    """(ceil(h / s), ceil(w / s), 3) RGB of one payload decoded at 1 / s, or the batch of an (n, bytes) one."""
    p = np.asarray(p, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([jpegd422_ref(q, w, h, s, trace) for q in p])
    return ycc422_ref(planes_ref(p, w, h, s, trace), -(-w // s), -(-h // s), fancy=s != 8)


# ---- the scan ---------------------------------------------------------------------------------
def block_place(w, h):
    """Per block of the scan (component, index among the component's real blocks in raster order,
    or -1 for a dummy block): jpegh_ref.block_place for the 4-block MCU."""
    ywb = (w + 7) // 8
    mw, mh = mcus(w, h)
    out = []
    for my in range(mh):
        for mx in range(mw):
            for j in range(2):
                bx = 2 * mx + j
                out.append((0, my * ywb + bx if bx < ywb else -1))
            out += [(1, my * mw + mx), (2, my * mw + mx)]
    return out


def payload_from_blocks(tables, scan_coefs, w, h):
    """The payload of a scan's blocks in scan order, (scan_blocks, 64) natural order, by block_place."""
    ywb, yhb, cwb, chb = block_grid(w, h)
    comps = [np.zeros((yhb * ywb, 64), np.int64), np.zeros((chb * cwb, 64), np.int64), np.zeros((chb * cwb, 64), np.int64)]
    for cur, (comp, i) in enumerate(block_place(w, h)):
        if i >= 0:
            comps[comp][i] = scan_coefs[cur]
    return payload(tables, comps)


class Stream422(jpegh_ref.Stream):
    """jpegh_ref's decoder model with the states of a 4-block MCU."""

    def __init__(self, data, luts, selectors, blocks):
        super().__init__(data, luts, selectors, ycc_ref.YCC_444, blocks)
        self.per_mcu = 4
        comp = [0, 0, 1, 2]
        self.dc = [luts[selectors[c]] for c in comp]
        self.ac = [luts[2 + selectors[3 + c]] for c in comp]


def scan_coefs(slot, w, h):
    """The blocks of an ordinary (no restart interval) 4:2:2 slot's scan in scan order, (scan_blocks, 64)
    int64 in natural order with the DC prediction undone, by one walk of the model; None when a rule breaks."""
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    length, _, selectors, tables = jpegh_ref.parse_slot(slot)
    data, marker = jpegh_ref.unstuff(slot[SLOT_HEADER_BYTES:SLOT_HEADER_BYTES + length].tobytes())
    luts = [jpegh_ref.lookup16(c, sy) for c, sy in tables]
    if marker or any(t is None for t in luts):
        return None
    blocks = scan_blocks(w, h)
    s = Stream422(data, luts, selectors, blocks)
    out = np.zeros((blocks, 64), np.int64)
    dcdiff = [0] * blocks

    def put(cur, k, val):
        out[cur, jpegh_ref.ZIGZAG[k]] = val

    _, _, _, done, bad = s.run(0, 0, 0, s.total, 0, dcdiff, put)
    if bad or done < blocks:
        return None
    pred = [0, 0, 0]
    for cur, (comp, _) in enumerate(block_place(w, h)):
        pred[comp] += dcdiff[cur]
        out[cur, 0] = pred[comp]
    return out


# ---- inputs -----------------------------------------------------------------------------------
def pillow_jpeg(px, quality, optimize=False, **kw):
    """The 4:2:2 file Pillow (libjpeg-turbo) writes; kw: restart_marker_blocks=, restart_marker_rows=, progressive=."""
    import io
    from PIL import Image, ImageFile
    prev, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 22
    try:
        b = io.BytesIO()
        Image.fromarray(px).save(b, "JPEG", quality=quality, subsampling=1, optimize=optimize, **kw)
        return b.getvalue()
    finally:
        ImageFile.MAXBLOCK = prev


def noise(w, h, seed=0):
    return np.random.default_rng(422000 + 1009 * w + h + 7 * seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(w + h - 2, 1)],
                    axis=-1).astype(np.uint8)


def synchronised(slot, w, h):
    """Whether the device's launches agree on every sequence's exit state of an ordinary 4:2:2 slot's
    scan (jpegh_ref.synchronised on the 4-block model); also the unstuffed scan's length."""
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    length, _, selectors, tables = jpegh_ref.parse_slot(slot)
    data, marker = jpegh_ref.unstuff(slot[SLOT_HEADER_BYTES:SLOT_HEADER_BYTES + length].tobytes())
    assert not marker
    luts = [jpegh_ref.lookup16(c, sy) for c, sy in tables]
    return jpegh_ref.synchronised(Stream422(data, luts, selectors, scan_blocks(w, h))), len(data)
