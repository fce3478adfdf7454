"""Plain numpy restatement of what libjpeg does with a one-component (JCS_GRAYSCALE) file, the
reference for the engine's MIPX_YCC_GREY layout (PARITY_ASSUMPTIONS.md row 26).  Not part of the
oracle.  It is the other restatements restricted to their first component: jpegd_ref / jpegds_ref's
inverse DCTs, jpegc_ref's forward DCT and quantisation, jpegh_ref's model of the entropy decoder
(the host writers in codec.py stand for the entropy coder, pinned to Pillow's files).  None of them
is changed.

  geometry: one plane, h x w; ceil(w / 8) x ceil(h / 8) blocks.  The scan is not interleaved: an MCU
      is one block, the blocks go in raster order, there are no dummy blocks.
  decode: dequantise with the file's one table, the N = 8 / s point inverse DCT at scale 1 / s; the
      plane, cropped to ceil(w / s) x ceil(h / s), is the 1-band image.  No upsampling, no conversion.
  encode: sample - 128 with the last column, then the last row repeated to whole blocks, the forward
      DCT, the luminance table of jpeg_set_quality(quality, TRUE).
"""
from __future__ import annotations

import io

import numpy as np

from jpegc_ref import _blocks, _pad, qtables
from jpegds_ref import idct_blocks_scaled

YCC_GREY = 6
HEADER_BYTES = 384          # MIPX_JPEGD_HEADER_BYTES: the size stays, only the first 128 bytes are read


# ---- geometry ---------------------------------------------------------------------------------
def block_grid(w, h):
    return (w + 7) // 8, (h + 7) // 8


def jpegc_bytes(w, h):
    wb, hb = block_grid(w, h)
    return 128 * wb * hb


def jpegd_bytes(w, h):
    return HEADER_BYTES + jpegc_bytes(w, h)


def out_size(w, h, s):
    return -(-w // s), -(-h // s)


def planes(w, h, s):
    """What JpegGeom(w, h, GREY).planes(s) says: (n0, n1, w0, h0, w1, h1, off0, off1, off2, bytes)."""
    ow, oh = out_size(w, h, s)
    return (8 // s, 8 // s, ow, oh, 0, 0, 0, ow * oh, ow * oh, ow * oh)


def geom(w, h):
    """The fields of JpegGeom(w, h, GREY) by the one-component sampling rule, in the order
    tests/c/jpeg_geom_grey_host.cpp prints them."""
    wb, hb = block_grid(w, h)
    return (1, 1, w, h, wb, hb, 0, 0, 0, 0, 0, 128 * wb * hb, 128 * wb * hb, 0, w * h, w * h, 128 * wb * hb, w * h,
            wb, hb, 1, wb * hb)


# ---- payloads ---------------------------------------------------------------------------------
def payload(coefs, table):
    """One image's payload, uint8: the table, zeros up to 384 bytes, the int16 coefficients."""
    head = np.zeros(HEADER_BYTES // 2, "<u2")
    head[:64] = np.asarray(table).ravel()
    return np.concatenate([head.view(np.uint8), np.ascontiguousarray(coefs, dtype="<i2").ravel().view(np.uint8)])


def split_payload(p, w, h):
    """(table (64,) int64, coefficients (hb, wb, 64) int64); what stands behind the table is not read."""
    p = np.ascontiguousarray(p, dtype=np.uint8).ravel()
    assert p.size == jpegd_bytes(w, h), (p.size, w, h)
    wb, hb = block_grid(w, h)
    return p[:128].view("<u2").astype(np.int64), p[HEADER_BYTES:].view("<i2").astype(np.int64).reshape(hb, wb, 64)


# ---- decode -----------------------------------------------------------------------------------
def jpegd_grey_ref(p, w, h, s=1, trace=None):
    """The (ceil(h / s), ceil(w / s), 1) image of one payload at 1 / s, or (n, ...) of an (n, bytes) batch."""
    assert s in (1, 2, 4, 8)
    p = np.asarray(p, dtype=np.uint8)
    if p.ndim == 2:
        return np.stack([jpegd_grey_ref(q, w, h, s, trace) for q in p])
    table, coefs = split_payload(p, w, h)
    ow, oh = out_size(w, h, s)
    plane = idct_blocks_scaled(coefs, table, 8 // s, trace)[:oh, :ow]
    assert plane.shape == (oh, ow)
    return np.ascontiguousarray(plane[:, :, None])


# ---- encode -----------------------------------------------------------------------------------
def jpegc_grey_ref(px, quality):
    """px (h, w), (h, w, 1) or (n, h, w, 1) uint8 -> (n, jpegc_bytes / 2) int16."""
    px = np.asarray(px, dtype=np.uint8)
    if px.ndim == 2:
        px = px[None, :, :, None]
    elif px.ndim == 3:
        px = px[None]
    n, h, w, b = px.shape
    assert b == 1
    lum, _ = qtables(quality)
    wb, hb = block_grid(w, h)
    out = []
    for img in px[..., 0].astype(np.int64):
        coefs = _blocks(_pad(img, 8 * hb, 8 * wb), lum).ravel()
        assert np.abs(coefs).max(initial=0) < 32768
        out.append(coefs.astype(np.int16))
    return np.stack(out)


# ---- test images ------------------------------------------------------------------------------
def noise(w, h, seed=0):
    return np.random.default_rng(6000 + 131 * w + 7 * h + seed).integers(0, 256, (h, w, 1), dtype=np.uint8)


def smooth(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x * 3 + y * 5) * 255) // max(3 * (w - 1) + 5 * (h - 1), 1)).astype(np.uint8)[:, :, None]


def pillow_jpeg(px, quality, optimize=False, **kw):
    """The file Pillow's libjpeg writes of a 1-band image (mode "L": JCS_GRAYSCALE)."""
    from PIL import Image
    b = io.BytesIO()
    Image.fromarray(np.asarray(px)[:, :, 0] if np.asarray(px).ndim == 3 else px, "L").save(
        b, "JPEG", quality=quality, optimize=optimize, **kw)
    return b.getvalue()


# ---- the scan -----------------------------------------------------------------------------------
# jpegh_ref's decoder model restricted to one component: an MCU is one block, the DC and AC tables
# are the ones bytes 400 and 403 of the slot name, one DC predictor, no dummy blocks; a restart
# interval counts blocks, and interval k starts behind marker FF D0 + (k & 7) with the predictor 0.
SLOT_HEADER_BYTES = 1504    # MIPX_JPEGH_HEADER_BYTES
OK, UNSYNCED, BAD = 0, 1, 2


def jpegh_bytes(w, h):
    return SLOT_HEADER_BYTES + jpegc_bytes(w, h)


def scan_blocks(w, h):
    wb, hb = block_grid(w, h)
    return wb * hb


def _one_component(data, luts, selectors, blocks):
    import jpegh_ref
    s = jpegh_ref.Stream(data, luts, [selectors[0]] * 3 + [selectors[3]] * 3, 0, blocks)   # Y's alone are read
    s.per_mcu, s.dc, s.ac = 1, [luts[selectors[0]]], [luts[2 + selectors[3]]]
    return s


def decode_slot(slot, w, h):
    """(status, payload): the status the device gives a grey slot, and for OK the payload of
    MIPX_OP_JPEGD (uint8, jpegd_bytes) it must write; None otherwise."""
    import re

    import jpegh_ref
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    cap, blocks = jpegc_bytes(w, h), scan_blocks(w, h)
    assert slot.size == SLOT_HEADER_BYTES + cap
    length, _, selectors, tables = jpegh_ref.parse_slot(slot)
    ri = int(slot[4:8].view("<u4")[0])
    if length > cap or selectors[0] > 1 or selectors[3] > 1 or ri > 65535:     # the other four are ignored
        return BAD, None
    luts = [jpegh_ref.lookup16(c, sy) for c, sy in tables]
    if any(t is None for t in luts):
        return BAD, None
    scan = slot[SLOT_HEADER_BYTES:SLOT_HEADER_BYTES + length].tobytes()
    restart = 1 <= ri < blocks
    if restart:                                       # the markers cut the scan; each carries its number
        parts, at = [], 0
        for k, hit in enumerate(re.finditer(rb"\xff[^\x00]", scan + b"\xff\xff")):
            if hit.start() >= len(scan):
                break
            if hit.group()[1] != 0xD0 + (k & 7):
                return BAD, None
            parts.append(scan[at:hit.start()])
            at = hit.start() + 2
        parts.append(scan[at:])
        if len(parts) != -(-blocks // ri):
            return BAD, None
    else:
        parts, ri = [scan], blocks
    coefs = np.zeros((blocks, 64), np.int64)
    for k, part in enumerate(parts):
        data, marker = jpegh_ref.unstuff(part)
        if marker:
            return BAD, None
        first, count = k * ri, min(ri, blocks - k * ri)
        s = _one_component(data, luts, selectors, count)
        if not restart and not jpegh_ref.synchronised(s):
            return UNSYNCED, None
        dcdiff = [0] * count

        def put(cur, kk, val):
            coefs[first + cur, jpegh_ref.ZIGZAG[kk]] = val

        _, _, _, done, bad = s.run(0, 0, 0, s.total, 0, dcdiff, put)
        if bad or done < count:
            return BAD, None
        pred = 0
        for cur in range(count):
            pred += dcdiff[cur]
            if not -32768 <= pred <= 32767:
                return BAD, None
            coefs[first + cur, 0] = pred
    return OK, np.concatenate([slot[16:400], coefs.astype("<i2").ravel().view(np.uint8)])
