"""The reference of restart intervals in the entropy-coded JPEG input (MIPX_OP_JPEGH, the uint32
`restart` at offset 4 of the slot; include/mipx.h): the slot builders, the files of the tests, and
the model of the device's decoder on such slots.

Write Ri for the header word, M for the scan's MCUs and K = ceil(M / Ri).  Ri = 0, or Ri <= 65535
with K < 2, is the ordinary scan of tests/jpegh_ref.py, statuses included; Ri > 65535 is BAD.
Otherwise the scan's `length` bytes are K entropy-coded intervals with K - 1 markers between them,
marker k = FF D0 + (k & 7), interval k the MCUs k Ri ... min((k + 1) Ri, M) - 1, decoded from a byte
boundary with the DC predictors 0 by the rules of jpegh_ref.Stream.run.  BAD: what is BAD in an
ordinary slot for its header, an FF that neither 00 nor D0..D7 follows (the last byte included),
another number of markers than K - 1, a marker with another number than its place's, a broken
rule of the decoder inside an interval's blocks, an interval that ends before its last block, a DC
of a real block outside int16.  Bits behind an interval's last block are ignored.  UNSYNCED does
not occur."""
import functools
import io

import numpy as np

import jpegh_ref
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes
from jpegh_ref import BAD, HEADER_BYTES, OK, TABLE_KEYS, ZIGZAG, scan_blocks

SIZES = [(17, 9), (9, 17), (33, 17), (37, 29), (197, 117)]


def mcus(w, h, layout):
    """(MCUs per row, MCU rows)."""
    s = 8 if layout == YCC_444 else 16
    return -(-w // s), -(-h // s)


def restart_of(slot):
    return int(np.ascontiguousarray(slot[4:8], np.uint8).view("<u4")[0])


def intervals(slot, w, h, layout):
    """K of the slot when it takes the restart path, else 0."""
    ri, (mw, mh) = restart_of(slot), mcus(w, h, layout)
    return -(-mw * mh // ri) if 1 <= ri <= 65535 and ri < mw * mh else 0


# ---- the slot ---------------------------------------------------------------------------------
def build_slot(w, h, layout, scan, qtables, selectors, tables, length=None, restart=0):
    """jpegh_ref.build_slot with the restart interval at offset 4; scan: the bytes between the SOS
    segment and FF D9 as the file has them, markers included."""
    slot = jpegh_ref.build_slot(w, h, layout, scan, qtables, selectors, tables, length)
    slot[4:8] = np.array([restart], "<u4").view(np.uint8)
    return slot


def file_scan(buf):
    """The bytes between the SOS segment and the first marker that is no restart marker."""
    p = 2
    while buf[p + 1] != 0xDA:
        p += 2 + int.from_bytes(buf[p + 2:p + 4], "big")
    p += 2 + int.from_bytes(buf[p + 2:p + 4], "big")
    end = p
    while not (buf[end] == 0xFF and buf[end + 1] != 0x00 and not 0xD0 <= buf[end + 1] <= 0xD7):
        end += 1
    return p, end


def file_slot(buf, layout):
    """The slot of a Pillow-written file by a marker walk of the tests' own (jpegh_ref.file_tables),
    with the file's DRI at offset 4."""
    w, h, _, qt, sel, dht, dri, _ = jpegh_ref.file_tables(buf)
    p, end = file_scan(buf)
    return build_slot(w, h, layout, bytes(buf[p:end]), qt, sel, dht, restart=dri)


def with_scan(slot, w, h, layout, scan, **kw):
    """The slot with another scan (and header words by kw: length, restart)."""
    _, q, sel, tables = jpegh_ref.parse_slot(slot)
    tabs = {key: (tables[i][0], tables[i][1]) for i, key in enumerate(TABLE_KEYS)}
    kw.setdefault("restart", restart_of(slot))
    return build_slot(w, h, layout, scan, q, sel, tabs, **kw)


def slot_scan(slot):
    length = int(np.ascontiguousarray(slot[:4], np.uint8).view("<u4")[0])
    return slot[HEADER_BYTES:HEADER_BYTES + length].tobytes()


# ---- the model ------------------------------------------------------------------------------------
def split(scan):
    """The scan cut at its restart markers: (the stuffed intervals, the markers' second bytes), or
    None for an FF that neither 00 nor D0..D7 follows."""
    parts, marks, at, i, n = [], [], 0, 0, len(scan)
    while i < n:
        if scan[i] != 0xFF:
            i += 1
            continue
        if i + 1 >= n:
            return None
        nxt = scan[i + 1]
        if 0xD0 <= nxt <= 0xD7:
            parts.append(scan[at:i])
            marks.append(nxt)
            at = i + 2
        elif nxt != 0x00:
            return None
        i += 2
    parts.append(scan[at:])
    return parts, marks


def decode_slot(slot, w, h, layout):
    """(status, payload) as jpegh_ref.decode_slot: the status the device gives the slot, and for OK
    the payload of MIPX_OP_JPEGD it must write."""
    slot = np.ascontiguousarray(slot, np.uint8).ravel()
    ri = restart_of(slot)
    if ri > 65535:
        return BAD, None
    count = intervals(slot, w, h, layout)
    if count < 2:
        return jpegh_ref.decode_slot(slot, w, h, layout)
    cap = jpegc_bytes(w, h, layout)
    assert slot.size == HEADER_BYTES + cap
    length, _, selectors, tables = jpegh_ref.parse_slot(slot)
    if length > cap or any(v > 1 for v in selectors):
        return BAD, None
    luts = [jpegh_ref.lookup16(c, sy) for c, sy in tables]
    cut = split(slot[HEADER_BYTES:HEADER_BYTES + length].tobytes())
    if cut is None or any(t is None for t in luts):
        return BAD, None
    parts, marks = cut
    if len(marks) != count - 1 or any(m != 0xD0 + (k & 7) for k, m in enumerate(marks)):
        return BAD, None
    blocks = scan_blocks(w, h, layout)
    per_mcu = 3 if layout == YCC_444 else 6
    place = jpegh_ref.block_place(w, h, layout)
    sizes = [max(i for c, i in place if c == comp) + 1 for comp in range(3)]
    coefs = [np.zeros((n, 64), np.int64) for n in sizes]

    def put(cur, k, val):
        comp, i = place[cur]
        if i >= 0:
            coefs[comp][i, ZIGZAG[k]] = val

    for k, part in enumerate(parts):
        data, marker = jpegh_ref.unstuff(part)
        assert not marker
        first, last = k * ri * per_mcu, min((k + 1) * ri * per_mcu, blocks)
        s = jpegh_ref.Stream(data, luts, selectors, layout, last)
        dcdiff = [0] * last
        _, _, _, done, bad = s.run(0, 0, 0, s.total, first, dcdiff, put)
        if bad or done < last - first:
            return BAD, None
        pred = [0, 0, 0]
        for cur in range(first, last):
            comp, i = place[cur]
            pred[comp] += dcdiff[cur]
            if i >= 0:
                if not -32768 <= pred[comp] <= 32767:
                    return BAD, None
                coefs[comp][i, 0] = pred[comp]
    body = np.concatenate([c.astype("<i2").ravel() for c in coefs]).view(np.uint8)
    return OK, np.concatenate([slot[16:400], body])


# ---- inputs -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pixels(w, h, n=3):
    """The noise of tests/test_jpegh_gpu.py."""
    px = np.random.default_rng(w * 100003 + h * 101 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    px.setflags(write=False)
    return px


def pillow_jpeg(px, layout, quality, optimize=False, **restart):
    """The file Pillow (libjpeg-turbo) writes, with restart_marker_blocks= or restart_marker_rows=."""
    from PIL import Image, ImageFile
    prev, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 22
    try:
        b = io.BytesIO()
        Image.fromarray(px).save(b, "JPEG", quality=quality, subsampling=0 if layout == YCC_444 else 2, optimize=optimize,
                                 **restart)
        return b.getvalue()
    finally:
        ImageFile.MAXBLOCK = prev


@functools.lru_cache(maxsize=None)
def restart_file(w, h, layout, quality, optimize, blocks=0, rows=0, i=0):
    """(file, slot by the tests' own marker walk, the host decoder's payload) of image i of
    pixels(w, h), saved with a restart interval of `blocks` MCUs or `rows` MCU rows; read-only."""
    from imaginary_amd import codec
    kw = dict(restart_marker_rows=rows) if rows else dict(restart_marker_blocks=blocks) if blocks else {}
    buf = pillow_jpeg(pixels(w, h)[i], layout, quality, optimize, **kw)
    slot = file_slot(buf, layout)
    payload, l2 = codec.decode_jpeg_coefs(buf)
    assert l2 == layout and slot.size == jpegh_ref.jpegh_bytes(w, h, layout) and payload.size == jpegh_ref.jpegd_bytes(w, h, layout)
    slot.setflags(write=False), payload.setflags(write=False)
    return buf, slot, payload


def damaged(slot, w, h, layout):
    """{name: slot}: the damage table of the restart path, made of an OK slot with K >= 4 whose
    first interval is longer than 3 bytes."""
    scan, ri = slot_scan(slot), restart_of(slot)
    parts, marks = split(scan)
    assert len(marks) >= 3 and len(parts[0]) > 3 and len(parts[1]) > 0
    at = [0]
    for p in parts[:-1]:
        at.append(at[-1] + len(p) + 2)      # at[k]: the first byte of interval k; its marker two bytes before

    def ws(s, **kw):
        return with_scan(slot, w, h, layout, s, **kw)

    m1 = at[2] - 2                          # marker 1
    out = {"marker 1 with the next number": ws(scan[:m1 + 1] + bytes([0xD0 + ((marks[1] - 0xD0 + 1) & 7)]) + scan[m1 + 2:]),
           "marker 1 removed": ws(scan[:m1] + scan[m1 + 2:]),
           "marker 1 twice": ws(scan[:m1] + scan[m1:m1 + 2] + scan[m1:]),
           "FF D8 inside": ws(scan[:at[1] + 1] + b"\xff\xd8" + scan[at[1] + 1:]),
           "FF last": ws(scan + b"\xff"),
           "Ri one more": ws(scan, restart=ri + 1),
           "Ri one less": ws(scan, restart=ri - 1) if ri > 1 else None,
           "Ri 65536": ws(scan, restart=65536),
           "marker 0 three bytes early": ws(scan[:at[1] - 5] + scan[at[1] - 2:at[1]] + scan[at[1] - 5:at[1] - 2] + scan[at[1]:])}
    return {k: v for k, v in out.items() if v is not None}


def as_file(buf, slot):
    """The file `buf` with the slot's scan and restart interval in the place of its own."""
    p, end = file_scan(buf)
    out = bytearray(buf[:p] + slot_scan(slot) + buf[end:])
    q = 2
    while out[q + 1] != 0xDA:
        if out[q + 1] == 0xDD:
            out[q + 4:q + 6] = (restart_of(slot) & 0xFFFF).to_bytes(2, "big")
        q += 2 + int.from_bytes(out[q + 2:q + 4], "big")
    return bytes(out)
