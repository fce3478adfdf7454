"""Host codec boundary: encoded bytes <-> decoded pixels.

The north star keeps decode/encode on the host (libvips in the Go service);
the engine only sees decoded pixels.  libvips is not installed in this image,
so this module is the host-side stand-in used by the byte-level operation
layer (imaginary.process_bytes) and its tests: Pillow decodes and encodes, and
JPEG shrink-on-load uses libjpeg's DCT-domain scaling (Pillow ``draft``), the
same mechanism libvips' jpegload ``shrink`` uses.  It never
touches pixels the engine computes — only the codec work either side of it.

Reference points: bimg.DetermineImageType / imaginary type.go:46-60 (MIME),
image.go:96-112 (encode fallback to JPEG for WEBP/HEIF/AVIF).
"""
from __future__ import annotations

import io
from dataclasses import dataclass
from typing import Optional

import numpy as np

try:
    from PIL import Image as _PIL
except ImportError:  # pragma: no cover - the codec is optional for the pixel engine
    _PIL = None

MIME = {"jpeg": "image/jpeg", "png": "image/png", "webp": "image/webp", "gif": "image/gif",
        "tiff": "image/tiff", "svg": "image/svg+xml", "pdf": "application/pdf", "heif": "image/heif",
        "avif": "image/avif"}
_PIL_FORMAT = {"jpeg": "JPEG", "png": "PNG", "webp": "WEBP", "gif": "GIF", "tiff": "TIFF"}
DEFAULT_QUALITY = 75  # bimg default Quality (libvips saver default Q)


class CodecError(Exception):
    pass


def sniff_type(buf: bytes) -> str:
    """bimg.DetermineImageType: magic bytes -> type name ("unknown" if none)."""
    b = bytes(buf[:16])
    if b[:3] == b"\xff\xd8\xff":
        return "jpeg"
    if b[:8] == b"\x89PNG\r\n\x1a\n":
        return "png"
    if b[:4] == b"RIFF" and b[8:12] == b"WEBP":
        return "webp"
    if b[:6] in (b"GIF87a", b"GIF89a"):
        return "gif"
    if b[:4] in (b"II*\x00", b"MM\x00*"):
        return "tiff"
    if b[:4] == b"%PDF":
        return "pdf"
    if b[4:8] == b"ftyp":
        return "avif" if b[8:12] in (b"avif", b"avis") else "heif"
    if b"<svg" in bytes(buf[:512]) or b[:5] == b"<?xml":
        return "svg"
    return "unknown"


def mime_type(t: str) -> str:
    """imaginary type.go GetImageMimeType."""
    return MIME.get(t, "application/octet-stream")


@dataclass
class Header:
    w: int
    h: int
    bands: int
    type: str
    orientation: int


_BANDS = {"L": 1, "LA": 2, "RGB": 3, "RGBA": 4}


def _open(buf: bytes):
    if _PIL is None:
        raise CodecError("no host codec (Pillow) available")
    try:
        return _PIL.open(io.BytesIO(buf))
    except Exception as e:  # noqa: BLE001 - any decoder failure is a bad request
        raise CodecError(f"cannot decode image: {e}") from e


def _target_mode(im) -> str:
    if im.mode in _BANDS:
        return im.mode
    if im.mode in ("P", "PA"):
        return "RGBA" if ("transparency" in im.info or im.mode == "PA") else "RGB"
    if im.mode in ("I;16", "I", "F", "1"):
        return "L"
    return "RGBA" if "A" in im.mode else "RGB"


def header(buf: bytes) -> Header:
    """What bimg reads before planning: size, bands, type, EXIF orientation."""
    im = _open(buf)
    orient = 0
    try:
        orient = int(im.getexif().get(274, 0) or 0)
    except Exception:  # noqa: BLE001
        orient = 0
    return Header(im.size[0], im.size[1], _BANDS[_target_mode(im)], sniff_type(buf), orient)


def decode(buf: bytes, shrink: int = 1) -> np.ndarray:
    """Decode to (h, w, bands) uint8.  shrink in (2, 4, 8) uses the JPEG DCT-domain
    downscale (libjpeg scale_denom), giving ceil(w / shrink) x ceil(h / shrink)."""
    im = _open(buf)
    mode = _target_mode(im)
    if shrink > 1 and im.format == "JPEG":
        w, h = im.size
        im.draft(mode if mode in ("L", "RGB") else "RGB", ((w + shrink - 1) // shrink, (h + shrink - 1) // shrink))
    if im.mode != mode:
        im = im.convert(mode)
    a = np.asarray(im, dtype=np.uint8)
    return a[:, :, None] if a.ndim == 2 else np.ascontiguousarray(a)


def decode_scale(w: int, h: int, shrink: int) -> int:
    """The scale decode(buf, shrink) really delivers for a w x h JPEG: Pillow's draft takes the
    largest of 1, 2, 4, 8 not above min(w // ceil(w / shrink), h // ceil(h / shrink)), so a
    53-wide file asked for 1/2 decodes at full size.  The decode is ceil(w / scale) x
    ceil(h / scale)."""
    if shrink <= 1:
        return 1
    fit = min(w // ((w + shrink - 1) // shrink), h // ((h + shrink - 1) // shrink))
    return max(s for s in (1, 2, 4, 8) if s <= max(fit, 1))


YCC_444 = 0   # MIPX_YCC_444: Cb and Cr at full size
YCC_420 = 1   # MIPX_YCC_420: Cb and Cr at ceil(w / 2) x ceil(h / 2)
YCC_422 = 3   # MIPX_YCC_422: Cb and Cr at ceil(w / 2) x h (libjpeg's h2v1); an input layout only
YCC_GREY = 6  # MIPX_YCC_GREY: one component, a 1-band image; coefficient input and output

# The samplings (h, v) of Y, Cb, Cr that the input paths take, by layout.  4:2:2 is opt-in
# (h2v1=True below): a caller that did not ask for it gets None for such a file, as before.
_SAMPLINGS = {((1, 1), (1, 1), (1, 1)): YCC_444, ((2, 2), (1, 1), (1, 1)): YCC_420}
_SAMPLINGS_H2V1 = {**_SAMPLINGS, ((2, 1), (1, 1), (1, 1)): YCC_422}
# Opt-in as well (grey=True below).  A scan of one component is not interleaved, so its sampling
# factors change nothing: 1 x 1 is what libjpeg writes by default and 2 x 2 what it writes when the
# caller asked for 4:2:0 of a grey image, as encode() does below Q 90.
_SAMPLING_GREY = {((1, 1),): YCC_GREY, ((2, 2),): YCC_GREY}


def _sampling_geometry(w: int, h: int, samp):
    """Per component (wb, hb, hs, vs): its real blocks across and down and its blocks across and
    down in one MCU; and the MCUs across and down.  samp: (hs, vs) per component."""
    hmax, vmax = max(a for a, _ in samp), max(b for _, b in samp)
    geo = [((-(-w * hs // hmax) + 7) // 8, (-(-h * vs // vmax) + 7) // 8, hs, vs) for hs, vs in samp]
    return geo, -(-w // (8 * hmax)), -(-h // (8 * vmax))


def decode_ycc(buf: bytes):
    """A JPEG's planes as the decoder has them before its upsample and colour conversion,
    packed for the engine's MIPX_OP_YCC step: (planes, layout) with planes a 1-D uint8 array
    of Y (h x w), then Cb, then Cr (ch x cw each), or None when the file is anything but a
    3-component YCbCr JPEG sampled 4:4:4 or 4:2:0 (the caller then takes decode()).

    Stand-in recipe: Pillow's libjpeg hands out YCbCr unconverted (draft "YCbCr"); for 4:2:0
    a second decode at scale 1/2 runs chroma through its full 8 x 8 IDCT with no upsampling,
    so its channels 1 and 2 are the raw chroma planes.  A real shim reads them in one decode
    (TurboJPEG tjDecompressToYUVPlanes, or libjpeg jpeg_read_raw_data)."""
    if _PIL is None or sniff_type(buf) != "jpeg":
        return None
    try:
        from PIL import JpegImagePlugin
        im = _open(buf)
        if im.format != "JPEG" or im.mode != "RGB" or getattr(im, "layers", 0) != 3:
            return None
        if im.info.get("adobe_transform") == 0:   # Adobe marker, transform 0: the components are RGB
            return None
        if ("jfif" not in im.info and "adobe" not in im.info
                and [c[0] for c in getattr(im, "layer", [])] == [82, 71, 66]):
            return None   # no JFIF / Adobe marker and component ids 'R' 'G' 'B': libjpeg takes it as RGB
        layout = {0: YCC_444, 2: YCC_420}.get(JpegImagePlugin.get_sampling(im))
        if layout is None:
            return None
        w, h = im.size
        im.draft("YCbCr", (w, h))
        full = np.asarray(im, dtype=np.uint8)
        if im.mode != "YCbCr" or full.shape != (h, w, 3):
            return None
        if layout == YCC_444:
            cb, cr = full[:, :, 1], full[:, :, 2]
        else:
            cw, ch = (w + 1) // 2, (h + 1) // 2
            half = _open(buf)
            half.draft("YCbCr", (max(w // 2, 1), max(h // 2, 1)))
            c = np.asarray(half, dtype=np.uint8)
            if half.decoderconfig[0] == 1:
                # a 1-pixel-wide or -high image cannot be drafted to 1/2.  With cw <= 2 libjpeg
                # replicates chroma, so every second sample of the full decode is the raw plane;
                # wider ones are interpolated and this stand-in cannot get at their planes.
                if min(w, h) > 1 or cw > 2:
                    return None
                c = c[::2, ::2]
            elif half.decoderconfig[0] != 2:
                return None
            if half.mode != "YCbCr" or c.shape != (ch, cw, 3):
                return None
            cb, cr = c[:, :, 1], c[:, :, 2]
    except Exception:  # noqa: BLE001 - whatever the planar decode cannot do, the RGB decode reports
        return None
    return np.concatenate([full[:, :, 0].ravel(), cb.ravel(), cr.ravel()]), layout


# ---- JPEG from quantised coefficients (the engine's MIPX_OP_JPEGC output) ----------------
# The four Huffman tables of Annex K.3 as (code counts per length 1..16, symbols): what every
# libjpeg encoder writes unless it optimises them.
_HUFF_DC_LUM = (bytes([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]), bytes(range(12)))
_HUFF_DC_CHR = (bytes([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]), bytes(range(12)))
_HUFF_AC_LUM = (bytes([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125]), bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738"
    "393a434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5"
    "a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"))
_HUFF_AC_CHR = (bytes([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119]), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3"
    "a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
HUFFMAN_TABLES = {0x00: _HUFF_DC_LUM, 0x10: _HUFF_AC_LUM, 0x01: _HUFF_DC_CHR, 0x11: _HUFF_AC_CHR}   # by DHT Tc/Th byte

# natural index of the k-th coefficient in zigzag order
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
          21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
          60, 61, 54, 47, 55, 62, 63)

_STD_QLUM = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
             14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
             49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
_STD_QCHR = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
             47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def jpeg_qtables(quality: int):
    """jpeg_set_quality(quality, TRUE) over the Annex K tables: (lum, chr), natural order.  The
    host twin of mipx_jpeg_qtables, so writing a file needs no engine."""
    if not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality {quality} outside 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple([min(max((q * s + 50) // 100, 1), 255) for q in t] for t in (_STD_QLUM, _STD_QCHR))


def _huff_codes(table):
    """symbol -> (code, length), canonical (Annex C)."""
    counts, symbols = table
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            codes[symbols[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return codes


def _jpegc_geometry(w: int, h: int, layout: int):
    """Per component (wb, hb, sampling factor), and the MCUs across and down."""
    ywb, yhb = (w + 7) // 8, (h + 7) // 8
    if layout == YCC_GREY:        # one component: the scan is not interleaved, an MCU is a block
        return [(ywb, yhb, 1)], ywb, yhb
    if layout == YCC_444:
        return [(ywb, yhb, 1)] * 3, ywb, yhb
    if layout != YCC_420:
        raise ValueError(f"unknown coefficient layout {layout}")
    cwb, chb = ((w + 1) // 2 + 7) // 8, ((h + 1) // 2 + 7) // 8
    return [(ywb, yhb, 2), (cwb, chb, 1), (cwb, chb, 1)], cwb, chb


def _padded_planes(coefs, w: int, h: int, layout: int):
    """The coefficients per component as (rows, columns, 64) int32 in zigzag order, padded to
    whole MCUs with libjpeg's dummy blocks; also the components and the MCU grid."""
    comps, mw, mh = _jpegc_geometry(w, h, layout)
    c = np.ascontiguousarray(coefs).view(np.int16).ravel() if np.asarray(coefs).dtype == np.uint8 \
        else np.asarray(coefs, dtype=np.int16).ravel()
    if c.size != 64 * sum(wb * hb for wb, hb, _ in comps):
        raise ValueError(f"{c.size} coefficients for {w}x{h} layout {layout}")
    planes, at = [], 0
    for wb, hb, s in comps:       # pad every component to whole MCUs with the dummy blocks
        full = np.zeros((mh * s, mw * s, 64), np.int16)
        full[:hb, :wb] = c[at:at + 64 * wb * hb].reshape(hb, wb, 64)
        at += 64 * wb * hb
        for x in range(wb, mw * s):
            full[:hb, x, 0] = full[:hb, x - 1, 0]
        for y in range(hb, mh * s):
            for m in range(mw):
                full[y, m * s:(m + 1) * s, 0] = full[y - 1, m * s + s - 1, 0]
        planes.append(full[:, :, list(ZIGZAG)].astype(np.int32))
    return planes, comps, mw, mh


def jpeg_header(w: int, h: int, layout: int, quality: int, tables=None, grey_sampling: int = 1) -> bytes:
    """SOI through SOS of the baseline JFIF file encode_jpeg_coefs writes: it depends on the
    size, the sampling (YCC_444 / YCC_420) and the quality only, not on the image, unless
    `tables` (as HUFFMAN_TABLES: by DHT Tc/Th byte, (16 code counts, symbols)) replace Annex K's.
    YCC_GREY writes what libjpeg writes for JCS_GRAYSCALE: one DQT (table 0), one component (id 1,
    1 x 1, table 0), DHT DC 0 and AC 0 only, an SOS of one component.  grey_sampling: the factor the
    one component declares both ways, 2 for the file libjpeg writes when its caller asked for 4:2:0
    (the scan is the same: it is not interleaved)."""
    comps, _, _ = _jpegc_geometry(w, h, layout)
    lum, chrom = jpeg_qtables(quality)
    tables = HUFFMAN_TABLES if tables is None else tables

    def seg(marker, body):
        return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body

    out = bytearray(b"\xff\xd8")
    out += seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, t in enumerate((lum, chrom)[:2 if len(comps) == 3 else 1]):
        out += seg(0xDB, bytes([i]) + bytes(t[k] for k in ZIGZAG))
    sof = bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([len(comps)])
    for i, (_, _, s) in enumerate(comps):
        if layout == YCC_GREY:
            s = grey_sampling
        sof += bytes([i + 1, (s << 4) | s, 0 if i == 0 else 1])
    out += seg(0xC0, sof)
    for tc in _table_ids(layout):
        out += seg(0xC4, bytes([tc]) + bytes(tables[tc][0]) + bytes(tables[tc][1]))
    if layout == YCC_GREY:
        out += seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0]))
    else:
        out += seg(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return bytes(out)


def _table_ids(layout: int):
    """The DHT Tc/Th bytes of the tables a file of `layout` carries, in the order it writes them."""
    return (0x00, 0x10) if layout == YCC_GREY else (0x00, 0x10, 0x01, 0x11)


def _scan_symbols(coefs, w: int, h: int, layout: int):
    """The symbols of the scan in order, with an MCU row's number: (row, Tc/Th byte of the table,
    symbol, value): per block, dummy blocks included, the DC category of the difference; per non-zero
    AC coefficient run << 4 | size, with 0xF0 per 16 zeros in front and 0x00 (EOB) unless coefficient
    63 is coded.  ValueError for a value that has no code."""
    planes, comps, mw, mh = _padded_planes(coefs, w, h, layout)
    pred = [0, 0, 0]
    for my in range(mh):
        for mx in range(mw):
            for ci, (_, _, s) in enumerate(comps):
                t = 0 if ci == 0 else 1
                for by in range(s):
                    for bx in range(s):
                        blk = planes[ci][my * s + by, mx * s + bx]
                        d = int(blk[0]) - pred[ci]
                        pred[ci] = int(blk[0])
                        size = abs(d).bit_length()
                        if size > 11:
                            raise ValueError(f"DC difference {d}: no Annex K code past 2047")
                        yield my, t, size, d
                        nz = np.flatnonzero(blk[1:]) + 1
                        prev = 0
                        for k in nz.tolist():
                            run = k - prev - 1
                            while run > 15:
                                yield my, 0x10 | t, 0xF0, 0
                                run -= 16
                            v = int(blk[k])
                            size = abs(v).bit_length()
                            if size > 10:
                                raise ValueError(f"AC coefficient {v}: no Annex K code past 1023")
                            yield my, 0x10 | t, (run << 4) | size, v
                            prev = k
                        if prev != 63:
                            yield my, 0x10 | t, 0x00, 0


def jpeg_symbol_counts(coefs, w: int, h: int, layout: int):
    """The scan's symbol counts by DHT Tc/Th byte, 256 each: Y counts into tables 0x00 and 0x10,
    Cb and Cr together into 0x01 and 0x11 (what libjpeg's optimize_coding pass gathers); YCC_GREY
    has tables 0x00 and 0x10 alone.  ValueError as jpeg_scan."""
    counts = {tc: [0] * 256 for tc in _table_ids(layout)}
    for _, tc, sym, _ in _scan_symbols(coefs, w, h, layout):
        counts[tc][sym] += 1
    return counts


def _jpeg_code_sizes(freq):
    """libjpeg's jpeg_gen_optimal_table up to the code sizes: per symbol its length before the
    limiting to 16 bits, 0 for a symbol that does not occur; the last entry is the reserved point's."""
    f = [int(v) for v in freq] + [1]     # the reserved point: no code is all ones
    if len(f) != 257 or min(f) < 0:
        raise ValueError("256 non-negative symbol counts")
    size, others = [0] * 257, [-1] * 257
    while True:
        # the least non-zero frequency, the largest index among equals (the library scans upward with <=)
        live = [(v, -i) for i, v in enumerate(f) if v]
        if len(live) < 2:
            return size
        live.sort()
        c1, c2 = -live[0][1], -live[1][1]
        f[c1] += f[c2]
        f[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1


def jpeg_optimal_table(freq):
    """The Huffman table libjpeg's optimize_coding makes of 256 symbol counts (jchuff.c
    jpeg_gen_optimal_table, tie-breaks included; PARITY_ASSUMPTIONS.md row 24) as (16 code counts,
    symbols), the form of HUFFMAN_TABLES' entries.  Counts that sum to 10^9 or more are outside
    the library's search."""
    size = _jpeg_code_sizes(freq)
    bits = [0] * (max(max(size), 16) + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(len(bits) - 1, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1                     # the reserved point's code
    symbols = sorted((s for s in range(256) if size[s]), key=lambda s: (size[s], s))
    return bytes(bits[1:17]), bytes(symbols)


def jpeg_scan_bits(coefs, w: int, h: int, layout: int, tables=None):
    """(scan, bits): jpeg_scan's bytes, and the scan's length in bits before the last byte is
    padded and the 0xFF bytes are stuffed (what the engine's slot header reports)."""
    tables = HUFFMAN_TABLES if tables is None else tables
    codes = {tc: _huff_codes(tables[tc]) for tc in _table_ids(layout)}
    acc, nbits, total = 0, 0, 0  # the bit buffer, as one growing integer per MCU row
    scan = bytearray()

    def flush(final=False):
        nonlocal acc, nbits
        if final and nbits % 8:
            pad = 8 - nbits % 8
            acc = (acc << pad) | ((1 << pad) - 1)
            nbits += pad
        whole = nbits // 8
        if whole:
            rest = nbits - 8 * whole
            scan.extend((acc >> rest).to_bytes(whole, "big").replace(b"\xff", b"\xff\x00"))
            acc &= (1 << rest) - 1
            nbits = rest

    row = 0
    for my, tc, sym, v in _scan_symbols(coefs, w, h, layout):
        if my != row:
            flush()
            row = my
        code, length = codes[tc][sym]
        size = sym & 15 if tc & 0x10 else sym
        # the code, then the `size` low bits of v, or of v - 1 when negative
        acc = (((acc << length) | code) << size) | ((v if v >= 0 else v - 1) & ((1 << size) - 1))
        nbits += length + size
        total += length + size
    flush(final=True)
    return bytes(scan), total


def jpeg_scan(coefs, w: int, h: int, layout: int, tables=None) -> bytes:
    """The entropy-coded scan of the engine's quantised coefficients (MIPX_OP_JPEGC: int16, Y
    then Cb then Cr, real blocks in raster order, natural order inside a block), without EOI:
    the Annex K Huffman tables (or `tables`, as jpeg_header takes them), one interleaved scan,
    libjpeg's dummy blocks where the real
    blocks do not fill whole MCUs (zero AC; DC copied from the block to the left, or, in a
    wholly dummy block row, from the last block of the same MCU's row above), the last byte
    padded with 1-bits, every 0xFF followed by 0x00.  What a plan that ends with MIPX_OP_JPEGE
    gives (PARITY_ASSUMPTIONS.md row 21).  ValueError for a coefficient no Annex K code exists
    for: an AC magnitude above 1023 or a DC difference magnitude above 2047."""
    return jpeg_scan_bits(coefs, w, h, layout, tables)[0]


def jpeg_from_scan(scan, w: int, h: int, layout: int, quality: int, tables=None, grey_sampling: int = 1) -> bytes:
    """The file: jpeg_header, the scan (jpeg_scan, or the bytes of an engine slot), EOI; `tables`
    are the ones the scan was coded with, None for Annex K's."""
    return jpeg_header(w, h, layout, quality, tables, grey_sampling) + bytes(scan) + b"\xff\xd9"


def encode_jpeg_coefs(coefs, w: int, h: int, layout: int, quality: int, tables=None, grey_sampling: int = 1) -> bytes:
    """A baseline JFIF file from the engine's quantised coefficients (MIPX_OP_JPEGC), made at
    `quality` in `layout` (YCC_444 / YCC_420, or YCC_GREY: Y's blocks alone).  Stand-in for libjpeg's jpeg_write_coefficients:
    jpeg_from_scan of jpeg_scan.  tables: None for Annex K's, "optimal" for the ones libjpeg's
    optimize_coding makes of the image (jpeg_optimal_table of jpeg_symbol_counts), or a dict as
    jpeg_header takes."""
    if isinstance(tables, str):
        if tables != "optimal":
            raise ValueError(f"tables {tables!r}")
        tables = {tc: jpeg_optimal_table(f) for tc, f in jpeg_symbol_counts(coefs, w, h, layout).items()}
    return jpeg_from_scan(jpeg_scan(coefs, w, h, layout, tables), w, h, layout, quality, tables, grey_sampling)


# ---- quantised coefficients from a JPEG (the engine's MIPX_OP_JPEGD input) -----------------
JPEGD_HEADER_BYTES = 384   # MIPX_JPEGD_HEADER_BYTES: the tables of Y, Cb, Cr, 64 uint16 each


def _huff_lookup(counts, symbols):
    """A 65536-entry table over the next 16 bits of the stream: (code length << 8) | symbol,
    0 where no code matches."""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= 1 << length:
                return None
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | symbols[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def _jpeg_segments(buf: bytes, dht=None, span=None, grey=False):
    """What decode_jpeg_coefs needs of a file's headers, or None for a file it does not take:
    (w, h, components [(id, h, v, tq, td, ta)], tables {tq: 64 natural-order values}, Huffman
    lookups {Tc/Th byte: lookup}, restart interval, the entropy-coded intervals).  dht: a dict
    that takes the Huffman tables as the file has them, {Tc/Th byte: (16 counts, symbols)}.
    span: a list that takes the offsets in buf of the scan's first byte and of its closing FF D9.
    grey: take one-component files too (SOF and SOS of one component, a non-interleaved scan)."""
    import re
    if buf[:2] != b"\xff\xd8":
        return None
    p, n = 2, len(buf)
    qt, huff, frame, restart = {}, {}, None, 0
    jfif, adobe = False, None
    while True:
        while p < n and buf[p] == 0xFF and p + 1 < n and buf[p + 1] == 0xFF:
            p += 1   # fill bytes
        if p + 4 > n or buf[p] != 0xFF:
            return None
        m = buf[p + 1]
        size = int.from_bytes(buf[p + 2:p + 4], "big")
        body = buf[p + 4:p + 2 + size]
        if size < 2 or len(body) != size - 2:
            return None
        p += 2 + size
        if m == 0xE0 and body[:5] == b"JFIF\x00":
            jfif = True
        elif m == 0xEE and body[:5] == b"Adobe" and len(body) >= 12:
            adobe = body[11]
        elif m == 0xDB:
            while body:
                if body[0] >> 4 or len(body) < 65:     # 16-bit tables
                    return None
                t = [0] * 64
                for k in range(64):
                    t[ZIGZAG[k]] = body[1 + k]
                qt[body[0] & 15] = t
                body = body[65:]
        elif m == 0xC4:
            while body:
                if len(body) < 17:
                    return None
                cnt = sum(body[1:17])
                if len(body) < 17 + cnt or cnt > 256:
                    return None
                huff[body[0]] = _huff_lookup(body[1:17], body[17:17 + cnt])
                if huff[body[0]] is None:
                    return None
                if dht is not None:
                    dht[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + cnt]))
                body = body[17 + cnt:]
        elif m in (0xC0, 0xC1):                         # baseline, extended sequential; Huffman
            if frame is not None or len(body) < 6 or body[0] != 8 or body[5] not in ((3, 1) if grey else (3,)) \
                    or len(body) != 6 + 3 * body[5]:
                return None
            frame = (int.from_bytes(body[3:5], "big"), int.from_bytes(body[1:3], "big"),
                     [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                      for i in range(body[5])])
        elif m == 0xDD:
            if len(body) != 2:
                return None
            restart = int.from_bytes(body, "big")
        elif m == 0xDA:
            break
        elif 0xC0 <= m <= 0xCF or m in (0xDC, 0xD8, 0xD9):   # progressive, lossless, arithmetic, DNL, ...
            return None
    w, h, comps = frame if frame is not None else (0, 0, [])
    nc = len(comps)
    if w <= 0 or h <= 0 or len(body) != 4 + 2 * nc or body[0] != nc or bytes(body[-3:]) != b"\x00\x3f\x00":
        return None                                          # one scan of every component and the whole spectrum
    full = []
    for i, (cid, ch, cv, tq) in enumerate(comps):
        if body[1 + 2 * i] != cid or tq not in qt:
            return None
        td, ta = body[2 + 2 * i] >> 4, 0x10 | (body[2 + 2 * i] & 15)
        if td not in huff or ta not in huff:
            return None
        full.append((cid, ch, cv, tq, td, ta))
    # the colour space by the rules decode_ycc applies
    if adobe == 0:                                           # Adobe marker, transform 0: the components are RGB
        return None
    if not jfif and adobe is None and [c[0] for c in full] == [82, 71, 66]:
        return None   # no JFIF / Adobe marker and component ids 'R' 'G' 'B': libjpeg takes it as RGB
    # the scan's bytes up to the next marker, cut at the restart markers
    parts, at, end = [], p, None
    for hit in re.finditer(rb"\xff[^\x00]", buf[p:]):
        b1, q = hit.group()[1], p + hit.start()
        if b1 == 0xFF:
            return None                                      # fill bytes inside a scan: not worth the care
        parts.append(buf[at:q])
        at = q + 2
        if not 0xD0 <= b1 <= 0xD7:
            end = b1
            break
    if end != 0xD9:                                          # truncated, or another scan follows
        return None
    if span is not None:
        span[:] = [p, at - 2]
    return w, h, full, qt, huff, restart, parts


def decode_jpeg_coefs(buf: bytes, h2v1: bool = False, grey: bool = False):
    """A JPEG's quantised DCT coefficients as its entropy decoder has them, packed for the
    engine's MIPX_OP_JPEGD step: (payload, layout) with payload a 1-D uint8 array of the file's
    quantisation tables (Y, Cb, Cr: 64 little-endian uint16 each, natural order) and then the
    int16 coefficients of the real blocks only (Y, Cb, Cr; blocks in raster order; natural order
    inside a block), or None (it never raises) for every file it does not take: anything but an
    8-bit baseline or extended-sequential Huffman JPEG of 3 YCbCr components sampled 4:4:4 or
    4:2:0 in one interleaved scan, so progressive, arithmetic-coded, grey, CMYK, RGB, 4:2:2 and
    truncated files, and what is no JPEG at all (the caller then takes decode()).

    h2v1=True takes 4:2:2 files too (sampling 2x1, 1x1, 1x1; layout YCC_422): chroma is
    ceil(ceil(w / 2) / 8) blocks across and ceil(h / 8) down, the MCU is Y left, Y right, Cb, Cr.

    grey=True takes one-component files too (sampling 1x1, one scan; layout YCC_GREY): the header
    keeps its 384 bytes, Y's table and zeros behind it, and the coefficients are Y's blocks alone.
    The scan is not interleaved: an MCU is one block, so a restart interval counts blocks.

    Stand-in for libjpeg's jpeg_read_coefficients: a pure-Python Huffman decoder (any tables,
    restart intervals) that looks codes up by the next 16 bits of the stream."""
    try:
        seg = _jpeg_segments(bytes(buf), grey=grey)
        if seg is None:
            return None
        w, h, comps, qt, huff, restart, parts = seg
        samp = tuple((c[1], c[2]) for c in comps)
        layout = (_SAMPLINGS_H2V1 if h2v1 else _SAMPLINGS).get(samp)
        if layout is None and grey:
            layout = _SAMPLING_GREY.get(samp)
            samp = ((1, 1),)   # whatever it declares, the one component's blocks are the image's
        if layout is None:
            return None
        geo, mw, mh = _sampling_geometry(w, h, samp)
        if restart == 0:
            restart = mw * mh
        if len(parts) != -(-mw * mh // restart):
            return None
        # a block is at least 2 bits (a DC code and an end-of-block): a header that promises more
        # blocks than the scan can hold is damaged, and must not size the arrays below
        if sum(hs * vs for _, _, hs, vs in geo) * mw * mh > 4 * sum(len(d) for d in parts):
            return None
        store = [[0] * (64 * mw * mh * hs * vs) for _, _, hs, vs in geo]
        order = []      # the blocks of one MCU: (component, row in the MCU, column in the MCU)
        for ci, (_, _, hs, vs) in enumerate(geo):
            order += [(ci, by, bx) for by in range(vs) for bx in range(hs)]
        dc = [huff[c[4]] for c in comps]
        ac = [huff[c[5]] for c in comps]
        zz = ZIGZAG
        mcu = 0
        for data in parts:
            avail = 8 * len(data.replace(b"\xff\x00", b"\xff"))
            data = data.replace(b"\xff\x00", b"\xff") + b"\x00" * 16
            acc, nbits, pos = 0, 0, 0
            pred = [0, 0, 0]
            for mcu in range(mcu, min(mcu + restart, mw * mh)):
                my, mx = divmod(mcu, mw)
                for ci, by, bx in order:
                    hs, vs = geo[ci][2:]
                    out = store[ci]
                    base = 64 * ((my * vs + by) * mw * hs + mx * hs + bx)
                    lut = dc[ci]
                    k = 0
                    while k < 64:
                        if nbits < 32:
                            acc = ((acc & ((1 << nbits) - 1)) << 32) | int.from_bytes(data[pos:pos + 4], "big")
                            pos += 4
                            nbits += 32
                        look = lut[(acc >> (nbits - 16)) & 0xFFFF]
                        if look == 0:
                            return None
                        nbits -= look >> 8
                        size = look & 15
                        if k == 0:
                            if look & 0xF0:
                                return None
                            lut = ac[ci]
                        else:
                            run = (look >> 4) & 15
                            if size == 0:
                                if run != 15:
                                    break          # end of block
                                k += 16
                                continue
                            k += run
                            if k > 63:
                                return None
                        v = 0
                        if size:
                            v = (acc >> (nbits - size)) & ((1 << size) - 1)
                            nbits -= size
                            if v < 1 << (size - 1):
                                v -= (1 << size) - 1
                        if k == 0:
                            v = pred[ci] = pred[ci] + v
                        out[base + zz[k]] = v
                        k += 1
                if 8 * pos - nbits > avail:
                    return None                    # ran past the interval's bytes
            mcu += 1
        if mcu != mw * mh:
            return None
        body = []
        for (wb, hb, hs, vs), flat in zip(geo, store):
            a = np.array(flat, dtype=np.int64).reshape(mh * vs, mw * hs, 64)[:hb, :wb]
            if a.size and (a.min() < -32768 or a.max() > 32767):
                return None
            body.append(a.astype("<i2").ravel())
        head = np.zeros(JPEGD_HEADER_BYTES // 2, "<u2")
        head[:64 * len(comps)] = np.array([qt[c[3]] for c in comps], dtype="<u2").ravel()
        return np.concatenate([head.view(np.uint8), np.concatenate(body).view(np.uint8)]), layout
    except Exception:  # noqa: BLE001 - whatever this decoder cannot read, the RGB decode reports
        return None


# ---- the entropy-coded scan of a JPEG (the engine's entropy decoder, MIPX_OP_JPEGH) ---------
JPEGH_HEADER_BYTES = 1504   # MIPX_JPEGH_HEADER_BYTES
JPEGH_OK, JPEGH_UNSYNCED, JPEGH_BAD = 0, 1, 2   # MIPX_JPEGH_*


def jpeg_huff_slot(buf: bytes, restart: bool = False, h2v1: bool = False, grey: bool = False):
    """A JPEG's entropy-coded scan as the file has it, packed for the engine's entropy decoder
    (MIPX_JPEGH_HEADER_BYTES in include/mipx.h): (slot, layout) with slot a 1-D uint8 array of
    the scan's length, the quantisation tables of Y, Cb, Cr, the components' Huffman table
    indices, the four Huffman tables and the scan bytes, padded with zeros to the slot's size
    (1504 + the coefficients' size; slot[:1504 + length] is all the engine reads).  The host
    reads markers only.  None (it never raises) for every file decode_jpeg_coefs does not take
    by its headers, and for files with a restart interval, a Huffman table index above 1 or a
    scan longer than the coefficients.

    restart=True takes files with a restart interval (DRI) too: the interval, in MCUs, goes into
    the header at offset 4 (0 for a file without one) and the scan is the file's bytes between the
    SOS segment and FF D9 as they are, restart markers included; the engine checks the markers.

    h2v1=True takes 4:2:2 files too, as decode_jpeg_coefs does (layout YCC_422).

    grey=True takes one-component files too, as decode_jpeg_coefs does (layout YCC_GREY): the header
    keeps its size; Y's quantisation table stands at byte 16 with zeros behind it, byte 400 is Y's DC
    table index and byte 403 its AC index (the other four are zero), every Huffman table the file
    defines stands at its place, and the interval at offset 4 counts blocks."""
    try:
        buf = bytes(buf)
        dht, span = {}, []
        seg = _jpeg_segments(buf, dht, span, grey=grey)
        if seg is None:
            return None
        w, h, comps, qt, _, interval, parts = seg
        samp = tuple((c[1], c[2]) for c in comps)
        layout = (_SAMPLINGS_H2V1 if h2v1 else _SAMPLINGS).get(samp)
        if layout is None and grey:
            layout = _SAMPLING_GREY.get(samp)
            samp = ((1, 1),)
        if layout is None:
            return None
        if not restart and (interval != 0 or len(parts) != 1):
            return None
        if any(c[4] > 1 or (c[5] & 15) > 1 for c in comps):
            return None
        geo, _, _ = _sampling_geometry(w, h, samp)
        cap = 128 * sum(g[0] * g[1] for g in geo)
        scan = buf[span[0]:span[1]] if restart else parts[0]
        if len(scan) > cap:
            return None
        slot = np.zeros(JPEGH_HEADER_BYTES + cap, np.uint8)
        slot[0:4] = np.frombuffer(len(scan).to_bytes(4, "little"), np.uint8)
        if restart:
            slot[4:8] = np.frombuffer(interval.to_bytes(4, "little"), np.uint8)
        slot[16:16 + 128 * len(comps)] = np.array([qt[c[3]] for c in comps], dtype="<u2").ravel().view(np.uint8)
        for i, c in enumerate(comps):
            slot[400 + i], slot[403 + i] = c[4], c[5] & 15
        for i, key in enumerate((0x00, 0x01, 0x10, 0x11)):
            if key in dht:
                counts, symbols = dht[key]
                at = 416 + 272 * i
                slot[at:at + 16] = np.frombuffer(counts, np.uint8)
                slot[at + 16:at + 16 + len(symbols)] = np.frombuffer(symbols, np.uint8)
        slot[JPEGH_HEADER_BYTES:JPEGH_HEADER_BYTES + len(scan)] = np.frombuffer(scan, np.uint8)
        return slot, layout
    except Exception:  # noqa: BLE001 - whatever this cannot read, the other decoders report
        return None


_SANS_FACES =("DejaVuSans.ttf", "LiberationSans-Regular.ttf", "NotoSans-Regular.ttf", "FreeSans.ttf", "Arial.ttf")
DEFAULT_FONT_POINTS = 10.0


def _sans_face(pixels: int):
    try:
        from PIL import ImageFont
    except ImportError as e:
        raise CodecError("no text renderer (Pillow) available") from e
    for name in _SANS_FACES:
        try:
            return ImageFont.truetype(name, pixels)
        except OSError:      # face not installed
            continue
        except ImportError as e:   # Pillow built without FreeType
            raise CodecError(f"no text renderer: {e}") from e
    raise CodecError("no text renderer: no sans TrueType face found")


def render_text(text: str, font: str = "sans 10", width: int = 0, dpi: int = 150) -> np.ndarray:
    """Opt-in stand-in for vips_text (the renderer imaginary.Watermark takes): the tight
    1-band coverage mask, (h, w) uint8, of `text` in a system sans face, wrapped at spaces to
    `width` pixels (0 = no wrapping).  `font` is a pango description; only its trailing
    point size is read, and the glyphs are points * dpi / 72 pixels high.  Pillow's
    FreeType rasteriser is not pango: the pixels differ from libvips', as Pillow's codecs
    differ from libvips' savers."""
    words = font.split()
    try:
        points = float(words[-1]) if words else DEFAULT_FONT_POINTS
    except ValueError:
        points = DEFAULT_FONT_POINTS
    face = _sans_face(max(1, int(round(points * dpi / 72.0))))
    from PIL import Image as PILImage, ImageDraw
    lines = []
    for para in text.split("\n"):
        line = ""
        for word in para.split(" "):
            trial = word if not line else line + " " + word
            if width > 0 and line and face.getlength(trial) > width:
                lines.append(line)
                line = word
            else:
                line = trial
        lines.append(line)
    body = "\n".join(lines)
    probe = ImageDraw.Draw(PILImage.new("L", (1, 1)))
    l, t, r, b = probe.multiline_textbbox((0, 0), body, font=face)
    if r <= l or b <= t:
        raise CodecError("text watermark: nothing to render")
    im = PILImage.new("L", (r - l, b - t), 0)
    ImageDraw.Draw(im).multiline_text((-l, -t), body, fill=255, font=face)
    box = im.getbbox()
    if box is None:
        raise CodecError("text watermark: nothing to render")
    return np.ascontiguousarray(np.asarray(im.crop(box), dtype=np.uint8))


def encode(px: np.ndarray, t: str, quality: Optional[int] = None, compression: Optional[int] = None) -> bytes:
    """Encode (h, w, bands) uint8 pixels as type t."""
    if _PIL is None:
        raise CodecError("no host codec (Pillow) available")
    fmt = _PIL_FORMAT.get(t)
    if fmt is None:
        raise CodecError(f"cannot encode to {t}")
    px = px if px.ndim == 3 else px[:, :, None]
    mode = {1: "L", 2: "LA", 3: "RGB", 4: "RGBA"}[px.shape[2]]
    im = _PIL.fromarray(px[:, :, 0] if mode == "L" else px, mode)
    if fmt == "JPEG" and mode in ("LA", "RGBA"):  # JPEG has no alpha: libvips drops it
        im = im.convert("L" if mode == "LA" else "RGB")
    out = io.BytesIO()
    kw = {}
    if fmt in ("JPEG", "WEBP"):
        kw["quality"] = quality or DEFAULT_QUALITY
    if fmt == "JPEG":
        # libvips jpegsave's automatic chroma subsampling: 4:2:0 below Q 90, 4:4:4 from Q 90
        kw["subsampling"] = 0 if kw["quality"] >= 90 else 2
    if fmt == "PNG" and compression is not None:
        kw["compress_level"] = compression
    try:
        im.save(out, fmt, **kw)
    except Exception as e:  # noqa: BLE001
        raise CodecError(f"encode {t}: {e}") from e
    return out.getvalue()
