"""The JPEG encoder's front half in numpy (PARITY_ASSUMPTIONS.md row 17): interleaved RGB in,
quantised DCT coefficients of the real blocks out, as libjpeg computes them with its default
settings (jccolor.c, jcsample.c h2v2_downsample, jfdctint.c, jcdctmgr.c, jpeg_set_quality).
tests/test_jpegc_cpu.py pins it to libjpeg-turbo inside Pillow; the GPU tests hold the kernel
to it.  Not part of the oracle.

Per image the coefficients are int16: component Y, then Cb, then Cr; each hb x wb blocks in
raster order; each block 64 coefficients in natural (row-major) order."""
import numpy as np

YCC_444 = 0
YCC_420 = 1

# Annex K.1 / K.2, natural order
STD_LUM = np.array([
    16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
STD_CHR = np.array([
    17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99], np.int64)


def qtables(quality):
    """jpeg_set_quality(quality, TRUE): (lum, chr), 64 values each in natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((t * s + 50) // 100, 1, 255) for t in (STD_LUM, STD_CHR))


def geometry(w, h, layout):
    """[(wb, hb)] of Y, Cb, Cr."""
    y = ((w + 7) // 8, (h + 7) // 8)
    if layout == YCC_444:
        return [y, y, y]
    c = (((w + 1) // 2 + 7) // 8, ((h + 1) // 2 + 7) // 8)
    return [y, c, c]


def jpegc_bytes(w, h, layout):
    return 128 * sum(wb * hb for wb, hb in geometry(w, h, layout))


def _pad(p, rows, cols):
    """Replicate the last column, then the last row."""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def _pass(d, first):
    """One 8-point pass of jfdctint.c over the last axis."""
    d = [d[..., k] for k in range(8)]
    t0, t7, t1, t6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    t2, t5, t3, t4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    if first:
        def D(x):
            return (x + 1024) >> 11
        o0, o4 = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        def D(x):
            return (x + 16384) >> 15
        o0, o4 = (t10 + t11 + 2) >> 2, (t10 - t11 + 2) >> 2
    z1 = (t12 + t13) * 4433
    o2, o6 = D(z1 + t13 * 6270), D(z1 - t12 * 15137)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    z3p, z4p = -z3 * 16069 + z5, -z4 * 3196 + z5
    o7 = D(t4 * 2446 - z1 * 7373 + z3p)
    o5 = D(t5 * 16819 - z2 * 20995 + z4p)
    o3 = D(t6 * 25172 - z2 * 20995 + z3p)
    o1 = D(t7 * 12299 - z1 * 7373 + z4p)
    return np.stack([o0, o1, o2, o3, o4, o5, o6, o7], axis=-1)


def _blocks(plane, q):
    """Quantised coefficients (hb, wb, 64) of a padded sample plane (8 hb x 8 wb)."""
    hb, wb = plane.shape[0] // 8, plane.shape[1] // 8
    b = plane.reshape(hb, 8, wb, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128   # hb, wb, row, col
    b = _pass(b, True)                                     # rows
    b = _pass(b.transpose(0, 1, 3, 2), False).transpose(0, 1, 3, 2)   # columns
    assert np.abs(b).max(initial=0) < 2 ** 31
    q8 = 8 * q.reshape(8, 8)
    v = (np.abs(b) + (q8 >> 1)) // q8
    return (np.sign(b) * v).reshape(hb, wb, 64)


def jpegc_ref(rgb, layout, quality):
    """rgb (h, w, 3) or (n, h, w, 3) uint8 -> (n, jpegc_bytes / 2) int16."""
    rgb = np.asarray(rgb, dtype=np.uint8)
    if rgb.ndim == 3:
        rgb = rgb[None]
    n, h, w, _ = rgb.shape
    lum, chrom = qtables(quality)
    geo = geometry(w, h, layout)
    out = []
    for img in rgb.astype(np.int64):
        R, G, B = img[..., 0], img[..., 1], img[..., 2]
        Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
        Cb = (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16
        Cr = (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16
        parts = [_blocks(_pad(Y, 8 * geo[0][1], 8 * geo[0][0]), lum)]
        for c in (Cb, Cr):
            wb, hb = geo[1]
            if layout == YCC_444:
                p = _pad(c, 8 * hb, 8 * wb)
            else:
                ch = (h + 1) // 2
                p = _pad(c, 2 * ch, 16 * wb)       # full resolution: columns out, one row when h is odd
                bias = np.tile(np.array([1, 2]), 8 * wb // 2)
                p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
                p = _pad(p, 8 * hb, 8 * wb)        # then the downsampled rows
            parts.append(_blocks(p, chrom))
        coefs = np.concatenate([p.ravel() for p in parts])
        assert np.abs(coefs).max(initial=0) < 32768
        out.append(coefs.astype(np.int16))
    return np.stack(out)


def with_dummy_blocks(coefs, w, h, layout):
    """What the entropy coder sees: per component a (hbm, wbm, 64) array padded to whole MCUs
    with libjpeg's dummy blocks (zero AC, DC copied; jccoefct.c compress_first_pass)."""
    coefs = np.asarray(coefs, dtype=np.int16).ravel()
    geo = geometry(w, h, layout)
    samp = [2, 1, 1] if layout == YCC_420 else [1, 1, 1]
    mw, mh = geo[1] if layout == YCC_420 else geo[0]    # MCUs across and down
    out, at = [], 0
    for (wb, hb), s in zip(geo, samp):
        real = coefs[at:at + 64 * wb * hb].reshape(hb, wb, 64)
        at += 64 * wb * hb
        full = np.zeros((mh * s, mw * s, 64), np.int16)
        full[:hb, :wb] = real
        for x in range(wb, mw * s):                         # right of a row that has real blocks
            full[:hb, x, 0] = full[:hb, x - 1, 0]
        for y in range(hb, mh * s):                         # a wholly dummy block row
            for m in range(mw):
                full[y, m * s:(m + 1) * s, 0] = full[y - 1, m * s + s - 1, 0]
        out.append(full)
    assert at == coefs.size
    return out
