"""The reference of the entropy-coded JPEG output (MIPX_OP_JPEGE, PARITY_ASSUMPTIONS.md row 21): one
output slot is a 16-byte header and codec.jpeg_scan of the coefficients, the baseline Huffman
writer that tests/test_jpegc_cpu.py pins to libjpeg-turbo inside Pillow byte for byte.  Also the
sizes include/mipx.h states in words, the per-block bit counts (for the tests that need to know
where a block ends) and the two hand-found inputs whose scans have an 0xFF at an awkward place."""
import functools

import numpy as np

from jpegc_ref import YCC_420, YCC_444, jpegc_bytes

HEADER_BYTES = 16
OK, OVERFLOW, UNCODABLE = 0, 1, 2
TILE, CHUNK = 256, 1024   # kJpegeTile blocks per workgroup of the coding kernels, kJpegeChunk bytes of the stuffing ones


def jpeg_scan_bytes(w, h, layout):
    """mipx_jpeg_scan_bytes: the header and the capacity, which is the coefficients' size."""
    n = jpegc_bytes(w, h, layout)
    return HEADER_BYTES + n if n else 0


def scan_blocks(w, h, layout):
    """Blocks of the scan, libjpeg's dummy blocks included."""
    if layout == YCC_444:
        return 3 * ((w + 7) // 8) * ((h + 7) // 8)
    return 6 * (((w + 1) // 2 + 7) // 8) * (((h + 1) // 2 + 7) // 8)


def workspace_bytes(n, w, h):
    """mipx_op_workspace_bytes(MIPX_OP_JPEGE, n, w, h, 3, 0, 0): sized without the layout, so by
    whichever needs more.  Per image cap = the 4:4:4 coefficients.  Parts, each rounded up to 256
    bytes: the coefficients (n cap), the per-image records (32 n), the scan before stuffing
    (n cap), a bit count per block (4 n blocks), the tile sums and their scan (4 + 8 bytes per
    tile of 256 blocks), the 0xFF counts per 1024 bytes of stream and their scan (4 + 8)."""
    def up(v):
        return (v + 255) // 256 * 256
    cap = jpegc_bytes(w, h, YCC_444)
    blocks = max(scan_blocks(w, h, YCC_444), scan_blocks(w, h, YCC_420))
    tiles, chunks = -(-blocks // TILE), -(-cap // CHUNK)
    return (up(n * cap) + up(32 * n) + up(n * cap) + up(4 * n * blocks) + up(4 * n * tiles) + up(8 * n * tiles)
            + up(4 * n * chunks) + up(8 * n * chunks))


class Slot:
    """What one image's slot must hold: the header, and `scan` (status OK only)."""

    def __init__(self, length, status, bits, scan):
        self.length, self.status, self.bits, self.scan = length, status, bits, scan

    def header(self):
        return np.array([self.length, self.status, self.bits, 0], "<u4")


def slot_ref(coefs, w, h, layout):
    """The Slot of one image's coefficients (int16, jpegc_bytes / 2 of them).  bits is None where the
    interface leaves it open (an uncodable coefficient)."""
    from imaginary_amd import codec
    cap = jpegc_bytes(w, h, layout)
    try:
        scan, bits = codec.jpeg_scan_bits(coefs, w, h, layout)
    except ValueError:
        return Slot(0, UNCODABLE, None, b"")
    if len(scan) > cap:
        return Slot(-(-bits // 8), OVERFLOW, bits, b"")
    return Slot(len(scan), OK, bits, scan)


def check_slot(got, want, what):
    """A downloaded slot (uint8) against its Slot: the header, and the bytes up to `length`."""
    got = np.ascontiguousarray(got, dtype=np.uint8).ravel()
    head = got[:HEADER_BYTES].view("<u4")
    if want.bits is None:
        assert head[0] == 0 and head[1] == want.status and head[3] == 0, (what, head.tolist())
        return
    assert head.tolist() == want.header().tolist(), f"{what}: header {head.tolist()}, want {want.header().tolist()}"
    if want.status != OK:
        return
    assert HEADER_BYTES + want.length <= got.size, (what, want.length, got.size)
    data = got[HEADER_BYTES:HEADER_BYTES + want.length].tobytes()
    if data != want.scan:
        at = next(i for i in range(want.length) if data[i] != want.scan[i])
        raise AssertionError(f"{what}: {want.length} scan bytes, the first difference at byte {at}: "
                             f"got {data[at:at + 8].hex()} want {want.scan[at:at + 8].hex()}")


def block_bits(coefs, w, h, layout):
    """Bits of every block of the scan, in scan order: a restatement of the rule that shares only
    the tables and the padded planes with codec.jpeg_scan (their sum must be its bit count)."""
    from imaginary_amd import codec
    planes, comps, mw, mh = codec._padded_planes(coefs, w, h, layout)
    dc = [codec._huff_codes(codec._HUFF_DC_LUM), codec._huff_codes(codec._HUFF_DC_CHR)]
    ac = [codec._huff_codes(codec._HUFF_AC_LUM), codec._huff_codes(codec._HUFF_AC_CHR)]
    out, pred = [], [0, 0, 0]
    for my in range(mh):
        for mx in range(mw):
            for ci, (_, _, s) in enumerate(comps):
                t = 1 if ci else 0
                for by in range(s):
                    for bx in range(s):
                        blk = planes[ci][my * s + by, mx * s + bx]
                        size = abs(int(blk[0]) - pred[ci]).bit_length()
                        pred[ci] = int(blk[0])
                        bits, run = dc[t][size][1] + size, 0
                        for v in blk[1:].tolist():
                            if v == 0:
                                run += 1
                                continue
                            bits += (run // 16) * ac[t][0xF0][1]
                            size = abs(v).bit_length()
                            bits += ac[t][((run % 16) << 4) | size][1] + size
                            run = 0
                        if run:
                            bits += ac[t][0x00][1]
                        out.append(bits)
    return out


def unstuffed(scan):
    return bytes(scan).replace(b"\xff\x00", b"\xff")


# ---- the two inputs found by search (tests/test_jpege_cpu.py asserts what they are) ----------
# Both are 8 x 8 in 4:4:4 (one MCU: Y, Cb, Cr) drawn from a seeded generator.  A block that ends
# with EOB ends with a 0 bit (1010 or 00), so an 0xFF at a block's end needs the block's
# coefficient 63 coded, with a value of 1-bits behind a long run's code (those begin 1111111); a
# large DC step makes the next block begin with 1-bits too.
def _small_blocks(seed):
    rng = np.random.default_rng(seed)
    c = np.zeros((3, 64), np.int16)
    c[:, :12] = rng.integers(-40, 41, (3, 12))
    c[:, 0] = rng.integers(-1000, 1001, 3)
    c[:, 63] = rng.integers(1, 8, 3)
    c = c.reshape(-1)
    c.setflags(write=False)
    return c


PADDING_FF_SEED = 8    # of seeds 0..2999 the first whose scan ends in a padded 0xFF and has no straddling one
STRADDLE_FF_SEED = 0   # ... and the first with a straddling 0xFF whose padded last byte is not 0xFF


@functools.lru_cache(maxsize=None)
def padding_ff_coefs():
    """8 x 8, 4:4:4: the scan's last byte is partly padding, and the padding makes it 0xFF, so the
    scan ends FF 00."""
    return _small_blocks(PADDING_FF_SEED)


@functools.lru_cache(maxsize=None)
def straddle_ff_coefs():
    """8 x 8, 4:4:4: a byte of the scan is 0xFF and a block ends inside it."""
    return _small_blocks(STRADDLE_FF_SEED)


def ends_in_padding_ff(coefs, w, h, layout):
    from imaginary_amd import codec
    scan, bits = codec.jpeg_scan_bits(coefs, w, h, layout)
    return bits % 8 != 0 and scan.endswith(b"\xff\x00")


def ff_straddles_blocks(coefs, w, h, layout):
    """Whether some 0xFF byte of the scan holds bits of two blocks."""
    from imaginary_amd import codec
    scan, bits = codec.jpeg_scan_bits(coefs, w, h, layout)
    counts = block_bits(coefs, w, h, layout)
    assert sum(counts) == bits
    ends = set(np.cumsum(counts)[:-1].tolist())
    raw = unstuffed(scan)
    return any(b == 0xFF and any(8 * i < e < 8 * i + 8 for e in ends) for i, b in enumerate(raw))
