"""The reference of entropy-coded JPEG output with optimised Huffman tables (MIPX_OP_JPEGE with
a[2] = 1, PARITY_ASSUMPTIONS.md row 24): one output slot is a 16-byte header (length, status, bits,
1), the four tables codec.jpeg_optimal_table makes of codec.jpeg_symbol_counts, 272 bytes each in
the order DC 0, DC 1, AC 0, AC 1, and codec.jpeg_scan with those tables.  tests/test_jpegeo_cpu.py
pins that writer to libjpeg-turbo's optimize_coding inside Pillow, byte for byte.  Also the sizes
include/mipx.h states in words, the pictures of the tests, and the hand-made coefficients whose
symbol counts are Fibonacci numbers."""
import functools

import numpy as np

import jpege_ref
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref  # noqa: F401
from jpege_ref import OK, OVERFLOW, UNCODABLE  # noqa: F401

HEADER_BYTES = 1104        # MIPX_JPEG_SCAN_OPT_HEADER_BYTES: 16 + 4 * 272
TABLE_BYTES = 272
SLOT_TABLES = (0x00, 0x01, 0x10, 0x11)   # the slot's order by DHT Tc/Th byte: DC 0, DC 1, AC 0, AC 1


def jpeg_scan_opt_bytes(w, h, layout):
    """mipx_jpeg_scan_opt_bytes: the header with the tables, and the capacity."""
    n = jpegc_bytes(w, h, layout)
    return HEADER_BYTES + n if n else 0


def workspace_bytes(n, w, h):
    """mipx_op_workspace_bytes(MIPX_OP_JPEGE, n, w, h, 3, 1.0, 0): the Annex K step's, then per image
    4 x 256 uint32 symbol counts and as many codes."""
    return jpege_ref.workspace_bytes(n, w, h) + 2 * n * 4 * 256 * 4


def optimal_tables(coefs, w, h, layout):
    from imaginary_amd import codec
    return {tc: codec.jpeg_optimal_table(f) for tc, f in codec.jpeg_symbol_counts(coefs, w, h, layout).items()}


def table_bytes(table):
    """One table as the slot holds it: 16 counts, the symbols, zeros up to 272 bytes."""
    counts, symbols = table
    out = np.zeros(TABLE_BYTES, np.uint8)
    out[:16] = np.frombuffer(bytes(counts), np.uint8)
    out[16:16 + len(symbols)] = np.frombuffer(bytes(symbols), np.uint8)
    return out


class Slot(jpege_ref.Slot):
    """What one image's slot must hold: the header, and for status OK the tables and the scan."""

    def __init__(self, length, status, bits, scan, tables):
        super().__init__(length, status, bits, scan)
        self.tables = tables

    def header(self):
        return np.array([self.length, self.status, self.bits, 1], "<u4")


def slot_ref(coefs, w, h, layout):
    from imaginary_amd import codec
    cap = jpegc_bytes(w, h, layout)
    try:
        tables = optimal_tables(coefs, w, h, layout)
        scan, bits = codec.jpeg_scan_bits(coefs, w, h, layout, tables)
    except ValueError:
        return Slot(0, UNCODABLE, None, b"", None)
    if len(scan) > cap:
        return Slot(-(-bits // 8), OVERFLOW, bits, b"", None)
    return Slot(len(scan), OK, bits, scan, tables)


def check_slot(got, want, what):
    """A downloaded slot (uint8) against its Slot: the header, the four tables, the scan."""
    got = np.ascontiguousarray(got, dtype=np.uint8).ravel()
    head = got[:16].view("<u4")
    if want.bits is None:
        assert head[0] == 0 and head[1] == want.status and head[3] == 1, (what, head.tolist())
        return
    assert head.tolist() == want.header().tolist(), f"{what}: header {head.tolist()}, want {want.header().tolist()}"
    if want.status != OK:
        return
    for k, tc in enumerate(SLOT_TABLES):
        t = got[16 + TABLE_BYTES * k:16 + TABLE_BYTES * (k + 1)]
        ref = table_bytes(want.tables[tc])
        assert np.array_equal(t, ref), (f"{what}: table {tc:#04x}: counts {t[:16].tolist()} want {ref[:16].tolist()}, "
                                        f"symbols {t[16:16 + int(ref[:16].sum())].tolist()} want "
                                        f"{ref[16:16 + int(ref[:16].sum())].tolist()}")
    assert HEADER_BYTES + want.length <= got.size, (what, want.length, got.size)
    data = got[HEADER_BYTES:HEADER_BYTES + want.length].tobytes()
    if data != want.scan:
        at = next(i for i in range(want.length) if data[i] != want.scan[i])
        raise AssertionError(f"{what}: {want.length} scan bytes, the first difference at byte {at}: "
                             f"got {data[at:at + 8].hex()} want {want.scan[at:at + 8].hex()}")


# ---- the pictures of the library pin ----------------------------------------------------------
PIN_SIZES = [(1, 1), (8, 8), (17, 9), (37, 29), (64, 48), (129, 67), (200, 120)]
PIN_QUALITIES = [1, 30, 75, 92, 100]
PICTURES = ["noise", "smooth", "flat"]


@functools.lru_cache(maxsize=None)
def picture(kind, w, h):
    """(h, w, 3) uint8, read-only: full-range noise, a smooth picture (ramps under a slow wave), a flat one."""
    if kind == "noise":
        px = np.random.default_rng(w * 100003 + h * 101).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "smooth":
        x, y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
        px = np.stack([127 + 120 * np.sin(x / 9.0) * np.cos(y / 7.0), x * 255 / max(w - 1, 1), (x + y) * 255 / max(w + h - 2, 1)],
                      -1).astype(np.uint8)
    else:
        px = np.empty((h, w, 3), np.uint8)
        px[:] = (200, 100, 50)
    px.setflags(write=False)
    return px


# ---- Fibonacci counts ---------------------------------------------------------------------------
# The Fibonacci numbers from the second 1 on: 1, 2, 3, 5, 8 ...  With the reserved point's 1 the two
# least are 1 and 1, then 2 and 2, and from there the merged node (the sum so far, F(k+3) - 1) and the
# next number are always the two least, strictly: the tree is a chain, k symbols reach a raw length of
# k, and no tie is left to the tie-break.  (With both 1s of the sequence the sums tie with the numbers
# and the library's tie-break halves the depth.)
def fibonacci(k):
    f = [1, 2]
    while len(f) < k:
        f.append(f[-1] + f[-2])
    return f[:k]


def fibonacci_histogram(k=30):
    """256 counts: the first k of the symbols run << 4 | size, sizes 1 to 10 and per size the runs 0 to
    15, hold fibonacci(k); k <= 160."""
    syms = [(r << 4) | s for s in range(1, 11) for r in range(16)][:k]
    freq = [0] * 256
    for s, f in zip(syms, fibonacci(k)):
        freq[s] = f
    return freq


FIB_DEVICE_SYMBOLS = 20  # 1 .. 10946, 28655 in all: raw lengths up to 20


@functools.lru_cache(maxsize=None)
def fibonacci_coefs():
    """(coefs, w, h): a 4:4:4 image whose Y AC symbol counts are the first FIB_DEVICE_SYMBOLS numbers of
    fibonacci(): EOB 610 times, once per Y block (no block codes coefficient 63), the other 19 over the
    symbols (run r, size s), r < 3 and s < 9, the large counts on the runs of 0.  They cost 28,795
    coefficients at r + 1 each, which at the 62 a block holds in front of its EOB need 465 blocks: 610
    is the least of the numbers that is enough, so 61 x 10 blocks is the smallest image.  Cb, Cr and
    every DC are zero."""
    from imaginary_amd import codec
    fib = fibonacci(FIB_DEVICE_SYMBOLS)
    blocks, wb, hb = 610, 61, 10
    assert blocks in fib
    syms = sorted((r, s) for s in range(1, 9) for r in (0, 1, 2))[:FIB_DEVICE_SYMBOLS - 1]
    todo = []
    for (r, s), f in zip(syms, sorted((f for f in fib if f != blocks), reverse=True)):
        todo += [(r, s)] * f
    assert sum(r + 1 for r, _ in todo) <= 62 * blocks
    c = np.zeros((3, blocks, 64), np.int16)
    b, k = 0, 1
    for i, (r, s) in enumerate(todo):
        if k + r > 62:
            b, k = b + 1, 1
        k += r
        c[0, b, codec.ZIGZAG[k]] = (1 << s) - 1 if i % 2 else -((1 << s) - 1)
        k += 1
    assert b < blocks
    c = c.reshape(-1)
    c.setflags(write=False)
    return c, 8 * wb, 8 * hb
