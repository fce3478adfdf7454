"""Restart intervals in the entropy-coded JPEG input, without a device: the model of
tests/jpegr_ref.py against codec.decode_jpeg_coefs on Pillow-written files, codec.jpeg_huff_slot's
`restart` option against the tests' own slot builder, the files that stay ordinary scans, and the
damage table."""
import numpy as np
import pytest

import jpegh_ref
import jpegr_ref
from jpegc_ref import YCC_420, YCC_444
from jpegh_ref import BAD, HEADER_BYTES, OK
from jpegr_ref import SIZES, mcus, restart_file

PIL = pytest.importorskip("PIL.Image")
LAYOUTS = [YCC_444, YCC_420]


def _intervals(w, h, layout):
    """The restart_marker_blocks of the matrix: 1, 2, 7, 8, one row, all but one MCU."""
    mw, mh = mcus(w, h, layout)
    return sorted({1, 2, 7, 8, mw, mw * mh - 1} - {0})


def _cases(w, h, layout):
    """(quality, optimize, blocks, rows) of one size: every interval at Q 50 with Annex K's tables, the
    other qualities and the optimised tables on a rotating one of them, one MCU row by rows=."""
    ris = _intervals(w, h, layout)
    out = [(50, False, ri, 0) for ri in ris]
    for j, (quality, optimize) in enumerate([(1, False), (100, False), (1, True), (50, True), (100, True)]):
        out.append((quality, optimize, ris[(j + w) % len(ris)], 0))
    out.append((50, False, 0, 1))
    return out


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_the_model_decodes_restart_files_to_what_the_host_decoder_gives(layout, size):
    w, h = size
    mw, mh = mcus(w, h, layout)
    for quality, optimize, blocks, rows in _cases(w, h, layout):
        buf, slot, payload = restart_file(w, h, layout, quality, optimize, blocks, rows)
        ri = blocks or rows * mw
        assert b"\xff\xdd\x00\x04" + ri.to_bytes(2, "big") in buf, (size, blocks, rows)      # DRI
        assert jpegr_ref.restart_of(slot) == ri
        scan = jpegr_ref.slot_scan(slot)
        if ri < mw * mh:
            assert b"\xff\xd0" in scan and jpegr_ref.intervals(slot, w, h, layout) == -(-mw * mh // ri)
            assert len(jpegr_ref.split(scan)[1]) == -(-mw * mh // ri) - 1
        status, got = jpegr_ref.decode_slot(slot, w, h, layout)
        assert status == OK and np.array_equal(got, payload), (size, layout, quality, optimize, blocks, rows)


def test_the_marker_numbers_wrap():
    for layout, count in ((YCC_444, 375), (YCC_420, 104)):
        _, slot, _ = restart_file(197, 117, layout, 50, False, 1)
        scan = jpegr_ref.slot_scan(slot)
        assert jpegr_ref.intervals(slot, 197, 117, layout) == count
        d7 = scan.index(b"\xff\xd7")
        assert scan.index(b"\xff\xd0", d7) > d7                 # a D0 behind a D7
        marks = jpegr_ref.split(scan)[1]
        assert marks == [0xD0 + (k & 7) for k in range(count - 1)]


# ---------------------------------------------------------------- the slot builder
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_jpeg_huff_slot_takes_restart_files_when_asked(layout):
    from imaginary_amd import codec
    for w, h in SIZES:
        mw, mh = mcus(w, h, layout)
        for blocks in (1, 7, mw, mw * mh - 1):
            buf, slot, _ = restart_file(w, h, layout, 50, blocks == 7, blocks)
            assert codec.jpeg_huff_slot(buf) is None and codec.jpeg_huff_slot(buf, restart=False) is None
            got, l2 = codec.jpeg_huff_slot(buf, restart=True)
            assert l2 == layout and got.dtype == np.uint8 and np.array_equal(got, slot)
            assert int(got[4:8].view("<u4")[0]) == blocks and not got[8:16].any()
            if blocks < mw * mh:
                assert b"\xff\xd0" in got[HEADER_BYTES:].tobytes()
        # a file without a restart interval: the same slot either way, the header word 0
        buf, _, _ = restart_file(w, h, layout, 50, False)
        a, b, c = codec.jpeg_huff_slot(buf), codec.jpeg_huff_slot(buf, restart=False), codec.jpeg_huff_slot(buf, restart=True)
        assert a[1] == b[1] == c[1] == layout and np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
        assert not a[0][4:16].any()
        assert np.array_equal(a[0], jpegr_ref.file_slot(buf, layout))


def test_jpeg_huff_slot_with_restart_declines_what_it_declined():
    import io
    from imaginary_amd import codec
    rgb = PIL.fromarray(jpegr_ref.pixels(32, 24)[0])

    def save(im, **kw):
        b = io.BytesIO()
        im.save(b, "JPEG", restart_marker_blocks=2, **kw)
        return b.getvalue()

    whole = save(rgb, quality=92)
    assert codec.jpeg_huff_slot(whole, restart=True) is not None
    assert codec.jpeg_huff_slot(save(rgb, quality=92, progressive=True), restart=True) is None
    assert codec.jpeg_huff_slot(save(rgb.convert("L"), quality=92), restart=True) is None
    assert codec.jpeg_huff_slot(save(rgb, quality=92, subsampling=1), restart=True) is None
    assert codec.jpeg_huff_slot(save(rgb.convert("CMYK"), quality=92), restart=True) is None
    scan = whole.index(b"\xff\xda")
    for cut in (scan + 14 + (len(whole) - scan - 14) // 2, len(whole) - 2, scan + 4):
        assert codec.jpeg_huff_slot(whole[:cut], restart=True) is None                       # truncated
    for buf in (b"", b"\xff\xd8\xff not a jpeg", np.random.default_rng(9).integers(0, 256, 4096, dtype=np.uint8).tobytes()):
        assert codec.jpeg_huff_slot(buf, restart=True) is None
    # Huffman tables 2 and 3: no room in the slot
    moved = bytearray(whole)
    p = 2
    while moved[p + 1] != 0xDA:
        size = int.from_bytes(moved[p + 2:p + 4], "big")
        if moved[p + 1] == 0xC4 and moved[p + 4] in (0x01, 0x11):
            moved[p + 4] += 1
        p += 2 + size
    moved[p + 8] = moved[p + 10] = 0x22
    assert codec.decode_jpeg_coefs(bytes(moved)) is not None and codec.jpeg_huff_slot(bytes(moved), restart=True) is None
    # damaged files: whatever it returns, it does not raise
    rng = np.random.default_rng(11)
    for _ in range(40):
        bad = bytearray(whole)
        for at in rng.integers(2, len(whole), 3):
            bad[at] = rng.integers(0, 256)
        got = codec.jpeg_huff_slot(bytes(bad), restart=True)
        assert got is None or (got[0].dtype == np.uint8 and got[0].ndim == 1 and got[1] in (YCC_444, YCC_420))


# ---------------------------------------------------------------- one interval: the ordinary scan
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_an_interval_of_all_mcus_or_more_is_an_ordinary_scan(layout):
    from imaginary_amd import codec
    w, h = 37, 29
    mw, mh = mcus(w, h, layout)
    plain = restart_file(w, h, layout, 50, False)
    for blocks in (mw * mh, mw * mh + 5):
        buf, slot, payload = restart_file(w, h, layout, 50, False, blocks)
        assert jpegr_ref.restart_of(slot) == blocks and jpegr_ref.intervals(slot, w, h, layout) == 0
        assert np.array_equal(codec.jpeg_huff_slot(buf, restart=True)[0], slot)
        assert b"\xff\xd0" not in jpegr_ref.slot_scan(slot) and jpegr_ref.slot_scan(slot) == jpegr_ref.slot_scan(plain[1])
        status, got = jpegr_ref.decode_slot(slot, w, h, layout)
        assert status == OK and np.array_equal(got, payload) and np.array_equal(got, plain[2])
        assert jpegh_ref.decode_slot(slot, w, h, layout)[0] == OK
        # an FF D0 in such a scan stays BAD
        scan = jpegr_ref.slot_scan(slot)
        spliced = jpegr_ref.with_scan(slot, w, h, layout, scan[:len(scan) // 3] + b"\xff\xd0" + scan[len(scan) // 3:])
        assert jpegr_ref.decode_slot(spliced, w, h, layout)[0] == BAD


# ---------------------------------------------------------------- damage
DAMAGE_W, DAMAGE_H, DAMAGE_RI = 129, 67, 3
# what codec.decode_jpeg_coefs, the stand-in for libjpeg, takes although the model says BAD
HOST_TAKES = {"marker 1 with the next number"}
NO_FILE = {"Ri 65536"}     # DRI holds 16 bits


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_the_damage_table_is_bad_in_the_model_and_declined_by_the_host_decoder(layout):
    """Each entry is BAD in the model, and codec.decode_jpeg_coefs returns None for the same change made
    to the file.  The two differ on one entry, legitimately: a marker with the wrong number.  The host
    decoder cuts the scan at every FF D0..D7 without looking at the number, and libjpeg itself answers
    an out-of-sequence marker with a resynchronisation heuristic (jdmarker.c, jpeg_resync_to_restart)
    and a warning, not an error; the engine reports BAD and the file is decoded on the host
    (PARITY_ASSUMPTIONS.md).  Ri = 65536 has no file: DRI holds 16 bits."""
    from imaginary_amd import codec
    w, h = DAMAGE_W, DAMAGE_H
    buf, slot, payload = restart_file(w, h, layout, 90, False, DAMAGE_RI)
    assert jpegr_ref.decode_slot(slot, w, h, layout)[0] == OK
    assert codec.decode_jpeg_coefs(jpegr_ref.as_file(buf, slot))[0].tobytes() == payload.tobytes()
    table = jpegr_ref.damaged(slot, w, h, layout)
    assert set(table) == {"marker 1 with the next number", "marker 1 removed", "marker 1 twice", "FF D8 inside", "FF last",
                          "Ri one more", "Ri one less", "Ri 65536", "marker 0 three bytes early"}
    for name, bad in table.items():
        assert jpegr_ref.decode_slot(bad, w, h, layout) == (BAD, None), name
        if name in NO_FILE:
            continue
        host = codec.decode_jpeg_coefs(jpegr_ref.as_file(buf, bad))
        assert (host is not None) == (name in HOST_TAKES), name
