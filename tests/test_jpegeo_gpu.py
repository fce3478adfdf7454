"""Entropy-coded JPEG output with optimised Huffman tables on the device (MIPX_OP_JPEGE with
a[2] = 1; k_jpege_hist and k_jpege_tables in front of k_jpege.hip's six launches) against
tests/jpegeo_ref.py: a slot's header, its four tables and codec.jpeg_scan with them, the host
writer that tests/test_jpegeo_cpu.py pins to libjpeg-turbo's optimize_coding inside Pillow.  Every
comparison is exact."""
import functools
import io
import os

import numpy as np
import pytest

import jpegeo_ref
import jpegh_ref
from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpegeo_ref import OK, UNCODABLE, check_slot, jpeg_scan_opt_bytes, slot_ref
from test_jpege_gpu import MULTI, SKEWS, _under, pixels

pytestmark = pytest.mark.gpu

# 1 x 1: one MCU, tables of one or two symbols; 17 x 9 and 9 x 17 have dummy Y blocks in 4:2:0; 197 x 117
# is several tiles per image (tests/test_jpege_gpu.py), so several workgroups add into one histogram
SIZES = [(1, 1), (8, 8), (17, 9), (9, 17), (37, 29), (129, 67), MULTI]
LAYOUTS = [YCC_444, YCC_420]
QUALITIES = [1, 50, 90, 100]


@functools.lru_cache(maxsize=None)
def coefficients(w, h, n, layout, quality):
    c = jpegc_ref(pixels(w, h, n), layout, quality)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def slots(w, h, n, layout, quality):
    """The reference slots of coefficients(...), one Slot per image."""
    return tuple(slot_ref(c, w, h, layout) for c in coefficients(w, h, n, layout, quality))


def _check(got, want, w, h, layout, what):
    assert got.dtype == np.uint8 and got.shape == (len(want), jpeg_scan_opt_bytes(w, h, layout)), (what, got.shape)
    for i, s in enumerate(want):
        check_slot(got[i], s, f"{what}, image {i}")


# ---------------------------------------------------------------- the two entry points
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_both_entry_points_equal_the_reference(gpu, layout, n):
    k = 0
    for w, h in SIZES:
        px = pixels(w, h, n)
        for quality in QUALITIES:
            want = slots(w, h, n, layout, quality)
            assert all(s.status == OK for s in want)
            si, so = SKEWS[k % 4]
            k += 1
            what = f"{n}x{h}x{w} layout {layout} Q {quality} skew {si},{so}"
            _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan(px, layout, quality, optimize=True)), want, w, h, layout,
                   "rgb_to_jpeg_scan " + what)
            coefs = coefficients(w, h, n, layout, quality)
            _check(_under(si, so, lambda: gpu.jpegc_to_scan(coefs, w, h, layout, optimize=True)), want, w, h, layout,
                   "jpegc_to_scan " + what)


def test_the_cases_are_what_they_are_for():
    from imaginary_amd import codec
    for layout in LAYOUTS:
        for s in slots(1, 1, 3, layout, 50):
            assert all(1 <= len(t[1]) <= 2 for t in s.tables.values())     # tables of one or two symbols
        assert jpegeo_ref.jpege_ref.scan_blocks(*MULTI, layout) > 2 * jpegeo_ref.jpege_ref.TILE
        assert all(s.tables != codec.HUFFMAN_TABLES for s in slots(37, 29, 3, layout, 90))


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_a_flat_image_has_ac_tables_of_eob_alone(gpu, layout):
    for w, h in [(17, 9), (37, 29)]:
        px = np.empty((2, h, w, 3), np.uint8)
        px[0], px[1] = (200, 100, 50), 0
        want = [slot_ref(c, w, h, layout) for c in jpegc_ref(px, layout, 90)]
        for s in want:
            assert s.status == OK and s.tables[0x10] == s.tables[0x11] == (bytes([1] + [0] * 15), bytes([0]))
        _check(_under(1, 3, lambda: gpu.rgb_to_jpeg_scan(px, layout, 90, optimize=True)), want, w, h, layout, "flat")


# ---------------------------------------------------------------- hand-made coefficients
def test_fibonacci_counts_run_the_limiting_on_the_device(gpu):
    """tests/jpegeo_ref.py fibonacci_coefs: the Y AC table's tree is a chain 20 deep (tests/test_jpegeo_cpu.py
    asserts it), so k_jpege_tables limits it to 16 bits as the library does."""
    c, w, h = jpegeo_ref.fibonacci_coefs()
    want = slot_ref(c, w, h, YCC_444)
    assert want.status == OK and max(k for k, n in enumerate(want.tables[0x10][0], 1) if n) == 16
    got = _under(2, 1, lambda: gpu.jpegc_to_scan(c, w, h, YCC_444, optimize=True))
    _check(got, [want], w, h, YCC_444, "fibonacci counts")
    # and an image of ordinary tables beside it, in either order
    other = jpegc_ref(pixels(w, h, 1), YCC_444, 50)[0]
    pair = [slot_ref(other, w, h, YCC_444), want]
    _check(gpu.jpegc_to_scan(np.stack([other, c]), w, h, YCC_444, optimize=True), pair, w, h, YCC_444, "noise, fibonacci")
    _check(gpu.jpegc_to_scan(np.stack([c, other]), w, h, YCC_444, optimize=True), pair[::-1], w, h, YCC_444, "fibonacci, noise")


# ---------------------------------------------------------------- independence
def _written(slot):
    """The bytes of a slot the interface specifies: header, tables, scan."""
    return slot[:jpegeo_ref.HEADER_BYTES + int(slot[:4].view("<u4")[0])].tobytes()


def test_images_of_a_batch_are_independent_and_runs_repeat(gpu):
    w, h = MULTI
    px = np.stack([pixels(w, h, 3)[0], pixels(w, h, 3)[1], np.full((h, w, 3), 200, np.uint8)])
    px[0, :, :, :] //= 64
    for layout in LAYOUTS:
        want = [slot_ref(c, w, h, layout) for c in jpegc_ref(px, layout, 90)]
        assert len({s.length for s in want}) == 3 and len({s.tables[0x10] for s in want}) == 3
        got = gpu.rgb_to_jpeg_scan(px, layout, 90, optimize=True)
        _check(got, want, w, h, layout, "a batch of three")
        again = gpu.rgb_to_jpeg_scan(px, layout, 90, optimize=True)
        for i in range(3):
            alone = gpu.rgb_to_jpeg_scan(px[i], layout, 90, optimize=True)
            check_slot(alone[0], want[i], f"image {i} alone")
            assert _written(alone[0]) == _written(got[i]) == _written(again[i])


# ---------------------------------------------------------------- inside the slot
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_an_uncodable_coefficient_is_reported_as_todays_step_does(gpu, layout):
    w, h = 37, 29
    c = coefficients(w, h, 3, layout, 90).copy()
    c[1, 64 * 7 + 9] = 1024
    want = [slot_ref(x, w, h, layout) for x in c]
    assert [s.status for s in want] == [OK, UNCODABLE, OK]
    got = _under(1, 3, lambda: gpu.jpegc_to_scan(c, w, h, layout, optimize=True))
    _check(got, want, w, h, layout, "uncodable")
    assert got[1][:8].view("<u4").tolist() == [0, UNCODABLE]
    assert gpu.jpegc_to_scan(c, w, h, layout)[1][:8].view("<u4").tolist() == [0, UNCODABLE]   # today's step
    assert gpu.scan_slot(got[1], tables=True) == (UNCODABLE, int(got[1][8:12].view("<u4")[0]), b"", None)


def test_near_capacity_scans_stay_inside_the_slot(gpu):
    """The inputs that overflow today's step (tests/jpege_ref.py: every AC +-1023, and every AC 127) do not
    overflow this one: with one AC symbol in the image its code is one bit, so a coefficient costs 11
    or 8 bits of its 16, and a byte of eight 1-bits needs more than one coefficient's value.  The
    first fills more than three quarters of its slot.  No input is known that overflows with these
    tables, so the OVERFLOW status, which the same kernels report as for today's step, is not reached
    here; the guard bands around the slots are checked by the wrapper."""
    w = h = 16
    for layout in LAYOUTS:
        cap = jpegc_bytes(w, h, layout)
        c = coefficients(w, h, 3, layout, 90).copy()
        c[1] = np.where(np.arange(c.shape[1]) % 2 == 0, 1023, -1023)
        c[1, ::64] = 0
        c[2] = 127
        c[2, ::64] = 0
        today = gpu.jpegc_to_scan(c, w, h, layout)
        assert [int(s[4:8].view("<u4")[0]) for s in today] == [0, 1, 1]                 # OVERFLOW there
        want = [slot_ref(x, w, h, layout) for x in c]
        assert [s.status for s in want] == [OK, OK, OK] and 3 * cap // 4 < want[1].length <= cap
        assert cap // 3 < want[2].length <= cap
        for si, so in [(0, 0), (1, 3), (3, 2)]:
            _check(_under(si, so, lambda: gpu.jpegc_to_scan(c, w, h, layout, optimize=True)), want, w, h, layout,
                   f"near capacity, layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_under_every_pointer_alignment(gpu, layout):
    for w, h in [(8, 8), (37, 29)]:
        px, coefs, want = pixels(w, h, 3), coefficients(w, h, 3, layout, 90), slots(w, h, 3, layout, 90)
        for si in range(4):
            for so in range(4):
                what = f"3x{h}x{w} layout {layout} skew {si},{so}"
                _check(_under(si, so, lambda: gpu.jpegc_to_scan(coefs, w, h, layout, optimize=True)), want, w, h, layout, what)
                _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan(px, layout, 90, optimize=True)), want, w, h, layout, what)


# ---------------------------------------------------------------- round trip on the device
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_the_decoder_reads_the_slot_back(gpu, layout):
    """The tables and the scan of an optimised slot, copied into a MIPX_OP_JPEGH slot (bytes 16..1103
    to 416..1503), decode to exactly the coefficients that went in."""
    for w, h, quality in [(37, 29, 90), MULTI + (50,)]:
        coefs = coefficients(w, h, 3, layout, quality)
        out = gpu.jpegc_to_scan(coefs, w, h, layout, optimize=True)
        back = np.zeros((3, jpegh_ref.jpegh_bytes(w, h, layout)), np.uint8)
        for i in range(3):
            length = int(out[i][:4].view("<u4")[0])
            assert out[i][4:8].view("<u4")[0] == OK
            back[i, 0:4] = out[i][0:4]
            back[i, 16:400] = np.ones(192, "<u2").view(np.uint8)
            back[i, 400:406] = [0, 1, 1, 0, 1, 1]
            back[i, 416:1504] = out[i][16:1104]
            back[i, 1504:1504 + length] = out[i][1104:1104 + length]
        payloads, status = gpu.jpegh_to_jpegd(back, w, h, layout)
        assert status.tolist() == [jpegh_ref.OK] * 3
        assert np.array_equal(payloads[:, 384:].view(np.int16), coefs)


# ---------------------------------------------------------------- as the last step of a plan, and the request path
def _plan(gpu, w, h, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


@pytest.mark.parametrize("layout,quality", [(YCC_444, 92), (YCC_420, 75)], ids=["444", "420"])
def test_plan_with_the_step_equals_the_reference_on_the_plans_rgb(gpu, layout, quality):
    src = pixels(128, 96, 2)
    p = _plan(gpu, 128, 96, width=60)
    rgb = gpu.execute(p, src, junk=0x3C)
    want = [slot_ref(c, p.out_w, p.out_h, layout) for c in jpegc_ref(rgb, layout, quality)]
    q = gpu.plan_set_jpeg_scan_output(_plan(gpu, 128, 96, width=60), layout, quality, optimize=True)
    _check(gpu.execute(q, src, junk=0x3C), want, p.out_w, p.out_h, layout, "plan")
    s0 = _plan(gpu, 128, 96, width=64)
    last = gpu.plan_set_jpeg_scan_output(_plan(gpu, s0.out_w, s0.out_h, width=40), layout, quality, optimize=True)
    chain = gpu.plan_chain([s0, last])
    plain = gpu.plan_chain([s0, _plan(gpu, s0.out_w, s0.out_h, width=40)])
    rgb = gpu.execute(plain, src)
    want = [slot_ref(c, chain.out_w, chain.out_h, layout) for c in jpegc_ref(rgb, layout, quality)]
    _check(gpu.execute(chain, src, junk=0xC3), want, chain.out_w, chain.out_h, layout, "chain")


def test_request_path_gives_whole_slots(gpu):
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        subs = []
        w, h, layout, quality = 37, 29, YCC_420, 75
        p = _plan(gpu, w, h, width=24)
        q = gpu.plan_set_jpeg_scan_output(_plan(gpu, w, h, width=24), layout, quality, optimize=True)
        for im in pixels(w, h, 3):
            want = slot_ref(jpegc_ref(eng.process(p, im)[None], layout, quality)[0], p.out_w, p.out_h, layout)
            subs.append((eng.submit(q, im), want))
        for (ticket, out), want in subs:
            eng.wait(ticket)
            assert out.dtype == np.uint8 and out.shape == (jpeg_scan_opt_bytes(p.out_w, p.out_h, layout),)
            check_slot(out, want, "request")
            assert gpu.scan_slot(out, tables=True) == (OK, want.bits, want.scan, want.tables)
        with pytest.raises(ValueError):     # the Annex K slot's size is refused by the wrapper
            eng.submit(q, im, out=np.zeros(out.size - 1088, np.uint8))
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
def _dhts(buf):
    out, i = {}, 2
    while buf[i + 1] != 0xDA:
        n = int.from_bytes(buf[i + 2:i + 4], "big")
        if buf[i + 1] == 0xC4:
            out[buf[i + 4]] = (bytes(buf[i + 5:i + 21]), bytes(buf[i + 21:i + 2 + n]))
        i += 2 + n
    return out


@pytest.mark.parametrize("quality", [80, 95])
def test_process_bytes_writes_a_smaller_file_of_the_same_pixels(gpu, quality):
    PIL = pytest.importorskip("PIL.Image")
    from imaginary_amd import codec, imaginary
    buf = open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read()
    opts = dict(width=300, quality=quality)
    plain = imaginary.process_bytes(buf, opts, jpeg_scan=True)
    got = imaginary.process_bytes(buf, opts, jpeg_scan=True, jpeg_optimize=True)
    assert got.mime == "image/jpeg" and _dhts(plain.body) == codec.HUFFMAN_TABLES
    mine = _dhts(got.body)
    assert set(mine) == set(codec.HUFFMAN_TABLES) and all(mine[tc] != codec.HUFFMAN_TABLES[tc] for tc in mine)
    a, b = PIL.open(io.BytesIO(got.body)), PIL.open(io.BytesIO(plain.body))
    assert a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b))
    assert len(got.body) <= len(plain.body)
    # the file is the one libjpeg writes of the same coefficients with optimize_coding
    payload, layout = codec.decode_jpeg_coefs(got.body)
    coefs = payload[384:].view(np.int16)
    assert got.body == codec.encode_jpeg_coefs(coefs, a.size[0], a.size[1], layout, quality, tables="optimal")
    # the keyword alone does nothing
    assert imaginary.process_bytes(buf, opts, jpeg_optimize=True).body == imaginary.process_bytes(buf, opts).body


def test_process_falls_back_to_coefficients_when_the_plan_refuses_the_step(gpu, monkeypatch):
    """What a result of 10^9 / 64 scan blocks or more gets from mipx_plan_set_jpeg_scan_output_optimized,
    MIPX_EINVAL, without an image of that size: the request runs with the coefficient step, as for a
    slot that is not OK."""
    from imaginary_amd import _abi, imaginary
    real = imaginary.plan_set_jpeg_scan_output

    def refusing(plan, layout, quality, optimize=False):
        if optimize:
            raise _abi.MipxError(_abi.MIPX_EINVAL, "mipx_plan_set_jpeg_scan_output_optimized")
        return real(plan, layout, quality)

    px = pixels(64, 48, 1)[0]
    src = imaginary.Decoded(px, "png", 0)
    want = imaginary.process(src, dict(width=32), jpeg_quality=75)
    monkeypatch.setattr(imaginary, "plan_set_jpeg_scan_output", refusing)
    out = imaginary.process(src, dict(width=32), jpeg_quality=75, jpeg_scan=True, jpeg_optimize=True)
    assert isinstance(out, imaginary.JpegCoefs) and np.array_equal(out.coefs, want.coefs)
    plain = imaginary.process(src, dict(width=32), jpeg_quality=75, jpeg_scan=True)
    assert isinstance(plain, imaginary.JpegScan) and plain.tables is None
