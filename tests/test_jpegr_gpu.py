"""Restart intervals in the entropy-coded JPEG input on the device (MIPX_OP_JPEGH with the slot's
`restart` word, k_jpegr_index / k_jpegr_decode in k_jpegh.hip): the decoder alone against the model
of tests/jpegr_ref.py and against codec.decode_jpeg_coefs on Pillow-written files, batches that mix
both kinds of slot, the damage table, then the calls to pixels, a plan, the request path and
process_bytes.  Every comparison is exact; the guard bands of every buffer are live."""
import io
import os

import numpy as np
import pytest

import jpegr_ref
from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import YCC_420, YCC_444
from jpegh_ref import BAD, OK
from jpegr_ref import mcus, restart_file
from test_jpegh_gpu import PH, PW, SKEWS, _decode, _plan_pair, _same, _under, pixels

pytestmark = pytest.mark.gpu
LAYOUTS = [YCC_444, YCC_420]

# (w, h, layout, quality, optimize, restart_marker_blocks, restart_marker_rows, images)
CASES = [
    (197, 117, YCC_444, 50, False, 1, 0, 3),    # 375 intervals: two workgroups, the second partial
    (197, 117, YCC_420, 50, False, 1, 0, 1),    # 104 intervals: the marker numbers wrap 13 times
    (17, 9, YCC_420, 50, False, 1, 0, 3),       # dummy blocks: a dummy Y row
    (9, 17, YCC_420, 90, False, 1, 0, 3),       # a dummy Y column
    (17, 9, YCC_444, 50, False, 2, 0, 1),
    (9, 17, YCC_444, 100, False, 1, 0, 3),
    (33, 17, YCC_444, 50, False, 5, 0, 3),      # Ri = mw: one row
    (37, 29, YCC_420, 50, False, 3, 0, 1),      # Ri = mw
    (197, 117, YCC_420, 90, False, 0, 1, 1),    # one row by restart_marker_rows
    (37, 29, YCC_444, 50, False, 0, 1, 3),
    (37, 29, YCC_444, 50, False, 19, 0, 3),     # Ri = M - 1: the last interval is one MCU
    (33, 17, YCC_420, 50, False, 5, 0, 1),      # Ri = M - 1
    (37, 29, YCC_444, 50, False, 20, 0, 3),     # Ri = M: the ordinary path, the header word not 0
    (37, 29, YCC_420, 50, False, 11, 0, 1),     # Ri > M
    (197, 117, YCC_444, 100, True, 7, 0, 1),    # optimised tables
    (37, 29, YCC_420, 1, True, 2, 0, 3),
    (33, 17, YCC_444, 50, True, 8, 0, 3),
    (37, 29, YCC_444, 1, False, 7, 0, 3),
    (197, 117, YCC_420, 100, False, 8, 0, 1),
    (33, 17, YCC_420, 100, True, 1, 0, 3),
    (37, 29, YCC_444, 100, False, 2, 0, 1),
    (129, 67, YCC_444, 90, False, 3, 0, 3),
    (129, 67, YCC_420, 90, False, 3, 0, 3),
]


def _id(case):
    w, h, layout, quality, optimize, blocks, rows, n = case
    return f"{w}x{h}-{'444' if layout == YCC_444 else '420'}-q{quality}{'-opt' if optimize else ''}-{'r%d' % rows if rows else blocks}-n{n}"


def test_the_pixels_are_the_ones_of_the_ordinary_tests():
    assert np.array_equal(pixels(37, 29), jpegr_ref.pixels(37, 29))


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_the_decoder_equals_the_model_and_the_host_decoder_on_restart_files(gpu, case):
    pytest.importorskip("PIL.Image")
    w, h, layout, quality, optimize, blocks, rows, n = case
    k = CASES.index(case)
    mw, mh = mcus(w, h, layout)
    f = [restart_file(w, h, layout, quality, optimize, blocks, rows, i) for i in range(n)]
    ri = blocks or rows * mw
    for _, slot, payload in f:
        assert jpegr_ref.restart_of(slot) == ri
        assert jpegr_ref.intervals(slot, w, h, layout) == (-(-mw * mh // ri) if ri < mw * mh else 0)
        status, want = jpegr_ref.decode_slot(slot, w, h, layout)
        assert status == OK and np.array_equal(want, payload)
    for m in sorted({1, n}):
        skews = SKEWS[(k + m) % 4]
        got, status = _decode(gpu, [s for _, s, _ in f[:m]], w, h, layout, skews)
        assert status == [OK] * m, (case, status)
        for i in range(m):
            _same(got[i], f[i][2], f"{_id(case)} skew {skews}, image {i} of {m}")


# ---------------------------------------------------------------- both kinds of slot in one call
def _spliced(slot, w, h, layout):
    scan = jpegr_ref.slot_scan(slot)
    return jpegr_ref.with_scan(slot, w, h, layout, scan[:len(scan) // 3] + b"\xff\xd0" + scan[len(scan) // 3:])


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_a_batch_mixes_ordinary_and_restart_slots(gpu, layout):
    pytest.importorskip("PIL.Image")
    w, h = 129, 67
    plain = [restart_file(w, h, layout, 90, False, 0, 0, i) for i in range(2)]
    three = restart_file(w, h, layout, 90, False, 3, 0, 1)
    one = restart_file(w, h, layout, 50, True, 1, 0, 2)
    damaged = jpegr_ref.damaged(restart_file(w, h, layout, 90, False, 3, 0, 0)[1], w, h, layout)["marker 1 removed"]
    slots = [plain[0][1], three[1], damaged, _spliced(plain[1][1], w, h, layout), one[1]]
    assert [jpegr_ref.restart_of(s) for s in slots] == [0, 3, 3, 0, 1]
    want = [jpegr_ref.decode_slot(s, w, h, layout) for s in slots]
    assert [s for s, _ in want] == [OK, OK, BAD, BAD, OK]
    for skews in (SKEWS[1], SKEWS[2]):
        got, status = _decode(gpu, slots, w, h, layout, skews)
        assert status == [s for s, _ in want], status
        for i, host in ((0, plain[0][2]), (1, three[2]), (4, one[2])):
            _same(got[i], want[i][1], f"slot {i} against the model")
            _same(got[i], host, f"slot {i} against the host decoder")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_damaged_restart_slots_are_bad_and_the_neighbours_stay_exact(gpu, layout):
    pytest.importorskip("PIL.Image")
    w, h = 129, 67
    good = [restart_file(w, h, layout, 90, False, 3, 0, 1), restart_file(w, h, layout, 90, False, 0, 0, 2)]
    table = jpegr_ref.damaged(restart_file(w, h, layout, 90, False, 3, 0, 0)[1], w, h, layout)
    assert len(table) == 9
    for k, (name, slot) in enumerate(table.items()):
        want, _ = jpegr_ref.decode_slot(slot, w, h, layout)
        assert want == BAD, name
        first, last = good[k % 2], good[(k + 1) % 2]       # a restart slot and an ordinary one, in turn
        got, status = _decode(gpu, [first[1], slot, last[1]], w, h, layout, SKEWS[k % 4])
        assert status == [OK, want, OK], (name, status)
        _same(got[0], first[2], f"{name}: the image before")
        _same(got[2], last[2], f"{name}: the image behind")


# ---------------------------------------------------------------- through the layers
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_restart_slots_to_pixels_and_through_a_plan(gpu, layout):
    pytest.importorskip("PIL.Image")
    f = [restart_file(PW, PH, layout, 90, False, 3, 0, i) for i in range(3)]
    slots, payloads = np.stack([s for _, s, _ in f]), np.stack([p for _, _, p in f])
    got, status = _under(1, 3, lambda: gpu.jpegh_to_rgb(slots, PW, PH, layout))
    assert status.tolist() == [OK] * 3
    _same(got, gpu.jpegd_to_rgb(payloads, PW, PH, layout), "full size")
    for k, shrink in enumerate((2, 8)):
        got, status = _under(*SKEWS[k + 2], lambda: gpu.jpegh_to_rgb_scaled(slots, PW, PH, layout, shrink))
        assert status.tolist() == [OK] * 3
        _same(got, gpu.jpegd_to_rgb_scaled(payloads, PW, PH, layout, shrink), f"at 1/{shrink}")
    for k, shrink in enumerate((1, 4)):
        pd, ph = _plan_pair(gpu, layout, shrink, "resize")
        want = gpu.execute(pd, payloads)
        got = _under(*SKEWS[k + 1], lambda: gpu.execute(ph, slots, junk=0x3C))
        assert gpu.execute_status().tolist() == [OK] * 3
        _same(got, want, f"a plan at 1/{shrink}")


def test_the_request_path_batches_ordinary_and_restart_slots(gpu):
    pytest.importorskip("PIL.Image")
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        for layout, shrink in [(YCC_420, 1), (YCC_444, 2)]:
            pd, ph = _plan_pair(gpu, layout, shrink, "resize")
            f = [restart_file(PW, PH, layout, 90, False, 2 * (i % 2), 0, i % 3) for i in range(8)]
            assert [jpegr_ref.restart_of(s) for _, s, _ in f] == [0, 2] * 4
            want = [eng.process(pd, p) for _, _, p in f]
            outs = [np.full((ph.out_h, ph.out_w, 3), 0x5A, np.uint8) for _ in f]
            tickets = [eng.submit(ph, s, out=o)[0] for (_, s, _), o in zip(f, outs)]
            for t in tickets:
                eng.wait(t)          # MIPX_EDATA would raise
            for i in range(8):
                _same(outs[i], want[i], f"layout {layout} at 1/{shrink}, request {i}")
    finally:
        eng.shutdown()


def test_process_bytes_takes_a_restart_file_as_its_scan(gpu, monkeypatch):
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from imaginary_amd import codec, imaginary
    buf = open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read()
    b = io.BytesIO()
    Image.open(io.BytesIO(buf)).save(b, "JPEG", quality=85, restart_marker_blocks=4)
    restart = b.getvalue()
    assert codec.jpeg_huff_slot(restart) is None and codec.jpeg_huff_slot(restart, restart=True) is not None
    hdr = codec.header(restart)
    calls = []
    real = codec.decode_jpeg_coefs
    monkeypatch.setattr(codec, "decode_jpeg_coefs", lambda data: calls.append(1) or real(data))
    # a full-size decode without and with jpeg_dct_shrink, and a shrink-on-load one
    for opts, shrink in ((dict(width=hdr.w - 8), False), (dict(width=hdr.w - 8), True), (dict(width=max(16, hdr.w // 5)), True)):
        want = imaginary.process_bytes(restart, dict(opts), jpeg_dct=True, jpeg_dct_shrink=shrink)
        assert len(calls) == 1
        del calls[:]
        got = imaginary.process_bytes(restart, dict(opts), jpeg_huff=True, jpeg_huff_restart=True, jpeg_dct_shrink=shrink)
        assert got.mime == want.mime and got.body == want.body, opts
        assert calls == [], "the host decoder ran: the engine did not take the scan"
        # the flag off: the same bytes by the coefficients, as before
        off = imaginary.process_bytes(restart, dict(opts), jpeg_huff=True, jpeg_dct_shrink=shrink)
        assert off.body == want.body and len(calls) == 1
        del calls[:]
