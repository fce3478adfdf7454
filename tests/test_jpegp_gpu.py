"""Packed scan slots on the device (k_jpege_place and the packed variants of k_jpege_tables and
k_jpege_stuff in k_jpege.hip; mipx_op_*_scan_packed) and the request path's trimmed download of a
scan answer, against tests/jpegp_ref.py over the slots of tests/jpege_ref.py and tests/jpegeo_ref.py.
Every comparison is exact: the directory, every byte of each slot's header and scan, and every
other byte of the output buffer, which must still be the guard's fill byte.

With optimised tables no coefficients are known that overflow (tests/test_jpegeo_gpu.py), so the
mixes with an OVERFLOW slot run with the Annex K tables; the same inputs run optimised against
whatever the reference says of them."""
import ctypes as C
import os

import numpy as np
import pytest

import jpege_ref
import jpegeo_ref
import test_jpege_gpu as annexk
import test_jpegeo_gpu as optimised
from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpege_ref import OK, OVERFLOW, UNCODABLE
from jpegp_ref import align16, check_packed, dir_ref, slot_span
from test_jpege_gpu import ALL_SKEWS, MULTI, SKEWS, _under, pixels

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (17, 9), (37, 29), MULTI]
LAYOUTS = [YCC_444, YCC_420]
QUALITIES = [50, 100]


def _head(optimize):
    return 1104 if optimize else 16


def _slots(w, h, n, layout, quality, optimize):
    """The reference slots, from the caches the unpacked tests fill."""
    return (optimised if optimize else annexk).slots(w, h, n, layout, quality)


def _slot_ref(optimize):
    return jpegeo_ref.slot_ref if optimize else jpege_ref.slot_ref


def _slot_bytes(w, h, layout, optimize):
    return _head(optimize) + jpegc_bytes(w, h, layout)


def _check(got, want, w, h, layout, optimize, what):
    d, packed = got
    assert packed.dtype == np.uint8 and packed.shape == (len(want) * _slot_bytes(w, h, layout, optimize),), (what, packed.shape)
    check_packed(d, packed, want, _head(optimize), what, FILL)


# ---------------------------------------------------------------- the two entry points
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimised"])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_both_packed_entry_points_equal_the_reference(gpu, layout, n, optimize):
    k = 0
    for w, h in SIZES:
        px = pixels(w, h, n)
        for quality in QUALITIES:
            want = _slots(w, h, n, layout, quality, optimize)
            assert all(s.status == OK for s in want)
            si, so = SKEWS[k % 4]
            k += 1
            what = f"{n}x{h}x{w} layout {layout} Q {quality} optimize {optimize} skew {si},{so}"
            _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan_packed(px, layout, quality, optimize)), want, w, h,
                   layout, optimize, "rgb_to_jpeg_scan_packed " + what)
            coefs = annexk.coefficients(w, h, n, layout, quality)
            _check(_under(si, so, lambda: gpu.jpegc_to_scan_packed(coefs, w, h, layout, optimize)), want, w, h,
                   layout, optimize, "jpegc_to_scan_packed " + what)


def test_the_large_size_spans_three_workgroups_of_every_coder_kernel():
    w, h = MULTI
    for layout in LAYOUTS:
        assert jpege_ref.scan_blocks(w, h, layout) > 2 * jpege_ref.TILE
        assert min(s.bits for s in annexk.slots(w, h, 3, layout, 50)) > 8 * 2 * jpege_ref.CHUNK
        assert min(s.bits for s in optimised.slots(w, h, 3, layout, 50)) > 8 * 2 * jpege_ref.CHUNK
        # ... and the packed slots are much shorter than the slots: the pads and the tail are most of the buffer
        assert int(dir_ref(annexk.slots(w, h, 3, layout, 50), 16)[-1]) * 2 < 3 * _slot_bytes(w, h, layout, False)


# ---------------------------------------------------------------- slots that are not OK
def _mixed(layout, kinds):
    """Coefficients at 16 x 16 whose Annex K slots have the statuses `kinds` (tests/test_jpege_gpu.py's recipes)."""
    c = annexk.coefficients(16, 16, 3, layout, 90)[:len(kinds)].copy()
    for i, kind in enumerate(kinds):
        if kind == OVERFLOW:                  # every AC +-1023: 26 bits for each 16-bit coefficient
            c[i] = np.where(np.arange(c.shape[1]) % 2 == 0, 1023, -1023)
            c[i, ::64] = 0
        elif kind == UNCODABLE:               # the scan's first block, predicted from 0: a DC step of 2048
            c[i, 0] = 2048
    return c


@pytest.mark.parametrize("kinds", [(OK, UNCODABLE, OK), (OK, OVERFLOW, OK), (OVERFLOW, UNCODABLE)],
                         ids=["ok-uncodable-ok", "ok-overflow-ok", "overflow-uncodable"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_slots_that_are_not_ok_are_their_headers_alone(gpu, layout, kinds):
    w = h = 16
    c = _mixed(layout, kinds)
    want = [jpege_ref.slot_ref(x, w, h, layout) for x in c]
    assert [s.status for s in want] == list(kinds)
    d = dir_ref(want, 16)
    for i, s in enumerate(want):
        assert int(d[i + 1] - d[i]) == (align16(16 + s.length) if s.status == OK else 16)
        assert s.status != OVERFLOW or s.length > jpegc_bytes(w, h, layout)    # a length that means no bytes
    for si, so in [(0, 0), (1, 3)]:
        got = _under(si, so, lambda: gpu.jpegc_to_scan_packed(c, w, h, layout))
        _check(got, want, w, h, layout, False, f"statuses {kinds} layout {layout}")
        for i, s in enumerate(want):
            if s.status != OK:
                header = got[1][int(d[i]):int(d[i]) + 16].view("<u4").tolist()
                assert header[:2] == [s.length, s.status] and header[3] == 0
                assert s.bits is None or header[2] == s.bits
    # the same inputs with optimised tables: an uncodable value has no code there either
    want = [jpegeo_ref.slot_ref(x, w, h, layout) for x in c]
    assert [s.status == UNCODABLE for s in want] == [k == UNCODABLE for k in kinds]
    got = _under(2, 1, lambda: gpu.jpegc_to_scan_packed(c, w, h, layout, optimize=True))
    _check(got, want, w, h, layout, True, f"statuses {kinds} layout {layout}, optimised")
    d = dir_ref(want, 1104)
    for i, s in enumerate(want):
        if s.status != OK:
            assert int(d[i + 1] - d[i]) == 1104
            assert got[1][int(d[i]):int(d[i]) + 16].view("<u4").tolist()[::3] == [0, 1]


# ---------------------------------------------------------------- more images than the place kernel's stride
@pytest.mark.parametrize("n", [257, 300])
def test_more_images_than_one_stride_of_the_place_kernel(gpu, n):
    """8 x 8 noise at Q 100: the lengths differ per image; 257 and 300 images are a second stride of the
    place kernel's 256 lanes, partial both times."""
    w = h = 8
    px = np.random.default_rng(n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    for layout, optimize in [(YCC_444, False), (YCC_420, True)]:
        c = jpegc_ref(px, layout, 100)
        want = [_slot_ref(optimize)(x, w, h, layout) for x in c]
        assert all(s.status == OK for s in want) and len({s.length for s in want}) > 8
        assert len({align16(slot_span(s, _head(optimize))) for s in want}) > 1      # steps differ, not only lengths
        _check(_under(1, 2, lambda: gpu.jpegc_to_scan_packed(c, w, h, layout, optimize)), want, w, h, layout, optimize,
               f"{n} images layout {layout} optimize {optimize}")


# ---------------------------------------------------------------- pointer alignment
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimised"])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_packed_under_every_pointer_alignment(gpu, layout, optimize):
    w, h = 37, 29
    px, coefs = pixels(w, h, 3), annexk.coefficients(w, h, 3, layout, 90)
    want = _slots(w, h, 3, layout, 90, optimize)
    for si, so in ALL_SKEWS:
        what = f"3x{h}x{w} layout {layout} optimize {optimize} skew {si},{so}"
        _check(_under(si, so, lambda: gpu.jpegc_to_scan_packed(coefs, w, h, layout, optimize)), want, w, h, layout,
               optimize, "jpegc_to_scan_packed " + what)
        _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan_packed(px, layout, 90, optimize)), want, w, h, layout,
               optimize, "rgb_to_jpeg_scan_packed " + what)


# ---------------------------------------------------------------- the request path
def _copy(gpu, p):
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _plan(gpu, w, h, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


def _requests(gpu, eng):
    """Two plans (128 x 96 -> width 64 at 4:2:0 Q 75; 37 x 29 at 4:4:4 Q 95), three requests each, and
    one plan with optimised tables: (plan, image, reference slot, head, slot bytes) per request."""
    reqs = []
    for w, h, layout, quality, optimize in [(128, 96, YCC_420, 75, False), (37, 29, YCC_444, 95, False),
                                            (128, 96, YCC_420, 75, True)]:
        p = _plan(gpu, w, h, width=max(8, w // 2))
        q = gpu.plan_set_jpeg_scan_output(_copy(gpu, p), layout, quality, optimize=optimize)
        for im in pixels(w, h, 3)[:1 if optimize else 3]:
            want = _slot_ref(optimize)(jpegc_ref(eng.process(p, im)[None], layout, quality)[0], p.out_w, p.out_h, layout)
            assert want.status == OK
            reqs.append((q, im, want, _head(optimize), _slot_bytes(p.out_w, p.out_h, layout, optimize)))
    return reqs


def _run(gpu, eng, reqs):
    """Submits all, waits for all: the outputs (pre-filled with 0xA5) and the D2H bytes and batches they took."""
    d0, b0 = eng.transfer_stats()[1], eng.stats()[0]
    outs = [np.full(size, FILL, np.uint8) for _, _, _, _, size in reqs]
    tickets = [eng.submit(q, im, out=out)[0] for (q, im, _, _, _), out in zip(reqs, outs)]
    for t in tickets:
        eng.wait(t)
    return outs, eng.transfer_stats()[1] - d0, eng.stats()[0] - b0


def test_request_path_downloads_the_scans_only(gpu, monkeypatch):
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    monkeypatch.setenv("MIPX_SCAN_TRIM", "1")
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        reqs = _requests(gpu, eng)
        trimmed, d2h, batches = _run(gpu, eng, reqs)
        for out, (_, _, want, head, size) in zip(trimmed, reqs):
            (jpegeo_ref.check_slot if head == 1104 else jpege_ref.check_slot)(out, want, "trimmed request")
            assert (out[head + want.length:] == FILL).all(), "bytes behind the scan were written"
        assert 3 <= batches <= len(reqs)
        assert d2h == sum(align16(head + want.length) for _, _, want, head, _ in reqs) + 8 * (len(reqs) + batches)
    finally:
        eng.shutdown()
    monkeypatch.setenv("MIPX_SCAN_TRIM", "0")
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        whole, d2h, batches = _run(gpu, eng, reqs)
        for out, cut, (_, _, want, head, size) in zip(whole, trimmed, reqs):
            assert np.array_equal(out[:head + want.length], cut[:head + want.length])
        assert d2h == sum(size for _, _, _, _, size in reqs)
    finally:
        eng.shutdown()


def _huff_file():
    from imaginary_amd import codec
    buf = open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read()
    hdr = codec.header(buf)
    slot, layout = codec.jpeg_huff_slot(buf)
    return np.ascontiguousarray(slot, dtype=np.uint8), layout, hdr.w, hdr.h


def test_scan_input_and_scan_output_in_one_plan(gpu, monkeypatch):
    """Entropy-coded input and entropy-coded output: the statuses and the directory share the workspace's
    head, and a request whose input does not decode fails alone."""
    pytest.importorskip("PIL.Image")
    slot, layout, w, h = _huff_file()
    gpu.lib.mipx_shutdown()
    monkeypatch.setenv("MIPX_SCAN_TRIM", "1")
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        base = _plan(gpu, w, h, width=w // 2)
        rgb_plan = gpu.plan_set_jpegh_input(_copy(gpu, base), layout)
        rgb = eng.process(rgb_plan, slot)
        for optimize in (False, True):
            want = _slot_ref(optimize)(jpegc_ref(rgb[None], YCC_420, 80)[0], base.out_w, base.out_h, YCC_420)
            assert want.status == OK
            q = gpu.plan_set_jpeg_scan_output(_copy(gpu, rgb_plan), YCC_420, 80, optimize=optimize)
            head, size = _head(optimize), _slot_bytes(base.out_w, base.out_h, YCC_420, optimize)
            cut = slot.copy()
            cut[:4] = np.array([int(slot[:4].view("<u4")[0]) // 2], "<u4").view(np.uint8)   # ends before its last block
            d0, b0 = eng.transfer_stats()[1], eng.stats()[0]
            outs = [np.full(size, FILL, np.uint8) for _ in range(3)]
            tickets = [eng.submit(q, s, out=o)[0] for s, o in zip((slot, cut, slot), outs)]
            codes = []
            for t in tickets:
                try:
                    eng.wait(t)
                    codes.append(0)
                except gpu.MipxError as e:
                    codes.append(e.code)
            assert codes == [0, -10, 0], codes                               # MIPX_EDATA for the middle one alone
            for out in (outs[0], outs[2]):
                (jpegeo_ref.check_slot if optimize else jpege_ref.check_slot)(out, want, "scan in, scan out")
                assert (out[head + want.length:] == FILL).all()
            assert (outs[1] == FILL).all()
            batches = eng.stats()[0] - b0
            # The middle request's pixels are unspecified, and what they coded to travels with its batch: at
            # least a header, at most a slot.  The rest is exact: two scans, a directory per batch, 3 statuses.
            least = 2 * align16(head + want.length) + head + 8 * (3 + batches) + 4 * 3
            assert least <= eng.transfer_stats()[1] - d0 <= least - head + size
    finally:
        eng.shutdown()


def test_a_scan_input_uploads_its_header_and_length_bytes(gpu):
    pytest.importorskip("PIL.Image")
    slot, layout, w, h = _huff_file()
    length = int(slot[:4].view("<u4")[0])
    assert 0 < length < slot.size - 1504
    gpu.lib.mipx_shutdown()
    eng = gpu.Engine(max_batch=8, batch_wait_us=0)
    try:
        plan = gpu.plan_set_jpegh_input(_plan(gpu, w, h, width=w // 2), layout)
        up0 = eng.transfer_stats()[0]
        eng.process(plan, slot)
        assert eng.transfer_stats()[0] - up0 == 1504 + length
        up0 = eng.transfer_stats()[0]
        subs = [eng.submit(plan, slot) for _ in range(3)]    # (ticket, out): the outputs live until their wait returns
        for t, _ in subs:
            eng.wait(t)
        assert eng.transfer_stats()[0] - up0 == 3 * (1504 + length)
    finally:
        eng.shutdown()
