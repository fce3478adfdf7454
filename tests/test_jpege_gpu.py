"""Entropy-coded JPEG output on the device (MIPX_OP_JPEGE, k_jpege.hip) against tests/jpege_ref.py:
a slot's header and codec.jpeg_scan, the host writer that tests/test_jpegc_cpu.py pins to
libjpeg-turbo inside Pillow.  The coder alone, behind k_jpegc, as the last step of plans,
through the request path, and end to end over encoded bytes.  Every comparison is exact."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import jpege_ref
from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpege_ref import OK, OVERFLOW, UNCODABLE, check_slot, jpeg_scan_bytes, slot_ref
from ycc_ref import ycc_bytes

pytestmark = pytest.mark.gpu

# 17 x 9, 9 x 17, 33 x 17 and 1 x 40 have dummy Y blocks in 4:2:0: on the right edge, the bottom edge or both
SIZES = [(1, 1), (7, 7), (8, 8), (9, 8), (8, 9), (16, 16), (17, 9), (9, 17), (24, 8), (8, 24), (33, 17), (37, 29),
         (129, 67), (1, 40), (40, 1)]
# The coding kernels take 256 blocks of the scan per workgroup, the stuffing kernels 1024 bytes of
# scan.  197 x 117 is 25 x 15 blocks: 1125 blocks of scan in 4:4:4 (5 workgroups, the last with 101);
# in 4:2:0 13 x 8 MCUs with a dummy Y column and a dummy Y row, 624 blocks (3 workgroups, the last
# with 112).  Its scans are 6 KiB and more from Q 50 up: 6 or more stuffing workgroups.  Were the
# tiles 1024 blocks, 4:4:4 would still be two of them; the test below asserts what it relies on.
MULTI = (197, 117)
LAYOUTS = [YCC_444, YCC_420]
QUALITIES = [1, 50, 90, 100]
SKEWS = [(0, 0), (1, 3), (2, 1), (3, 2)]
ALL_SKEWS = [(i, o) for i in range(4) for o in range(4)]


@functools.lru_cache(maxsize=None)
def pixels(w, h, n):
    """Full-range random RGB, (n, h, w, 3).  Computed once, read-only."""
    px = np.random.default_rng(w * 100003 + h * 101 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def coefficients(w, h, n, layout, quality):
    c = jpegc_ref(pixels(w, h, n), layout, quality)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def slots(w, h, n, layout, quality):
    """The reference slots of coefficients(...), one Slot per image."""
    return tuple(slot_ref(c, w, h, layout) for c in coefficients(w, h, n, layout, quality))


def _under(skew_in, skew_out, call):
    from imaginary_amd import engine
    prev = engine.set_guard(FILL, skew_in, skew_out)
    try:
        before = engine.guarded_calls()
        out = call()
        assert engine.guarded_calls() > before, "the guard was not live"
        return out
    finally:
        engine.set_guard(*prev)


def _check(got, want, w, h, layout, what):
    assert got.dtype == np.uint8 and got.shape == (len(want), jpeg_scan_bytes(w, h, layout)), (what, got.shape)
    for i, s in enumerate(want):
        check_slot(got[i], s, f"{what}, image {i}")


# ---------------------------------------------------------------- the two entry points
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_both_entry_points_equal_the_reference(gpu, layout, n):
    k = 0
    for w, h in SIZES + [MULTI]:
        px = pixels(w, h, n)
        for quality in QUALITIES:
            want = slots(w, h, n, layout, quality)
            assert all(s.status == OK for s in want)     # noise fits at these sizes, also at Q 100
            si, so = SKEWS[k % 4]
            k += 1
            what = f"{n}x{h}x{w} layout {layout} Q {quality} skew {si},{so}"
            _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan(px, layout, quality)), want, w, h, layout,
                   "rgb_to_jpeg_scan " + what)
            coefs = coefficients(w, h, n, layout, quality)
            _check(_under(si, so, lambda: gpu.jpegc_to_scan(coefs, w, h, layout)), want, w, h, layout,
                   "jpegc_to_scan " + what)


def test_the_large_size_spans_three_workgroups_of_every_kernel():
    w, h = MULTI
    for layout in LAYOUTS:
        assert jpege_ref.scan_blocks(w, h, layout) > 2 * jpege_ref.TILE
        assert min(s.bits for s in slots(w, h, 3, layout, 50)) > 8 * 2 * jpege_ref.CHUNK
    assert jpegc_bytes(w, h, YCC_420) // 128 < jpege_ref.scan_blocks(w, h, YCC_420)   # dummy blocks


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_under_every_pointer_alignment(gpu, layout):
    for w, h in [(8, 8), (37, 29), MULTI]:
        px, coefs, want = pixels(w, h, 3), coefficients(w, h, 3, layout, 90), slots(w, h, 3, layout, 90)
        for si, so in ALL_SKEWS:
            what = f"3x{h}x{w} layout {layout} skew {si},{so}"
            _check(_under(si, so, lambda: gpu.jpegc_to_scan(coefs, w, h, layout)), want, w, h, layout, "jpegc_to_scan " + what)
            _check(_under(si, so, lambda: gpu.rgb_to_jpeg_scan(px, layout, 90)), want, w, h, layout,
                   "rgb_to_jpeg_scan " + what)


# ---------------------------------------------------------------- hand-made coefficients
LONE_AT = (1, 15, 16, 17, 32, 33, 48, 49, 63)   # zigzag positions: runs of 0 to 62 zeros in front, 0 to 3 ZRLs


def _run_coefs(gpu, c, w, h, layout, what):
    c = np.ascontiguousarray(c, dtype=np.int16)
    c = c[None] if c.ndim == 1 else c
    want = [slot_ref(x, w, h, layout) for x in c]
    assert all(s.status == OK for s in want), what       # these inputs are all codable, and fit
    got = gpu.jpegc_to_scan(c, w, h, layout)
    _check(got, want, w, h, layout, what)
    return got, want


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_hand_made_coefficients(gpu, layout):
    from imaginary_amd import codec
    w, h = 17, 9                              # 4:2:0: a dummy Y column and a dummy Y row
    size = jpegc_bytes(w, h, layout) // 2
    blocks = size // 64
    _run_coefs(gpu, np.zeros(size, np.int16), w, h, layout, "all zero")
    batch = []
    for k in LONE_AT:                         # a lone coefficient: 0 to 3 ZRLs in front, and no EOB behind 63
        nat = codec.ZIGZAG[k]
        for v in (1, -1, 1023, -1023):
            c = np.zeros(size, np.int16)
            c[nat::64] = v
            c[64 * (blocks - 1) + nat] = -v   # the last block differs
            batch.append(c)
    _run_coefs(gpu, np.stack(batch), w, h, layout, "lone coefficients")
    # DC steps of +-2047 between neighbours in scan order, per component; 0 elsewhere
    c = np.zeros(size, np.int16)
    c[0::128] = 1023
    c[64::128] = -1024
    up_down = c.copy()
    c = np.zeros(size, np.int16)
    c[0::64] = np.where(np.arange(blocks) % 3 == 0, 2047, 0)
    _run_coefs(gpu, np.stack([up_down, -up_down - (up_down != 0), c, -c]), w, h, layout, "DC steps")
    # a smooth ramp at Q 30: long zero runs, early EOBs
    x, y = np.meshgrid(np.arange(37), np.arange(29))
    ramp = np.stack([x * 255 // 36, y * 255 // 28, (x + y) * 255 // 64], -1).astype(np.uint8)
    _run_coefs(gpu, jpegc_ref(ramp[None], layout, 30), 37, 29, layout, "ramp at Q 30")


def test_the_two_found_inputs(gpu):
    """An 0xFF that the padding completes, and an 0xFF made of two blocks' bits."""
    a, b = jpege_ref.padding_ff_coefs(), jpege_ref.straddle_ff_coefs()
    got, want = _run_coefs(gpu, np.stack([a, b, a]), 8, 8, YCC_444, "the found inputs")
    assert want[0].scan[-2:] == b"\xff\x00" and got[0][16 + want[0].length - 2:16 + want[0].length].tolist() == [0xFF, 0]


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
@pytest.mark.parametrize("kind", ["ac", "dc"])
def test_an_uncodable_coefficient_is_reported_and_the_neighbours_are_exact(gpu, layout, kind):
    w, h = 37, 29
    c = coefficients(w, h, 3, layout, 90).copy()
    if kind == "ac":
        c[1, 64 * 7 + 9] = 1024
    else:
        c[1, 0] = 2048                        # the scan's first block, predicted from 0: a DC step of 2048
    want = [slot_ref(x, w, h, layout) for x in c]
    assert [s.status for s in want] == [OK, UNCODABLE, OK]
    got = gpu.jpegc_to_scan(c, w, h, layout)
    _check(got, want, w, h, layout, f"uncodable {kind}")
    assert got[1][:8].view("<u4").tolist() == [0, UNCODABLE]


def test_an_overflow_is_reported_and_stays_inside_the_slot(gpu):
    """16 x 16 with every AC +-1023 in image 1 of 3: 26 bits for each 16-bit coefficient."""
    w = h = 16
    for layout in LAYOUTS:
        c = coefficients(w, h, 3, layout, 90).copy()
        c[1] = np.where(np.arange(c.shape[1]) % 2 == 0, 1023, -1023)
        c[1, ::64] = 0
        want = [slot_ref(x, w, h, layout) for x in c]
        assert [s.status for s in want] == [OK, OVERFLOW, OK]
        assert want[1].length == -(-want[1].bits // 8) > jpegc_bytes(w, h, layout)
        for si, so in [(0, 0), (1, 3)]:       # the guard bands around the slots are checked by the wrapper
            got = _under(si, so, lambda: gpu.jpegc_to_scan(c, w, h, layout))
            _check(got, want, w, h, layout, f"overflow layout {layout}")
            assert got[1][:12].view("<u4").tolist() == [want[1].length, OVERFLOW, want[1].bits]


def test_an_overflow_that_only_the_stuffing_causes(gpu):
    """Every AC 127: 14 or 15 bits per coefficient with 11 or 12 of them 1s, so the scan fits the slot
    before stuffing and a third of its bytes are 0xFF (tests/test_jpege_cpu.py).  The verdict then
    comes from the second scan, after the bits were packed."""
    w = h = 16
    for layout in LAYOUTS:
        c = coefficients(w, h, 3, layout, 90).copy()
        c[1] = 127
        c[1, ::64] = 0
        want = [slot_ref(x, w, h, layout) for x in c]
        assert [s.status for s in want] == [OK, OVERFLOW, OK]
        assert want[1].length == -(-want[1].bits // 8) <= jpegc_bytes(w, h, layout)
        got = _under(2, 1, lambda: gpu.jpegc_to_scan(c, w, h, layout))
        _check(got, want, w, h, layout, f"stuffing overflow layout {layout}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    """Three images of different scan lengths; the middle slot is what it is alone."""
    w, h = 37, 29
    px = np.stack([pixels(w, h, 3)[0], pixels(w, h, 3)[1], np.full((h, w, 3), 200, np.uint8)])
    px[0, :, :, :] //= 64
    want = [slot_ref(c, w, h, YCC_420) for c in jpegc_ref(px, YCC_420, 90)]
    assert len({s.length for s in want}) == 3
    got = gpu.rgb_to_jpeg_scan(px, YCC_420, 90)
    _check(got, want, w, h, YCC_420, "a batch of three lengths")
    alone = gpu.rgb_to_jpeg_scan(px[1], YCC_420, 90)
    check_slot(alone[0], want[1], "the middle image alone")
    other = px.copy()
    other[0], other[2] = 255 - other[0], 255 - other[2]
    check_slot(gpu.rgb_to_jpeg_scan(other, YCC_420, 90)[1], want[1], "the middle image among others")


def test_wrappers_refuse_other_inputs(gpu):
    with pytest.raises(ValueError):
        gpu.rgb_to_jpeg_scan(np.zeros((8, 8, 4), np.uint8), YCC_420, 75)
    with pytest.raises(ValueError):
        gpu.rgb_to_jpeg_scan(np.zeros((8, 8, 3), np.uint8), 2, 75)
    with pytest.raises(gpu.MipxError):
        gpu.rgb_to_jpeg_scan(np.zeros((8, 8, 3), np.uint8), YCC_420, 0)
    with pytest.raises(ValueError):
        gpu.jpegc_to_scan(np.zeros(3 * 64 - 1, np.int16), 8, 8, YCC_444)


# ---------------------------------------------------------------- as the last step of a plan
W, H = 128, 96


def _copy(gpu, p):
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _plan(gpu, w=W, h=H, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


@pytest.mark.parametrize("layout,quality", [(YCC_444, 92), (YCC_420, 75)], ids=["444", "420"])
@pytest.mark.parametrize("name", ["reduce", "ycc+reduce", "rot90", "chain", "empty", "textmark"])
def test_plan_with_the_step_equals_the_reference_on_the_plans_rgb(gpu, name, layout, quality):
    """Each plan runs without the step, then with it: the slots are the reference's of the
    engine's own RGB result (the cases of tests/test_jpegc_gpu.py)."""
    wm = None
    src = pixels(W, H, 2)
    if name == "reduce":
        p = _plan(gpu, width=60)
    elif name == "ycc+reduce":
        p = gpu.plan_set_ycc_input(_plan(gpu, width=60), YCC_420)
        src = np.random.default_rng(5).integers(0, 256, (2, ycc_bytes(W, H, YCC_420)), dtype=np.uint8)
    elif name == "rot90":
        p = _plan(gpu, w=37, h=29, rotate=90)
        src = pixels(37, 29, 2)
        assert (p.out_w, p.out_h) == (29, 37)
    elif name == "chain":
        s0 = _plan(gpu, width=64)
        p = gpu.plan_chain([s0, _plan(gpu, w=s0.out_w, h=s0.out_h, width=40, height=20, crop=1, sigma=1.2)])
    elif name == "textmark":
        p = _plan(gpu)
        gpu.plan_add_textmark(p, 33, 14, 20, 0.6, (255, 40, 0))
        wm = np.random.default_rng(3).integers(0, 256, (14, 33, 1), dtype=np.uint8)
    else:
        p = _plan(gpu)
    rgb = gpu.execute(p, src, wm=wm, junk=0x3C)
    assert rgb.shape[3] == 3
    want = [slot_ref(c, p.out_w, p.out_h, layout) for c in jpegc_ref(rgb, layout, quality)]
    q = gpu.plan_set_jpeg_scan_output(_copy(gpu, p), layout, quality)
    assert q.n_steps == p.n_steps + 1 and (q.out_w, q.out_h, q.out_bands) == (p.out_w, p.out_h, 3)
    got = gpu.execute(q, src, wm=wm, junk=0x3C)
    _check(got, want, p.out_w, p.out_h, layout, f"{name} layout {layout}")
    one = gpu.execute(q, src[1], wm=wm, junk=0xC3)
    check_slot(one[0], want[1], f"{name} layout {layout}, one image")
    if name == "chain":   # the step inside the last stage of the chain
        s0 = _plan(gpu, width=64)
        last = _plan(gpu, w=s0.out_w, h=s0.out_h, width=40, height=20, crop=1, sigma=1.2)
        gpu.plan_set_jpeg_scan_output(last, layout, quality)
        assert bytes(gpu.plan_chain([s0, last])) == bytes(q)


# ---------------------------------------------------------------- the request path
def test_request_path_gives_slots(gpu):
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        subs = []
        for k, (w, h) in enumerate([(128, 96), (37, 29)]):
            layout, quality = [(YCC_420, 75), (YCC_444, 95)][k % 2]
            p = _plan(gpu, w=w, h=h, width=max(8, w // 2))
            q = gpu.plan_set_jpeg_scan_output(_copy(gpu, p), layout, quality)
            for im in pixels(w, h, 3):
                want = slot_ref(jpegc_ref(eng.process(p, im)[None], layout, quality)[0], p.out_w, p.out_h, layout)
                subs.append((eng.submit(q, im), want, (p.out_w, p.out_h, layout)))
        for (ticket, out), want, (w, h, layout) in subs:
            eng.wait(ticket)
            assert out.dtype == np.uint8 and out.shape == (jpeg_scan_bytes(w, h, layout),)
            check_slot(out, want, "request")
            assert gpu.scan_slot(out) == (OK, want.bits, want.scan)
        with pytest.raises(ValueError):     # a wrong-sized out is refused by the wrapper
            eng.submit(q, im, out=np.zeros(16, np.uint8))
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
@pytest.fixture
def step_calls(monkeypatch):
    """Counts the requests that left the engine as scans, and as coefficients."""
    from imaginary_amd import imaginary
    calls = {"scan": [], "coefs": []}
    real_scan, real_coefs = imaginary.plan_set_jpeg_scan_output, imaginary.plan_set_jpegc_output

    def spy_scan(plan, layout, quality):
        calls["scan"].append((layout, quality))
        return real_scan(plan, layout, quality)

    def spy_coefs(plan, layout, quality):
        calls["coefs"].append((layout, quality))
        return real_coefs(plan, layout, quality)

    monkeypatch.setattr(imaginary, "plan_set_jpeg_scan_output", spy_scan)
    monkeypatch.setattr(imaginary, "plan_set_jpegc_output", spy_coefs)
    return calls


@pytest.mark.parametrize("quality,layout", [(80, YCC_420), (95, YCC_444)])
@pytest.mark.parametrize("name", ["imaginary.jpg", "large.jpg"])
def test_process_bytes_gives_the_same_bytes(gpu, step_calls, name, quality, layout):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = open(os.path.join(GOLDEN, "testdata", name), "rb").read()
    opts = dict(width=300, quality=quality)
    want = imaginary.process_bytes(buf, opts, jpeg_coefs=True)
    assert step_calls == {"scan": [], "coefs": [(layout, quality)]}
    got = imaginary.process_bytes(buf, opts, jpeg_scan=True)
    assert step_calls == {"scan": [(layout, quality)], "coefs": [(layout, quality)]}   # the scan step ran, and sufficed
    assert got.mime == want.mime == "image/jpeg" and got.body == want.body
    if name == "imaginary.jpg" and quality == 80:
        # other outputs keep the RGB path: a PNG answer, a grey answer
        del step_calls["scan"][:], step_calls["coefs"][:]
        png = imaginary.process_bytes(buf, dict(width=100, type="png"), jpeg_scan=True)
        assert png.body == imaginary.process_bytes(buf, dict(width=100, type="png")).body
        grey = dict(width=100, interpretation=26)
        assert imaginary.process_bytes(buf, grey, jpeg_scan=True).body == imaginary.process_bytes(buf, grey).body
        assert step_calls == {"scan": [], "coefs": []}


def test_process_falls_back_to_coefficients_when_the_slot_is_not_ok(gpu, step_calls, monkeypatch):
    from imaginary_amd import codec, imaginary
    real = imaginary.scan_slot
    monkeypatch.setattr(imaginary, "scan_slot", lambda slot: (OVERFLOW, real(slot)[1], b""))
    px = pixels(64, 48, 1)[0]
    out = imaginary.process(imaginary.Decoded(px, "png", 0), dict(width=32), jpeg_quality=75, jpeg_scan=True)
    assert isinstance(out, imaginary.JpegCoefs) and step_calls == {"scan": [(YCC_420, 75)], "coefs": [(YCC_420, 75)]}
    monkeypatch.setattr(imaginary, "scan_slot", real)
    again = imaginary.process(imaginary.Decoded(px, "png", 0), dict(width=32), jpeg_quality=75, jpeg_scan=True)
    assert isinstance(again, imaginary.JpegScan)
    assert again.scan == codec.jpeg_scan(out.coefs, out.w, out.h, out.layout)
