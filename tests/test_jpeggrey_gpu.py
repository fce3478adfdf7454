"""Grey (one-component) JPEGs on the device (MIPX_YCC_GREY): the coefficient decode at every scale
against tests/jpeggrey_ref.py on Pillow-written files and on coefficients no encoder writes, the
entropy decoder against codec.decode_jpeg_coefs on ordinary, optimised-table and restart files, the
coefficient output against the reference, the entropy coder against Pillow's files byte for byte,
then plans, the request path and process_bytes.  Every comparison is exact; the
guard bands of every buffer are live, on both skews.

The shapes are the smallest at which a specific thing can go wrong:
  1x1, 8x8     the smallest images
  9x17         a partial block on both axes
  131x37       odd, 17 blocks across
  264x64       33 blocks across: one past k_jpegd's run of 32
  1032x9       129 blocks across: one past k_jpegds's run of 128 at N = 2
  392x9        49 blocks across: one past the 48 blocks (384 pixels) of the grey k_jpegc strip"""
import functools
import threading

import numpy as np
import pytest

import jpeggrey_ref as R
from footprint import FILL, guarded  # noqa: F401
from jpeggrey_ref import YCC_GREY

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (8, 8), (9, 17), (131, 37), (264, 64), (1032, 9), (392, 9)]
SKEWS = [(0, 0), (1, 3)]
QUALITIES = (1, 30, 75, 92, 100)
KINDS = [dict(), dict(optimize=True), dict(restart_marker_blocks=1), dict(restart_marker_blocks=8), dict(restart_marker_rows=1)]
KIND_IDS = ["plain", "optimized", "ri1", "ri8", "row"]
OK, BAD = R.OK, R.BAD


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


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        d = np.flatnonzero(got.ravel() != want.ravel())
        at = int(d[0])
        raise AssertionError(f"{what}: {d.size} of {got.size} values differ, the first at {at}: "
                             f"got {got.ravel()[at:at + 8].tolist()} want {want.ravel()[at:at + 8].tolist()}")


@functools.lru_cache(maxsize=None)
def files(w, h, n=3):
    """n Pillow files of w x h noise at different qualities (so different tables), the host decoder's
    payloads and Pillow's decodes at every scale it delivers; read-only."""
    from imaginary_amd import codec
    out = []
    for i, quality in zip(range(n), (75, 92, 30)):
        buf = R.pillow_jpeg(R.noise(w, h, i), quality)
        payload, layout = codec.decode_jpeg_coefs(buf, grey=True)
        assert layout == YCC_GREY and payload.size == R.jpegd_bytes(w, h)
        payload.setflags(write=False)
        out.append((buf, payload))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def decoded(w, h, s):
    """The reference's image at 1 / s of files(w, h)'s payloads, (3, oh, ow, 1); read-only."""
    px = R.jpegd_grey_ref(np.stack([p for _, p in files(w, h)]), w, h, s)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def images(w, h):
    """Three different 1-band images: noise, a smooth ramp, noise of another seed; read-only."""
    px = np.stack([R.noise(w, h), R.smooth(w, h), R.noise(w, h, 7)])
    px.setflags(write=False)
    return px


def _copy(gpu, p):
    import ctypes as C
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _base(gpu, w, h, bands=1, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, bands, "png"))


# ---------------------------------------------------------------- 1. coefficient input
@pytest.mark.parametrize("shrink", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_coefficient_decode_equals_the_reference_and_pillow(gpu, shape, shrink):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    w, h = shape
    p = np.stack([pl for _, pl in files(w, h)])
    want = decoded(w, h, shrink)
    for si, so in SKEWS:
        if shrink == 1:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb(p, w, h, YCC_GREY))
        else:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, YCC_GREY, shrink))
        _same(got, want, f"jpegd 3x{h}x{w} at 1/{shrink} skew {si},{so}")
    if codec.decode_scale(w, h, shrink) == shrink:                 # where Pillow's draft delivers this scale
        for i, (buf, _) in enumerate(files(w, h)):
            _same(want[i], codec.decode(buf, shrink), f"the reference and Pillow, {h}x{w} at 1/{shrink}, file {i}")
    one = gpu.jpegd_to_rgb_scaled(p[1], w, h, YCC_GREY, shrink)
    _same(one[0], want[1], f"jpegd {h}x{w} at 1/{shrink}, one image")


def test_the_coefficient_rule_is_total(gpu):
    """Coefficients no encoder writes: full-range random int16 with a random table, where pass 1
    saturates and the dequantisation wraps; random bytes behind the table, which nothing reads.  The
    reference alone is the yardstick here."""
    rng = np.random.default_rng(66)
    w, h = 264, 19
    coefs = rng.integers(-32768, 32768, (3, R.jpegc_bytes(w, h) // 2), dtype=np.int16)
    p = np.stack([R.payload(c, rng.integers(1, 256, 64)) for c in coefs])
    p[:, 128:384] = rng.integers(0, 256, (3, 256), dtype=np.uint8)
    for shrink in (1, 2, 4, 8):
        trace = {}
        want = R.jpegd_grey_ref(p, w, h, shrink, trace)
        assert shrink == 8 or trace["saturated"] > 0          # the saturation really fires
        got = _under(1, 3, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, YCC_GREY, shrink))
        _same(got, want, f"random coefficients {h}x{w} at 1/{shrink}")


# ---------------------------------------------------------------- 2. coefficient output
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_coefficient_output_equals_the_reference(gpu, shape):
    w, h = shape
    px = images(w, h)
    for k, quality in enumerate(QUALITIES):
        want = R.jpegc_grey_ref(px, quality)
        si, so = SKEWS[k % 2]
        got = _under(si, so, lambda: gpu.rgb_to_jpegc(px, YCC_GREY, quality))
        _same(got, want, f"jpegc 3x{h}x{w} Q{quality} skew {si},{so}")
    flat = np.stack([np.zeros((h, w, 1), np.uint8), np.full((h, w, 1), 255, np.uint8), R.noise(w, h, 3)])
    for si, so in SKEWS:
        got = _under(si, so, lambda: gpu.rgb_to_jpegc(flat, YCC_GREY, 100))
        _same(got, R.jpegc_grey_ref(flat, 100), f"jpegc of all-0 and all-255, {h}x{w} skew {si},{so}")
    one = gpu.rgb_to_jpegc(px[2], YCC_GREY, 75)
    _same(one[0], R.jpegc_grey_ref(px[2], 75)[0], f"jpegc {h}x{w}, one image")


@pytest.mark.parametrize("shape", [(9, 17), (131, 37), (392, 9)], ids=lambda s: "%dx%d" % s)
def test_the_engines_coefficients_make_pillows_file(gpu, shape):
    """Engine coefficients, host entropy coder: byte for byte the file Pillow writes of the pixels,
    with Annex K's tables and with the image's own."""
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    w, h = shape
    px = images(w, h)
    for quality in (30, 92, 100):
        got = _under(1, 3, lambda: gpu.rgb_to_jpegc(px, YCC_GREY, quality))
        for i in range(3):
            assert codec.encode_jpeg_coefs(got[i], w, h, YCC_GREY, quality) == R.pillow_jpeg(px[i], quality), (quality, i)
            assert codec.encode_jpeg_coefs(got[i], w, h, YCC_GREY, quality, tables="optimal") == \
                R.pillow_jpeg(px[i], quality, optimize=True), (quality, i)


# ---------------------------------------------------------------- 2b. the scan to coefficients and pixels
@functools.lru_cache(maxsize=None)
def slots(w, h, kind=0, quality=75, n=3):
    """n files of w x h noise (KINDS[kind]) with their slots and the host decoder's payloads; read-only."""
    from imaginary_amd import codec
    out = []
    for i in range(n):
        buf = R.pillow_jpeg(R.noise(w, h, i), quality, **KINDS[kind])
        (slot, l1), (payload, l2) = codec.jpeg_huff_slot(buf, restart=True, grey=True), codec.decode_jpeg_coefs(buf, grey=True)
        assert l1 == l2 == YCC_GREY and slot.size == R.jpegh_bytes(w, h) and payload.size == R.jpegd_bytes(w, h)
        slot.setflags(write=False), payload.setflags(write=False)
        out.append((buf, slot, payload))
    return tuple(out)


def _decode(gpu, some, w, h, skews=(0, 0)):
    payloads, status = _under(*skews, lambda: gpu.jpegh_to_jpegd(np.stack(some), w, h, YCC_GREY))
    assert payloads.shape == (len(some), R.jpegd_bytes(w, h)) and status.shape == (len(some),)
    return payloads, status.tolist()


@pytest.mark.parametrize("kind", range(5), ids=KIND_IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_decoder_equals_the_host_decoder(gpu, shape, kind):
    pytest.importorskip("PIL.Image")
    w, h = shape
    f = slots(w, h, kind)
    ri = [0, 0, 1, 8, -(-w // 8)][kind]
    for _, slot, _ in f:
        assert int(slot[4:8].view("<u4")[0]) == ri                 # a restart interval counts blocks
    for n in (1, 3):
        skews = SKEWS[(kind + n) % 2]
        got, status = _decode(gpu, [s for _, s, _ in f[:n]], w, h, skews)
        assert status == [OK] * n, (shape, kind, status)
        for i in range(n):
            _same(got[i], f[i][2], f"{h}x{w} {KIND_IDS[kind]} skew {skews}, image {i} of {n}")


def _flipped(slot):
    """An ordinary slot with one scan byte's bits flipped: a 00 that no FF precedes and no 00 follows
    becomes an FF that no 00 follows, which include/mipx.h says is BAD."""
    length = int(slot[:4].view("<u4")[0])
    scan = slot[1504:1504 + length]
    at = [i for i in range(1, length - 1) if scan[i] == 0 and scan[i - 1] != 0xFF and scan[i + 1] != 0]
    assert at, "no such byte in this scan"
    out = slot.copy()
    out[1504 + at[len(at) // 2]] ^= 0xFF
    return out


def _wrong_marker(slot):
    """A restart slot whose second marker carries another number."""
    length = int(slot[:4].view("<u4")[0])
    scan = slot[1504:1504 + length].tobytes()
    at = scan.index(b"\xff\xd1")
    out = slot.copy()
    out[1504 + at + 1] = 0xD3
    return out


def test_a_batch_mixes_ordinary_and_restart_slots_and_damaged_ones_are_bad(gpu):
    pytest.importorskip("PIL.Image")
    w, h = 264, 64
    plain, one, eight = slots(w, h, 0), slots(w, h, 2), slots(w, h, 3)
    batch = [plain[0][1], eight[1][1], _flipped(plain[1][1]), one[2][1], _wrong_marker(eight[0][1]), plain[2][1]]
    good = {0: plain[0][2], 1: eight[1][2], 3: one[2][2], 5: plain[2][2]}
    for i, slot in enumerate(batch):                              # the model agrees on who is damaged
        assert R.decode_slot(slot, w, h)[0] == (OK if i in good else BAD)
    for skews in SKEWS:
        got, status = _decode(gpu, batch, w, h, skews)
        assert status == [OK, OK, BAD, OK, BAD, OK], status
        for i, want in good.items():
            _same(got[i], want, f"slot {i} skew {skews}")


def test_a_file_may_use_table_1_and_the_other_index_bytes_are_ignored(gpu):
    pytest.importorskip("PIL.Image")
    w, h = 131, 37
    f = slots(w, h, 1)
    moved = f[0][1].copy()                                # DC 0 -> DC 1, AC 0 -> AC 1, and bytes 400 and 403 say so
    moved[416 + 272:416 + 2 * 272], moved[416 + 3 * 272:416 + 4 * 272] = f[0][1][416:416 + 272], f[0][1][416 + 2 * 272:416 + 3 * 272]
    moved[416:416 + 272] = 0
    moved[416 + 2 * 272:416 + 3 * 272] = 0
    moved[400], moved[403] = 1, 1
    ignored = f[1][1].copy()
    ignored[401], ignored[402], ignored[404], ignored[405] = 7, 1, 200, 3
    named = f[2][1].copy()
    named[403] = 2                                        # Y's own AC index names no table: BAD
    assert [R.decode_slot(s, w, h)[0] for s in (moved, ignored, named)] == [OK, OK, BAD]
    got, status = _decode(gpu, [moved, ignored, named], w, h, SKEWS[1])
    assert status == [OK, OK, BAD], status
    _same(got[0], f[0][2], "tables 1")
    _same(got[1], f[1][2], "ignored index bytes")


def test_a_scan_that_crosses_a_sequence_boundary(gpu):
    pytest.importorskip("PIL.Image")
    import jpegh_ref
    w, h = 136, 328
    f = slots(w, h, 0, 92, 1)
    length = int(f[0][1][:4].view("<u4")[0])
    assert jpegh_ref.SEQ_BYTES == 32768 < length < 2 * jpegh_ref.SEQ_BYTES     # two sequences
    assert len(jpegh_ref.unstuff(f[0][1][1504:1504 + length].tobytes())[0]) > jpegh_ref.SEQ_BYTES
    assert R.decode_slot(f[0][1], w, h)[0] == OK                                # the model: they lock
    got, status = _decode(gpu, [f[0][1]], w, h, SKEWS[1])
    assert status == [OK]
    _same(got[0], f[0][2], "a scan of two sequences")


@pytest.mark.parametrize("shape", [(9, 17), (264, 64), (1032, 9)], ids=lambda s: "%dx%d" % s)
def test_the_scan_decodes_to_pixels_at_every_scale(gpu, shape):
    pytest.importorskip("PIL.Image")
    w, h = shape
    for kind in (0, 3):
        f = slots(w, h, kind)
        some = np.stack([s for _, s, _ in f])
        for k, shrink in enumerate((1, 2, 4, 8)):
            if shrink == 1:
                got, status = _under(*SKEWS[k % 2], lambda: gpu.jpegh_to_rgb(some, w, h, YCC_GREY))
            else:
                got, status = _under(*SKEWS[k % 2], lambda: gpu.jpegh_to_rgb_scaled(some, w, h, YCC_GREY, shrink))
            assert status.tolist() == [OK] * 3
            want = R.jpegd_grey_ref(np.stack([p for _, _, p in f]), w, h, shrink)
            _same(got, want, f"jpegh to pixels {h}x{w} {KIND_IDS[kind]} at 1/{shrink}")


# ---------------------------------------------------------------- 2c. the scan out
def _file_of(gpu, codec, slot, w, h, quality, optimize):
    """header + scan + FF D9 of one output slot, whose status must be OK: no case is skipped for it."""
    status, bits, scan, tables = gpu.scan_slot(slot, tables=True)
    assert status == 0, f"slot status {status} at {w}x{h} Q{quality}"
    assert (tables is not None) == optimize
    if optimize:                                          # DC 1 and AC 1: "a table the file does not define"
        assert not slot[16 + 272:16 + 2 * 272].any() and not slot[16 + 3 * 272:16 + 4 * 272].any()
        assert tables[0x01] == (bytes(16), b"") and tables[0x11] == (bytes(16), b"")
    assert 0 < bits <= 8 * len(scan)
    return codec.jpeg_from_scan(scan, w, h, YCC_GREY, quality, tables)


@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimized"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_scan_output_is_pillows_file(gpu, shape, optimize):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    w, h = shape
    px = images(w, h)
    head = 1104 if optimize else 16
    need = (gpu.jpeg_scan_opt_bytes if optimize else gpu.jpeg_scan_bytes)(w, h, YCC_GREY)
    for k, quality in enumerate((30, 92, 100)):
        si, so = SKEWS[k % 2]
        want = [R.pillow_jpeg(px[i], quality, optimize=optimize) for i in range(3)]
        got = _under(si, so, lambda: gpu.rgb_to_jpeg_scan(px, YCC_GREY, quality, optimize))
        assert got.shape == (3, need)
        for i in range(3):
            assert _file_of(gpu, codec, got[i], w, h, quality, optimize) == want[i], (quality, i)
        # from the coefficients, and packed: the same slots
        coefs = R.jpegc_grey_ref(px, quality)
        again = _under(so, si, lambda: gpu.jpegc_to_scan(coefs, w, h, YCC_GREY, optimize))
        d, packed = _under(si, so, lambda: gpu.rgb_to_jpeg_scan_packed(px, YCC_GREY, quality, optimize))
        d2, packed2 = _under(so, si, lambda: gpu.jpegc_to_scan_packed(coefs, w, h, YCC_GREY, optimize))
        assert d.tolist() == d2.tolist() and d[0] == 0
        for i in range(3):
            length = int(got[i][:4].view("<u4")[0])
            _same(again[i][:head + length], got[i][:head + length], f"jpegc_to_scan slot {i} Q{quality}")
            assert int(d[i + 1] - d[i]) == -(-(head + length) // 16) * 16
            for dd, pp in ((d, packed), (d2, packed2)):
                one = gpu.scan_unpack(dd, pp, i, head, need)
                _same(one[:head + length], got[i][:head + length], f"packed slot {i} Q{quality}")


# ---------------------------------------------------------------- 3. plans
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimized"])
def test_a_one_band_plan_takes_a_grey_scan_and_gives_one(gpu, optimize):
    """Resize, then blur, on 1 band: scan in and scan out equal the same plan on the decoded pixels
    followed by the host writer."""
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    w, h = 264, 64
    f = slots(w, h, 3 if optimize else 0)
    some, payloads = np.stack([s for _, s, _ in f]), np.stack([p for _, _, p in f])
    base = _base(gpu, w, h, width=88, sigma=1.2)
    pixels = gpu.execute(base, R.jpegd_grey_ref(payloads, w, h), junk=0x3C)
    q = gpu.plan_set_jpeg_scan_output(gpu.plan_set_jpegh_input(_copy(gpu, base), YCC_GREY), YCC_GREY, 75, optimize)
    assert q.steps[0].op == 20 and q.steps[q.n_steps - 1].op == 19 and q.out_bands == 1
    got = _under(1, 3, lambda: gpu.execute(q, some, junk=0x3C))
    assert gpu.execute_status().tolist() == [OK] * 3
    for i in range(3):
        want = codec.encode_jpeg_coefs(R.jpegc_grey_ref(pixels[i], 75)[0], q.out_w, q.out_h, YCC_GREY, 75,
                                       tables="optimal" if optimize else None)
        assert _file_of(gpu, codec, got[i], q.out_w, q.out_h, 75, optimize) == want, i
        assert want == R.pillow_jpeg(pixels[i], 75, optimize=optimize)


def test_a_colour_plan_that_ends_in_bw_gives_a_grey_scan(gpu):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    w, h = 131, 37
    rgb = np.random.default_rng(3).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    base = _base(gpu, w, h, 3, width=60, interpretation=gpu._abi.INTERPRETATION_BW)
    pixels = gpu.execute(base, rgb, junk=0x3C)
    for optimize in (False, True):
        q = gpu.plan_set_jpeg_scan_output(_copy(gpu, base), YCC_GREY, 92, optimize)
        got = _under(1, 1, lambda: gpu.execute(q, rgb, junk=0x3C))
        for i in range(3):
            assert _file_of(gpu, codec, got[i], q.out_w, q.out_h, 92, optimize) == R.pillow_jpeg(pixels[i], 92, optimize=optimize)


@pytest.mark.parametrize("shrink", [1, 2, 8])
def test_a_one_band_plan_takes_grey_coefficients_and_gives_them(gpu, shrink):
    """Resize, then blur, on 1 band: coefficients in and out equal the same plan on the decoded pixels
    followed by the reference's encoder."""
    w, h = 264, 64
    ow, oh = -(-w // shrink), -(-h // shrink)
    payloads = np.stack([p for _, p in files(w, h)])
    base = _base(gpu, ow, oh, width=max(ow // 3, 9), sigma=1.2)
    names = [s[0] for s in base.describe()]
    assert "reduce" in names and names[-1] == "blur" and base.out_bands == 1
    pixels = gpu.execute(base, decoded(w, h, shrink), junk=0x3C)
    q = _copy(gpu, base)
    if shrink == 1:
        gpu.plan_set_jpegd_input(q, YCC_GREY)
    else:
        gpu.plan_set_jpegd_input_scaled(q, YCC_GREY, shrink, w, h)
    assert q.steps[0].op == 17 and q.steps[0].a[0] == YCC_GREY and q.steps[0].out_bands == 1
    _same(_under(1, 3, lambda: gpu.execute(q, payloads, junk=0x3C)), pixels, f"a plan on grey coefficients at 1/{shrink}")
    gpu.plan_set_jpegc_output(q, YCC_GREY, 75)
    assert [s[0] for s in q.describe()] == ["jpegd"] + names + ["jpegc"]
    got = _under(0, 1, lambda: gpu.execute(q, payloads, junk=0x3C))
    _same(got, R.jpegc_grey_ref(pixels, 75), f"grey coefficients in and out at 1/{shrink}")


def test_a_colour_plan_that_ends_in_bw_gives_grey_coefficients(gpu):
    w, h = 131, 37
    rgb = np.random.default_rng(3).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    base = _base(gpu, w, h, 3, width=60, interpretation=gpu._abi.INTERPRETATION_BW)
    assert base.out_bands == 1 and base.describe()[-1][0] == "bw"
    pixels = gpu.execute(base, rgb, junk=0x3C)
    q = gpu.plan_set_jpegc_output(_copy(gpu, base), YCC_GREY, 92)
    got = _under(1, 1, lambda: gpu.execute(q, rgb, junk=0x3C))
    _same(got, R.jpegc_grey_ref(pixels, 92), "a colorspace=bw plan's coefficients")


# ---------------------------------------------------------------- 4. the request path
def test_the_request_path_batches_grey_requests(gpu):
    """Requests with different tables, coefficients in and coefficients out, from several submitters."""
    w, h = 264, 64
    f = files(w, h)
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        for shrink in (1, 2):
            ow, oh = -(-w // shrink), -(-h // shrink)
            plan = _base(gpu, ow, oh, width=40)
            if shrink == 1:
                gpu.plan_set_jpegd_input(plan, YCC_GREY)
            else:
                gpu.plan_set_jpegd_input_scaled(plan, YCC_GREY, shrink, w, h)
            gpu.plan_set_jpegc_output(plan, YCC_GREY, 75)
            want = gpu.execute(plan, np.stack([p for _, p in f]))      # the op-level result
            outs = [np.full(want.shape[1:], 0x5A5A, np.int16) for _ in range(9)]
            errors = []

            def submitter(k):
                try:
                    tickets = [eng.submit(plan, f[i % 3][1], out=outs[i])[0] for i in range(k, 9, 3)]
                    for t in tickets:
                        eng.wait(t)
                except Exception as e:  # noqa: BLE001 - reported by the asserting thread
                    errors.append(e)

            threads = [threading.Thread(target=submitter, args=(k,)) for k in range(3)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            for i in range(9):
                _same(outs[i], want[i % 3], f"grey request {i} at 1/{shrink}")
    finally:
        eng.shutdown()


def test_the_request_path_takes_grey_scans_and_gives_them(gpu):
    """Scan in, scan out, from several submitters; a damaged scan completes with MIPX_EDATA and its
    neighbours are exact."""
    pytest.importorskip("PIL.Image")
    w, h = 264, 64
    plain, eight = slots(w, h, 0), slots(w, h, 3)
    gpu.lib.mipx_shutdown()
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        for optimize in (False, True):
            plan = gpu.plan_set_jpeg_scan_output(gpu.plan_set_jpegh_input(_base(gpu, w, h, width=40), YCC_GREY), YCC_GREY, 75,
                                                 optimize)
            want = gpu.execute(plan, np.stack([s for _, s, _ in plain]))
            want8 = gpu.execute(plan, np.stack([s for _, s, _ in eight]))
            head = 1104 if optimize else 16
            reqs = [(plain, want, 0), (eight, want8, 1), (plain, want, 2), (eight, want8, 0), (plain, want, 1), (eight, want8, 2)]
            outs = [np.full(want.shape[1:], 0x5A, np.uint8) for _ in reqs]
            errors = []

            def submitter(k):
                try:
                    tickets = [eng.submit(plan, reqs[i][0][reqs[i][2]][1], out=outs[i])[0] for i in range(k, 6, 2)]
                    for t in tickets:
                        eng.wait(t)
                except Exception as e:  # noqa: BLE001 - reported by the asserting thread
                    errors.append(e)

            threads = [threading.Thread(target=submitter, args=(k,)) for k in range(2)]
            for t in threads:
                t.start()
            for t in threads:
                t.join()
            assert not errors, errors
            for i, (_, wanted, j) in enumerate(reqs):
                length = int(wanted[j][:4].view("<u4")[0])
                assert gpu.scan_slot(outs[i])[0] == 0
                _same(outs[i][:head + length], wanted[j][:head + length], f"grey scan request {i} optimize {optimize}")
        # a damaged scan among good ones
        plan = gpu.plan_set_jpegh_input(_base(gpu, w, h, width=40), YCC_GREY)
        want = gpu.execute(plan, np.stack([s for _, s, _ in plain]))
        batch = [plain[0][1], _flipped(plain[1][1]), plain[2][1]]
        outs = [np.full(want.shape[1:], 0x5A, np.uint8) for _ in batch]
        tickets = [eng.submit(plan, s, out=o)[0] for s, o in zip(batch, outs)]
        codes = []
        for t in tickets:
            try:
                eng.wait(t)
                codes.append(0)
            except gpu.MipxError as e:
                codes.append(e.code)
        assert codes == [0, -10, 0], codes                               # MIPX_EDATA for the middle one alone
        _same(outs[0], want[0], "the neighbour before a damaged scan")
        _same(outs[2], want[2], "the neighbour behind a damaged scan")
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- 5. end to end over bytes
def _counting(monkeypatch, codec, imaginary):
    """Count what the request's path used: the host's decode and encode, the engine's grey steps."""
    calls = []
    real = dict(decode=codec.decode, coefs=codec.decode_jpeg_coefs, encode=codec.encode,
                jpegd=imaginary.plan_set_jpegd_input, jpegds=imaginary.plan_set_jpegd_input_scaled,
                jpegc=imaginary.plan_set_jpegc_output, jpegh=imaginary.plan_set_jpegh_input,
                jpeghs=imaginary.plan_set_jpegh_input_scaled, jpege=imaginary.plan_set_jpeg_scan_output)
    monkeypatch.setattr(codec, "decode", lambda *a, **k: calls.append("decode") or real["decode"](*a, **k))
    monkeypatch.setattr(codec, "decode_jpeg_coefs", lambda *a, **k: calls.append("coefs") or real["coefs"](*a, **k))
    monkeypatch.setattr(codec, "encode", lambda *a, **k: calls.append("encode") or real["encode"](*a, **k))
    monkeypatch.setattr(imaginary, "plan_set_jpegd_input", lambda p, l: calls.append(("jpegd", l)) or real["jpegd"](p, l))
    monkeypatch.setattr(imaginary, "plan_set_jpegd_input_scaled",
                        lambda p, l, *a: calls.append(("jpegd", l)) or real["jpegds"](p, l, *a))
    monkeypatch.setattr(imaginary, "plan_set_jpegc_output", lambda p, l, q: calls.append(("jpegc", l)) or real["jpegc"](p, l, q))
    monkeypatch.setattr(imaginary, "plan_set_jpegh_input", lambda p, l: calls.append(("jpegh", l)) or real["jpegh"](p, l))
    monkeypatch.setattr(imaginary, "plan_set_jpegh_input_scaled",
                        lambda p, l, *a: calls.append(("jpegh", l)) or real["jpeghs"](p, l, *a))
    monkeypatch.setattr(imaginary, "plan_set_jpeg_scan_output",
                        lambda p, l, q, *a: calls.append(("jpege", l)) or real["jpege"](p, l, q, *a))
    return calls


def _photo(w, h):
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x * y) % 256)], axis=-1).astype(np.uint8)
    return (px.astype(int) + np.repeat(R.noise(w, h), 3, axis=2) // 8).clip(0, 255).astype(np.uint8)


@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimized"])
def test_process_bytes_takes_grey_on_the_engine(gpu, monkeypatch, optimize):
    pytest.importorskip("PIL.Image")
    import io
    from PIL import Image
    from imaginary_amd import codec, imaginary
    w, h = 261, 147
    rgb = _photo(w, h)
    grey = R.pillow_jpeg(rgb[:, :, 1:2], 85)
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, "JPEG", quality=85)
    colour = b.getvalue()
    assert codec.decode_jpeg_coefs(grey) is None and codec.decode_jpeg_coefs(grey, grey=True)[1] == YCC_GREY
    flags = dict(jpeg_huff=True, jpeg_dct=True, jpeg_dct_shrink=True, jpeg_scan=True, jpeg_optimize=optimize)
    requests = [(grey, dict(width=w - 8), True), (grey, dict(width=40), True),            # a resize; a thumbnail that shrinks on load
                (colour, dict(width=w - 8, interpretation=gpu._abi.INTERPRETATION_BW), False)]   # 1-band answer of a colour file
    for buf, opts, grey_in in requests:
        want = imaginary.process_bytes(buf, dict(opts))
        assert codec.header(want.body).bands == 1
        # with optimised tables: the file libjpeg writes of the same coefficients with optimize_coding
        hdr, at = codec.header(want.body), want.body.index(b"\xff\xc0")
        best = codec.encode_jpeg_coefs(codec.decode_jpeg_coefs(want.body, grey=True)[0][384:].view(np.int16), hdr.w, hdr.h,
                                       YCC_GREY, codec.DEFAULT_QUALITY, tables="optimal", grey_sampling=want.body[at + 11] >> 4)
        calls = _counting(monkeypatch, codec, imaginary)
        got = imaginary.process_bytes(buf, dict(opts), jpeg_grey=True, **flags)
        assert got.mime == want.mime
        used = list(calls)
        del calls[:]
        if optimize:          # the scan decodes to the same pixels and is Pillow's optimised coding of them
            assert np.array_equal(codec.decode(got.body), codec.decode(want.body)) and got.body == best, opts
            assert len(got.body) <= len(want.body)
        else:
            assert got.body == want.body, opts
        assert ("jpege", YCC_GREY) in used and "encode" not in used and ("jpegc", YCC_GREY) not in used, used
        if grey_in:           # the scan went to the engine: the host neither decoded nor entropy-decoded
            assert ("jpegh", YCC_GREY) in used and "decode" not in used and "coefs" not in used, used
        del calls[:]
        # by the coefficients alone: the host entropy-decodes and entropy-codes, the engine does the rest
        again = imaginary.process_bytes(buf, dict(opts), jpeg_dct=True, jpeg_dct_shrink=True, jpeg_coefs=True, jpeg_grey=True)
        assert again.body == want.body and ("jpegc", YCC_GREY) in calls and "encode" not in calls, calls
        if grey_in:
            assert ("jpegd", YCC_GREY) in calls and "coefs" in calls and "decode" not in calls, calls
        del calls[:]
        # with the flag off nothing of it is used: today's path
        off = imaginary.process_bytes(buf, dict(opts), **flags)
        assert off.body == want.body
        assert not [c for c in calls if isinstance(c, tuple) and c[1] == YCC_GREY], calls
        assert "encode" in calls and ("decode" in calls) == grey_in, calls
        monkeypatch.undo()
