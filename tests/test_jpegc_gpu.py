"""JPEG coefficient output on the device (MIPX_OP_JPEGC, k_jpegc.hip) against tests/jpegc_ref.py,
the numpy restatement of libjpeg's colour conversion, downsample, forward DCT and quantisation
that tests/test_jpegc_cpu.py pins to libjpeg-turbo itself: the kernel alone, as the last step
of plans, through the request path, and end to end over encoded bytes.  Every comparison is
exact."""
import ctypes as C
import functools
import io
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from ycc_ref import ycc_bytes

pytestmark = pytest.mark.gpu

# the CPU parity sizes; then: a workgroup makes a strip of 128 columns by 16 rows (4:2:0) or
# 8 rows (4:4:4), so 129 x 17 and 129 x 9 leave a last workgroup with one column / one row in
# both directions; 300 x 50 is several workgroups across and down
SIZES = [(1, 1), (2, 5), (3, 3), (7, 7), (8, 8), (8, 9), (9, 8), (16, 5), (5, 16), (8, 16), (16, 8), (24, 8),
         (8, 24), (40, 8), (24, 24), (25, 24), (17, 9), (33, 17), (15, 31), (37, 29), (64, 48), (129, 67), (1, 40),
         (40, 1), (129, 17), (129, 9), (300, 50)]
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
def reference(w, h, n, layout, quality):
    want = jpegc_ref(pixels(w, h, n), layout, quality)
    want.setflags(write=False)
    return want


def _same(got, want, what):
    assert got.dtype == want.dtype == np.int16 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        at = tuple(d[0])
        raise AssertionError(f"{what}: {len(d)} coefficients differ, first at {at} (block {at[-1] // 64}, "
                             f"coefficient {at[-1] % 64}): got {got[at]} want {want[at]}")


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


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_matches_the_reference(gpu, layout, n):
    for w, h in SIZES:
        px = pixels(w, h, n)
        for quality in QUALITIES:
            want = reference(w, h, n, layout, quality)
            assert want.shape == (n, jpegc_bytes(w, h, layout) // 2)
            for si, so in SKEWS:
                got = _under(si, so, lambda: gpu.rgb_to_jpegc(px, layout, quality))
                _same(got, want, f"rgb_to_jpegc {n}x{h}x{w} layout {layout} Q {quality} skew {si},{so}")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_under_every_pointer_alignment(gpu, layout):
    for w, h in [(8, 8), (37, 29), (129, 17), (129, 9)]:
        px, want = pixels(w, h, 3), reference(w, h, 3, layout, 90)
        for si, so in ALL_SKEWS:
            got = _under(si, so, lambda: gpu.rgb_to_jpegc(px, layout, 90))
            _same(got, want, f"rgb_to_jpegc 3x{h}x{w} layout {layout} skew {si},{so}")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_saturated_inputs_fit_int16(gpu, layout):
    """All 0, all 255 and {0, 255} patterns at Q 100 (every divisor 1): the largest coefficients."""
    w, h = 37, 29
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    checker = (((x + y) & 1) * 255).astype(np.uint8)
    rng = np.random.default_rng(11)
    imgs = np.stack([np.zeros((h, w, 3), np.uint8), np.full((h, w, 3), 255, np.uint8),
                     np.repeat(checker[:, :, None], 3, 2), np.repeat(255 - checker[:, :, None], 3, 2),
                     np.stack([checker, 255 - checker, checker], -1),
                     (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)])
    want = jpegc_ref(imgs, layout, 100)
    assert np.abs(want.astype(np.int32)).max() >= 1016        # a block of 255s: DC = 8 * 127 at divisor 1
    got = gpu.rgb_to_jpegc(imgs, layout, 100)
    _same(got, want, f"saturated, layout {layout}")
    for quality in (1, 50):
        _same(gpu.rgb_to_jpegc(imgs, layout, quality), jpegc_ref(imgs, layout, quality), f"saturated Q {quality}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    w, h = 37, 29
    px, want = pixels(w, h, 3), reference(w, h, 3, YCC_420, 90)
    other = px.copy()
    other[0] = 255 - other[0]
    other[2] = 255 - other[2]
    got = gpu.rgb_to_jpegc(other, YCC_420, 90)
    _same(got[1], want[1], "the middle image")


def test_wrapper_refuses_other_inputs(gpu):
    with pytest.raises(ValueError):
        gpu.rgb_to_jpegc(np.zeros((8, 8, 4), np.uint8), YCC_420, 75)
    with pytest.raises(ValueError):
        gpu.rgb_to_jpegc(np.zeros((8, 8, 3), np.uint8), 2, 75)
    with pytest.raises(gpu.MipxError):
        gpu.rgb_to_jpegc(np.zeros((8, 8, 3), np.uint8), YCC_420, 0)


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
    """Each plan runs without the step, then with it: the coefficients are the reference's of
    the engine's own RGB result."""
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
    want = jpegc_ref(rgb, layout, quality)
    q = gpu.plan_set_jpegc_output(_copy(gpu, p), layout, quality)
    assert q.n_steps == p.n_steps + 1 and (q.out_w, q.out_h, q.out_bands) == (p.out_w, p.out_h, 3)
    got = gpu.execute(q, src, wm=wm, junk=0x3C)
    _same(got, want, f"{name} layout {layout}")
    one = gpu.execute(q, src[1], wm=wm, junk=0xC3)
    _same(one[0], want[1], f"{name} layout {layout}, one image")
    if name == "chain":   # the step inside the last stage of the chain
        s0 = _plan(gpu, width=64)
        last = _plan(gpu, w=s0.out_w, h=s0.out_h, width=40, height=20, crop=1, sigma=1.2)
        gpu.plan_set_jpegc_output(last, layout, quality)
        assert bytes(gpu.plan_chain([s0, last])) == bytes(q)


# ---------------------------------------------------------------- the request path
def test_request_path_gives_coefficients(gpu):
    from imaginary_amd._abi import MipxImg
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        jobs = []     # (plan with the step, image, reference)
        for k, (w, h) in enumerate([(128, 96), (37, 29), (129, 17), (64, 48)]):
            layout, quality = [(YCC_420, 75), (YCC_444, 95)][k % 2]
            p = _plan(gpu, w=w, h=h, width=max(8, w // 2))
            q = gpu.plan_set_jpegc_output(_copy(gpu, p), layout, quality)
            for im in pixels(w, h, 3):
                jobs.append((q, im, jpegc_ref(eng.process(p, im), layout, quality)[0]))
        results = [None] * len(jobs)
        errors = []

        def work(t):
            try:
                subs = [(k, eng.submit(jobs[k][0], jobs[k][1])) for k in range(t, len(jobs), 4)]
                for k, (ticket, out) in subs:
                    eng.wait(ticket)
                    results[k] = out
            except Exception as e:  # noqa: BLE001 - reported by the main thread
                errors.append(e)

        threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        for k, (q, _, want) in enumerate(jobs):
            _same(results[k], want, f"request {k}")
        # a wrong-sized out is refused: by the wrapper, and by the library
        q, im, want = jobs[0]
        with pytest.raises(ValueError):
            eng.submit(q, im, out=np.zeros(want.size - 64, np.int16))
        with pytest.raises(ValueError):
            eng.submit(q, im, out=np.zeros((q.out_h, q.out_w, 3), np.uint8))
        dst = np.zeros(want.size, np.int16)
        t = C.c_uint64()
        src = MipxImg(im.ctypes.data, q.in_w, q.in_h, 3, 0)
        for w, h, b, stride in [(q.out_w, q.out_h, 3, 3 * q.out_w), (q.out_w, q.out_h, 1, 0), (128, want.size // 64, 1, 0),
                                (q.in_w, q.in_h, 3, 0)]:
            out = MipxImg(dst.ctypes.data, w, h, b, stride)
            assert gpu.lib.mipx_submit(-1, C.byref(q), C.byref(src), None, C.byref(out), C.byref(t)) == -1
        _same(eng.process(q, im), want, "after the refusals")
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
def _scan(buf):
    i = buf.index(b"\xff\xda")
    return buf[i + 2 + int.from_bytes(buf[i + 2:i + 4], "big"):-2]


@pytest.fixture
def coef_calls(monkeypatch):
    """Counts the requests that really left the engine as coefficients."""
    from imaginary_amd import imaginary
    calls = []
    real = imaginary.plan_set_jpegc_output

    def spy(plan, layout, quality):
        calls.append((layout, quality))
        return real(plan, layout, quality)

    monkeypatch.setattr(imaginary, "plan_set_jpegc_output", spy)
    return calls


@pytest.mark.parametrize("quality,layout", [(80, YCC_420), (95, YCC_444)])
@pytest.mark.parametrize("name", ["imaginary.jpg", "large.jpg"])
def test_process_bytes_gives_the_same_scan(gpu, coef_calls, name, quality, layout):
    PIL = pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = open(os.path.join(GOLDEN, "testdata", name), "rb").read()
    opts = dict(width=300, quality=quality)
    want = imaginary.process_bytes(buf, opts)
    assert coef_calls == []                        # the default changes nothing
    got = imaginary.process_bytes(buf, opts, jpeg_coefs=True)
    assert coef_calls == [(layout, quality)]
    assert got.mime == want.mime == "image/jpeg"
    assert _scan(got.body) == _scan(want.body)
    a, b = PIL.open(io.BytesIO(got.body)), PIL.open(io.BytesIO(want.body))
    assert a.size == b.size and np.array_equal(np.asarray(a), np.asarray(b))
    if name == "imaginary.jpg" and quality == 80:
        del coef_calls[:]
        # planar input and coefficient output together, at full size (no shrink-on-load)
        opts = dict(width=500, quality=quality)
        both = imaginary.process_bytes(buf, opts, ycc=True, jpeg_coefs=True)
        assert coef_calls == [(layout, quality)]
        assert _scan(both.body) == _scan(imaginary.process_bytes(buf, opts).body)
        del coef_calls[:]
        # other outputs keep the RGB path: a PNG answer, a grey answer
        png = imaginary.process_bytes(buf, dict(width=100, type="png"), jpeg_coefs=True)
        assert png.body == imaginary.process_bytes(buf, dict(width=100, type="png")).body
        grey = dict(width=100, interpretation=26)
        assert imaginary.process_bytes(buf, grey, jpeg_coefs=True).body == imaginary.process_bytes(buf, grey).body
        assert coef_calls == []
