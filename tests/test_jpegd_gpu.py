"""JPEG coefficient input on the device (MIPX_OP_JPEGD, k_jpegd.hip + k_ycc.hip) against
tests/jpegd_ref.py and tests/ycc_ref.py, the numpy restatements of libjpeg's dequantisation and
inverse DCT and of its upsample and colour conversion, which tests/test_jpegd_cpu.py and
tests/test_ycc_cpu.py pin to libjpeg-turbo itself: the kernel alone, as step 0 of plans, through
the request path, and end to end over encoded bytes.  Every comparison is exact."""
import ctypes as C
import functools
import io
import os
import threading

import numpy as np
import pytest

from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegc_ref import jpegc_bytes, jpegc_ref, qtables
from jpegd_ref import YCC_420, YCC_444, jpegd_bytes, jpegd_ref, payload
from ycc_ref import ycc_ref

pytestmark = pytest.mark.gpu

RUN = 32    # k_jpegd.hip kRun: a workgroup takes 32 consecutive blocks of a block row, 8 RUN samples
# tests/test_jpegc_gpu.py's sizes; then, from RUN: 8 RUN + 1 = 257 columns leave a last workgroup
# of one block that has one real column, 9 rows a last block row with one real row (Y, and
# 4:4:4 chroma); 8 RUN - 1 = 255 x 8 is one workgroup short of one column; 16 RUN + 1 = 513 x 17
# does to the 257 x 9 chroma planes of 4:2:0 what 257 x 9 does to Y; 300 x 50 is several
# workgroups across and down
SIZES = [(1, 1), (2, 5), (3, 3), (7, 7), (8, 8), (8, 9), (9, 8), (16, 5), (5, 16), (8, 16), (16, 8), (24, 8),
         (8, 24), (40, 8), (24, 24), (25, 24), (17, 9), (33, 17), (15, 31), (37, 29), (64, 48), (129, 67), (1, 40),
         (40, 1), (129, 17), (129, 9), (300, 50),
         (8 * RUN + 1, 9), (8 * RUN - 1, 8), (16 * RUN + 1, 17)]
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
def case(w, h, n, layout, quality):
    """(payloads (n, bytes), the reference's RGB (n, h, w, 3)): the coefficients an encoder makes of
    random pixels at `quality`, with that quality's tables.  Computed once, read-only."""
    coefs = jpegc_ref(pixels(w, h, n), layout, quality)
    p = np.stack([payload(c, qtables(quality)) for c in coefs])
    assert p.shape == (n, jpegd_bytes(w, h, layout))
    rgb = ycc_ref(jpegd_ref(p, w, h, layout), w, h, layout)
    p.setflags(write=False)
    rgb.setflags(write=False)
    return p, rgb


def _same(got, want, what):
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        at = tuple(d[0])
        raise AssertionError(f"{what}: {len(d)} bytes differ, first at {at}: got {got[at]} want {want[at]}")


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
        for quality in QUALITIES:
            p, want = case(w, h, n, layout, quality)
            for si, so in SKEWS:
                got = _under(si, so, lambda: gpu.jpegd_to_rgb(p, w, h, layout))
                _same(got, want, f"jpegd_to_rgb {n}x{h}x{w} layout {layout} Q {quality} skew {si},{so}")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_under_every_pointer_alignment(gpu, layout):
    for w, h in [(8, 8), (37, 29), (129, 17), (8 * RUN + 1, 9)]:
        p, want = case(w, h, 3, layout, 90)
        for si, so in ALL_SKEWS:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb(p, w, h, layout))
            _same(got, want, f"jpegd_to_rgb 3x{h}x{w} layout {layout} skew {si},{so}")


def _hand_made(w, h, layout):
    """Payloads whose first blocks are tests/test_jpegd_cpu.py's saturating and wrapping ones."""
    blocks = [({0: 257}, 255), ({0: 300}, 255), ({0: 32767}, 1), ({0: -32768}, 1), ({0: 20000, 4: -8000}, 1),
              ({0: -20000, 4: 8000, 32: 32767, 63: -32768}, 1), ({k: 32767 for k in range(64)}, 255),
              ({k: -32768 if k & 1 else 32767 for k in range(64)}, 1)]
    out = []
    for values, q in blocks:
        c = np.zeros(jpegc_bytes(w, h, layout) // 2, np.int16)
        for at in range(0, c.size, 64 * 3):            # every third block of every component
            for k, v in values.items():
                c[at + k] = v
        out.append(payload(c, [np.full(64, q)]))
    return np.stack(out)


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_the_rule_is_total(gpu, layout):
    """Coefficients no encoder writes: full-range random int16 with random tables, and hand-made
    blocks that saturate pass 1 and wrap the dequantisation.  The reference alone is the
    yardstick here (libjpeg-turbo's SIMD inverse DCT differs on such input)."""
    rng = np.random.default_rng(77)
    for w, h in [(37, 29), (129, 17)]:
        n = 3
        coefs = rng.integers(-32768, 32768, (n, jpegc_bytes(w, h, layout) // 2), dtype=np.int16)
        p = np.stack([payload(c, rng.integers(1, 256, (3, 64))) for c in coefs])
        trace = {}
        want = ycc_ref(jpegd_ref(p, w, h, layout, trace), w, h, layout)
        assert trace["saturated"] > 0                  # the saturation really fires
        for si, so in SKEWS:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb(p, w, h, layout))
            _same(got, want, f"random coefficients {h}x{w} layout {layout} skew {si},{so}")
        p = _hand_made(w, h, layout)
        trace = {}
        want = ycc_ref(jpegd_ref(p, w, h, layout, trace), w, h, layout)
        assert trace["saturated"] > 0
        _same(gpu.jpegd_to_rgb(p, w, h, layout), want, f"hand-made blocks {h}x{w} layout {layout}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    w, h = 37, 29
    p, want = case(w, h, 3, YCC_420, 90)
    other = p.copy()
    other[0] = case(w, h, 3, YCC_420, 50)[0][0]
    other[2] = case(w, h, 3, YCC_420, 1)[0][2]
    got = gpu.jpegd_to_rgb(other, w, h, YCC_420)
    _same(got[1], want[1], "the middle image")
    assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[2], want[2])


def test_wrapper_refuses_other_inputs(gpu):
    p, _ = case(16, 8, 1, YCC_444, 90)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb(p[:, :-1], 16, 8, YCC_444)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb(p, 16, 8, 2)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb(p, 16, 8, YCC_420)    # 4 blocks, not 6


# ---------------------------------------------------------------- as step 0 of a plan
W, H = 128, 96


def _copy(gpu, p):
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _plan(gpu, w=W, h=H, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


@pytest.mark.parametrize("layout,quality", [(YCC_444, 92), (YCC_420, 75)], ids=["444", "420"])
@pytest.mark.parametrize("name", ["reduce", "rot90", "chain", "empty", "textmark", "+jpegc output"])
def test_plan_with_the_step_equals_the_plan_on_the_references_rgb(gpu, name, layout, quality):
    """Each plan runs on RGB = ycc_ref(jpegd_ref(payload)), then on the payload with the step."""
    wm = None
    w, h = (37, 29) if name == "rot90" else (W, H)
    src, rgb = case(w, h, 2, layout, quality)
    if name == "reduce":
        p = _plan(gpu, width=60)
    elif name == "rot90":
        p = _plan(gpu, w=37, h=29, rotate=90)
        assert (p.out_w, p.out_h) == (29, 37)
    elif name == "chain":
        s0 = _plan(gpu, width=64)
        p = gpu.plan_chain([s0, _plan(gpu, w=s0.out_w, h=s0.out_h, width=40, height=20, crop=1, sigma=1.2)])
    elif name == "textmark":
        p = _plan(gpu)
        gpu.plan_add_textmark(p, 33, 14, 20, 0.6, (255, 40, 0))
        wm = np.random.default_rng(3).integers(0, 256, (14, 33, 1), dtype=np.uint8)
    elif name == "+jpegc output":
        p = gpu.plan_set_jpegc_output(_plan(gpu, width=60), YCC_420, 80)
    else:
        p = _plan(gpu)
    want = gpu.execute(p, rgb, wm=wm, junk=0x3C)
    q = gpu.plan_set_jpegd_input(_copy(gpu, p), layout)
    assert q.n_steps == p.n_steps + 1 and (q.out_w, q.out_h, q.out_bands) == (p.out_w, p.out_h, p.out_bands)
    got = gpu.execute(q, src, wm=wm, junk=0x3C)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), f"{name} layout {layout}"
    if name == "empty":
        _same(got, rgb, "the step alone")
    one = gpu.execute(q, src[1], wm=wm, junk=0xC3)   # (bytes,) input, another junk byte
    assert np.array_equal(one[0], want[1]), f"{name} layout {layout}, one image"
    if name == "chain":   # the step inside stage 0 of the chain
        s0 = gpu.plan_set_jpegd_input(_plan(gpu, width=64), layout)
        last = _plan(gpu, w=s0.out_w, h=s0.out_h, width=40, height=20, crop=1, sigma=1.2)
        assert bytes(gpu.plan_chain([s0, last])) == bytes(q)


def test_execute_refuses_payloads_of_the_wrong_size(gpu):
    src, _ = case(W, H, 2, YCC_420, 75)
    q = gpu.plan_set_jpegd_input(_plan(gpu, width=60), YCC_420)
    with pytest.raises(ValueError):
        gpu.execute(q, src[:, :-1])
    with pytest.raises(ValueError):
        gpu.execute(q, case(W, H, 2, YCC_444, 92)[0])


# ---------------------------------------------------------------- the request path
def test_request_path_takes_coefficients(gpu):
    from imaginary_amd._abi import MipxImg
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        jobs = []     # (plan with the step, payload, what the plan makes of the reference's RGB)
        for k, (w, h) in enumerate([(128, 96), (37, 29), (129, 17), (64, 48)]):
            layout = [YCC_420, YCC_444][k % 2]
            p = _plan(gpu, w=w, h=h, width=max(8, w // 2))
            q = gpu.plan_set_jpegd_input(_copy(gpu, p), layout)
            # one plan, requests with different tables: they may share a batch
            for quality in (30, 92):
                src, rgb = case(w, h, 3, layout, quality)
                for i in range(3):
                    jobs.append((q, src[i], eng.process(p, rgb[i])))
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
        # refused: the wrong number of bytes (the wrapper), a stride or another shape (the library)
        q, src, want = jobs[0]
        with pytest.raises(ValueError):
            eng.submit(q, src[:-1])
        with pytest.raises(ValueError):
            eng.submit(q, case(128, 96, 3, YCC_420, 30)[1][0])
        dst = np.zeros((q.out_h, q.out_w, 3), np.uint8)
        out = MipxImg(dst.ctypes.data, q.out_w, q.out_h, 3, 0)
        t = C.c_uint64()
        for w, h, b, stride in [(q.in_w, q.in_h, 3, 3 * q.in_w), (q.in_w, q.in_h, 3, 128), (q.in_w, q.in_h, 1, 0),
                                (128, src.size // 128, 1, 0), (q.out_w, q.out_h, 3, 0)]:
            img = MipxImg(src.ctypes.data, w, h, b, stride)
            assert gpu.lib.mipx_submit(-1, C.byref(q), C.byref(img), None, C.byref(out), C.byref(t)) == -1
        _same(eng.process(q, src), want, "after the refusals")
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
@functools.lru_cache(maxsize=None)
def _jpeg(quality, subsampling):
    """A 320 x 240 JPEG of a crop of a photograph: small, so the Python entropy decode is short."""
    from PIL import Image
    from imaginary_amd import codec
    px = codec.decode(open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read())[200:440, 100:420]
    assert px.shape == (240, 320, 3)
    out = io.BytesIO()
    Image.fromarray(px).save(out, "JPEG", quality=quality, subsampling=subsampling)
    return out.getvalue()


@pytest.fixture
def dct_calls(monkeypatch):
    """Counts the requests that really went to the engine as coefficients."""
    from imaginary_amd import imaginary
    calls = []
    real = imaginary.plan_set_jpegd_input

    def spy(plan, layout):
        calls.append(layout)
        return real(plan, layout)

    monkeypatch.setattr(imaginary, "plan_set_jpegd_input", spy)
    return calls


@pytest.mark.parametrize("quality,subsampling,layout", [(80, 2, YCC_420), (95, 0, YCC_444)])
def test_process_bytes_gives_the_same_bytes(gpu, dct_calls, quality, subsampling, layout):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = _jpeg(quality, subsampling)
    for opts in (dict(width=300), dict(width=200, height=200, crop=1), dict(rotate=90)):
        del dct_calls[:]
        want = imaginary.process_bytes(buf, opts)
        assert dct_calls == []                         # the default changes nothing
        got = imaginary.process_bytes(buf, opts, jpeg_dct=True)
        assert dct_calls == [layout], opts
        assert got.body == want.body and got.mime == want.mime, opts
    # coefficients in and coefficients out: the host only entropy-decodes and entropy-codes
    del dct_calls[:]
    opts = dict(width=300, quality=quality)
    both = imaginary.process_bytes(buf, opts, jpeg_dct=True, jpeg_coefs=True)
    assert dct_calls == [layout]
    assert both.body == imaginary.process_bytes(buf, opts, jpeg_coefs=True).body
    # with ycc too, the coefficients are tried first
    del dct_calls[:]
    assert imaginary.process_bytes(buf, dict(width=300), ycc=True, jpeg_dct=True).body == \
        imaginary.process_bytes(buf, dict(width=300)).body
    assert dct_calls == [layout]
    # not taken: a shrink-on-load request, and a file that is no JPEG
    del dct_calls[:]
    opts = dict(width=100)
    assert imaginary.process_bytes(buf, opts, jpeg_dct=True).body == imaginary.process_bytes(buf, opts).body
    png = open(os.path.join(GOLDEN, "testdata", "test.png"), "rb").read()
    assert imaginary.process_bytes(png, opts, jpeg_dct=True).body == imaginary.process_bytes(png, opts).body
    assert dct_calls == []
