"""JPEG coefficient input at 1/2, 1/4 and 1/8 on the device (the scaled MIPX_OP_JPEGD step,
k_jpegds in k_jpegd.hip + k_ycc.hip) against tests/jpegds_ref.py and tests/ycc_ref.py, the numpy
restatements of libjpeg's shrink-on-load and of its colour conversion, which
tests/test_jpegds_cpu.py and tests/test_ycc_cpu.py pin to libjpeg-turbo itself: the kernel alone,
as step 0 of plans, through the request path, and end to end over encoded bytes.  Every comparison
is exact.  Files smaller than the scale in either dimension cannot be asked of Pillow: for those
the restatement alone is the yardstick."""
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
from jpegd_ref import YCC_420, YCC_444, jpegd_bytes, payload
from jpegds_ref import idct_sizes, jpegds_ref, out_size
from ycc_ref import ycc_ref

pytestmark = pytest.mark.gpu

# k_jpegds: a workgroup takes a run of 256 / N consecutive blocks of a block row for the N x N
# inverse DCT, and 1024 blocks of the (linear) block grid for N = 1
RUN = {8: 32, 4: 64, 2: 128}
DC_GROUP = 1024
LAYOUTS = [YCC_444, YCC_420]
SCALES = [2, 4, 8]
SKEWS = [(0, 0), (1, 3), (2, 1), (3, 2)]
ALL_SKEWS = [(i, o) for i in range(4) for o in range(4)]
# the smallest files at which the kernel can go wrong: below one block, one block, one block and
# one column or row, MCU padding in 4:2:0, several blocks with partial edges
BASE = [(1, 1), (2, 5), (7, 7), (8, 8), (9, 8), (8, 9), (15, 31), (16, 16), (17, 9), (33, 17), (37, 29), (129, 67)]
ALL_QUALITIES = [(8, 8), (37, 29), (129, 67)]      # the full quality list runs on these
QUALITIES = [1, 50, 90, 100]


def sizes(layout, s):
    """BASE, then the sizes the run lengths give.  For a component with run R, file width
    8 R + 1 (16 R + 1 for 4:2:0 chroma) leaves a last workgroup of one block that has one real
    column; height 9 (17) a last block row with one real row; 8 R - 1 is one column short of a
    full run; 300 x 50 is several workgroups across and down; 321 x 201 is 41 x 26 = 1066 blocks,
    a second N = 1 workgroup whose last lane has 2 of its 4 blocks."""
    out = list(BASE) + [(300, 50), (321, 201)]
    ny, nc, _ = idct_sizes(layout, s)
    if ny in RUN:
        out += [(8 * RUN[ny] + 1, 9), (8 * RUN[ny] - 1, 8)]
    if nc in RUN:
        out += [(16 * RUN[nc] + 1, 17)] if layout == YCC_420 else [(8 * RUN[nc] + 1, 9)]
    return sorted(set(out))


@functools.lru_cache(maxsize=None)
def pixels(w, h, n):
    """Full-range random RGB, (n, h, w, 3).  Computed once, read-only."""
    px = np.random.default_rng(w * 100003 + h * 101 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def payloads(w, h, n, layout, quality):
    """(n, bytes): the coefficients an encoder makes of random pixels at `quality`, with that
    quality's tables.  Computed once, read-only."""
    coefs = jpegc_ref(pixels(w, h, n), layout, quality)
    p = np.stack([payload(c, qtables(quality)) for c in coefs])
    assert p.shape == (n, jpegd_bytes(w, h, layout))
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def case(w, h, n, layout, quality, s):
    """(payloads, the reference's RGB (n, oh, ow, 3)) of w x h files decoded at 1/s."""
    p = payloads(w, h, n, layout, quality)
    ow, oh = out_size(w, h, s)
    rgb = ycc_ref(jpegds_ref(p, w, h, layout, s), ow, oh, YCC_444)
    assert rgb.shape == (n, oh, ow, 3)
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


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_matches_the_reference(gpu, layout, s, n):
    for w, h in sizes(layout, s):
        for quality in (QUALITIES if (w, h) in ALL_QUALITIES else (50, 100)):
            p, want = case(w, h, n, layout, quality, s)
            for si, so in SKEWS:
                got = _under(si, so, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, layout, s))
                _same(got, want, f"jpegd_to_rgb_scaled {n}x{h}x{w} layout {layout} 1/{s} Q {quality} skew {si},{so}")


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_under_every_pointer_alignment(gpu, layout, s):
    for w, h in [(8, 8), (37, 29), (129, 67), sizes(layout, s)[-1]]:
        p, want = case(w, h, 3, layout, 90, s)
        for si, so in ALL_SKEWS:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, layout, s))
            _same(got, want, f"jpegd_to_rgb_scaled 3x{h}x{w} layout {layout} 1/{s} skew {si},{so}")


def test_shrink_one_is_the_full_size_call(gpu):
    p = payloads(37, 29, 2, YCC_420, 90)
    _same(gpu.jpegd_to_rgb_scaled(p, 37, 29, YCC_420, 1), gpu.jpegd_to_rgb(p, 37, 29, YCC_420), "shrink 1")


def _hand_made(w, h, layout):
    """Payloads whose blocks are tests/test_jpegd_gpu.py's saturating and wrapping ones."""
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


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_the_rule_is_total(gpu, layout, s):
    """Coefficients no encoder writes: full-range random int16 with random tables, and hand-made
    blocks that saturate pass 1 and wrap the dequantisation.  The restatement alone is the
    yardstick here."""
    rng = np.random.default_rng(77 + s)
    passes = any(n > 1 for n in idct_sizes(layout, s))   # N = 1 has no pass 1 to saturate
    for w, h in [(37, 29), (129, 17)]:
        n = 3
        ow, oh = out_size(w, h, s)
        coefs = rng.integers(-32768, 32768, (n, jpegc_bytes(w, h, layout) // 2), dtype=np.int16)
        p = np.stack([payload(c, rng.integers(1, 256, (3, 64))) for c in coefs])
        trace = {}
        want = ycc_ref(jpegds_ref(p, w, h, layout, s, trace), ow, oh, YCC_444)
        assert (trace.get("saturated", 0) > 0) == passes   # the saturation really fires
        for si, so in SKEWS:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, layout, s))
            _same(got, want, f"random coefficients {h}x{w} layout {layout} 1/{s} skew {si},{so}")
        p = _hand_made(w, h, layout)
        trace = {}
        want = ycc_ref(jpegds_ref(p, w, h, layout, s, trace), ow, oh, YCC_444)
        assert (trace.get("saturated", 0) > 0) == passes
        _same(gpu.jpegd_to_rgb_scaled(p, w, h, layout, s), want, f"hand-made blocks {h}x{w} layout {layout} 1/{s}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    w, h, s = 37, 29, 2
    p, want = case(w, h, 3, YCC_420, 90, s)
    other = p.copy()
    other[0] = payloads(w, h, 3, YCC_420, 50)[0]
    other[2] = payloads(w, h, 3, YCC_420, 1)[2]
    got = gpu.jpegd_to_rgb_scaled(other, w, h, YCC_420, s)
    _same(got[1], want[1], "the middle image")
    assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[2], want[2])


def test_wrapper_refuses_other_inputs(gpu):
    p = payloads(16, 8, 1, YCC_444, 90)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb_scaled(p[:, :-1], 16, 8, YCC_444, 2)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb_scaled(p, 16, 8, YCC_444, 3)
    with pytest.raises(ValueError):
        gpu.jpegd_to_rgb_scaled(p, 16, 8, YCC_420, 2)    # 4 blocks, not 6


# ---------------------------------------------------------------- as step 0 of a plan
W, H = 257, 131     # the file


def _copy(gpu, p):
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _plan(gpu, w, h, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


@pytest.mark.parametrize("layout,quality", [(YCC_444, 92), (YCC_420, 75)], ids=["444", "420"])
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["reduce", "crop", "flip", "empty", "chain", "+jpegc output"])
def test_plan_with_the_step_equals_the_plan_on_the_references_rgb(gpu, name, s, layout, quality):
    """Each plan runs on RGB = ycc_ref(jpegds_ref(payload)), then on the payload with the step."""
    src, rgb = case(W, H, 2, layout, quality, s)
    ow, oh = out_size(W, H, s)
    if name == "reduce":
        p = _plan(gpu, ow, oh, width=max(ow * 2 // 3, 1))
    elif name == "crop":
        p = _plan(gpu, ow, oh, width=max(ow // 2, 1), height=max(oh // 3, 1), crop=1)
    elif name == "flip":
        p = _plan(gpu, ow, oh, flip=1)
    elif name == "chain":
        s0 = _plan(gpu, ow, oh, width=max(ow // 2, 2))
        p = gpu.plan_chain([s0, _plan(gpu, s0.out_w, s0.out_h, flop=1)])
    elif name == "+jpegc output":
        p = gpu.plan_set_jpegc_output(_plan(gpu, ow, oh, width=max(ow * 2 // 3, 1)), YCC_420, 80)
    else:
        p = _plan(gpu, ow, oh)
    want = gpu.execute(p, rgb, junk=0x3C)
    q = gpu.plan_set_jpegd_input_scaled(_copy(gpu, p), layout, s, W, H)
    assert q.n_steps == p.n_steps + 1 and (q.out_w, q.out_h, q.out_bands) == (p.out_w, p.out_h, p.out_bands)
    got = gpu.execute(q, src, junk=0x3C)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), f"{name} layout {layout} 1/{s}"
    if name == "empty":
        _same(got, rgb, "the step alone")
        # ... and with the coefficient step right behind it: the encoder's rule on that RGB
        both = gpu.plan_set_jpegc_output(_copy(gpu, q), YCC_420, 80)
        assert np.array_equal(gpu.execute(both, src, junk=0x3C), jpegc_ref(rgb, YCC_420, 80))
    one = gpu.execute(q, src[1], junk=0xC3)   # (bytes,) input, another junk byte
    assert np.array_equal(one[0], want[1]), f"{name} layout {layout} 1/{s}, one image"


def test_execute_refuses_payloads_of_the_wrong_size(gpu):
    ow, oh = out_size(W, H, 2)
    q = gpu.plan_set_jpegd_input_scaled(_plan(gpu, ow, oh, width=60), YCC_420, 2, W, H)
    with pytest.raises(ValueError):
        gpu.execute(q, payloads(W, H, 2, YCC_420, 75)[:, :-1])
    with pytest.raises(ValueError):
        gpu.execute(q, payloads(W, H, 2, YCC_444, 92))
    with pytest.raises(ValueError):   # the payload of a file of the DECODED size
        gpu.execute(q, payloads(ow, oh, 2, YCC_420, 75))


# ---------------------------------------------------------------- the request path
def test_request_path_takes_coefficients_at_a_scale(gpu):
    from imaginary_amd._abi import MipxImg
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        jobs = []     # (plan with the step, payload, what the plan makes of the reference's RGB)
        for k, (w, h, s) in enumerate([(257, 131, 2), (129, 67, 4), (300, 50, 8), (37, 29, 2), (64, 48, 4)]):
            layout = [YCC_420, YCC_444][k % 2]
            ow, oh = out_size(w, h, s)
            p = _plan(gpu, ow, oh, width=max(2, ow // 2))
            q = gpu.plan_set_jpegd_input_scaled(_copy(gpu, p), layout, s, w, h)
            # one plan, requests with different tables: they may share a batch
            for quality in (30, 92):
                src, rgb = case(w, h, 3, layout, quality, s)
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
        dst = np.zeros((q.out_h, q.out_w, 3), np.uint8)
        out = MipxImg(dst.ctypes.data, q.out_w, q.out_h, 3, 0)
        t = C.c_uint64()
        for w, h, b, stride in [(q.in_w, q.in_h, 3, 3 * q.in_w), (q.in_w, q.in_h, 1, 0), (257, 131, 3, 0),
                                (q.out_w, q.out_h, 3, 0)]:
            img = MipxImg(src.ctypes.data, w, h, b, stride)
            assert gpu.lib.mipx_submit(-1, C.byref(q), C.byref(img), None, C.byref(out), C.byref(t)) == -1
        _same(eng.process(q, src), want, "after the refusals")
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
@functools.lru_cache(maxsize=None)
def _jpeg(quality, subsampling, w, h):
    """A small JPEG of a crop of a photograph: small, so the Python entropy decode is short."""
    from PIL import Image
    from imaginary_amd import codec
    px = codec.decode(open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read())[200:200 + h, 100:100 + w]
    assert px.shape == (h, w, 3)
    out = io.BytesIO()
    Image.fromarray(px).save(out, "JPEG", quality=quality, subsampling=subsampling)
    return out.getvalue()


@pytest.fixture
def scaled_calls(monkeypatch):
    """Records the requests that really went to the engine as coefficients through the new setter."""
    from imaginary_amd import imaginary
    calls = []
    real = imaginary.plan_set_jpegd_input_scaled

    def spy(plan, layout, shrink, file_w, file_h):
        calls.append((layout, shrink, file_w, file_h))
        return real(plan, layout, shrink, file_w, file_h)

    monkeypatch.setattr(imaginary, "plan_set_jpegd_input_scaled", spy)
    return calls


def _load_shrink(gpu, w, h, opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "jpeg")).load_shrink


@pytest.mark.parametrize("w,h", [(320, 240), (317, 211)], ids=lambda v: str(v))
@pytest.mark.parametrize("quality,subsampling,layout", [(80, 2, YCC_420), (95, 0, YCC_444)])
def test_process_bytes_gives_the_same_bytes(gpu, scaled_calls, quality, subsampling, layout, w, h):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec, imaginary
    buf = _jpeg(quality, subsampling, w, h)
    seen = set()
    for width, shrink in [(100, 2), (40, 4), (18, 8)]:
        opts = dict(width=width)
        assert _load_shrink(gpu, w, h, opts) == shrink
        scale = codec.decode_scale(w, h, shrink)
        seen.add((shrink, scale))
        del scaled_calls[:]
        want = imaginary.process_bytes(buf, opts)
        assert imaginary.process_bytes(buf, opts, jpeg_dct=True).body == want.body
        assert scaled_calls == []                      # without the new flag nothing changes
        got = imaginary.process_bytes(buf, opts, jpeg_dct=True, jpeg_dct_shrink=True)
        assert scaled_calls == [(layout, scale, w, h)], opts
        assert got.body == want.body and got.mime == want.mime, opts
    if (w, h) == (320, 240):
        assert seen == {(2, 2), (4, 4), (8, 8)}
    else:   # 317 // ceil(317 / 2) = 1, 317 // 80 = 3, 317 // 40 = 7: the codec delivers less than asked
        assert seen == {(2, 1), (4, 2), (8, 4)}
    # a crop, and coefficients in at 1/s and coefficients out
    del scaled_calls[:]
    opts = dict(width=80, height=50, crop=1, quality=quality)
    shrink = _load_shrink(gpu, w, h, dict(width=80, height=50, crop=1))
    assert shrink > 1
    both = imaginary.process_bytes(buf, opts, jpeg_dct=True, jpeg_dct_shrink=True, jpeg_coefs=True)
    assert scaled_calls == [(layout, codec.decode_scale(w, h, shrink), w, h)]
    assert both.body == imaginary.process_bytes(buf, opts, jpeg_coefs=True).body
    assert imaginary.process_bytes(buf, opts, jpeg_dct=True, jpeg_dct_shrink=True).body == \
        imaginary.process_bytes(buf, opts).body


def test_process_bytes_keeps_todays_path_elsewhere(gpu, scaled_calls):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = _jpeg(80, 2, 320, 240)
    flags = dict(jpeg_dct=True, jpeg_dct_shrink=True)
    # a request that rotates and shrinks on load: the rotate-and-re-encode path
    opts = dict(width=60, rotate=90)
    assert _load_shrink(gpu, 320, 240, opts) > 1
    assert imaginary.process_bytes(buf, opts, **flags).body == imaginary.process_bytes(buf, opts).body
    # a file that is no JPEG
    png = open(os.path.join(GOLDEN, "testdata", "test.png"), "rb").read()
    opts = dict(width=100)
    assert imaginary.process_bytes(png, opts, **flags).body == imaginary.process_bytes(png, opts).body
    # the new flag alone, and a file the coefficient reader declines (progressive)
    from PIL import Image
    out = io.BytesIO()
    Image.open(io.BytesIO(buf)).save(out, "JPEG", quality=80, progressive=True)
    opts = dict(width=70)
    assert imaginary.process_bytes(buf, opts, jpeg_dct_shrink=True).body == imaginary.process_bytes(buf, opts).body
    assert imaginary.process_bytes(out.getvalue(), opts, **flags).body == \
        imaginary.process_bytes(out.getvalue(), opts).body
    assert scaled_calls == []
    # a full-size request under both flags is today's coefficient request
    assert imaginary.process_bytes(buf, dict(width=300), **flags).body == \
        imaginary.process_bytes(buf, dict(width=300)).body
    assert scaled_calls == []
