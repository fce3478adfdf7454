"""Planar JPEG input on the device (MIPX_OP_YCC, k_ycc.hip) against tests/ycc_ref.py, the
numpy restatement of libjpeg's upsample and colour conversion that tests/test_ycc_cpu.py pins
to libjpeg-turbo itself: the kernel alone, as step 0 of plans, through the request path, and
end to end over encoded bytes.  Every comparison is exact."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from ycc_ref import YCC_420, YCC_444, ycc_bytes, ycc_ref

pytestmark = pytest.mark.gpu

# the CPU parity sizes (cw <= 2: 1x1 .. 2x5; one lane group; edges on both sides), then one
# past a lane group's multiple and one with several blocks across and down and a last wave
# that is partly empty
SIZES = [(1, 1), (2, 3), (3, 3), (4, 2), (5, 2), (2, 5), (6, 5), (17, 9), (37, 29), (64, 48), (129, 67),
         (130, 67), (515, 259)]
LAYOUTS = [YCC_444, YCC_420]
SKEWS = [(0, 0), (1, 3), (2, 1), (3, 2)]
ALL_SKEWS = [(i, o) for i in range(4) for o in range(4)]


@functools.lru_cache(maxsize=None)
def case(w, h, layout, n):
    """(planes (n, bytes), reference (n, h, w, 3)): full-range random planes, so the
    conversion clamps at both ends.  Computed once, read-only."""
    rng = np.random.default_rng(w * 100003 + h * 101 + layout * 7 + n)
    planes = rng.integers(0, 256, (n, ycc_bytes(w, h, layout)), dtype=np.uint8)
    want = ycc_ref(planes, w, h, layout)
    planes.setflags(write=False)
    want.setflags(write=False)
    return planes, want


def _same(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(d)} bytes differ, first at {tuple(d[0])}: "
                             f"got {got[tuple(d[0])]} want {want[tuple(d[0])]}")


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
    seen = set()
    for w, h in SIZES:
        planes, want = case(w, h, layout, n)
        seen |= set(np.unique(want).tolist())
        if w * h >= 100:
            assert want.min() == 0 and want.max() == 255, (w, h)
        for si, so in SKEWS:
            got = _under(si, so, lambda: gpu.ycc_to_rgb(planes, w, h, layout))
            _same(got, want, f"ycc_to_rgb {n}x{h}x{w} layout {layout} skew {si},{so}")
    assert 0 in seen and 255 in seen


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_under_every_pointer_alignment(gpu, layout):
    for w, h in [(5, 2), (37, 29), (130, 67)]:
        planes, want = case(w, h, layout, 3)
        for si, so in ALL_SKEWS:
            got = _under(si, so, lambda: gpu.ycc_to_rgb(planes, w, h, layout))
            _same(got, want, f"ycc_to_rgb 3x{h}x{w} layout {layout} skew {si},{so}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    """Images sit back to back at odd offsets: each output depends on its own planes only."""
    w, h = 37, 29
    planes, want = case(w, h, YCC_420, 3)
    other = planes.copy()
    other[0] = 255 - other[0]
    other[2] = 255 - other[2]
    got = gpu.ycc_to_rgb(other, w, h, YCC_420)
    _same(got[1], want[1], "the middle image")


# ---------------------------------------------------------------- as step 0 of a plan
W, H = 128, 96
PLANS = {
    "reduce2x2+extract": None,        # written out in _plan: 128x96 -> 64x48, then a 40x30 crop
    "rot90+flip": dict(rotate=90, flip=1),
    "blur": dict(sigma=1.5),
    "empty": dict(),
}


def _plan(gpu, name):
    if name == "reduce2x2+extract":   # written out: a 2 x 2 reduce to 64 x 48, then the crop
        p = gpu.plan_make(gpu.make_opts(width=64, height=48, force=1), gpu.make_input(W, H, 3, "png"))
        assert [s[0] for s in p.describe()] == ["reduce"] and p.steps[0].d[0] == 2.0 and p.steps[0].d[1] == 2.0
        s = p.steps[1]
        s.op = 5   # MIPX_OP_EXTRACT
        s.a[0], s.a[1], s.a[2], s.a[3] = 12, 9, 40, 30
        s.out_w, s.out_h, s.out_bands = 40, 30, 3
        p.n_steps = 2
        p.out_w, p.out_h = 40, 30
        return p
    return gpu.plan_make(gpu.make_opts(**PLANS[name]), gpu.make_input(W, H, 3, "png"))


def _copy(gpu, p):
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
@pytest.mark.parametrize("name", list(PLANS) + ["textmark"])
def test_plan_on_planes_equals_plan_on_rgb(gpu, name, layout):
    planes, rgb = case(W, H, layout, 2)
    wm = None
    if name == "textmark":
        p = _plan(gpu, "empty")
        gpu.plan_add_textmark(p, 33, 14, 20, 0.6, (255, 40, 0))
        wm = np.random.default_rng(3).integers(0, 256, (14, 33, 1), dtype=np.uint8)
    else:
        p = _plan(gpu, name)
    want = gpu.execute(p, rgb, wm=wm, junk=0x3C)
    q = gpu.plan_set_ycc_input(_copy(gpu, p), layout)
    assert q.n_steps == p.n_steps + 1
    got = gpu.execute(q, planes, wm=wm, junk=0x3C)
    assert got.shape == (2, p.out_h, p.out_w, p.out_bands)
    _same(got, want, f"{name} layout {layout}")
    if name == "empty":
        _same(got, rgb, "the step alone")
    one = gpu.execute(q, planes[1], wm=wm, junk=0xC3)   # (bytes,) input, another junk byte
    _same(one[0], want[1], f"{name} layout {layout}, one image")


def test_execute_refuses_planes_of_the_wrong_size(gpu):
    planes, _ = case(W, H, YCC_420, 2)
    q = gpu.plan_set_ycc_input(_plan(gpu, "blur"), YCC_420)
    with pytest.raises(ValueError):
        gpu.execute(q, planes[:, :-1])
    with pytest.raises(ValueError):
        gpu.execute(q, case(W, H, YCC_444, 2)[0])


# ---------------------------------------------------------------- the request path
def test_request_path_takes_planes(gpu):
    from imaginary_amd._abi import MipxImg
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        for layout in LAYOUTS:
            planes, rgb = case(W, H, layout, 2)
            more, more_rgb = case(W, H, layout, 3)
            p = _plan(gpu, "reduce2x2+extract")
            q = gpu.plan_set_ycc_input(_copy(gpu, p), layout)
            want = [eng.process(p, im) for im in list(rgb) + list(more_rgb)]
            _same(eng.process(q, planes[0]), want[0], f"process, layout {layout}")
            before = eng.stats(0)
            subs = [eng.submit(q, pl) for pl in list(planes) + list(more)]   # same plan: these fuse into batches
            for k, (t, out) in enumerate(subs):
                eng.wait(t)
                _same(out, want[k], f"batched submit {k}, layout {layout}")
            after = eng.stats(0)
            assert after[1] - before[1] == len(subs)
            # refused: the wrong number of bytes (here), a stride or another shape (the library)
            with pytest.raises(ValueError):
                eng.submit(q, planes[0][:-1])
            with pytest.raises(ValueError):
                eng.submit(q, rgb[0])
            dst = np.zeros((q.out_h, q.out_w, 3), np.uint8)
            out = MipxImg(dst.ctypes.data, q.out_w, q.out_h, 3, 0)
            t = C.c_uint64()
            for w, h, b, stride in [(W, H, 3, 3 * W), (W, H, 3, W), (W, H, 1, 0), (W, H + H // 2, 1, 0)]:
                src = MipxImg(planes[0].ctypes.data, w, h, b, stride)
                assert gpu.lib.mipx_submit(-1, C.byref(q), C.byref(src), None, C.byref(out), C.byref(t)) == -1
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
def _jpeg(w, h, subsampling):
    from PIL import Image
    px = np.random.default_rng(w * 7 + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    # smooth it a little so the planes are not pure noise, keep the full range
    px = ((px.astype(np.uint16) + np.roll(px, 1, 0) + np.roll(px, 1, 1)) // 3).astype(np.uint8)
    out = io.BytesIO()
    Image.fromarray(px).save(out, "JPEG", quality=92, subsampling=subsampling)
    return out.getvalue()


@pytest.fixture
def planar_calls(monkeypatch):
    """Counts the requests that really went to the engine as planes."""
    from imaginary_amd import imaginary
    calls = []
    real = imaginary.plan_set_ycc_input

    def spy(plan, layout):
        calls.append(layout)
        return real(plan, layout)

    monkeypatch.setattr(imaginary, "plan_set_ycc_input", spy)
    return calls


@pytest.mark.parametrize("w,h,subsampling,layout", [(131, 77, 2, YCC_420), (64, 48, 0, YCC_444)])
def test_process_bytes_gives_the_same_bytes(gpu, planar_calls, w, h, subsampling, layout):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = _jpeg(w, h, subsampling)
    for opts in (dict(width=60), dict(width=40, height=40, crop=1), dict()):
        del planar_calls[:]
        want = imaginary.process_bytes(buf, opts)
        assert planar_calls == []                      # the default changes nothing
        got = imaginary.process_bytes(buf, opts, ycc=True)
        assert planar_calls == [layout], opts
        assert got.body == want.body and got.mime == want.mime, opts
    del planar_calls[:]
    opts = dict(width=12)                              # shrink-on-load: the RGB decode
    assert imaginary.process_bytes(buf, opts, ycc=True).body == imaginary.process_bytes(buf, opts).body
    assert planar_calls == []


def test_process_bytes_on_a_rotated_file(gpu, planar_calls):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = open(os.path.join(GOLDEN, "testdata", "orient6.jpg"), "rb").read()
    opts = dict(width=300)       # EXIF rotation, then shrink-on-load: bimg's rotate and re-encode branch
    want = imaginary.process_bytes(buf, opts)
    got = imaginary.process_bytes(buf, opts, ycc=True)
    assert planar_calls == []
    assert got.body == want.body
    opts = dict(width=800)       # EXIF rotation at full size: planes, then the rotation on the engine
    got = imaginary.process_bytes(buf, opts, ycc=True)
    assert planar_calls == [YCC_420]
    assert got.body == imaginary.process_bytes(buf, opts).body
    png = open(os.path.join(GOLDEN, "testdata", "test.png"), "rb").read()
    del planar_calls[:]
    assert imaginary.process_bytes(png, dict(width=100), ycc=True).body == \
        imaginary.process_bytes(png, dict(width=100)).body
    assert planar_calls == []
