"""The JPEG round trip on the device (MIPX_OP_JPEGRT, k_jpegrt.hip + k_ycc.hip) against
tests/jpegrt_ref.py, the composition of the numpy restatements of libjpeg's encoder front half,
of its decoder at 1/1, 1/2, 1/4 and 1/8 and of its colour conversion, which
tests/test_jpegrt_cpu.py pins to libjpeg-turbo's encode -> decode itself: the kernel alone, as a
step in the middle of plans, through the request path, and end to end over encoded bytes, where
the step stands in for the host's re-encode and decode between pipeline stages and in front of a
rotated shrink-on-load.  Every comparison is exact."""
import functools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from footprint import FILL, guarded  # noqa: F401
from jpegrt_ref import YCC_420, YCC_444, jpegrt_ref

pytestmark = pytest.mark.gpu

LAYOUTS = [YCC_444, YCC_420]
SCALES = [1, 2, 4, 8]
QUALITIES = [1, 75, 90, 100]
SKEWS = [(0, 0), (1, 3), (2, 1), (3, 2)]
# below one block, one block, MCU padding in 4:2:0, partial edges, sizes where ceil(w / 8) is 1;
# 127 / 129 / 130 / 256 / 257 wide: one column short of a strip of 128, one and two past it, two
# whole strips and one column more; 129 x 16 and 256 x 8: a whole 4:2:0 and 4:4:4 strip row
SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 17), (37, 29), (127, 33), (130, 18), (257, 31),
         (129, 16), (256, 8)]
N = 3      # odd image strides put the second and third image on odd bytes


@functools.lru_cache(maxsize=None)
def pixels(w, h, kind):
    """(N, h, w, 3): full-range random, 0 / 255 only, or one constant colour per image.  Read-only."""
    rng = np.random.default_rng(w * 100003 + h * 101)
    if kind == "random":
        px = rng.integers(0, 256, (N, h, w, 3), dtype=np.uint8)
    elif kind == "0/255":
        px = (rng.integers(0, 2, (N, h, w, 3)) * 255).astype(np.uint8)
    else:
        px = np.broadcast_to(rng.integers(0, 256, (N, 1, 1, 3), dtype=np.uint8), (N, h, w, 3)).copy()
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def case(w, h, kind, layout, quality, s):
    """(pixels, the reference's round trip of them).  Computed once, read-only."""
    px = pixels(w, h, kind)
    want = jpegrt_ref(px, layout, quality, s)
    assert want.shape == (N, -(-h // s), -(-w // s), 3)
    want.setflags(write=False)
    return px, want


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
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_kernel_matches_the_reference(gpu, layout, s):
    for k, (w, h) in enumerate(SIZES):
        for kind in ("random", "0/255", "constant"):
            for quality in (QUALITIES if kind == "random" else (75,)):
                px, want = case(w, h, kind, layout, quality, s)
                si, so = SKEWS[(k + quality) % 4]
                got = _under(si, so, lambda: gpu.jpeg_roundtrip(px, layout, quality, s))
                _same(got, want, f"jpeg_roundtrip {N}x{h}x{w} {kind} layout {layout} Q {quality} 1/{s} skew {si},{so}")


@pytest.mark.parametrize("layout", LAYOUTS, ids=["444", "420"])
def test_one_image_and_every_pointer_alignment(gpu, layout):
    for s in SCALES:
        px, want = case(37, 29, "random", layout, 75, s)
        for si in range(4):
            for so in range(4):
                got = _under(si, so, lambda: gpu.jpeg_roundtrip(px[1], layout, 75, s))
                _same(got, want[1:2], f"one image, layout {layout} 1/{s} skew {si},{so}")


def test_one_image_of_a_batch_does_not_reach_into_the_next(gpu):
    px, want = case(37, 29, "random", YCC_420, 75, 2)
    other = px.copy()
    other[0], other[2] = 255 - px[0], px[2][::-1]
    got = gpu.jpeg_roundtrip(other, YCC_420, 75, 2)
    _same(got[1], want[1], "the middle image")
    assert not np.array_equal(got[0], want[0]) and not np.array_equal(got[2], want[2])


# ---------------------------------------------------------------- in the middle of a plan
W, H = 257, 131


def _plan(gpu, w, h, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


@pytest.mark.parametrize("layout,quality,s", [(YCC_420, 75, 1), (YCC_444, 92, 2), (YCC_420, 30, 4), (YCC_420, 75, 8)])
def test_plan_with_the_step_in_the_middle(gpu, layout, quality, s):
    """reduce -> JPEGRT -> extract as one plan equals the engine's own reduce, the reference's round
    trip of that, and the engine's extract of that; through mipx_execute_dev and the request path."""
    px = pixels(W, H, "random")[:2]
    front = _plan(gpu, W, H, width=150)
    mid = gpu.execute(front, px, junk=0x3C)
    rt = jpegrt_ref(mid, layout, quality, s)
    back = _plan(gpu, rt.shape[2], rt.shape[1], area_width=rt.shape[2] // 2, area_height=rt.shape[1] // 2, top=3, left=5)
    assert [st[0] for st in back.describe()] == ["extract"]
    want = gpu.execute(back, rt, junk=0x3C)
    gpu.plan_add_jpeg_roundtrip(front, layout, quality, s)
    one = gpu.plan_chain([front, back])
    assert [st[0] for st in one.describe()] == ["reduce", "jpegrt", "extract"]
    _same(gpu.execute(one, px, junk=0xC3), want, f"one plan, layout {layout} Q {quality} 1/{s}")
    if s == 2:
        gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
        eng = gpu.Engine(max_batch=4)
        try:
            _same(eng.process(one, px[1]), want[1], "through mipx_submit")
        finally:
            eng.shutdown()


# ---------------------------------------------------------------- end to end over bytes
def _read(name):
    return open(os.path.join(GOLDEN, "testdata", name), "rb").read()


@pytest.fixture
def runs(monkeypatch):
    """The plans of the engine runs of the operation layer, as MipxPlan.describe() gives them."""
    from imaginary_amd import imaginary
    calls = []
    real = imaginary._run

    def spy(plan, px, wm):
        calls.append(plan.describe())
        return real(plan, px, wm)

    monkeypatch.setattr(imaginary, "_run", spy)
    return calls


def _ops(*stages):
    return [dict(operation=name, params=params) for name, params in stages]


FUSED = {
    "crop-blur": _ops(("crop", dict(width=300, height=260)), ("blur", dict(sigma=2.0))),
    "resize-quarter-flip": _ops(("resize", dict(width=137)), ("flip", {})),      # 550 x 740 at 1/4 on the host
    # the third stage's file, 400 x 538, would shrink on load: the boundary in front of it decodes at that scale
    "resize-flip-resize": _ops(("resize", dict(width=400)), ("flip", {}), ("resize", dict(width=60))),
    "resize-png-rotate": _ops(("resize", dict(width=240)), ("convert", dict(type="png")), ("rotate", dict(rotate=90))),
    "quality-95": _ops(("resize", dict(width=333, quality=95)), ("crop", dict(width=200, height=150))),
    "rotate-shrinks-on-load": _ops(("crop", dict(width=500, height=600)), ("resize", dict(width=100, rotate=90))),
}


@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_pipeline_gives_the_same_bytes_in_one_run(gpu, runs, name):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = _read("imaginary.jpg")
    o = imaginary.ImageOptions(operations=FUSED[name])
    want = imaginary.Pipeline(buf, o)
    assert len(runs) >= len(FUSED[name])
    del runs[:]
    got = imaginary.Pipeline(buf, o, fused=True)
    assert len(runs) == 1, runs
    assert got.mime == want.mime and got.body == want.body, name
    steps = [st[0] for st in runs[0]]
    if name == "resize-png-rotate":
        assert steps.count("jpegrt") == 1      # the JPEG boundary only: PNG boundaries concatenate
    elif name == "rotate-shrinks-on-load":
        assert steps.count("jpegrt") == 2 and steps.index("rot") > steps.index("jpegrt")
    else:
        assert steps.count("jpegrt") == len(FUSED[name]) - 1


def test_the_boundary_shrinks_on_load(gpu, runs):
    """The third stage of resize-flip-resize plans load_shrink 4 on a 400 x 538 file, which the codec
    delivers at 1/2 (538 // 135 = 3): the boundary in front of it carries that scale, the first none."""
    from imaginary_amd import codec, imaginary
    imaginary.Pipeline(_read("imaginary.jpg"), imaginary.ImageOptions(operations=FUSED["resize-flip-resize"]), fused=True)
    rts = [st for st in runs[0] if st[0] == "jpegrt"]
    assert gpu.plan_make(gpu.make_opts(width=60, embed=1), gpu.make_input(400, 538, 3, "jpeg")).load_shrink == 4
    assert codec.decode_scale(400, 538, 4) == 2
    assert [st[1][:3] for st in rts] == [(YCC_420, 75, 1), (YCC_420, 75, 2)]
    assert [st[3] for st in rts] == [(400, 538, 3), (200, 269, 3)]


@pytest.mark.parametrize("name,stages", [
    ("bw", _ops(("resize", dict(width=200, colorspace="bw")), ("flip", {}))),
    ("two-watermarks", _ops(("watermarkImage", dict(image="x", opacity=0.5)), ("watermarkImage", dict(image="x", left=9)),
                            ("flip", {}))),
])
def test_pipelines_the_chain_cannot_stand_for_fall_back(gpu, runs, name, stages):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec, imaginary
    buf = _read("imaginary.jpg")
    kw = dict(wm=codec.decode(_read("test.png"))[:40, :60]) if name == "two-watermarks" else {}
    o = imaginary.ImageOptions(operations=stages)
    want = imaginary.Pipeline(buf, o, **kw)
    per_stage = len(runs)
    del runs[:]
    got = imaginary.Pipeline(buf, o, fused=True, **kw)
    assert len(runs) == per_stage >= 2     # today's loop ran
    assert got.mime == want.mime and got.body == want.body


ROTATED = [("orient6.jpg", {"width": 300}), ("orient6.jpg", {"width": 200, "height": 200}),
           ("imaginary.jpg", {"width": 200, "rotate": 90}), ("imaginary.jpg", {"width": 120, "flip": "true"})]


@pytest.mark.parametrize("fixture,query", ROTATED, ids=[f"{f}-{'-'.join(q)}" for f, q in ROTATED])
def test_device_reencode_gives_the_same_bytes_in_one_run(gpu, runs, fixture, query):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import imaginary
    buf = _read(fixture)
    o = imaginary.build_params_from_query({k: str(v) for k, v in query.items()})
    opts = imaginary.bimg_options(o)
    opts["embed"] = 1
    want = imaginary.process_bytes(buf, opts)
    assert len(runs) == 2 and all(st[0] != "jpegrt" for r in runs for st in r)
    del runs[:]
    got = imaginary.process_bytes(buf, opts, device_reencode=True)
    assert len(runs) == 1 and [st[0] for st in runs[0]].count("jpegrt") == 1, runs
    assert got.mime == want.mime and got.body == want.body
    # requests that do not rotate and shrink keep their path
    del runs[:]
    plain = dict(width=500)
    assert imaginary.process_bytes(_read("imaginary.jpg"), plain, device_reencode=True).body == \
        imaginary.process_bytes(_read("imaginary.jpg"), plain).body
    assert all(st[0] != "jpegrt" for r in runs for st in r)
