"""Text watermark on the device (k_textmark.hip, MIPX_OP_TEXTMARK), bit for bit against
a numpy restatement of PARITY_ASSUMPTIONS.md's text-watermark rows: per op over odd
sizes, both band counts, batches whose images start at every alignment, masks that wrap,
clip, vanish or exceed the image; at skewed buffer alignments; as a plan step; through
the request path; and through imaginary.Watermark with a stub renderer."""
import itertools
import os

import numpy as np
import pytest

from conftest import ROOT
from footprint import FILL, guarded  # noqa: F401

pytestmark = pytest.mark.gpu
TESTDATA = os.path.join(ROOT, "tests", "golden", "testdata")


# ---------------------------------------------------------------- the reference (numpy, from the parity rows)
def ref_textmark(img, T, margin, opacity, colour):
    """img (h, w, b) with b 1 or 3, T (th, tw) uint8 -> (h, w, 3) uint8."""
    h, w, b = img.shape
    th, tw = T.shape
    f = T.astype(np.float32) * np.float32(opacity)                       # vips_linear1, float32
    M = np.clip(np.trunc(f), 0, 255).astype(np.uint8)                    # vips_cast: truncate, clip
    Tw, Th = tw + margin, th + margin
    tile = np.zeros((Th, Tw), np.uint8)                                  # vips_embed at (100, 100), black
    if Th > 100 and Tw > 100:
        tile[100:100 + th, 100:100 + tw] = M[:Th - 100, :Tw - 100]
    m = tile[np.arange(h) % Th][:, np.arange(w) % Tw].astype(np.int64)[:, :, None]   # replicate + crop
    base = img.astype(np.int64) if b == 3 else np.repeat(img.astype(np.int64), 3, axis=2)
    c = np.asarray(colour, np.int64)[None, None, :]
    return ((m * c + (255 - m) * base + 128) // 255).astype(np.uint8)    # vips_ifthenelse(blend)


def assert_same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    d = np.argwhere(got != want)
    assert d.size == 0, (what, len(d), "first at", d[0].tolist(), int(got[tuple(d[0])]), int(want[tuple(d[0])]))


# ---------------------------------------------------------------- per op
IMAGES = [(1, 1), (3, 5), (101, 101), (130, 259), (240, 331)]
MASKS = [(8, 12, 100), (20, 30, 90), (5, 9, 1), (40, 60, 0), (1, 1, 250)]     # (th, tw, margin)
OPACITY = [0.25, 0.5, 0.999, 1.0]
COLOUR = [(0, 0, 0), (255, 255, 255), (1, 128, 254)]


def _cases():
    """Every (image, bands, n) with the masks, opacities and colours dealt round, twice with
    different deals: 40 cases in which every listed value occurs."""
    shapes = list(itertools.product(IMAGES, (1, 3), (1, 3)))
    out = []
    for rnd in range(2):
        for i, ((h, w), b, n) in enumerate(shapes):
            k = i + 7 * rnd
            out.append((h, w, b, n, MASKS[(k + 2 * rnd) % 5], OPACITY[(k + rnd) % 4], COLOUR[k % 3]))
    return out


CASES = _cases()


# every listed value occurs
assert 24 <= len(CASES) <= 60
assert {(c[0], c[1]) for c in CASES} == set(IMAGES) and {c[2] for c in CASES} == {1, 3}
assert {c[3] for c in CASES} == {1, 3} and {c[4] for c in CASES} == set(MASKS)
assert {c[5] for c in CASES} == set(OPACITY) and {c[6] for c in CASES} == set(COLOUR)


@pytest.mark.parametrize("h,w,b,n,mask,opacity,colour", CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}-n{c[3]}-m{c[4][0]}x{c[4][1]}+{c[4][2]}-o{c[5]}-c{c[6][1]}"
                              for c in CASES])
def test_op_matches_the_reference(gpu, h, w, b, n, mask, opacity, colour):
    r = np.random.default_rng(h * 1000 + w * 10 + b + n)
    th, tw, margin = mask
    imgs = r.integers(0, 256, (n, h, w, b), dtype=np.uint8)
    T = r.integers(0, 256, (th, tw), dtype=np.uint8)
    T.flat[0], T.flat[-1] = 255, 0
    got = gpu.run_op("textmark", imgs, mask=T, margin=margin, opacity=opacity, colour=colour)
    assert got.shape == (n, h, w, 3)
    for i in range(n):
        assert_same(got[i], ref_textmark(imgs[i], T, margin, opacity, colour), f"image {i}")


def test_zero_mask_reproduces_the_input(gpu):
    r = np.random.default_rng(5)
    imgs = r.integers(0, 256, (2, 67, 131, 3), dtype=np.uint8)
    got = gpu.run_op("textmark", imgs, mask=np.zeros((30, 40), np.uint8), margin=3, opacity=1.0, colour=(255, 0, 9))
    assert_same(got, imgs, "all-zero mask")
    grey = r.integers(0, 256, (2, 67, 131, 1), dtype=np.uint8)
    got = gpu.run_op("textmark", grey, mask=np.zeros((30, 40), np.uint8), margin=3, opacity=1.0, colour=(255, 0, 9))
    assert_same(got, np.repeat(grey, 3, axis=3), "all-zero mask, grey")


@pytest.mark.parametrize("skew_in,skew_out,b", [(1, 0, 3), (2, 0, 3), (3, 0, 3), (0, 1, 3), (0, 2, 3), (0, 3, 3),
                                                (3, 1, 3), (1, 2, 1), (2, 3, 1), (3, 0, 1), (0, 1, 1)])
def test_any_buffer_alignment(gpu, skew_in, skew_out, b):
    """The ABI allows image pointers of any byte alignment: the aligned core moves, the
    head and tail bytes change, the result does not, and the guards stay clean (run_op
    checks them before it returns)."""
    from imaginary_amd import engine
    r = np.random.default_rng(10 * skew_in + skew_out + b)
    imgs = r.integers(0, 256, (3, 37, 53, b), dtype=np.uint8)
    T = r.integers(0, 256, (9, 14), dtype=np.uint8)
    prev = engine.set_guard(FILL, skew_in, skew_out)
    try:
        before = engine.guarded_calls()
        got = gpu.run_op("textmark", imgs, mask=T, margin=97, opacity=0.75, colour=(250, 3, 77))
        assert engine.guarded_calls() == before + 1
    finally:
        engine.set_guard(*prev)
    for i in range(3):
        assert_same(got[i], ref_textmark(imgs[i], T, 97, 0.75, (250, 3, 77)), f"image {i}")


# ---------------------------------------------------------------- as a plan step
def test_plan_resize_textmark_bw(gpu, oracle):
    r = np.random.default_rng(11)
    imgs = r.integers(0, 256, (2, 216, 384, 3), dtype=np.uint8)
    T = r.integers(0, 256, (14, 33), dtype=np.uint8)
    opts = dict(width=192, height=108, embed=1)
    plan = gpu.plan_make(gpu.make_opts(interpretation=26, **opts), gpu.make_input(384, 216, 3, "png"))
    assert [s[0] for s in plan.describe()] == ["reduce", "bw"]
    gpu.plan_add_textmark(plan, 33, 14, 70, 0.0, (255, 40, 0))             # opacity 0 -> 0.25
    assert [s[0] for s in plan.describe()] == ["reduce", "textmark", "bw"]
    got = gpu.execute(plan, imgs, wm=T[:, :, None], junk=0x3C)
    e, rp = oracle.plan(opts, dict(w=384, h=216, bands=3, type=3))
    assert e == 0
    for i in range(2):
        small = oracle.execute(rp, imgs[i])
        assert small.shape == (108, 192, 3)
        assert_same(got[i], oracle.bw(ref_textmark(small, T, 70, 0.25, (255, 40, 0))), f"image {i}")


def test_plan_on_a_grey_image(gpu, oracle):
    r = np.random.default_rng(12)
    img = r.integers(0, 256, (1, 90, 150, 1), dtype=np.uint8)
    T = r.integers(0, 256, (6, 21), dtype=np.uint8)
    plan = gpu.plan_make(gpu.make_opts(sigma=1.5, min_ampl=0.2), gpu.make_input(150, 90, 1, "png"))
    gpu.plan_add_textmark(plan, 21, 6, 95, 0.6, (7, 200, 90))
    assert [s[0] for s in plan.describe()] == ["blur", "textmark"] and plan.out_bands == 3
    got = gpu.execute(plan, img, wm=T[:, :, None], junk=0x3C)
    blurred = oracle.gaussblur(img[0], 1.5, 0.2).reshape(90, 150, 1)
    assert_same(got[0], ref_textmark(blurred, T, 95, np.float32(0.6), (7, 200, 90)), "grey")


# ---------------------------------------------------------------- request path
def test_requests_keep_their_own_text(gpu):
    """Three requests in flight on one plan, two with the same mask and one with another
    mask of the same size: each gets its own text (a batch shares only byte-identical masks)."""
    from imaginary_amd import imaginary as im
    r = np.random.default_rng(13)
    plan = gpu.plan_make(gpu.make_opts(), gpu.make_input(157, 93, 3, "png"))
    gpu.plan_add_textmark(plan, 25, 10, 40, 0.9, (10, 20, 30))
    imgs = [r.integers(0, 256, (93, 157, 3), dtype=np.uint8) for _ in range(3)]
    a = r.integers(0, 256, (10, 25, 1), dtype=np.uint8)
    b = r.integers(0, 256, (10, 25, 1), dtype=np.uint8)
    masks = [a, b, a.copy()]
    eng = im.engine()
    assert_same(eng.process(plan, imgs[0], masks[0]),
                ref_textmark(imgs[0], a[:, :, 0], 40, np.float32(0.9), (10, 20, 30)), "process")
    tickets = [eng.submit(plan, img, m) for img, m in zip(imgs, masks)]
    for (t, out), img, m in zip(tickets, imgs, masks):
        eng.wait(t)
        assert_same(out, ref_textmark(img, m[:, :, 0], 40, np.float32(0.9), (10, 20, 30)), "submit")
    with pytest.raises(gpu.MipxError) as e:
        eng.submit(plan, imgs[0], np.zeros((10, 24, 1), np.uint8))
    assert e.value.code == gpu.MIPX_EINVAL


# ---------------------------------------------------------------- imaginary.Watermark
def _stub(mask, asked):
    def render(text, font, width, dpi):
        asked.append((text, font, width, dpi))
        return mask
    return render


def test_watermark_on_decoded_pixels(gpu):
    from imaginary_amd import imaginary as im
    r = np.random.default_rng(14)
    px = r.integers(0, 256, (120, 212, 3), dtype=np.uint8)
    mask = r.integers(0, 256, (11, 28), dtype=np.uint8)
    asked = []
    o = im.build_params_from_query({"text": "engine", "opacity": "0.8", "color": "255,200,0", "margin": "110"})
    got = im.Watermark(im.Decoded(px, type="png"), o, render=_stub(mask, asked))
    assert asked == [("engine", "sans 10", 212 // 6, 150)]
    assert_same(got, ref_textmark(px, mask, 110, np.float32(0.8), (255, 200, 0)), "Watermark(Decoded)")
    # the Go defaults: margin 0 -> the text width, opacity 0 -> 0.25, no colour -> black
    got = im.Watermark(im.Decoded(px, type="png"), im.build_params_from_query({"text": "engine"}),
                       render=_stub(mask, asked))
    assert_same(got, ref_textmark(px, mask, 212 // 6, 0.25, (0, 0, 0)), "defaults")


def test_watermark_as_a_pipeline_stage(gpu, oracle):
    from imaginary_amd import imaginary as im
    r = np.random.default_rng(15)
    px = r.integers(0, 256, (216, 384, 3), dtype=np.uint8)
    mask = r.integers(0, 256, (9, 31), dtype=np.uint8)
    ops = [{"operation": "resize", "params": {"width": 192, "height": 108}},
           {"operation": "watermark", "params": {"text": "t", "margin": 101, "opacity": 1, "color": "0,255,0"}},
           {"operation": "flip", "params": {}}]
    got = im.Pipeline(im.Decoded(px, type="png"), im.build_params_from_query({"operations": ops}),
                      render=_stub(mask, []))
    small = oracle.reduce(px, 2.0, 2.0)
    assert_same(got, oracle.flip(ref_textmark(small, mask, 101, 1.0, (0, 255, 0)), 0), "pipeline")


def test_watermark_over_encoded_bytes(gpu):
    from imaginary_amd import codec
    from imaginary_amd import imaginary as im
    with open(os.path.join(TESTDATA, "imaginary.jpg"), "rb") as f:
        body = f.read()
    asked = []
    mask = np.full((12, 40), 255, np.uint8)
    img = im.Watermark(body, im.build_params_from_query({"text": "hello", "opacity": "0.5", "color": "255,0,0"}),
                       render=_stub(mask, asked))
    assert img.mime == "image/jpeg"
    h = codec.header(img.body)
    assert (h.w, h.h) == (550, 740)
    assert asked == [("hello", "sans 10", 550 // 6, 150)]


def test_watermark_on_an_alpha_image_falls_back(gpu):
    from imaginary_amd import imaginary as im
    px = np.zeros((40, 60, 4), np.uint8)
    with pytest.raises(im.EngineUnsupported):
        im.Watermark(im.Decoded(px, type="png"), im.build_params_from_query({"text": "x"}),
                     render=_stub(np.ones((3, 4), np.uint8), []))
