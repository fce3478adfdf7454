"""The JPEG round trip (MIPX_OP_JPEGRT), the parts that need no GPU:

 - the pixel rule (tests/jpegrt_ref.py: jpegc_ref -> jpegd_ref / jpegds_ref -> ycc_ref, unchanged,
   which the GPU tests hold the kernel to) is pinned to a real upstream library: it equals
   libjpeg-turbo's encode -> decode inside Pillow (draft for s > 1), bit for bit, at every scale
   Pillow can be made to decode at (every file not smaller than s; that includes every case in
   which codec.decode_scale says the codec delivers s), and pass 1 never saturates on the way;
 - the planner entry point, the plan validation and the argument checks of the C-ABI.
"""
import ctypes as C
import io

import numpy as np
import pytest

from jpegrt_ref import YCC_420, YCC_444, jpegrt_ref

SIZES = [(1, 1), (7, 5), (8, 8), (16, 16), (17, 9), (33, 17), (37, 29), (127, 33), (130, 18), (257, 31)]
QUALITIES = [1, 30, 75, 90, 100]
SCALES = [1, 2, 4, 8]
SUBSAMPLING = {YCC_444: 0, YCC_420: 2}   # Pillow's names for 4:4:4 and 4:2:0
OP_JPEGRT = 18


def picture(w, h, kind):
    rng = np.random.default_rng(1000 * w + h)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "0/255":
        return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    y, x = np.mgrid[0:h, 0:w]   # smooth: a gradient per band plus a little noise
    px = np.stack([(3 * x + 2 * y) % 256, (255 - 2 * x + y) % 256, (x * y // 4) % 256], axis=-1)
    return np.clip(px + rng.integers(-3, 4, px.shape), 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- real-library parity
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_composed_reference_equals_libjpeg_encode_then_decode(w, h, layout):
    PIL = pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    for kind in ("random", "smooth", "0/255"):
        px = picture(w, h, kind)
        for quality in QUALITIES:
            out = io.BytesIO()
            PIL.fromarray(px).save(out, "JPEG", quality=quality, subsampling=SUBSAMPLING[layout])
            for s in SCALES:
                if min(w, h) < s:
                    assert codec.decode_scale(w, h, s) < s
                    continue   # Pillow cannot be asked for less than one sample: the GPU tests run these
                im = PIL.open(io.BytesIO(out.getvalue()))
                if s > 1:
                    im.draft("RGB", (w // s, h // s))
                    assert im.decoderconfig[0] == s, (w, h, s, im.decoderconfig)
                want = np.asarray(im.convert("RGB"), dtype=np.uint8)
                trace = {}
                got = jpegrt_ref(px, layout, quality, s, trace)
                assert trace.get("saturated", 0) == 0, (w, h, layout, kind, quality, s, trace)
                assert got.shape == (1,) + want.shape and np.array_equal(got[0], want), (w, h, layout, kind, quality, s)


# ---------------------------------------------------------------- planner
def _plan(ia, w, h, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def _copy(ia, p):
    return ia.MipxPlan.from_buffer_copy(bytes(p))


def test_abi_version_stays():
    from imaginary_amd import _abi
    assert _abi.lib.mipx_abi_version() == 6 and _abi.OP_JPEGRT == OP_JPEGRT and _abi.OP_NAMES[18] == "jpegrt"


@pytest.mark.parametrize("shrink", [0, 1, 2, 4, 8])
def test_the_step_is_appended_with_the_scaled_geometry(shrink):
    import imaginary_amd as ia
    s = max(shrink, 1)
    for layout, quality in [(YCC_444, 92), (YCC_420, 75), (YCC_420, 1), (YCC_444, 100)]:
        p = _plan(ia, 129, 67, width=61)
        before, (w, h) = p.describe(), (p.out_w, p.out_h)
        geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands)
        assert ia.lib.mipx_plan_add_jpeg_roundtrip(C.byref(p), layout, quality, shrink) == 0
        ow, oh = -(-w // s), -(-h // s)
        assert p.describe() == before + [("jpegrt", (layout, quality, shrink, 0, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 3))]
        assert (p.load_shrink, p.in_w, p.in_h, p.in_bands) == geom and (p.out_w, p.out_h, p.out_bands) == (ow, oh, 3)
        # the plan validates: its workspace holds the step's input and its planes
        assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= 2 * 3 * (w * h + ow * oh)
    # on an empty plan the step is the whole plan
    e = ia.plan_add_jpeg_roundtrip(_plan(ia, 37, 29), YCC_420, 75, s)
    assert [st[0] for st in e.describe()] == ["jpegrt"] and (e.out_w, e.out_h) == (-(-37 // s), -(-29 // s))
    need = 3 * 3 * e.out_w * e.out_h
    assert need <= ia.lib.mipx_workspace_bytes(C.byref(e), 3) < need + 4096
    assert ia.lib.mipx_op_workspace_bytes(OP_JPEGRT, 3, 37, 29, 3, float(shrink), 0.0) >= need
    assert ia.lib.mipx_op_workspace_bytes(OP_JPEGRT, 3, 37, 29, 3, float(shrink), 0.0) <= 3 * 37 * 29 * 3 + 256


def test_refusals_leave_the_plan_untouched():
    import imaginary_amd as ia
    add = ia.lib.mipx_plan_add_jpeg_roundtrip
    p = _plan(ia, 129, 67, width=61)
    untouched = bytes(p)
    assert add(None, YCC_420, 75, 1) == -1
    for layout in (2, -1, 7):
        assert add(C.byref(p), layout, 75, 1) == -1
    for quality in (0, 101, -5, 1000):
        assert add(C.byref(p), YCC_420, quality, 1) == -1
    for shrink in (3, 5, 6, 7, 16, -1, -2):
        assert add(C.byref(p), YCC_420, 75, shrink) == -1
    assert bytes(p) == untouched
    for bands, opts in [(1, {}), (4, {}), (3, dict(interpretation=26))]:       # out_bands != 3
        q = _plan(ia, 64, 48, bands, **opts)
        assert q.out_bands != 3
        before = bytes(q)
        assert add(C.byref(q), YCC_420, 75, 1) == -1 and bytes(q) == before
    c = ia.plan_set_jpegc_output(_plan(ia, 64, 48, width=32), YCC_420, 75)       # ends with JPEGC
    before = bytes(c)
    assert add(C.byref(c), YCC_420, 75, 1) == -1 and bytes(c) == before
    full = _plan(ia, 64, 48)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = 64, 48, 3
    before = bytes(full)
    assert add(C.byref(full), YCC_420, 75, 1) == -1 and bytes(full) == before
    big = _plan(ia, 30000, 30000)   # 4:4:4 coefficients of 2^32 bytes or more; the 4:2:0 ones fit
    before = bytes(big)
    assert ia.jpegd_bytes(30000, 30000, YCC_444) > 2 ** 32 > ia.jpegd_bytes(30000, 30000, YCC_420)
    assert add(C.byref(big), YCC_444, 75, 1) == -1 and bytes(big) == before
    assert add(C.byref(big), YCC_420, 75, 1) == 0


def test_the_step_composes_with_the_text_watermark_and_coefficient_output():
    import imaginary_amd as ia
    a = _plan(ia, 129, 67, width=61)
    ia.plan_add_textmark(a, 10, 4, 3, 0.5, (1, 2, 3))
    ia.plan_add_jpeg_roundtrip(a, YCC_420, 75, 2)
    ia.plan_set_jpegc_output(a, YCC_444, 95)
    b = _plan(ia, 129, 67, width=61)
    ia.plan_add_jpeg_roundtrip(b, YCC_420, 75, 2)
    ia.plan_set_jpegc_output(b, YCC_444, 95)
    ia.plan_add_textmark(b, 10, 4, 3, 0.5, (1, 2, 3))    # goes in front of both
    assert [st[0] for st in a.describe()] == ["reduce", "textmark", "jpegrt", "jpegc"]
    assert a.describe() == b.describe() and bytes(a) == bytes(b)
    assert (a.out_w, a.out_h) == (31, 16) and a.describe()[1][3] == (61, 32, 3)
    assert ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    c = _plan(ia, 129, 67, width=61)
    ia.plan_add_jpeg_roundtrip(c, YCC_444, 100, 1)
    ia.plan_add_textmark(c, 10, 4, 3, 0.5, (1, 2, 3))
    assert [st[0] for st in c.describe()] == ["reduce", "textmark", "jpegrt"]
    assert ia.lib.mipx_workspace_bytes(C.byref(c), 1) > 0
    # two round trips in a row are legal: the step may stand anywhere
    ia.plan_add_jpeg_roundtrip(c, YCC_420, 30, 4)
    assert [st[0] for st in c.describe()][-2:] == ["jpegrt", "jpegrt"] and ia.lib.mipx_workspace_bytes(C.byref(c), 1) > 0


def test_chain_takes_the_step_in_any_stage():
    import imaginary_amd as ia
    s0 = ia.plan_add_jpeg_roundtrip(_plan(ia, 257, 131, width=120), YCC_420, 75, 1)
    # the next stage would shrink on load at 1/2: the shrink rides in the middle stage's round trip
    s1 = ia.plan_add_jpeg_roundtrip(_plan(ia, s0.out_w, s0.out_h, flip=1), YCC_444, 95, 2)
    s2 = _plan(ia, s1.out_w, s1.out_h, width=20)
    merged = ia.plan_chain([s0, s1, s2])
    assert [st[0] for st in merged.describe()][:4] == ["reduce", "jpegrt", "flip", "jpegrt"]
    assert merged.n_steps == s0.n_steps + s1.n_steps + s2.n_steps
    assert (s1.out_w, s1.out_h) == (60, 31) and (merged.out_w, merged.out_h) == (s2.out_w, s2.out_h)
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    first = ia.plan_chain([ia.plan_add_jpeg_roundtrip(_plan(ia, 64, 48), YCC_420, 75, 4), _plan(ia, 16, 12, flop=1)])
    assert [st[0] for st in first.describe()] == ["jpegrt", "flip"] and ia.lib.mipx_workspace_bytes(C.byref(first), 1) > 0


def _hand_plan(ia, a, w, h, bands=3, index=0):
    """A plan written by hand: flips with a JPEGRT step with arguments `a` at `index`."""
    s = a[2] if len(a) > 2 and a[2] in (2, 4, 8) else 1
    ow, oh = -(-w // s), -(-h // s)
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = ow, oh, bands
    p.n_steps = 3
    for i in range(3):
        p.steps[i].op = OP_JPEGRT if i == index else 2
        after = i >= index
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = (ow, oh, bands) if after else (w, h, bands)
    for k, v in enumerate(a):
        p.steps[index].a[k] = v
    return p


def test_hand_written_steps_are_validated_before_any_device_work():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    for index in (0, 1, 2):
        for a in [(YCC_420, 75, 0), (YCC_444, 100, 1), (YCC_420, 1, 2), (YCC_444, 50, 4), (YCC_420, 90, 8)]:
            assert L.mipx_workspace_bytes(C.byref(_hand_plan(ia, a, 33, 17, index=index)), 1) > 0, (index, a)
    # what the planner call writes is what a hand-written plan must hold
    made = ia.plan_add_jpeg_roundtrip(_plan(ia, 33, 17, flip=1), YCC_420, 75, 2)
    hand = _hand_plan(ia, (YCC_420, 75, 2), 33, 17, index=1)
    hand.n_steps = 2
    assert made.describe() == hand.describe()
    bad = [_hand_plan(ia, (7, 75, 1), 33, 17), _hand_plan(ia, (-1, 75, 1), 33, 17),        # unknown layout
           _hand_plan(ia, (YCC_420, 0, 1), 33, 17), _hand_plan(ia, (YCC_420, 101, 1), 33, 17),   # quality
           _hand_plan(ia, (YCC_420, -3, 1), 33, 17),
           _hand_plan(ia, (YCC_420, 75, 3), 33, 17), _hand_plan(ia, (YCC_420, 75, 16), 33, 17),  # shrink
           _hand_plan(ia, (YCC_420, 75, -2), 33, 17, index=1),
           _hand_plan(ia, (YCC_420, 75, 1), 33, 17, bands=1), _hand_plan(ia, (YCC_420, 75, 1), 33, 17, bands=4),
           _hand_plan(ia, (YCC_444, 75, 1), 30000, 30000, index=2)]                        # 2^32 bytes
    wrong = _hand_plan(ia, (YCC_420, 75, 2), 33, 17, index=1)    # the step says the unscaled size
    wrong.steps[1].out_w, wrong.steps[1].out_h = 33, 17
    for p in bad + [wrong]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, None, None, None, None, 0, None) == -1
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
        if p.in_w > 1000:
            continue
        data = np.zeros((p.in_h, p.in_w, p.in_bands), np.uint8)
        dst = np.zeros((p.out_h, p.out_w, p.out_bands), np.uint8)
        src = MipxImg(data.ctypes.data, p.in_w, p.in_h, p.in_bands, 0)
        out = MipxImg(dst.ctypes.data, p.out_w, p.out_h, p.out_bands, 0)
        t = C.c_uint64()
        assert L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t)) == -1


def test_entry_point_rejects_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    L = ia.lib
    EINVAL = -1
    big = 1 << 40
    f = L.mipx_op_jpeg_roundtrip
    for s in (0, 1, 2, 4, 8):
        assert f(None, 1, 1, 8, 8, YCC_420, 75, s, 1, big, None) == EINVAL
        assert f(1, None, 1, 8, 8, YCC_420, 75, s, 1, big, None) == EINVAL
        assert f(1, 1, 0, 8, 8, YCC_420, 75, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 0, 8, YCC_420, 75, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, -1, YCC_444, 75, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, 8, 2, 75, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, 8, YCC_420, 0, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, 8, YCC_420, 101, s, 1, big, None) == EINVAL
        need = L.mipx_op_workspace_bytes(OP_JPEGRT, 2, 37, 29, 3, float(s), 0.0)
        assert need >= 2 * 3 * -(-37 // max(s, 1)) * -(-29 // max(s, 1))
        assert f(1, 1, 2, 37, 29, YCC_420, 75, s, None, big, None) == EINVAL
        assert f(1, 1, 2, 37, 29, YCC_420, 75, s, 1, need - 1, None) == EINVAL
        assert f(1, 1, 1, 30000, 30000, YCC_444, 75, s, 1, big, None) == -2
    for s in (3, 5, 16, -1):
        assert f(1, 1, 1, 8, 8, YCC_420, 75, s, 1, big, None) == EINVAL


def test_wrapper_checks_its_arguments_without_a_device():
    import imaginary_amd as ia
    with pytest.raises(ValueError):
        ia.jpeg_roundtrip(np.zeros((8, 8, 4), np.uint8), YCC_444, 75)
    with pytest.raises(ValueError):
        ia.jpeg_roundtrip(np.zeros((8, 8, 3), np.uint8), YCC_444, 75, 3)
    with pytest.raises(ValueError):
        ia.jpeg_roundtrip(np.zeros((8, 8, 3), np.uint8), 2, 75)
