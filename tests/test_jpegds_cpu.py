"""JPEG coefficient input at 1/2, 1/4 and 1/8 (the scaled MIPX_OP_JPEGD step), the parts that need
no GPU:

 - the pixel rule (tests/jpegds_ref.py, which the GPU tests hold the kernel to) is pinned to a real
   upstream library: libjpeg-turbo inside Pillow.  jpegds_ref of what codec.decode_jpeg_coefs reads
   from a file equals Pillow's draft("YCbCr") decode of that file plane by plane, and ycc_ref of it
   equals the draft("RGB") decode, bit for bit, on every file here; none is excluded.  Pillow
   cannot be asked for a scale that leaves less than one sample (a file smaller than s in either
   dimension): for those the restatement alone is the yardstick, and the GPU tests run them;
 - codec.decode_scale against the shape codec.decode really returns;
 - known answers of the reference;
 - the planner entry point, the plan validation and the argument checks of the C-ABI.
"""
import ctypes as C
import functools
import io

import numpy as np
import pytest

from jpegc_ref import jpegc_bytes
from jpegd_ref import YCC_420, YCC_444, jpegd_bytes, payload
from jpegds_ref import idct_sizes, jpegds_ref, out_size
from ycc_ref import ycc_ref

PIL = pytest.importorskip("PIL.Image")

SIZES = [(8, 8), (9, 8), (8, 9), (17, 9), (16, 16), (33, 17), (37, 29), (53, 37), (64, 48), (129, 67), (257, 9)]
SCALES = [2, 4, 8]
QUALITIES = [1, 30, 75, 95, 100]
SUBSAMPLING = {YCC_444: 0, YCC_420: 2}   # Pillow's names for 4:4:4 and 4:2:0


def save(im, fmt="JPEG", **kw):
    out = io.BytesIO()
    im.save(out, fmt, **kw)
    return out.getvalue()


def picture(w, h, kind, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    # smooth: a gradient per band plus a little noise, what a photograph's blocks look like
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([(3 * x + 2 * y) % 256, (255 - 2 * x + y) % 256, (x * y // 4) % 256], axis=-1)
    return np.clip(px + rng.integers(-3, 4, px.shape), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def encoded(w, h, layout, quality, kind):
    """(file, its coefficient payload): the pure-Python entropy decode runs once per file."""
    from imaginary_amd import codec
    buf = save(PIL.fromarray(picture(w, h, kind, quality)), quality=quality, subsampling=SUBSAMPLING[layout])
    got = codec.decode_jpeg_coefs(buf)
    assert got is not None and got[1] == layout and got[0].shape == (jpegd_bytes(w, h, layout),)
    return buf, got[0]


def drafted(buf, mode, w, h, s):
    """Pillow's decode of the file at 1/s, in `mode`; the scale it really took is asserted."""
    im = PIL.open(io.BytesIO(buf))
    im.draft(mode, (w // s, h // s))
    assert im.decoderconfig[0] == s, (w, h, s, im.decoderconfig)
    assert im.mode == mode
    return np.asarray(im, dtype=np.uint8)


# ---------------------------------------------------------------- real-library parity
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_reference_equals_libjpeg_scaled_decode(w, h, layout):
    for quality in QUALITIES:
        for kind in ("random", "smooth"):
            buf, p = encoded(w, h, layout, quality, kind)
            for s in SCALES:
                ow, oh = out_size(w, h, s)
                trace = {}
                planes = jpegds_ref(p, w, h, layout, s, trace)
                assert planes.shape == (3 * ow * oh,)
                assert trace.get("saturated", 0) == 0, trace   # an encoder's coefficients never saturate
                what = (w, h, layout, quality, kind, s)
                ycc = drafted(buf, "YCbCr", w, h, s)
                assert ycc.shape == (oh, ow, 3), what
                for k, name in enumerate(("Y", "Cb", "Cr")):
                    assert np.array_equal(planes[k * ow * oh:(k + 1) * ow * oh].reshape(oh, ow), ycc[:, :, k]), \
                        what + (name,)
                assert np.array_equal(ycc_ref(planes, ow, oh, YCC_444), drafted(buf, "RGB", w, h, s)), what


def test_decode_scale_is_the_scale_the_codec_delivers():
    from imaginary_amd import codec
    assert codec.decode_scale(53, 37, 2) == 1          # 53 // 27 = 1: Pillow cannot reach 27 columns at 1/2
    assert codec.decode_scale(64, 48, 8) == 8 and codec.decode_scale(64, 48, 1) == 1
    sizes = sorted({(w, h) for w in (8, 9, 15, 16, 17, 23, 24, 25, 31, 32, 33, 53, 63, 64, 65)
                    for h in (8, 9, 16, 17, 37, 64)})
    for w, h in sizes:
        buf = save(PIL.fromarray(picture(w, h, "smooth")), quality=75)
        for s in (1, 2, 4, 8):
            scale = codec.decode_scale(w, h, s)
            assert scale in (1, 2, 4, 8) and scale <= s
            assert codec.decode(buf, s).shape == (-(-h // scale), -(-w // scale), 3), (w, h, s, scale)


# ---------------------------------------------------------------- known answers of the reference
def _planes(values, q, w, h, layout, s):
    """The three planes of a w x h file whose every block has coefficients {natural index: value}."""
    c = np.zeros(jpegc_bytes(w, h, layout) // 2, np.int16)
    for at in range(0, c.size, 64):
        for k, v in values.items():
            c[at + k] = v
    trace = {}
    ow, oh = out_size(w, h, s)
    return jpegds_ref(payload(c, [np.full(64, q)]), w, h, layout, s, trace).reshape(3, oh, ow).astype(int), trace


def test_reference_known_answers():
    for layout in (YCC_444, YCC_420):
        for s in SCALES:
            assert idct_sizes(layout, s)[0] == 8 // s
            assert (_planes({}, 1, 16, 16, layout, s)[0] == 128).all()
            # DC only: every N gives round(dc * q / 8), as the full-size decode does
            for dc, q in [(1, 1), (-1, 1), (3, 1), (4, 1), (-5, 1), (10, 16), (-10, 16), (50, 8), (-64, 16), (30, 255)]:
                got, trace = _planes({0: dc}, q, 16, 16, layout, s)
                want = min(max(((dc * q + 4) >> 3) + 128, 0), 255)
                assert (got == want).all() and trace.get("saturated", 0) == 0, (layout, s, dc, q)
    assert idct_sizes(YCC_420, 2) == [4, 8, 8] and idct_sizes(YCC_420, 4) == [2, 4, 4]
    assert idct_sizes(YCC_420, 8) == [1, 2, 2] and idct_sizes(YCC_444, 8) == [1, 1, 1]
    # the rows and columns a pass never reads do not matter: row 4 and column 4 at N = 4 ...
    a, _ = _planes({1: 40, 8: -30, 9: 7}, 2, 8, 8, YCC_444, 2)
    b, _ = _planes({1: 40, 8: -30, 9: 7, 4: 500, 32: -500, 36: 99, 12: 77, 33: -77}, 2, 8, 8, YCC_444, 2)
    assert np.array_equal(a, b) and len(np.unique(a)) > 1
    # ... and rows and columns 2, 4, 6 at N = 2
    a, _ = _planes({1: 40, 8: -30, 9: 7}, 2, 8, 8, YCC_444, 4)
    b, _ = _planes({1: 40, 8: -30, 9: 7, 2: 500, 16: -500, 4: 300, 32: 300, 6: -300, 48: 100, 18: 55}, 2, 8, 8,
                   YCC_444, 4)
    assert np.array_equal(a, b) and len(np.unique(a)) > 1
    # N = 1 reads the DC term alone
    a, _ = _planes({0: 24}, 1, 8, 8, YCC_444, 8)
    b, _ = _planes({0: 24, 1: 500, 8: -500, 63: 9}, 1, 8, 8, YCC_444, 8)
    assert np.array_equal(a, b) and (a == 131).all()


def test_reference_is_total_where_exact_arithmetic_stops():
    # dequantisation keeps the low 16 bits: 257 * 255 = 65535 is -1, and (-1 + 4) >> 3 = 0
    for s in SCALES:
        got, trace = _planes({0: 257}, 255, 8, 8, YCC_444, s)
        assert (got == 128).all() and trace.get("saturated", 0) == 0
    # pass 1 saturates: N = 4 gives 32767 << 2, N = 2 gives 32767 << 2 too (<< 15 then >> 13)
    for s in (2, 4):
        got, trace = _planes({0: 32767}, 1, 8, 8, YCC_444, s)
        assert (got == 255).all() and trace["saturated"] > 0
        got, trace = _planes({0: -32768}, 1, 8, 8, YCC_444, s)
        assert (got == 0).all() and trace["saturated"] > 0


# ---------------------------------------------------------------- planner
W, H = 129, 67     # the file


def _plan(ia, w, h, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def _decoded_plan(ia, s, bands=3, **opts):
    """A plan made for the W x H file's decode at 1/s."""
    ow, oh = out_size(W, H, s)
    return _plan(ia, ow, oh, bands, **opts)


def test_abi_version_stays():
    from imaginary_amd import _abi
    assert _abi.lib.mipx_abi_version() == 6 and _abi.OP_JPEGD == 17


def test_scaled_setter_at_shrink_one_is_the_full_size_setter():
    import imaginary_amd as ia
    for opts in (dict(), dict(width=60), dict(width=40, height=30, crop=1)):
        a = ia.plan_set_jpegd_input(_plan(ia, W, H, **opts), YCC_420)
        b = _plan(ia, W, H, **opts)
        assert ia.plan_set_jpegd_input_scaled(b, YCC_420, 1, W, H) is b
        assert bytes(a) == bytes(b)


@pytest.mark.parametrize("s", SCALES)
def test_scaled_setter_puts_the_step_first_and_keeps_the_geometry(s):
    import imaginary_amd as ia
    ow, oh = out_size(W, H, s)
    for layout in (YCC_444, YCC_420):
        p = _decoded_plan(ia, s, width=max(ow // 2, 1))
        before = p.describe()
        geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands)
        ia.plan_set_jpegd_input_scaled(p, layout, s, W, H)
        assert p.describe() == [("jpegd", (layout, s, W, H, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 3))] + before
        assert (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands) == geom
        # the plan validates; its workspace holds the planes at the OUTPUT size
        assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= 2 * 3 * ow * oh
        e = ia.plan_set_jpegd_input_scaled(_decoded_plan(ia, s), layout, s, W, H)
        assert [st[0] for st in e.describe()] == ["jpegd"] and (e.out_w, e.out_h, e.out_bands) == (ow, oh, 3)
        assert 3 * 3 * ow * oh <= ia.lib.mipx_workspace_bytes(C.byref(e), 3) < 3 * 3 * ow * oh + 4096
    # every file size that gives this decoded size is taken, no other
    p = _decoded_plan(ia, s)
    for fw in range(W - 2 * s, W + 2 * s):
        q = ia.MipxPlan.from_buffer_copy(bytes(p))
        e = ia.lib.mipx_plan_set_jpegd_input_scaled(C.byref(q), YCC_420, s, fw, H)
        assert (e == 0) == (-(-fw // s) == ow), (s, fw)


def test_scaled_setter_composes_with_the_text_watermark_and_coefficient_output():
    import imaginary_amd as ia
    s = 4
    a = _decoded_plan(ia, s, width=20)
    ia.plan_add_textmark(a, 10, 4, 3, 0.5, (1, 2, 3))
    ia.plan_set_jpegc_output(a, YCC_420, 75)
    ia.plan_set_jpegd_input_scaled(a, YCC_420, s, W, H)
    b = _decoded_plan(ia, s, width=20)
    ia.plan_set_jpegd_input_scaled(b, YCC_420, s, W, H)
    ia.plan_set_jpegc_output(b, YCC_420, 75)
    ia.plan_add_textmark(b, 10, 4, 3, 0.5, (1, 2, 3))
    assert [st[0] for st in a.describe()] == ["jpegd", "reduce", "textmark", "jpegc"]
    assert a.describe() == b.describe() and bytes(a) == bytes(b)
    assert ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    d = _decoded_plan(ia, s)
    ia.plan_set_jpegc_output(d, YCC_444, 90)
    ia.plan_set_jpegd_input_scaled(d, YCC_420, s, W, H)
    assert [st[0] for st in d.describe()] == ["jpegd", "jpegc"] and ia.lib.mipx_workspace_bytes(C.byref(d), 1) > 0


def test_scaled_setter_refusals_leave_the_plan_untouched():
    import imaginary_amd as ia
    L = ia.lib
    s = 2
    ow, oh = out_size(W, H, s)
    p = _decoded_plan(ia, s, width=30)
    untouched = bytes(p)
    set_ = L.mipx_plan_set_jpegd_input_scaled
    assert set_(C.byref(p), 2, s, W, H) == -1                  # unknown layout
    assert set_(C.byref(p), -1, s, W, H) == -1
    assert set_(None, YCC_420, s, W, H) == -1
    for shrink in (0, 3, 5, 6, 7, 16, -2):                     # a shrink outside 1, 2, 4, 8
        assert set_(C.byref(p), YCC_420, shrink, W, H) == -1, shrink
    for fw, fh, shrink in [(W + 2, H, s), (W, H + 2, s), (W, H, 4), (W, H, 1), (0, H, s), (W, 0, s), (-W, -H, s),
                           (ow, oh, s), (2 ** 31 - 1, H, s)]:  # a file that does not give in_w x in_h
        assert set_(C.byref(p), YCC_420, shrink, fw, fh) == -1, (fw, fh, shrink)
    assert bytes(p) == untouched
    for bands in (1, 2, 4):
        q = _decoded_plan(ia, s, bands=bands, width=30)
        before = bytes(q)
        assert set_(C.byref(q), YCC_420, s, W, H) == -1        # in_bands != 3
        assert bytes(q) == before
    assert set_(C.byref(p), YCC_420, s, W, H) == 0
    taken = bytes(p)
    assert set_(C.byref(p), YCC_420, s, W, H) == -1            # already coefficient input
    assert L.mipx_plan_set_jpegd_input(C.byref(p), YCC_420) == -1
    assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_420) == -1
    assert bytes(p) == taken
    y = ia.plan_set_ycc_input(_decoded_plan(ia, s, width=30), YCC_420)
    taken = bytes(y)
    assert set_(C.byref(y), YCC_420, s, W, H) == -1            # already planar
    assert bytes(y) == taken
    full = _decoded_plan(ia, s)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = ow, oh, 3
    taken = bytes(full)
    assert set_(C.byref(full), YCC_420, s, W, H) == -1         # full plan
    assert bytes(full) == taken


def test_chain_takes_the_scaled_step_in_stage_zero_only():
    import imaginary_amd as ia
    s = 2
    s0 = _decoded_plan(ia, s, width=32)
    s1 = _plan(ia, s0.out_w, s0.out_h, width=16)
    d0 = ia.plan_set_jpegd_input_scaled(_decoded_plan(ia, s, width=32), YCC_420, s, W, H)
    merged = ia.plan_chain([d0, s1])
    assert [st[0] for st in merged.describe()] == ["jpegd", "reduce", "reduce"]
    assert merged.describe()[0][1][:4] == (YCC_420, s, W, H)
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    # a stage 1 whose input is the decode of some file: still refused
    d1 = ia.plan_set_jpegd_input_scaled(_plan(ia, s0.out_w, s0.out_h, width=16), YCC_420, s, 2 * s0.out_w,
                                        2 * s0.out_h)
    arr = (ia.MipxPlan * 2)(s0, d1)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain(arr, 2, C.byref(out)) == -1


def _hand_plan(ia, a, w, h, then=()):
    """A plan written by hand: a JPEGD step with arguments `a`, then flips."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, 3
    p.out_w, p.out_h, p.out_bands = w, h, 3
    p.n_steps = 1 + len(then)
    for i, op in enumerate((17,) + tuple(then)):
        p.steps[i].op = op
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, 3
    for k, v in enumerate(a):
        p.steps[0].a[k] = v
    return p


def test_hand_written_scaled_steps_are_validated_before_any_device_work():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    good = [_hand_plan(ia, (YCC_420, 2, 33, 17), 17, 9), _hand_plan(ia, (YCC_444, 4, 33, 17), 9, 5, then=(2,)),
            _hand_plan(ia, (YCC_420, 8, 33, 17), 5, 3), _hand_plan(ia, (YCC_420, 8, 40, 24), 5, 3),
            _hand_plan(ia, (YCC_420, 1, 0, 0), 33, 17), _hand_plan(ia, (YCC_420, 0, 0, 0), 33, 17)]
    for p in good:
        assert L.mipx_workspace_bytes(C.byref(p), 1) > 0
    # what the scaled setter writes is what a hand-written plan must hold
    assert bytes(ia.plan_set_jpegd_input_scaled(_plan(ia, 17, 9), YCC_420, 2, 33, 17)) == bytes(good[0])
    bad = [_hand_plan(ia, (YCC_420, 3, 33, 17), 11, 6),      # a[1] is not one of 0, 1, 2, 4, 8
           _hand_plan(ia, (YCC_420, 16, 33, 17), 3, 2),
           _hand_plan(ia, (YCC_420, -2, 33, 17), 17, 9),
           _hand_plan(ia, (YCC_420, 2, 33, 17), 16, 9),      # a[2..3] disagree with in_w x in_h
           _hand_plan(ia, (YCC_420, 2, 33, 17), 17, 8),
           _hand_plan(ia, (YCC_420, 2, 36, 17), 17, 9),
           _hand_plan(ia, (YCC_420, 4, 33, 17), 17, 9),
           _hand_plan(ia, (YCC_420, 2, 0, 17), 17, 9),       # zero or negative file size
           _hand_plan(ia, (YCC_420, 2, 0, 0), 17, 9),
           _hand_plan(ia, (YCC_420, 2, 33, -17), 17, 9),
           _hand_plan(ia, (7, 2, 33, 17), 17, 9)]            # unknown layout
    for p in bad:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, None, None, None, None, 0, None) == -1
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
        data = np.zeros(jpegd_bytes(36, 17, YCC_444), np.uint8)
        dst = np.zeros((p.out_h, p.out_w, 3), np.uint8)
        src, out = MipxImg(data.ctypes.data, p.in_w, p.in_h, 3, 0), MipxImg(dst.ctypes.data, p.out_w, p.out_h, 3, 0)
        t = C.c_uint64()
        assert L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t)) == -1
    # a payload of 2^32 bytes or more: refused here too
    w, h = 30000, 30000
    assert 3 * (w // 2) * (h // 2) < 2 ** 32 < ia.jpegd_bytes(w, h, YCC_444)
    assert L.mipx_workspace_bytes(C.byref(_hand_plan(ia, (YCC_444, 2, w, h), w // 2, h // 2)), 1) == 0
    # after the step, the second position is still refused
    two = _hand_plan(ia, (YCC_420, 2, 33, 17), 17, 9, then=(17,))
    two.steps[1].a[0], two.steps[1].a[1], two.steps[1].a[2], two.steps[1].a[3] = YCC_420, 2, 33, 17
    assert L.mipx_workspace_bytes(C.byref(two), 1) == 0


def test_submit_takes_the_decoded_shape_and_the_files_payload():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    p = ia.plan_set_jpegd_input_scaled(_plan(ia, 17, 9, width=8), YCC_420, 2, 33, 17)
    data = np.zeros(jpegd_bytes(33, 17, YCC_420), np.uint8)
    dst = np.zeros((p.out_h, p.out_w, 3), np.uint8)
    out = MipxImg(dst.ctypes.data, p.out_w, p.out_h, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, ptr=data.ctypes.data):
        src = MipxImg(ptr, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t))

    assert submit(33, 17, 3, 0) == -1             # the file's size: the image is described as the DECODE
    assert submit(17, 9, 3, 51) == -1             # a stride
    assert submit(17, 9, 1, 0) == -1
    assert submit(17, 9, 3, 0, None) == -1
    if ia.device_count() == 0:
        assert submit(17, 9, 3, 0) == -7          # well-formed: only the engine is missing


def test_entry_point_rejects_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    L = ia.lib
    EINVAL = -1
    big = 1 << 40
    f = L.mipx_op_jpegd_to_rgb_scaled
    for s in (1, 2, 4, 8):
        assert f(None, 1, 1, 8, 8, YCC_420, s, 1, big, None) == EINVAL
        assert f(1, None, 1, 8, 8, YCC_420, s, 1, big, None) == EINVAL
        assert f(1, 1, 0, 8, 8, YCC_420, s, 1, big, None) == EINVAL
        assert f(1, 1, -3, 8, 8, YCC_444, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 0, 8, YCC_420, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, -1, YCC_444, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, 8, 2, s, 1, big, None) == EINVAL
        assert f(1, 1, 1, 8, 8, -1, s, 1, big, None) == EINVAL
        # no workspace, or one byte short of mipx_op_workspace_bytes at the OUTPUT size
        ow, oh = out_size(37, 29, s)
        need = L.mipx_op_workspace_bytes(17, 2, ow, oh, 3, 0.0, 0.0)
        assert need >= 2 * ow * oh * 3
        assert f(1, 1, 2, 37, 29, YCC_420, s, None, big, None) == EINVAL
        assert f(1, 1, 2, 37, 29, YCC_420, s, 1, need - 1, None) == EINVAL
        assert f(1, 1, 2, 37, 29, YCC_444, s, 1, 0, None) == EINVAL
        # the payload past the kernels' 32-bit byte offsets inside an image
        assert 2 ** 32 < ia.jpegd_bytes(30000, 30000, YCC_444)
        assert f(1, 1, 1, 30000, 30000, YCC_444, s, 1, big, None) == -2
    for s in (0, 3, 5, 16, -1):
        assert f(1, 1, 1, 8, 8, YCC_420, s, 1, big, None) == EINVAL
    # a 4:2:0 payload that fits: only the workspace is missing (no device is touched here)
    assert ia.jpegd_bytes(30000, 30000, YCC_420) < 2 ** 32
    assert f(1, 1, 1, 30000, 30000, YCC_420, 2, 1, 0, None) == EINVAL


def test_wrappers_check_the_payload_size_without_a_device():
    import imaginary_amd as ia
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb_scaled(np.zeros(jpegd_bytes(16, 16, YCC_444) - 1, np.uint8), 16, 16, YCC_444, 2)
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb_scaled(np.zeros(jpegd_bytes(16, 16, YCC_444), np.uint8), 16, 16, YCC_444, 3)
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb_scaled(np.zeros(jpegd_bytes(8, 8, YCC_444), np.uint8), 16, 16, YCC_444, 2)   # the decode's
    # execute reads the file's size from the step, not the plan's input size
    p = ia.plan_set_jpegd_input_scaled(_plan(ia, 17, 9), YCC_420, 2, 33, 17)
    with pytest.raises(ValueError):
        ia.execute(p, np.zeros((2, jpegd_bytes(17, 9, YCC_420)), np.uint8))
