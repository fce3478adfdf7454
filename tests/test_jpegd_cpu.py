"""JPEG coefficient input (MIPX_OP_JPEGD), the parts that need no GPU:

 - the pixel rule (tests/jpegd_ref.py, which the GPU tests hold the kernel to) is pinned to a
   real upstream library: libjpeg-turbo inside Pillow.  ycc_ref of jpegd_ref of what
   codec.decode_jpeg_coefs reads from a file equals Pillow's own RGB decode of that file, bit for
   bit, on every file here; none is excluded;
 - codec.decode_jpeg_coefs: what it declines, and the round trip with codec.encode_jpeg_coefs;
 - known answers of the reference, including where the total rule departs from exact arithmetic;
 - the planner entry points, the plan validation and the argument checks of the C-ABI.
"""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN
from jpegc_ref import jpegc_bytes, jpegc_ref, qtables
from jpegd_ref import HEADER_BYTES, YCC_420, YCC_444, jpegd_bytes, jpegd_ref, payload
from ycc_ref import ycc_bytes, ycc_ref

PIL = pytest.importorskip("PIL.Image")

# tests/test_ycc_cpu.py's sizes, then sizes around one block and with MCU padding blocks
SIZES = [(1, 1), (2, 3), (3, 3), (4, 2), (5, 2), (2, 5), (6, 5), (17, 9), (37, 29), (64, 48), (129, 67),
         (7, 7), (8, 8), (9, 8), (16, 5), (33, 17)]
SUBSAMPLING = {YCC_444: 0, YCC_420: 2}   # Pillow's names for 4:4:4 and 4:2:0


def save(im, fmt="JPEG", **kw):
    out = io.BytesIO()
    im.save(out, fmt, **kw)
    return out.getvalue()


def picture(w, h, kind, seed=0):
    rng = np.random.default_rng(1000 * w + h + seed)
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)      # {0, 255}: the largest coefficients


def decoded_by_the_rule(buf, w, h, layout, trace=None):
    from imaginary_amd import codec
    got = codec.decode_jpeg_coefs(buf)
    assert got is not None
    p, lay = got
    assert lay == layout and p.dtype == np.uint8 and p.shape == (jpegd_bytes(w, h, layout),)
    planes = jpegd_ref(p, w, h, layout, trace)
    assert planes.shape == (ycc_bytes(w, h, layout),)
    return ycc_ref(planes, w, h, layout)


# ---------------------------------------------------------------- real-library parity
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_reference_equals_libjpeg_rgb_decode(w, h, layout):
    from imaginary_amd import codec
    for quality in (1, 30, 75, 100):
        for kind in ("random", "extreme"):
            buf = save(PIL.fromarray(picture(w, h, kind, quality)), quality=quality, subsampling=SUBSAMPLING[layout])
            trace = {}
            got = decoded_by_the_rule(buf, w, h, layout, trace)
            assert np.array_equal(got, codec.decode(buf)), (w, h, layout, quality, kind)
            assert trace["saturated"] == 0, trace    # what an encoder writes never meets the rule's saturation


def test_reference_equals_libjpeg_with_optimised_tables_and_restart_markers():
    from imaginary_amd import codec
    for layout in (YCC_444, YCC_420):
        buf = save(PIL.fromarray(picture(70, 50, "random")), quality=80, subsampling=SUBSAMPLING[layout],
                   optimize=True, restart_marker_blocks=3)
        assert b"\xff\xdd" in buf and b"\xff\xd0" in buf          # DRI and a restart marker are really there
        assert np.array_equal(decoded_by_the_rule(buf, 70, 50, layout), codec.decode(buf))


@functools.lru_cache(maxsize=None)
def fixture(name):
    from imaginary_amd import codec
    buf = open(os.path.join(GOLDEN, "testdata", name), "rb").read()
    return buf, codec.header(buf), codec.decode_jpeg_coefs(buf)


def test_reference_equals_libjpeg_on_a_fixture():
    """A photograph, baseline 4:2:0."""
    from imaginary_amd import codec
    buf, hd, got = fixture("imaginary.jpg")
    assert got is not None and got[1] == YCC_420
    planes = jpegd_ref(got[0], hd.w, hd.h, YCC_420)
    assert np.array_equal(ycc_ref(planes, hd.w, hd.h, YCC_420), codec.decode(buf))
    # the planes are the decoder's own, too
    assert np.array_equal(planes, codec.decode_ycc(buf)[0])


# ---------------------------------------------------------------- the entropy decoder
def test_decode_jpeg_coefs_declines_everything_else():
    from imaginary_amd import codec
    rgb = PIL.fromarray(picture(32, 24, "random"))
    assert codec.decode_jpeg_coefs(save(rgb, quality=92)) is not None
    assert codec.decode_jpeg_coefs(save(rgb, quality=92, progressive=True)) is None
    assert codec.decode_jpeg_coefs(save(rgb, quality=92, subsampling=1)) is None             # 4:2:2
    assert codec.decode_jpeg_coefs(save(rgb.convert("L"), quality=92)) is None               # grey
    assert codec.decode_jpeg_coefs(save(rgb.convert("CMYK"), quality=92)) is None            # CMYK
    assert codec.decode_jpeg_coefs(save(rgb, quality=92, keep_rgb=True)) is None             # Adobe transform 0
    assert codec.decode_jpeg_coefs(save(rgb, "PNG")) is None
    for name in ("test.png", "test.webp"):
        assert codec.decode_jpeg_coefs(open(os.path.join(GOLDEN, "testdata", name), "rb").read()) is None
    assert codec.decode_jpeg_coefs(b"\xff\xd8\xff not a jpeg") is None
    assert codec.decode_jpeg_coefs(b"") is None
    rng = np.random.default_rng(9)
    assert codec.decode_jpeg_coefs(rng.integers(0, 256, 4096, dtype=np.uint8).tobytes()) is None
    whole = save(rgb, quality=92)
    # damaged files: whatever it returns, it does not raise
    for _ in range(40):
        bad = bytearray(whole)
        for at in rng.integers(2, len(whole), 3):
            bad[at] = rng.integers(0, 256)
        got = codec.decode_jpeg_coefs(bytes(bad))
        assert got is None or (got[0].dtype == np.uint8 and got[0].ndim == 1 and got[1] in (YCC_444, YCC_420))
    scan = whole.index(b"\xff\xda")
    for cut in (scan + 14 + (len(whole) - scan - 14) // 2, len(whole) - 2, scan + 4):
        assert codec.decode_jpeg_coefs(whole[:cut]) is None                                  # truncated
    # the colour space and sampling rules are decode_ycc's: both take a file or neither does
    for kw in (dict(subsampling=0), dict(subsampling=2), dict(subsampling=1), dict(keep_rgb=True)):
        buf = save(rgb, quality=92, **kw)
        assert (codec.decode_jpeg_coefs(buf) is None) == (codec.decode_ycc(buf) is None), kw


@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", [(8, 8), (17, 9), (33, 17), (37, 29)], ids=lambda v: str(v))
def test_round_trip_with_the_projects_own_writer(w, h, layout):
    """17 x 9 and 33 x 17 have MCU padding blocks in 4:2:0: the writer adds them, the reader drops them."""
    from imaginary_amd import codec
    for quality in (30, 92):
        c = jpegc_ref(picture(w, h, "random", quality), layout, quality)[0]
        got = codec.decode_jpeg_coefs(codec.encode_jpeg_coefs(c, w, h, layout, quality))
        assert got is not None and got[1] == layout
        lum, chrom = qtables(quality)
        assert np.array_equal(got[0], payload(c, [lum, chrom]))
        assert np.array_equal(got[0][HEADER_BYTES:].view(np.int16), c)
        tables = got[0][:HEADER_BYTES].view(np.uint16).reshape(3, 64)
        want = codec.jpeg_qtables(quality)
        assert tables[0].tolist() == want[0] and tables[1].tolist() == tables[2].tolist() == want[1]


# ---------------------------------------------------------------- known answers of the reference
def _block(values, q=1):
    """The 8 x 8 samples of one Y block (4:4:4, 8 x 8) with coefficients {natural index: value}."""
    c = np.zeros(3 * 64, np.int16)
    for k, v in values.items():
        c[k] = v
    trace = {}
    planes = jpegd_ref(payload(c, [np.full(64, q)]), 8, 8, YCC_444, trace)
    return planes[:64].reshape(8, 8).astype(int), trace


def test_reference_known_answers():
    zero, _ = _block({})
    assert (zero == 128).all()
    # DC only: libjpeg's shortcut, pass 1 gives dc << 2 and pass 2 descales by PASS1_BITS + 3
    for dc, q in [(1, 1), (-1, 1), (3, 1), (4, 1), (-5, 1), (10, 16), (-10, 16), (50, 8), (-64, 16), (30, 255)]:
        got, trace = _block({0: dc}, q)
        want = min(max(((((dc * q) << 2) + 16) >> 5) + 128, 0), 255)
        assert (got == want).all() and trace["saturated"] == 0, (dc, q, got[0, 0], want)


def test_reference_is_total_where_exact_arithmetic_stops():
    """Hand-made blocks at the two points where the rule is not exact arithmetic.  (With int16
    inputs the 32-bit sums of a pass stay below 61212 * 32768 + 2^17 < 2^31, the sum of the
    absolute DCT weights times the largest input, so the only wraps that can fire are the
    dequantisation's.)"""
    # dequantisation keeps the low 16 bits: 257 * 255 = 65535 is -1, and (-1 + 4) >> 3 = 0
    got, trace = _block({0: 257}, 255)
    assert (got == 128).all() and trace["saturated"] == 0
    # 300 * 255 = 76500 is 10964: (10964 + 4) >> 3 = 1371, clamped
    assert (_block({0: 300}, 255)[0] == 255).all()
    # pass 1 saturates: 32767 << 2 becomes 32767, and (32767 * 8192 + 2^17) >> 18 = 1024 (the
    # trace also sees the two all-zero chroma blocks)
    got, trace = _block({0: 32767})
    assert (got == 255).all() and trace["saturated"] == 8 and trace["pass2"] == (0, 1024)
    got, trace = _block({0: -32768})
    assert (got == 0).all() and trace["saturated"] == 8 and trace["pass2"] == (-1024, 0)
    # ... and the saturation shows in the samples: column 0 is 20000 << 2 -> 32767, column 4 is
    # -8000 << 2 = -32000; pass 2 gives ((32767 - 32000) * 8192 + 2^17) >> 18 = 24 in columns
    # 0, 3, 4, 7 (exact arithmetic would give 1500 there) and 2024 in the others
    got, trace = _block({0: 20000, 4: -8000})
    assert trace["saturated"] == 8
    assert (got == np.array([152, 255, 255, 152, 152, 255, 255, 152])).all()


# ---------------------------------------------------------------- planner
def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def test_jpegd_bytes():
    import imaginary_amd as ia
    for w, h in [(1, 1), (2, 2), (5, 3), (17, 9), (64, 48), (37, 29), (3840, 2160)]:
        for layout in (YCC_444, YCC_420):
            assert ia.jpegd_bytes(w, h, layout) == jpegd_bytes(w, h, layout) == 384 + jpegc_bytes(w, h, layout)
            assert ia.jpegd_bytes(w, h, layout) == 384 + ia.jpegc_bytes(w, h, layout)
    assert ia.jpegd_bytes(8, 8, YCC_444) == 384 + 3 * 128
    assert ia.jpegd_bytes(17, 9, YCC_420) == 384 + 128 * (3 * 2 + 2 * 2 * 1)
    assert ia.jpegd_bytes(0, 3, YCC_420) == 0 and ia.jpegd_bytes(3, -1, YCC_444) == 0 and ia.jpegd_bytes(3, 3, 2) == 0
    # the workspace holds n images' packed planes
    for layout in (YCC_444, YCC_420):
        assert ia.lib.mipx_op_workspace_bytes(17, 4, 37, 29, 3, 0.0, 0.0) >= 4 * ycc_bytes(37, 29, layout)
    assert ia.lib.mipx_op_workspace_bytes(17, 0, 37, 29, 3, 0.0, 0.0) == 0


def test_op_number_is_appended():
    from imaginary_amd import _abi
    assert _abi.OP_JPEGC == 16 and _abi.OP_JPEGD == 17 and _abi.OP_NAMES[17] == "jpegd"
    assert _abi.lib.mipx_abi_version() == 6


def test_set_jpegd_input_puts_the_step_first_and_keeps_the_geometry():
    import imaginary_amd as ia
    p = _plan(ia, width=60, height=40, crop=1)
    before = p.describe()
    geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands)
    assert ia.plan_set_jpegd_input(p, YCC_420) is p
    assert p.describe() == [("jpegd", (YCC_420, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (128, 96, 3))] + before
    assert (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands) == geom
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= 2 * ycc_bytes(128, 96, YCC_420)   # the plan validates
    e = _plan(ia)
    assert e.n_steps == 0
    ia.plan_set_jpegd_input(e, YCC_444)
    assert [s[0] for s in e.describe()] == ["jpegd"] and (e.out_w, e.out_h, e.out_bands) == (128, 96, 3)
    assert ia.lib.mipx_workspace_bytes(C.byref(e), 3) >= 3 * ycc_bytes(128, 96, YCC_444)


def test_set_jpegd_input_composes_with_the_text_watermark_and_coefficient_output():
    import imaginary_amd as ia
    a = _plan(ia, width=60)
    ia.plan_add_textmark(a, 20, 8, 5, 0.5, (1, 2, 3))
    ia.plan_set_jpegc_output(a, YCC_420, 75)
    ia.plan_set_jpegd_input(a, YCC_420)
    b = _plan(ia, width=60)
    ia.plan_set_jpegd_input(b, YCC_420)
    ia.plan_set_jpegc_output(b, YCC_420, 75)
    ia.plan_add_textmark(b, 20, 8, 5, 0.5, (1, 2, 3))
    assert [s[0] for s in a.describe()] == ["jpegd", "reduce", "textmark", "jpegc"]
    assert a.describe() == b.describe() and bytes(a) == bytes(b)
    assert ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    c = _plan(ia)
    ia.plan_set_jpegd_input(c, YCC_444)
    ia.plan_add_textmark(c, 20, 8, 5, 0.5)
    assert [s[0] for s in c.describe()] == ["jpegd", "textmark"]
    assert ia.plan_textmark_geometry(c) == (128, 96, 3)
    # coefficients in, coefficients out, nothing between
    d = _plan(ia)
    ia.plan_set_jpegc_output(d, YCC_444, 90)
    ia.plan_set_jpegd_input(d, YCC_420)
    assert [s[0] for s in d.describe()] == ["jpegd", "jpegc"] and ia.lib.mipx_workspace_bytes(C.byref(d), 1) > 0


def test_set_jpegd_input_refusals():
    import imaginary_amd as ia
    L = ia.lib
    p = _plan(ia, width=60)
    untouched = bytes(p)
    assert L.mipx_plan_set_jpegd_input(C.byref(p), 2) == -1            # unknown layout
    assert L.mipx_plan_set_jpegd_input(C.byref(p), -1) == -1
    assert L.mipx_plan_set_jpegd_input(None, YCC_420) == -1
    assert bytes(p) == untouched
    for bands in (1, 2, 4):
        q = _plan(ia, bands=bands, width=60)
        before = bytes(q)
        assert L.mipx_plan_set_jpegd_input(C.byref(q), YCC_420) == -1  # in_bands != 3
        assert bytes(q) == before
    assert L.mipx_plan_set_jpegd_input(C.byref(p), YCC_420) == 0
    taken = bytes(p)
    assert L.mipx_plan_set_jpegd_input(C.byref(p), YCC_420) == -1      # already coefficient input
    assert L.mipx_plan_set_jpegd_input(C.byref(p), YCC_444) == -1
    assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_420) == -1        # ... and not planar on top
    assert bytes(p) == taken
    y = _plan(ia, width=60)
    ia.plan_set_ycc_input(y, YCC_420)
    taken = bytes(y)
    assert L.mipx_plan_set_jpegd_input(C.byref(y), YCC_420) == -1      # already planar
    assert bytes(y) == taken
    full = _plan(ia)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = 128, 96, 3
    assert L.mipx_plan_set_jpegd_input(C.byref(full), YCC_420) == -1   # full plan
    assert full.n_steps == 64 and full.steps[0].op == 2


def _hand_plan(ia, ops, bands=3, w=16, h=12):
    """A plan of flips, YCC, JPEGC and JPEGD steps written by hand (geometry consistent)."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op in (15, 16, 17):
            p.steps[i].a[0] = YCC_420
        if op == 16:
            p.steps[i].a[1] = 75
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_step_is_legal_only_first_and_on_three_bands():
    """Checked in the plan validation, before any device work: the pointers are never used."""
    import imaginary_amd as ia
    L = ia.lib
    for ok in (_hand_plan(ia, [17, 2]), _hand_plan(ia, [17]), _hand_plan(ia, [17, 16])):
        assert L.mipx_workspace_bytes(C.byref(ok), 1) > 0
    cases = [_hand_plan(ia, [2, 17]), _hand_plan(ia, [17, 17]), _hand_plan(ia, [17, 15]), _hand_plan(ia, [15, 17]),
             _hand_plan(ia, [17], bands=4), _hand_plan(ia, [17], bands=1)]
    bad_layout = _hand_plan(ia, [17])
    bad_layout.steps[0].a[0] = 7
    for p in cases + [bad_layout]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, None, None, None, None, 0, None) == -1
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
    four = _hand_plan(ia, [17], bands=4)
    four.steps[0].out_bands = 3
    four.out_bands = 3
    assert L.mipx_workspace_bytes(C.byref(four), 1) == 0
    assert L.mipx_execute_dev(C.byref(four), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1


def test_chain_takes_the_step_in_stage_zero_only():
    import imaginary_amd as ia
    s0 = _plan(ia, width=64)
    s1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    d0 = _plan(ia, width=64)
    ia.plan_set_jpegd_input(d0, YCC_420)
    merged = ia.plan_chain([d0, s1])
    assert [s[0] for s in merged.describe()] == ["jpegd", "reduce", "reduce"]
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    d1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    ia.plan_set_jpegd_input(d1, YCC_420)
    arr = (ia.MipxPlan * 2)(s0, d1)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain(arr, 2, C.byref(out)) == -1


def test_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    EINVAL = -1
    big = 1 << 40
    assert L.mipx_op_jpegd_to_rgb(None, 1, 1, 8, 8, YCC_420, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, None, 1, 8, 8, YCC_420, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 0, 8, 8, YCC_420, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, -3, 8, 8, YCC_444, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 0, 8, YCC_420, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 8, -1, YCC_444, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 8, 8, 2, 1, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 8, 8, -1, 1, big, None) == EINVAL
    # no workspace, or one byte short of mipx_op_workspace_bytes
    need = L.mipx_op_workspace_bytes(17, 2, 37, 29, 3, 0.0, 0.0)
    assert need >= 2 * 37 * 29 * 3
    assert L.mipx_op_jpegd_to_rgb(1, 1, 2, 37, 29, YCC_420, None, big, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 2, 37, 29, YCC_420, 1, need - 1, None) == EINVAL
    assert L.mipx_op_jpegd_to_rgb(1, 1, 2, 37, 29, YCC_444, 1, 0, None) == EINVAL
    # past the kernels' 32-bit byte offsets inside an image: the RGB, and already the payload
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 40000, 40000, YCC_420, 1, big, None) == -2
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 40000, 40000, YCC_444, 1, big, None) == -2
    assert 3 * 30000 * 30000 < 2 ** 32 < ia.jpegd_bytes(30000, 30000, YCC_444)
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 30000, 30000, YCC_444, 1, big, None) == -2

    # mipx_submit for a coefficient-input plan: w x h x 3, stride 0, data = the payload
    p = _plan(ia, w=16, h=12, width=8)
    ia.plan_set_jpegd_input(p, YCC_420)
    data = np.zeros(jpegd_bytes(16, 12, YCC_420), np.uint8)
    dst = np.zeros((p.out_h, p.out_w, 3), np.uint8)
    out = MipxImg(dst.ctypes.data, p.out_w, p.out_h, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, ptr=data.ctypes.data):
        src = MipxImg(ptr, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t))

    assert submit(16, 12, 3, 48) == EINVAL        # a stride, even the natural one of RGB rows
    assert submit(16, 12, 3, 128) == EINVAL
    assert submit(16, 12, 1, 0) == EINVAL
    assert submit(128, data.size // 128, 1, 0) == EINVAL   # described as rows of one block
    assert submit(8, 6, 3, 0) == EINVAL
    assert submit(16, 12, 3, 0, None) == EINVAL
    if ia.device_count() == 0:
        assert submit(16, 12, 3, 0) == -7         # well-formed: only the engine is missing


def test_wrappers_check_the_payload_size_without_a_device():
    import imaginary_amd as ia
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb(np.zeros(jpegd_bytes(8, 8, YCC_444) - 1, np.uint8), 8, 8, YCC_444)
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb(np.zeros(jpegd_bytes(8, 8, YCC_444), np.uint8), 8, 8, 2)
    p = ia.plan_set_jpegd_input(_plan(ia, w=16, h=12), YCC_420)
    with pytest.raises(ValueError):
        ia.execute(p, np.zeros((2, jpegc_bytes(16, 12, YCC_420)), np.uint8))   # the header is missing
