"""Planar JPEG input (MIPX_OP_YCC), the parts that need no GPU:

 - the pixel rule (tests/ycc_ref.py, which the GPU tests hold the kernel to) is pinned to a
   real upstream library: libjpeg-turbo inside Pillow.  ycc_ref of the planes that
   codec.decode_ycc extracts equals Pillow's own RGB decode of the same file, bit for bit,
   including the sizes with cw <= 2, where libjpeg replicates chroma;
 - the planner entry points, the plan validation and the argument checks of the C-ABI.
"""
import ctypes as C
import io
import os

import numpy as np
import pytest

from conftest import GOLDEN
from ycc_ref import YCC_420, YCC_444, ycc_bytes, ycc_ref

PIL = pytest.importorskip("PIL.Image")

SIZES = [(1, 1), (2, 3), (3, 3), (4, 2), (5, 2), (2, 5), (6, 5), (17, 9), (37, 29), (64, 48), (129, 67)]
SUBSAMPLING = {YCC_444: 0, YCC_420: 2}   # Pillow's names for 4:4:4 and 4:2:0


def jpeg(w, h, layout=YCC_420, seed=0, **kw):
    px = np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    out = io.BytesIO()
    PIL.fromarray(px).save(out, "JPEG", quality=92, subsampling=SUBSAMPLING[layout], **kw)
    return out.getvalue()


# ---------------------------------------------------------------- real-library parity
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_reference_equals_libjpeg_rgb_decode(w, h, layout):
    """No size had to be excluded: with cw <= 2 (2x3, 3x3, 4x2, 2x5) replication matches."""
    from imaginary_amd import codec
    buf = jpeg(w, h, layout)
    got = codec.decode_ycc(buf)
    assert got is not None
    planes, lay = got
    assert lay == layout and planes.dtype == np.uint8 and planes.shape == (ycc_bytes(w, h, layout),)
    assert np.array_equal(ycc_ref(planes, w, h, layout), codec.decode(buf))


@pytest.mark.parametrize("name", ["imaginary.jpg", "large.jpg", "orient6.jpg", "smart-crop.jpg"])
def test_reference_equals_libjpeg_on_the_fixtures(name):
    """The repository's JPEG fixtures (photographs, all 4:2:0; one without a JFIF marker)."""
    from imaginary_amd import codec
    buf = open(os.path.join(GOLDEN, "testdata", name), "rb").read()
    hd = codec.header(buf)
    planes, layout = codec.decode_ycc(buf)
    assert layout == YCC_420
    assert np.array_equal(ycc_ref(planes, hd.w, hd.h, layout), codec.decode(buf))


def test_decode_ycc_declines_everything_else():
    from imaginary_amd import codec
    px = np.random.default_rng(5).integers(0, 256, (24, 32, 3), dtype=np.uint8)

    def save(im, fmt, **kw):
        out = io.BytesIO()
        im.save(out, fmt, **kw)
        return out.getvalue()

    rgb = PIL.fromarray(px)
    assert codec.decode_ycc(save(rgb, "JPEG", quality=92, subsampling=1)) is None          # 4:2:2
    assert codec.decode_ycc(save(rgb.convert("L"), "JPEG", quality=92)) is None            # grey
    assert codec.decode_ycc(save(rgb.convert("CMYK"), "JPEG", quality=92)) is None         # CMYK
    assert codec.decode_ycc(save(rgb, "JPEG", quality=92, keep_rgb=True)) is None          # Adobe transform 0
    assert codec.decode_ycc(save(rgb, "PNG")) is None
    for name in ("test.png", "test.webp"):
        assert codec.decode_ycc(open(os.path.join(GOLDEN, "testdata", name), "rb").read()) is None
    assert codec.decode_ycc(b"\xff\xd8\xff not a jpeg") is None
    # the stand-in cannot get at the planes of a one-row 4:2:0 file that libjpeg interpolates
    assert codec.decode_ycc(jpeg(9, 1)) is None
    assert codec.decode_ycc(jpeg(3, 1)) is not None


# ---------------------------------------------------------------- planner
def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def test_ycc_bytes():
    import imaginary_amd as ia
    for w, h in [(1, 1), (2, 2), (5, 3), (64, 48), (37, 29), (3840, 2160)]:
        for layout in (YCC_444, YCC_420):
            assert ia.ycc_bytes(w, h, layout) == ycc_bytes(w, h, layout)
    assert ia.ycc_bytes(5, 3, YCC_420) == 15 + 2 * 3 * 2
    assert ia.ycc_bytes(5, 3, YCC_444) == 45
    assert ia.ycc_bytes(3840, 2160, YCC_420) == 3840 * 2160 * 3 // 2
    assert ia.ycc_bytes(0, 3, YCC_420) == 0 and ia.ycc_bytes(3, -1, YCC_444) == 0 and ia.ycc_bytes(3, 3, 2) == 0
    assert ia.lib.mipx_op_workspace_bytes(15, 4, 64, 48, 3, 0.0, 0.0) == 0


def test_op_number_is_appended():
    from imaginary_amd import _abi
    assert _abi.OP_TEXTMARK == 14 and _abi.OP_YCC == 15 and _abi.OP_NAMES[15] == "ycc"
    assert _abi.lib.mipx_abi_version() == 6


def test_set_ycc_input_puts_the_step_first_and_keeps_the_geometry():
    import imaginary_amd as ia
    p = _plan(ia, width=60, height=40, crop=1)
    before = p.describe()
    geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands)
    assert ia.plan_set_ycc_input(p, YCC_420) is p
    assert p.describe() == [("ycc", (YCC_420, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (128, 96, 3))] + before
    assert (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands) == geom
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) > 0   # the plan validates
    # the empty plan: the step alone
    e = _plan(ia)
    assert e.n_steps == 0
    ia.plan_set_ycc_input(e, YCC_444)
    assert [s[0] for s in e.describe()] == ["ycc"] and (e.out_w, e.out_h, e.out_bands) == (128, 96, 3)


def test_set_ycc_input_composes_with_the_text_watermark():
    import imaginary_amd as ia
    a = _plan(ia, width=60)
    ia.plan_add_textmark(a, 20, 8, 5, 0.5, (1, 2, 3))
    ia.plan_set_ycc_input(a, YCC_420)
    b = _plan(ia, width=60)
    ia.plan_set_ycc_input(b, YCC_420)
    ia.plan_add_textmark(b, 20, 8, 5, 0.5, (1, 2, 3))
    assert a.describe() == b.describe()
    assert [s[0] for s in a.describe()] == ["ycc", "reduce", "textmark"]
    assert bytes(a) == bytes(b)
    # on the empty plan the text mark lands after the conversion either way
    c = _plan(ia)
    ia.plan_set_ycc_input(c, YCC_444)
    ia.plan_add_textmark(c, 20, 8, 5, 0.5)
    assert [s[0] for s in c.describe()] == ["ycc", "textmark"]
    assert ia.plan_textmark_geometry(c) == (128, 96, 3)


def test_set_ycc_input_refusals():
    import imaginary_amd as ia
    L = ia.lib
    p = _plan(ia, width=60)
    assert L.mipx_plan_set_ycc_input(C.byref(p), 2) == -1            # unknown layout
    assert L.mipx_plan_set_ycc_input(C.byref(p), -1) == -1
    assert L.mipx_plan_set_ycc_input(None, YCC_420) == -1
    assert p.n_steps == 1
    for bands in (1, 2, 4):
        q = _plan(ia, bands=bands, width=60)
        n = q.n_steps
        assert L.mipx_plan_set_ycc_input(C.byref(q), YCC_420) == -1  # in_bands != 3
        assert q.n_steps == n
    assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_420) == 0
    assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_420) == -1      # already planar
    assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_444) == -1
    full = _plan(ia)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = 128, 96, 3
    assert L.mipx_plan_set_ycc_input(C.byref(full), YCC_420) == -1   # full plan
    assert full.n_steps == 64 and full.steps[0].op == 2


def _hand_plan(ia, ops, bands=3, w=16, h=12):
    """A plan of flips and YCC steps written by hand (geometry consistent)."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op == 15:
            p.steps[i].a[0] = YCC_420
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_step_is_legal_only_first_and_on_three_bands():
    """Checked in the plan validation, before any device work: the pointers are never used."""
    import imaginary_amd as ia
    L = ia.lib
    ok = _hand_plan(ia, [15, 2])
    assert L.mipx_workspace_bytes(C.byref(ok), 1) > 0
    cases = [_hand_plan(ia, [2, 15]), _hand_plan(ia, [15, 15]), _hand_plan(ia, [15], bands=4),
             _hand_plan(ia, [15], bands=1)]
    bad_layout = _hand_plan(ia, [15])
    bad_layout.steps[0].a[0] = 7
    for p in cases + [bad_layout]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
    # on 4 bands the step would claim 3: the step's own out_bands does not rescue it
    four = _hand_plan(ia, [15], bands=4)
    four.steps[0].out_bands = 3
    four.out_bands = 3
    assert L.mipx_workspace_bytes(C.byref(four), 1) == 0
    assert L.mipx_execute_dev(C.byref(four), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1


def test_chain_takes_the_step_in_stage_zero_only():
    import imaginary_amd as ia
    s0 = _plan(ia, width=64)
    s1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    y0 = _plan(ia, width=64)
    ia.plan_set_ycc_input(y0, YCC_420)
    merged = ia.plan_chain([y0, s1])
    assert [s[0] for s in merged.describe()] == ["ycc", "reduce", "reduce"]
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    y1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    ia.plan_set_ycc_input(y1, YCC_420)
    arr = (ia.MipxPlan * 2)(s0, y1)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain(arr, 2, C.byref(out)) == -1


def test_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    EINVAL = -1
    assert L.mipx_op_ycc_to_rgb(None, 1, 1, 8, 8, YCC_420, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, None, 1, 8, 8, YCC_420, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, 0, 8, 8, YCC_420, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, -3, 8, 8, YCC_444, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 0, 8, YCC_420, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 8, -1, YCC_444, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 8, 8, 2, None) == EINVAL
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 8, 8, -1, None) == EINVAL
    # 2^32 / 3 pixels or more: past the kernel's 32-bit byte offsets
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 40000, 40000, YCC_420, None) == -2
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 40000, 40000, YCC_444, None) == -2

    # mipx_submit for a planar plan: w x h x 3, stride 0, data = the packed planes
    p = _plan(ia, w=16, h=12, width=8)
    ia.plan_set_ycc_input(p, YCC_420)
    planes = np.zeros(ycc_bytes(16, 12, YCC_420), np.uint8)
    dst = np.zeros((p.out_h, p.out_w, 3), np.uint8)
    out = MipxImg(dst.ctypes.data, p.out_w, p.out_h, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, data=planes.ctypes.data):
        src = MipxImg(data, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t))

    assert submit(16, 12, 3, 48) == EINVAL        # a stride, even the natural one of RGB rows
    assert submit(16, 12, 3, 16) == EINVAL
    assert submit(16, 12, 1, 0) == EINVAL         # described as the Y plane
    assert submit(16, 18, 1, 0) == EINVAL         # described as the stacked planes
    assert submit(8, 6, 3, 0) == EINVAL
    assert submit(16, 12, 3, 0, None) == EINVAL
    if ia.device_count() == 0:
        assert submit(16, 12, 3, 0) == -7         # well-formed: only the engine is missing


def test_c_client_builds_against_the_header(tmp_path):
    """tests/c/mipx_e2e_ycc.c, the request-path measurement with planar input, compiles
    cleanly against include/mipx.h and links the three new entry points."""
    import subprocess
    from conftest import ROOT
    exe = os.path.join(str(tmp_path), "mipx_e2e_ycc")
    subprocess.run(["gcc", "-O2", "-Wall", "-Wextra", "-Werror", "-std=c11", "-D_DEFAULT_SOURCE",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "mipx_e2e_ycc.c"),
                    "-L", os.path.join(ROOT, "imaginary_amd"), "-lmipx", "-lpthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "imaginary_amd"), "-o", exe], check=True)
    assert os.path.exists(exe)
