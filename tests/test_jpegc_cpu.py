"""JPEG coefficient output (MIPX_OP_JPEGC), the parts that need no GPU:

 - the pixel rule (tests/jpegc_ref.py, which the GPU tests hold the kernel to) is pinned to a
   real upstream library: libjpeg-turbo inside Pillow.  The reference coefficients, written
   out by codec.encode_jpeg_coefs, give the entropy-coded scan that Pillow's own save of the
   same pixels gives, byte for byte, at every size, both samplings and four qualities;
 - the quantisation tables against the ones Pillow reports, for every quality;
 - the kernel's reciprocal division against the plain one, exhaustively, on the host builder;
 - the planner entry points, the plan validation and the argument checks of the C-ABI.
"""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from jpegc_ref import YCC_420, YCC_444, geometry, jpegc_bytes, jpegc_ref, qtables, with_dummy_blocks

PIL = pytest.importorskip("PIL.Image")

SIZES = [(1, 1), (2, 5), (3, 3), (7, 7), (8, 8), (8, 9), (9, 8), (16, 5), (5, 16), (8, 16), (16, 8), (24, 8),
         (8, 24), (40, 8), (24, 24), (25, 24), (17, 9), (33, 17), (15, 31), (37, 29), (64, 48), (129, 67), (1, 40),
         (40, 1)]
QUALITIES = [30, 75, 92, 100]
SUBSAMPLING = {YCC_444: 0, YCC_420: 2}   # Pillow's names for 4:4:4 and 4:2:0


def pillow_jpeg(px, layout, quality):
    out = io.BytesIO()
    PIL.fromarray(px).save(out, "JPEG", quality=quality, subsampling=SUBSAMPLING[layout])
    return out.getvalue()


def segments(buf):
    """[(marker, body)] up to and including SOS, then the entropy-coded scan (up to EOI)."""
    assert buf[:2] == b"\xff\xd8" and buf[-2:] == b"\xff\xd9"
    segs, i = [], 2
    while True:
        assert buf[i] == 0xFF
        marker, n = buf[i + 1], int.from_bytes(buf[i + 2:i + 4], "big")
        segs.append((marker, buf[i + 4:i + 2 + n]))
        i += 2 + n
        if marker == 0xDA:
            return segs, buf[i:-2]


def same_file(got, want, what):
    gs, gscan = segments(got)
    ws, wscan = segments(want)
    assert gscan == wscan, f"{what}: the entropy-coded scans differ ({len(gscan)} and {len(wscan)} bytes)"
    a = np.asarray(PIL.open(io.BytesIO(got)).convert("RGB"))
    b = np.asarray(PIL.open(io.BytesIO(want)).convert("RGB"))
    assert np.array_equal(a, b), f"{what}: the files decode to different pixels"


# ---------------------------------------------------------------- real-library parity
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_reference_coefficients_give_libjpegs_scan(w, h, layout):
    """No case is excluded: every size, both samplings, Q 30 / 75 / 92 / 100."""
    from imaginary_amd import codec
    px = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for quality in QUALITIES:
        coefs = jpegc_ref(px, layout, quality)[0]
        assert coefs.dtype == np.int16 and coefs.nbytes == jpegc_bytes(w, h, layout)
        got = codec.encode_jpeg_coefs(coefs, w, h, layout, quality)
        same_file(got, pillow_jpeg(px, layout, quality), f"{w}x{h} layout {layout} Q {quality}")


@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("kind", ["saturated", "ramp"])
def test_reference_on_saturated_and_smooth_images(kind, layout):
    from imaginary_amd import codec
    w, h = 37, 29
    if kind == "saturated":
        px = (np.random.default_rng(7).integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)
    else:
        x, y = np.meshgrid(np.arange(w), np.arange(h))
        px = np.stack([x * 255 // (w - 1), y * 255 // (h - 1), (x + y) * 255 // (w + h - 2)], -1).astype(np.uint8)
    coefs = jpegc_ref(px, layout, 85)[0]
    same_file(codec.encode_jpeg_coefs(coefs, w, h, layout, 85), pillow_jpeg(px, layout, 85), kind)


def test_encoder_takes_the_engines_bytes_too():
    """The coefficients as the raw little-endian bytes a C caller holds."""
    from imaginary_amd import codec
    px = np.random.default_rng(3).integers(0, 256, (17, 33, 3), dtype=np.uint8)
    coefs = jpegc_ref(px, YCC_420, 75)[0]
    raw = np.frombuffer(coefs.astype("<i2").tobytes(), np.uint8)
    assert codec.encode_jpeg_coefs(raw, 33, 17, YCC_420, 75) == codec.encode_jpeg_coefs(coefs, 33, 17, YCC_420, 75)
    with pytest.raises(ValueError):
        codec.encode_jpeg_coefs(coefs[:-64], 33, 17, YCC_420, 75)
    with pytest.raises(ValueError):
        codec.encode_jpeg_coefs(coefs, 33, 17, 2, 75)


def test_dummy_blocks_of_the_reference_and_the_encoder_agree():
    """16 x 8 in 4:2:0: one MCU whose lower Y block row is wholly dummy; 24 x 24: a dummy column."""
    for w, h in [(16, 8), (24, 24), (8, 8), (40, 8)]:
        px = np.random.default_rng(w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        coefs = jpegc_ref(px, YCC_420, 75)[0]
        y, cb, cr = with_dummy_blocks(coefs, w, h, YCC_420)
        (ywb, yhb), (cwb, chb), _ = geometry(w, h, YCC_420)
        assert y.shape == (2 * chb, 2 * cwb, 64) and cb.shape == cr.shape == (chb, cwb, 64)
        assert not y[yhb:, :, 1:].any() and not y[:, ywb:, 1:].any()
        if ywb < 2 * cwb:
            assert np.array_equal(y[:yhb, ywb, 0], y[:yhb, ywb - 1, 0])
        if yhb < 2 * chb:
            assert np.array_equal(y[yhb, 0::2, 0], y[yhb - 1, 1::2, 0]) and np.array_equal(y[yhb, 0::2], y[yhb, 1::2])


def test_huffman_tables_are_the_ones_libjpeg_writes():
    from imaginary_amd import codec
    px = np.random.default_rng(1).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    segs, _ = segments(pillow_jpeg(px, YCC_420, 75))
    seen = {}
    for marker, body in segs:
        while marker == 0xC4 and body:
            n = sum(body[1:17])
            seen[body[0]] = (bytes(body[1:17]), bytes(body[17:17 + n]))
            body = body[17 + n:]
    assert seen == codec.HUFFMAN_TABLES
    assert sorted(codec.ZIGZAG) == list(range(64)) and codec.ZIGZAG[:4] == (0, 1, 8, 16) and codec.ZIGZAG[-1] == 63


def test_qtables_equal_pillows_for_every_quality():
    import imaginary_amd as ia
    from imaginary_amd import codec
    px = np.random.default_rng(2).integers(0, 256, (8, 8, 3), dtype=np.uint8)
    for quality in range(1, 101):
        im = PIL.open(io.BytesIO(pillow_jpeg(px, YCC_420, quality)))
        lum, chrom = ia.jpeg_qtables(quality)
        # this Pillow reports the tables in natural order: the standard luminance table begins
        # 16 11 10 16 (in zigzag order it begins 16 11 12 14), so at Q 50 entry 2 is 10
        if quality == 50:
            assert list(im.quantization[0][:4]) == [16, 11, 10, 16]
        assert list(im.quantization[0]) == lum.tolist(), quality
        assert list(im.quantization[1]) == chrom.tolist(), quality
        rl, rc = qtables(quality)
        assert rl.tolist() == lum.tolist() and rc.tolist() == chrom.tolist()
        assert codec.jpeg_qtables(quality) == (lum.tolist(), chrom.tolist())
    lum = (C.c_uint8 * 64)()
    for bad in (0, -1, 101):
        assert ia.lib.mipx_jpeg_qtables(bad, lum, lum) == -1
    assert ia.lib.mipx_jpeg_qtables(50, None, lum) == -1 and ia.lib.mipx_jpeg_qtables(50, lum, None) == -1


def test_reciprocal_division_is_exact(tmp_path):
    """tests/c/jpegc_recips_host.cpp: every divisor 8 q, q in 1..255, against every numerator
    below 2^15 (the rule's largest is under 9000), then the host builder's table of every
    quality against those reciprocals.  Built as tests/test_tables_host.py builds its program."""
    exe = tmp_path / "jpegc_recips_host"
    csrc = os.path.join(ROOT, "imaginary_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "jpegc_recips_host.cpp"), os.path.join(csrc, "mipx_tables.cpp"),
                    os.path.join(csrc, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout


# ---------------------------------------------------------------- planner
def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def test_jpegc_bytes():
    import imaginary_amd as ia
    for w, h in SIZES + [(3840, 2160)]:
        for layout in (YCC_444, YCC_420):
            assert ia.jpegc_bytes(w, h, layout) == jpegc_bytes(w, h, layout)
    # 17 x 9 in 4:2:0: Y 3 x 2 blocks; chroma is 9 x 5 samples, so 2 x 1 blocks per component
    assert ia.jpegc_bytes(17, 9, YCC_420) == 128 * (3 * 2 + 2 * 2 * 1)
    assert ia.jpegc_bytes(16, 9, YCC_420) == 128 * (2 * 2 + 2 * 1 * 1)
    assert ia.jpegc_bytes(17, 9, YCC_444) == 128 * 3 * 3 * 2
    assert ia.jpegc_bytes(16, 8, YCC_420) == 128 * (2 + 2)
    assert ia.jpegc_bytes(3840, 2160, YCC_420) == 3840 * 2160 * 3      # 2 bytes per sample, 1.5 samples per pixel
    assert ia.jpegc_bytes(0, 3, YCC_420) == 0 and ia.jpegc_bytes(3, -1, YCC_444) == 0 and ia.jpegc_bytes(3, 3, 2) == 0
    assert ia.lib.mipx_op_workspace_bytes(16, 4, 64, 48, 3, 0.0, 0.0) == 0


def test_op_number_is_appended():
    from imaginary_amd import _abi
    assert _abi.OP_YCC == 15 and _abi.OP_JPEGC == 16 and _abi.OP_NAMES[16] == "jpegc"
    assert _abi.lib.mipx_abi_version() == 6


def test_set_jpegc_output_puts_the_step_last_and_keeps_the_geometry():
    import imaginary_amd as ia
    p = _plan(ia, width=60, height=40, crop=1)
    before = p.describe()
    geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands)
    assert ia.plan_set_jpegc_output(p, YCC_420, 80) is p
    assert p.describe() == before + [("jpegc", (YCC_420, 80, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (60, 40, 3))]
    assert (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands) == geom
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) > 0   # the plan validates
    e = _plan(ia)                                           # the empty plan: the step alone, no workspace
    assert e.n_steps == 0
    ia.plan_set_jpegc_output(e, YCC_444, 100)
    assert [s[0] for s in e.describe()] == ["jpegc"] and (e.out_w, e.out_h, e.out_bands) == (128, 96, 3)


def test_set_jpegc_output_composes_with_planar_input_and_the_text_watermark():
    import imaginary_amd as ia
    a = _plan(ia, width=60)
    ia.plan_set_ycc_input(a, YCC_420)
    ia.plan_set_jpegc_output(a, YCC_420, 75)
    assert [s[0] for s in a.describe()] == ["ycc", "reduce", "jpegc"]
    assert ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    b = _plan(ia, width=60)
    ia.plan_set_jpegc_output(b, YCC_420, 75)
    ia.plan_set_ycc_input(b, YCC_420)
    assert bytes(a) == bytes(b)
    # the text mark lands in front of the coefficient step either way
    c = _plan(ia, width=60)
    ia.plan_add_textmark(c, 20, 8, 5, 0.5, (1, 2, 3))
    ia.plan_set_jpegc_output(c, YCC_444, 90)
    d = _plan(ia, width=60)
    ia.plan_set_jpegc_output(d, YCC_444, 90)
    ia.plan_add_textmark(d, 20, 8, 5, 0.5, (1, 2, 3))
    assert [s[0] for s in c.describe()] == ["reduce", "textmark", "jpegc"] and bytes(c) == bytes(d)
    assert ia.lib.mipx_workspace_bytes(C.byref(c), 1) > 0
    # and a watermark image
    w = ia.plan_make(ia.make_opts(width=60, wm_enable=1), ia.make_input(128, 96, 3, "png", wm_w=10, wm_h=10, wm_bands=4))
    assert w.out_bands == 4
    assert ia.lib.mipx_plan_set_jpegc_output(C.byref(w), YCC_420, 75) == -1   # RGBA out: no coefficients


def test_set_jpegc_output_refusals():
    import imaginary_amd as ia
    L = ia.lib
    p = _plan(ia, width=60)
    assert L.mipx_plan_set_jpegc_output(C.byref(p), 2, 75) == -1            # unknown layout
    assert L.mipx_plan_set_jpegc_output(C.byref(p), -1, 75) == -1
    for q in (0, -5, 101, 1000):
        assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_420, q) == -1   # quality outside 1..100
    assert L.mipx_plan_set_jpegc_output(None, YCC_420, 75) == -1
    assert p.n_steps == 1
    for bands in (1, 2, 4):
        q = _plan(ia, bands=bands, width=60)
        n = q.n_steps
        assert q.out_bands == bands
        assert L.mipx_plan_set_jpegc_output(C.byref(q), YCC_420, 75) == -1  # out_bands != 3
        assert q.n_steps == n
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_420, 1) == 0
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_420, 1) == -1       # already ends with the step
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_444, 100) == -1
    assert p.n_steps == 2
    full = _plan(ia)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = 128, 96, 3
    assert L.mipx_plan_set_jpegc_output(C.byref(full), YCC_420, 75) == -1   # full plan
    assert full.n_steps == 64 and full.steps[63].op == 2


def _hand_plan(ia, ops, bands=3, w=16, h=12):
    """A plan of flips and coefficient steps written by hand (geometry consistent)."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op == 16:
            p.steps[i].a[0], p.steps[i].a[1] = YCC_420, 75
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_step_is_legal_only_last_and_on_three_bands():
    """Checked in the plan validation, before any device work: the pointers are never used."""
    import imaginary_amd as ia
    L = ia.lib
    ok = _hand_plan(ia, [2, 16])
    assert L.mipx_workspace_bytes(C.byref(ok), 1) > 0
    cases = [_hand_plan(ia, [16, 2]), _hand_plan(ia, [16, 16]), _hand_plan(ia, [2, 16, 2]),
             _hand_plan(ia, [2, 16], bands=4), _hand_plan(ia, [2, 16], bands=1)]
    bad_layout = _hand_plan(ia, [2, 16])
    bad_layout.steps[1].a[0] = 7
    bad_quality = _hand_plan(ia, [2, 16])
    bad_quality.steps[1].a[1] = 0
    too_good = _hand_plan(ia, [2, 16])
    too_good.steps[1].a[1] = 101
    for p in cases + [bad_layout, bad_quality, too_good]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
    # on 4 bands the step would claim 3: the step's own out_bands does not rescue it
    four = _hand_plan(ia, [2, 16], bands=4)
    four.steps[1].out_bands = 3
    four.out_bands = 3
    assert L.mipx_workspace_bytes(C.byref(four), 1) == 0
    assert L.mipx_execute_dev(C.byref(four), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1


def test_chain_takes_the_step_in_the_last_stage_only():
    import imaginary_amd as ia
    s0 = _plan(ia, width=64)
    s1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    last = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    ia.plan_set_jpegc_output(last, YCC_420, 75)
    y0 = _plan(ia, width=64)
    ia.plan_set_ycc_input(y0, YCC_420)
    merged = ia.plan_chain([y0, last])
    assert [s[0] for s in merged.describe()] == ["ycc", "reduce", "reduce", "jpegc"]
    assert (merged.out_w, merged.out_h, merged.out_bands) == (last.out_w, last.out_h, 3)
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    first = _plan(ia, width=64)
    ia.plan_set_jpegc_output(first, YCC_420, 75)
    arr = (ia.MipxPlan * 2)(first, s1)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain(arr, 2, C.byref(out)) == -1
    arr = (ia.MipxPlan * 3)(s0, last, _plan(ia, w=last.out_w, h=last.out_h, flip=1))
    assert ia.lib.mipx_plan_chain(arr, 3, C.byref(out)) == -1


def test_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    EINVAL = -1
    f = L.mipx_op_rgb_to_jpegc
    assert f(None, 1, 1, 8, 8, YCC_420, 75, None) == EINVAL
    assert f(1, None, 1, 8, 8, YCC_420, 75, None) == EINVAL
    assert f(1, 1, 0, 8, 8, YCC_420, 75, None) == EINVAL
    assert f(1, 1, -3, 8, 8, YCC_444, 75, None) == EINVAL
    assert f(1, 1, 1, 0, 8, YCC_420, 75, None) == EINVAL
    assert f(1, 1, 1, 8, -1, YCC_444, 75, None) == EINVAL
    assert f(1, 1, 1, 8, 8, 2, 75, None) == EINVAL
    assert f(1, 1, 1, 8, 8, -1, 75, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 0, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 101, None) == EINVAL
    # an image of 2^32 bytes or more, in or out: past the kernel's 32-bit byte offsets
    assert f(1, 1, 1, 40000, 40000, YCC_420, 75, None) == -2
    assert f(1, 1, 1, 40000, 40000, YCC_444, 75, None) == -2
    assert f(1, 1, 1, 30000, 30000, YCC_444, 75, None) == -2      # 2.7e9 bytes in, 5.4e9 out

    # mipx_submit for a coefficient plan: out is w x h x 3, stride 0, data = jpegc_bytes
    p = _plan(ia, w=16, h=12, width=8)
    ia.plan_set_jpegc_output(p, YCC_420, 75)
    src = np.zeros((12, 16, 3), np.uint8)
    dst = np.zeros(jpegc_bytes(p.out_w, p.out_h, YCC_420) // 2, np.int16)
    img = MipxImg(src.ctypes.data, 16, 12, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, data=dst.ctypes.data):
        out = MipxImg(data, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(img), None, C.byref(out), C.byref(t))

    assert (p.out_w, p.out_h) == (8, 6)
    assert submit(8, 6, 3, 24) == EINVAL          # a stride, even the natural one of RGB rows
    assert submit(8, 6, 3, 128) == EINVAL
    assert submit(8, 6, 1, 0) == EINVAL
    assert submit(128, 3, 1, 0) == EINVAL         # described as rows of blocks
    assert submit(16, 12, 3, 0) == EINVAL
    assert submit(8, 6, 3, 0, None) == EINVAL
    if ia.device_count() == 0:
        assert submit(8, 6, 3, 0) == -7           # well-formed: only the engine is missing
