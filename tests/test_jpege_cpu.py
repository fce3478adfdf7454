"""Entropy-coded JPEG output (MIPX_OP_JPEGE), the parts that need no GPU:

 - codec.encode_jpeg_coefs, which tests/test_jpegc_cpu.py pins to libjpeg-turbo inside Pillow, is
   jpeg_header + jpeg_scan + EOI, and Pillow decodes jpeg_from_scan like its own file;
 - the reference slot (tests/jpege_ref.py, which the GPU tests hold the kernels to): statuses,
   lengths, and the two inputs with an 0xFF at an awkward place;
 - mipx_jpeg_scan_bytes, the workspace formula, the planner entry point, the plan validation and
   the argument checks of the C-ABI;
 - the host-built Huffman code table against codec._huff_codes.
"""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpege_ref
from conftest import ROOT
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpege_ref import OK, OVERFLOW, UNCODABLE, check_slot, jpeg_scan_bytes, slot_ref

PIL = pytest.importorskip("PIL.Image")

# the sizes of tests/test_jpegc_cpu.py
SIZES = [(1, 1), (2, 5), (3, 3), (7, 7), (8, 8), (8, 9), (9, 8), (16, 5), (5, 16), (8, 16), (16, 8), (24, 8),
         (8, 24), (40, 8), (24, 24), (25, 24), (17, 9), (33, 17), (15, 31), (37, 29), (64, 48), (129, 67), (1, 40),
         (40, 1)]
QUALITIES = [30, 75, 92, 100]
OP_JPEGE = 19


# ---------------------------------------------------------------- the split of the host writer
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", SIZES, ids=lambda v: str(v))
def test_header_scan_and_eoi_are_the_file(w, h, layout):
    from imaginary_amd import codec
    px = np.random.default_rng(1000 * w + h).integers(0, 256, (h, w, 3), dtype=np.uint8)
    for quality in QUALITIES:
        coefs = jpegc_ref(px, layout, quality)[0]
        whole = codec.encode_jpeg_coefs(coefs, w, h, layout, quality)
        header, scan = codec.jpeg_header(w, h, layout, quality), codec.jpeg_scan(coefs, w, h, layout)
        assert header + scan + b"\xff\xd9" == whole
        assert codec.jpeg_from_scan(scan, w, h, layout, quality) == whole
        assert header[:2] == b"\xff\xd8" and header[-14:-12] == b"\xff\xda"     # SOI ... SOS (12-byte body)
        got, bits = codec.jpeg_scan_bits(coefs, w, h, layout)
        assert got == scan and len(jpege_ref.unstuffed(scan)) == -(-bits // 8)
        assert sum(jpege_ref.block_bits(coefs, w, h, layout)) == bits
        assert len(jpege_ref.block_bits(coefs, w, h, layout)) == jpege_ref.scan_blocks(w, h, layout)


@pytest.mark.parametrize("layout,quality", [(YCC_444, 92), (YCC_420, 75)], ids=["444", "420"])
def test_pillow_decodes_jpeg_from_scan_like_its_own_file(layout, quality):
    from imaginary_amd import codec
    for w, h in [(37, 29), (17, 9), (129, 67)]:
        px = np.random.default_rng(w * h).integers(0, 256, (h, w, 3), dtype=np.uint8)
        coefs = jpegc_ref(px, layout, quality)[0]
        mine = codec.jpeg_from_scan(codec.jpeg_scan(coefs, w, h, layout), w, h, layout, quality)
        out = io.BytesIO()
        PIL.fromarray(px).save(out, "JPEG", quality=quality, subsampling={YCC_444: 0, YCC_420: 2}[layout])
        a, b = PIL.open(io.BytesIO(mine)), PIL.open(io.BytesIO(out.getvalue()))
        assert a.size == b.size == (w, h) and np.array_equal(np.asarray(a), np.asarray(b))


def test_jpeg_scan_refuses_what_annex_k_cannot_code():
    from imaginary_amd import codec
    z = np.zeros(3 * 64, np.int16)
    for k, v, ok in [(5, 1023, True), (5, -1023, True), (5, 1024, False), (5, -1024, False), (63, -32768, False),
                     (0, 2047, True), (0, -2047, True), (0, 2048, False), (0, -2048, False), (64, 2048, False)]:
        c = z.copy()
        c[k] = v
        if ok:
            assert codec.jpeg_scan(c, 8, 8, YCC_444)
            assert slot_ref(c, 8, 8, YCC_444).status == OK
        else:
            with pytest.raises(ValueError):
                codec.jpeg_scan(c, 8, 8, YCC_444)
            s = slot_ref(c, 8, 8, YCC_444)
            assert (s.status, s.length) == (UNCODABLE, 0)
    # the difference counts, not the value: 1100 after -1100 in the next Y block is a step of 2200
    c = np.zeros(6 * 64, np.int16)
    c[0], c[64] = -1100, 1100
    with pytest.raises(ValueError):
        codec.jpeg_scan(c, 16, 8, YCC_444)
    c[64] = 900
    assert codec.jpeg_scan(c, 16, 8, YCC_444)


# ---------------------------------------------------------------- the reference slot
def test_reference_slot_statuses_and_lengths():
    px = np.random.default_rng(5).integers(0, 256, (29, 37, 3), dtype=np.uint8)
    coefs = jpegc_ref(px, YCC_420, 75)[0]
    s = slot_ref(coefs, 37, 29, YCC_420)
    assert s.status == OK and s.length == len(s.scan) <= jpegc_bytes(37, 29, YCC_420) and 0 < s.bits <= 8 * s.length
    assert s.header().tolist() == [s.length, 0, s.bits, 0]
    # every AC +-1023: 26 bits per coefficient, more than the 16 it takes
    w = h = 16
    full = np.where(np.arange(jpegc_bytes(w, h, YCC_420) // 2) % 2 == 0, 1023, -1023).astype(np.int16)
    full[::64] = 0
    s = slot_ref(full, w, h, YCC_420)
    assert s.status == OVERFLOW and s.length == -(-s.bits // 8) > jpegc_bytes(w, h, YCC_420) and s.scan == b""
    assert s.bits == sum(jpege_ref.block_bits(full, w, h, YCC_420))
    slot = np.zeros(jpeg_scan_bytes(w, h, YCC_420), np.uint8)
    slot[:16] = s.header().view(np.uint8)
    check_slot(slot, s, "overflow")
    with pytest.raises(AssertionError):
        slot[4] = 0
        check_slot(slot, s, "overflow read as ok")


def test_a_scan_can_fit_before_stuffing_and_not_after():
    """Every AC 127 (a short code and seven 1-bits): the second way to overflow, which the GPU tests run."""
    from imaginary_amd import codec
    w = h = 16
    for layout in (YCC_444, YCC_420):
        cap = jpegc_bytes(w, h, layout)
        c = np.full(cap // 2, 127, np.int16)
        c[::64] = 0
        scan, bits = codec.jpeg_scan_bits(c, w, h, layout)
        assert -(-bits // 8) <= cap < len(scan)
        s = slot_ref(c, w, h, layout)
        assert (s.status, s.length, s.bits) == (OVERFLOW, -(-bits // 8), bits)


def test_random_noise_at_q100_fits_the_slot():
    """What the GPU tests rely on: at their sizes full-range noise at Q 100, the longest scans an
    8-bit image gives, stays under the capacity (a block of it codes to about 100 of its 128 bytes)."""
    for layout in (YCC_444, YCC_420):
        for w, h in [(8, 8), (16, 16), (37, 29), (129, 67), (1, 1), (1, 40)]:
            px = np.random.default_rng(w * 100003 + h * 101 + 3).integers(0, 256, (3, h, w, 3), dtype=np.uint8)
            for c in jpegc_ref(px, layout, 100):
                assert slot_ref(c, w, h, layout).status == OK


def test_the_two_found_inputs_are_what_they_are_for():
    from imaginary_amd import codec
    a, b = jpege_ref.padding_ff_coefs(), jpege_ref.straddle_ff_coefs()
    assert a.size == b.size == 3 * 64
    scan, bits = codec.jpeg_scan_bits(a, 8, 8, YCC_444)
    assert bits % 8 != 0 and scan[-2:] == b"\xff\x00"          # the padding completed an 0xFF, and it is stuffed
    assert jpege_ref.ends_in_padding_ff(a, 8, 8, YCC_444) and not jpege_ref.ff_straddles_blocks(a, 8, 8, YCC_444)
    assert jpege_ref.ff_straddles_blocks(b, 8, 8, YCC_444) and not jpege_ref.ends_in_padding_ff(b, 8, 8, YCC_444)
    # the straddling byte, spelled out: an 0xFF of the unstuffed scan with a block's end inside it
    scan, bits = codec.jpeg_scan_bits(b, 8, 8, YCC_444)
    ends = np.cumsum(jpege_ref.block_bits(b, 8, 8, YCC_444))[:-1]
    raw = jpege_ref.unstuffed(scan)
    assert any(raw[e // 8] == 0xFF and e % 8 for e in ends.tolist())
    assert slot_ref(a, 8, 8, YCC_444).status == OK and slot_ref(b, 8, 8, YCC_444).status == OK


# ---------------------------------------------------------------- sizes
def test_jpeg_scan_bytes():
    import imaginary_amd as ia
    for w, h in SIZES + [(3840, 2160), (520, 264)]:
        for layout in (YCC_444, YCC_420):
            assert ia.jpeg_scan_bytes(w, h, layout) == jpeg_scan_bytes(w, h, layout) == 16 + ia.jpegc_bytes(w, h, layout)
    assert ia.jpeg_scan_bytes(17, 9, YCC_420) == 16 + 128 * 10
    assert ia.jpeg_scan_bytes(8, 8, YCC_444) == 16 + 384
    assert ia.jpeg_scan_bytes(0, 3, YCC_420) == 0 and ia.jpeg_scan_bytes(3, -1, YCC_444) == 0
    assert ia.jpeg_scan_bytes(3, 3, 2) == 0 and ia.jpeg_scan_bytes(3, 3, -1) == 0


def test_workspace_formula():
    import imaginary_amd as ia
    f = ia.lib.mipx_op_workspace_bytes
    for n in (1, 3, 64):
        for w, h in SIZES + [(520, 264), (3840, 2160)]:
            assert f(OP_JPEGE, n, w, h, 3, 0.0, 0.0) == jpege_ref.workspace_bytes(n, w, h), (n, w, h)
    assert f(OP_JPEGE, 1, 8, 8, 3, 0.0, 0.0) == 2 * 512 + 6 * 256      # 384 bytes twice, six small parts: each rounds up to 256
    assert f(OP_JPEGE, 0, 8, 8, 3, 0.0, 0.0) == 0 and f(OP_JPEGE, 1, 0, 8, 3, 0.0, 0.0) == 0
    # a 1 x 1 image has 3 real blocks, and 6 in a 4:2:0 scan: the bound is the larger
    assert jpege_ref.scan_blocks(1, 1, YCC_420) == 6 > jpege_ref.scan_blocks(1, 1, YCC_444)
    # a plan that ends with the step asks for it
    p = _plan(ia, w=64, h=48)
    ia.plan_set_jpeg_scan_output(p, YCC_420, 75)
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= jpege_ref.workspace_bytes(2, 64, 48)


def test_op_number_is_appended():
    from imaginary_amd import _abi
    assert _abi.OP_JPEGRT == 18 and _abi.OP_JPEGE == OP_JPEGE and _abi.OP_NAMES[19] == "jpege"
    assert _abi.lib.mipx_abi_version() == 6
    assert (_abi.JPEG_SCAN_OK, _abi.JPEG_SCAN_OVERFLOW, _abi.JPEG_SCAN_UNCODABLE) == (OK, OVERFLOW, UNCODABLE)


# ---------------------------------------------------------------- the code table
def test_host_built_code_table_is_codecs(tmp_path):
    """tests/c/jpege_codes_host.cpp prints build_jpege_codes' table; built as
    tests/test_tables_host.py builds its program."""
    from imaginary_amd import codec
    exe = tmp_path / "jpege_codes_host"
    csrc = os.path.join(ROOT, "imaginary_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "jpege_codes_host.cpp"), os.path.join(csrc, "mipx_tables.cpp"),
                    os.path.join(csrc, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {}
    for line in out.stdout.split("\n"):
        if line:
            t, sym, code, length = map(int, line.split())
            assert (t, sym) not in got
            got[t, sym] = (code, length)
    want = {}
    for t, tc in enumerate((0x00, 0x10, 0x01, 0x11)):      # DC lum, AC lum, DC chr, AC chr
        for sym, cl in codec._huff_codes(codec.HUFFMAN_TABLES[tc]).items():
            want[t, sym] = cl
    assert got == want
    assert len(want) == 12 + 162 + 12 + 162


# ---------------------------------------------------------------- planner
def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def test_set_jpeg_scan_output_puts_the_step_last_and_keeps_the_geometry():
    import imaginary_amd as ia
    p = _plan(ia, width=60, height=40, crop=1)
    before = p.describe()
    geom = (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands)
    assert ia.plan_set_jpeg_scan_output(p, YCC_420, 80) is p
    assert p.describe() == before + [("jpege", (YCC_420, 80, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (60, 40, 3))]
    assert (p.load_shrink, p.in_w, p.in_h, p.in_bands, p.out_w, p.out_h, p.out_bands) == geom
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) > 0   # the plan validates
    e = _plan(ia)                                           # the empty plan: the step alone
    ia.plan_set_jpeg_scan_output(e, YCC_444, 100)
    assert [s[0] for s in e.describe()] == ["jpege"] and (e.out_w, e.out_h, e.out_bands) == (128, 96, 3)
    assert ia.lib.mipx_workspace_bytes(C.byref(e), 1) >= jpege_ref.workspace_bytes(1, 128, 96)


def test_set_jpeg_scan_output_composes_like_the_coefficient_step():
    import imaginary_amd as ia
    a = _plan(ia, width=60)
    ia.plan_set_ycc_input(a, YCC_420)
    ia.plan_set_jpeg_scan_output(a, YCC_420, 75)
    assert [s[0] for s in a.describe()] == ["ycc", "reduce", "jpege"]
    b = _plan(ia, width=60)
    ia.plan_set_jpeg_scan_output(b, YCC_420, 75)
    ia.plan_set_ycc_input(b, YCC_420)
    assert bytes(a) == bytes(b) and ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    j = _plan(ia, width=128)
    ia.plan_set_jpeg_scan_output(j, YCC_420, 75)
    ia.plan_set_jpegd_input(j, YCC_420)
    assert [s[0] for s in j.describe()][0] == "jpegd" and [s[0] for s in j.describe()][-1] == "jpege"
    # the text mark lands in front of the step either way
    c = _plan(ia, width=60)
    ia.plan_add_textmark(c, 20, 8, 5, 0.5, (1, 2, 3))
    ia.plan_set_jpeg_scan_output(c, YCC_444, 90)
    d = _plan(ia, width=60)
    ia.plan_set_jpeg_scan_output(d, YCC_444, 90)
    ia.plan_add_textmark(d, 20, 8, 5, 0.5, (1, 2, 3))
    assert [s[0] for s in c.describe()] == ["reduce", "textmark", "jpege"] and bytes(c) == bytes(d)
    assert ia.lib.mipx_workspace_bytes(C.byref(c), 1) > 0
    # after a round trip
    r = _plan(ia, width=60)
    ia.plan_add_jpeg_roundtrip(r, YCC_420, 80, 2)
    ia.plan_set_jpeg_scan_output(r, YCC_420, 75)
    assert [s[0] for s in r.describe()] == ["reduce", "jpegrt", "jpege"] and ia.lib.mipx_workspace_bytes(C.byref(r), 1) > 0


def test_set_jpeg_scan_output_refusals():
    import imaginary_amd as ia
    L = ia.lib
    f = L.mipx_plan_set_jpeg_scan_output
    p = _plan(ia, width=60)
    assert f(C.byref(p), 2, 75) == -1            # unknown layout
    assert f(C.byref(p), -1, 75) == -1
    for q in (0, -5, 101, 1000):
        assert f(C.byref(p), YCC_420, q) == -1   # quality outside 1..100
    assert f(None, YCC_420, 75) == -1
    assert p.n_steps == 1
    for bands in (1, 2, 4):
        q = _plan(ia, bands=bands, width=60)
        n = q.n_steps
        assert f(C.byref(q), YCC_420, 75) == -1  # out_bands != 3
        assert q.n_steps == n
    w = ia.plan_make(ia.make_opts(width=60, wm_enable=1), ia.make_input(128, 96, 3, "png", wm_w=10, wm_h=10, wm_bands=4))
    assert w.out_bands == 4 and f(C.byref(w), YCC_420, 75) == -1   # RGBA out
    assert f(C.byref(p), YCC_420, 1) == 0
    assert f(C.byref(p), YCC_420, 1) == -1       # already ends with the step
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_420, 75) == -1      # ... and takes no coefficient step
    assert L.mipx_plan_add_jpeg_roundtrip(C.byref(p), YCC_420, 75, 1) == -1  # ... nor a round trip behind it
    assert p.n_steps == 2
    c = _plan(ia, width=60)
    ia.plan_set_jpegc_output(c, YCC_420, 75)
    assert f(C.byref(c), YCC_420, 75) == -1      # ends with MIPX_OP_JPEGC
    assert c.n_steps == 2
    full = _plan(ia)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2   # flips
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = 128, 96, 3
    assert f(C.byref(full), YCC_420, 75) == -1   # full plan
    assert full.n_steps == 64 and full.steps[63].op == 2


def _hand_plan(ia, ops, bands=3, w=16, h=12):
    """A plan of flips, coefficient steps (16) and scan steps (19) written by hand."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op in (16, OP_JPEGE):
            p.steps[i].a[0], p.steps[i].a[1] = YCC_420, 75
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_step_is_legal_only_last_on_three_bands_and_without_the_coefficient_step():
    """Checked in the plan validation, before any device work: the pointers are never used."""
    import imaginary_amd as ia
    L = ia.lib
    ok = _hand_plan(ia, [2, OP_JPEGE])
    assert L.mipx_workspace_bytes(C.byref(ok), 1) > 0
    cases = [_hand_plan(ia, [OP_JPEGE, 2]), _hand_plan(ia, [OP_JPEGE, OP_JPEGE]), _hand_plan(ia, [2, OP_JPEGE, 2]),
             _hand_plan(ia, [2, OP_JPEGE], bands=4), _hand_plan(ia, [2, OP_JPEGE], bands=1),
             _hand_plan(ia, [16, OP_JPEGE]), _hand_plan(ia, [OP_JPEGE, 16]), _hand_plan(ia, [2, 16, OP_JPEGE])]
    bad_layout = _hand_plan(ia, [2, OP_JPEGE])
    bad_layout.steps[1].a[0] = 7
    bad_quality = _hand_plan(ia, [2, OP_JPEGE])
    bad_quality.steps[1].a[1] = 0
    too_good = _hand_plan(ia, [2, OP_JPEGE])
    too_good.steps[1].a[1] = 101
    for p in cases + [bad_layout, bad_quality, too_good]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
    four = _hand_plan(ia, [2, OP_JPEGE], bands=4)
    four.steps[1].out_bands = 3
    four.out_bands = 3
    assert L.mipx_workspace_bytes(C.byref(four), 1) == 0


def test_chain_takes_the_step_in_the_last_stage_only():
    import imaginary_amd as ia
    s0 = _plan(ia, width=64)
    s1 = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    last = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    ia.plan_set_jpeg_scan_output(last, YCC_420, 75)
    merged = ia.plan_chain([s0, last])
    assert [s[0] for s in merged.describe()] == ["reduce", "reduce", "jpege"]
    assert (merged.out_w, merged.out_h, merged.out_bands) == (last.out_w, last.out_h, 3)
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    first = _plan(ia, width=64)
    ia.plan_set_jpeg_scan_output(first, YCC_420, 75)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain((ia.MipxPlan * 2)(first, s1), 2, C.byref(out)) == -1
    arr = (ia.MipxPlan * 3)(s0, last, _plan(ia, w=last.out_w, h=last.out_h, flip=1))
    assert ia.lib.mipx_plan_chain(arr, 3, C.byref(out)) == -1


def test_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    EINVAL = -1
    f, g = L.mipx_op_rgb_to_jpeg_scan, L.mipx_op_jpegc_to_scan
    W = 4096   # a "workspace pointer": 16-byte aligned, never used
    assert f(None, 1, 1, 8, 8, YCC_420, 75, W, None) == EINVAL
    assert f(1, None, 1, 8, 8, YCC_420, 75, W, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 75, None, None) == EINVAL
    assert f(1, 1, 0, 8, 8, YCC_420, 75, W, None) == EINVAL
    assert f(1, 1, 1, 0, 8, YCC_420, 75, W, None) == EINVAL
    assert f(1, 1, 1, 8, -1, YCC_444, 75, W, None) == EINVAL
    assert f(1, 1, 1, 8, 8, 2, 75, W, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 0, W, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 101, W, None) == EINVAL
    assert f(1, 1, 1, 8, 8, YCC_420, 75, W + 4, None) == EINVAL       # a misaligned workspace
    assert g(None, 1, 1, 8, 8, YCC_420, W, None) == EINVAL
    assert g(1, None, 1, 8, 8, YCC_420, W, None) == EINVAL
    assert g(1, 1, 1, 8, 8, YCC_420, None, None) == EINVAL
    assert g(1, 1, -2, 8, 8, YCC_420, W, None) == EINVAL
    assert g(1, 1, 1, 8, 0, YCC_420, W, None) == EINVAL
    assert g(1, 1, 1, 8, 8, -1, W, None) == EINVAL
    assert g(1, 1, 1, 8, 8, YCC_444, W + 8, None) == EINVAL
    # an image whose payload or RGB is 2^32 bytes or more, as mipx_op_jpegd_to_rgb refuses it
    for layout in (YCC_420, YCC_444):
        assert f(1, 1, 1, 40000, 40000, layout, 75, W, None) == -2
        assert g(1, 1, 1, 40000, 40000, layout, W, None) == -2
    assert g(1, 1, 1, 30000, 30000, YCC_444, W, None) == -2

    # mipx_submit for a scan plan: out is w x h x 3, stride 0, data = one slot
    p = _plan(ia, w=16, h=12, width=8)
    ia.plan_set_jpeg_scan_output(p, YCC_420, 75)
    src = np.zeros((12, 16, 3), np.uint8)
    dst = np.zeros(jpeg_scan_bytes(p.out_w, p.out_h, YCC_420), np.uint8)
    img = MipxImg(src.ctypes.data, 16, 12, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, data=dst.ctypes.data):
        out = MipxImg(data, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(img), None, C.byref(out), C.byref(t))

    assert (p.out_w, p.out_h) == (8, 6)
    assert submit(8, 6, 3, 24) == EINVAL          # a stride, even the natural one of RGB rows
    assert submit(8, 6, 1, 0) == EINVAL
    assert submit(16, dst.size // 16, 1, 0) == EINVAL   # described as rows of 16 bytes
    assert submit(16, 12, 3, 0) == EINVAL
    assert submit(8, 6, 3, 0, None) == EINVAL
    if ia.device_count() == 0:
        assert submit(8, 6, 3, 0) == -7           # well-formed: only the engine is missing
