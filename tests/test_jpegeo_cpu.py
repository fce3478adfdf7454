"""Entropy-coded JPEG output with optimised Huffman tables (MIPX_OP_JPEGE with a[2] = 1,
PARITY_ASSUMPTIONS.md row 24), the parts that need no GPU:

 - codec.encode_jpeg_coefs(..., tables="optimal") is byte for byte the file libjpeg-turbo inside
   Pillow writes with optimize=True, also where the library's limiting to 16 bits runs;
 - a table of Fibonacci counts is a legal one;
 - the host builder (mipx_tables.cpp jpeg_optimal_table, the serial form the kernel is held to)
   against codec.jpeg_optimal_table, also under the address and undefined-behaviour sanitizers;
 - mipx_jpeg_scan_opt_bytes, the workspace formula, the plan step's a[2], the planner entry point and
   the argument checks of the two new op calls.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import jpege_ref
import jpegeo_ref
from conftest import ROOT
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes, jpegc_ref
from jpegeo_ref import PICTURES, PIN_QUALITIES, PIN_SIZES, picture
from jpegr_ref import pillow_jpeg

OP_JPEGE = 19
EINVAL = -1
TABLE_KEYS = (0x00, 0x10, 0x01, 0x11)


# ---------------------------------------------------------------- the library pin
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
@pytest.mark.parametrize("w,h", PIN_SIZES, ids=lambda v: str(v))
def test_optimal_tables_give_pillows_optimized_file(w, h, layout):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    for kind in PICTURES:
        px = picture(kind, w, h)
        for quality in PIN_QUALITIES:
            coefs = jpegc_ref(px[None], layout, quality)[0]
            mine = codec.encode_jpeg_coefs(coefs, w, h, layout, quality, tables="optimal")
            assert mine == pillow_jpeg(px, layout, quality, optimize=True), (kind, quality)
            tables = jpegeo_ref.optimal_tables(coefs, w, h, layout)
            assert mine == codec.jpeg_from_scan(codec.jpeg_scan(coefs, w, h, layout, tables), w, h, layout, quality, tables)
            # and without the keyword nothing changed
            assert codec.encode_jpeg_coefs(coefs, w, h, layout, quality) == pillow_jpeg(px, layout, quality)


# found by search over noise of three seeds at 129 x 67, 200 x 120 and 333 x 211, both samplings, Q 30 to 100
LIMITED = [(333, 211, 1, YCC_444, 97, 0x11), (333, 211, 2, YCC_420, 100, 0x10)]   # raw lengths up to 18


@pytest.mark.parametrize("w,h,seed,layout,quality,table", LIMITED)
def test_a_table_whose_raw_lengths_exceed_16_is_limited_as_the_library_does(w, h, seed, layout, quality, table):
    pytest.importorskip("PIL.Image")
    from imaginary_amd import codec
    px = np.random.default_rng(seed * 1000 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    coefs = jpegc_ref(px[None], layout, quality)[0]
    counts = codec.jpeg_symbol_counts(coefs, w, h, layout)
    assert max(codec._jpeg_code_sizes(counts[table])) > 16          # the limiting ran
    assert max(k for k, c in enumerate(codec.jpeg_optimal_table(counts[table])[0], 1) if c) == 16
    assert codec.encode_jpeg_coefs(coefs, w, h, layout, quality, tables="optimal") == pillow_jpeg(px, layout, quality, optimize=True)


def test_symbol_counts_are_the_scans_symbols():
    """Counted once more from the bits: the optimal scan's length is the sum over the symbols of
    count x (code length + value bits)."""
    from imaginary_amd import codec
    for layout in (YCC_444, YCC_420):
        w, h = 37, 29
        coefs = jpegc_ref(picture("noise", w, h)[None], layout, 75)[0]
        counts = codec.jpeg_symbol_counts(coefs, w, h, layout)
        assert sum(counts[0x00]) + sum(counts[0x01]) == jpege_ref.scan_blocks(w, h, layout)
        for tables in (codec.HUFFMAN_TABLES, jpegeo_ref.optimal_tables(coefs, w, h, layout)):
            bits = 0
            for tc in TABLE_KEYS:
                codes = codec._huff_codes(tables[tc])
                bits += sum(n * (codes[s][1] + (s & 15 if tc & 0x10 else s)) for s, n in enumerate(counts[tc]) if n)
            assert bits == codec.jpeg_scan_bits(coefs, w, h, layout, None if tables is codec.HUFFMAN_TABLES else tables)[1]
    with pytest.raises(ValueError):
        c = np.zeros(3 * 64, np.int16)
        c[5] = 1024
        codec.jpeg_symbol_counts(c, 8, 8, YCC_444)


# ---------------------------------------------------------------- one table
def _check_table(table, freq):
    from imaginary_amd import codec
    counts, symbols = table
    assert len(counts) == 16 and sum(counts) == len(symbols) == sum(1 for f in freq if f)
    assert sorted(symbols) == [s for s, f in enumerate(freq) if f]
    kraft = sum(c * 2 ** (16 - length) for length, c in enumerate(counts, 1))
    assert kraft < 2 ** 16                                   # the reserved point leaves room
    codes = codec._huff_codes(table)
    assert all(code != (1 << length) - 1 for code, length in codes.values())   # no code is all ones
    assert codec._huff_lookup(counts, symbols) is not None
    return codes


def test_fibonacci_frequencies_give_a_legal_table():
    from imaginary_amd import codec
    freq = jpegeo_ref.fibonacci_histogram(30)
    assert sum(1 for f in freq if f) == 30 and max(freq) == 1346269
    assert max(codec._jpeg_code_sizes(freq)) == 30           # a chain (tests/jpegeo_ref.py): the limiting runs
    table = codec.jpeg_optimal_table(freq)
    codes = _check_table(table, freq)
    assert max(length for _, length in codes.values()) == 16
    by_count = sorted((f, s) for s, f in enumerate(freq) if f)
    assert [codes[s][1] for _, s in by_count] == sorted((codes[s][1] for _, s in by_count), reverse=True)


def test_the_hand_made_coefficients_have_fibonacci_counts_and_a_deep_tree():
    from imaginary_amd import codec
    c, w, h = jpegeo_ref.fibonacci_coefs()
    assert c.size * 2 == jpegc_bytes(w, h, YCC_444) and (w, h) == (488, 80)
    counts = codec.jpeg_symbol_counts(c, w, h, YCC_444)
    assert sorted(f for f in counts[0x10] if f) == jpegeo_ref.fibonacci(20) and counts[0x10][0] == 610
    assert max(codec._jpeg_code_sizes(counts[0x10])) == 20
    assert [f for f in counts[0x11] if f] == [1220] and [f for f in counts[0x00] if f] == [610]
    assert jpegeo_ref.slot_ref(c, w, h, YCC_444).status == jpegeo_ref.OK


def test_small_tables():
    from imaginary_amd import codec
    one = [0] * 256
    one[0] = 7
    assert codec.jpeg_optimal_table(one) == (bytes([1] + [0] * 15), bytes([0]))       # EOB alone: the code 0
    two = [0] * 256
    two[3], two[200] = 5, 5
    table = codec.jpeg_optimal_table(two)
    assert table == (bytes([1, 1] + [0] * 14), bytes([3, 200]))   # the reserved point pairs with 200 first
    _check_table(table, two)
    assert codec.jpeg_optimal_table([0] * 256) == (bytes(16), b"")


# ---------------------------------------------------------------- the host builder
def _histograms():
    from imaginary_amd import codec
    out = []
    for w, h in PIN_SIZES[:4]:
        for layout in (YCC_444, YCC_420):
            for kind in PICTURES:
                coefs = jpegc_ref(picture(kind, w, h)[None], layout, 75)[0]
                out += list(codec.jpeg_symbol_counts(coefs, w, h, layout).values())
    out.append(jpegeo_ref.fibonacci_histogram(30))
    out.append(jpegeo_ref.fibonacci_histogram(40))      # raw lengths up to 40
    c, w, h = jpegeo_ref.fibonacci_coefs()               # what the GPU test feeds the device
    out += list(codec.jpeg_symbol_counts(c, w, h, YCC_444).values())
    for s, f in [(0, 1), (0, 1000), (255, 3), (0xF0, 1)]:
        one = [0] * 256
        one[s] = f
        out.append(one)
    out.append([0] * 256)
    out.append([1] * 256)                                 # every symbol, equal counts: ties everywhere
    out.append([(7 * i) % 5 for i in range(256)])
    return out


def _build_host(tmp_path, name, extra):
    exe = tmp_path / name
    csrc = os.path.join(ROOT, "imaginary_amd", "csrc")
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__"] + extra +
                   ["-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "jpego_tables_host.cpp"), os.path.join(csrc, "mipx_tables.cpp"),
                    os.path.join(csrc, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    return exe


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan+ubsan"])
def test_host_builder_is_codecs(tmp_path, sanitize):
    """tests/c/jpego_tables_host.cpp, a program of its own: with the sanitizers it is this program that
    runs under them, nothing loaded into Python."""
    from imaginary_amd import codec
    hists = _histograms()
    path = tmp_path / "histograms.txt"
    path.write_text("".join(" ".join(map(str, f)) + "\n" for f in hists))
    # the sanitizers' runtimes are linked into the program itself, so it runs in whatever environment the suite has
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]
    exe = _build_host(tmp_path, "jpego_tables_host", flags if sanitize else [])
    out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    assert len(lines) == 4 * len(hists) + 1 and lines[-1] == ""
    for i, freq in enumerate(hists):
        raw, counts, symbols, codes = lines[4 * i:4 * i + 4]
        want = codec.jpeg_optimal_table(freq)
        assert int(raw) == max(codec._jpeg_code_sizes(freq)), i
        assert bytes(map(int, counts.split())) == want[0], (i, counts)
        assert bytes(map(int, symbols.split())) == want[1], (i, symbols)
        words = codes.split()
        assert words[0] == "codes"
        v = list(map(int, words[1:]))
        assert {v[k]: (v[k + 1], v[k + 2]) for k in range(0, len(v), 3)} == codec._huff_codes(want), i


# ---------------------------------------------------------------- sizes
SIZES = [(1, 1), (8, 8), (17, 9), (9, 17), (37, 29), (129, 67), (197, 117), (1, 40), (3840, 2160)]


def test_jpeg_scan_opt_bytes():
    import imaginary_amd as ia
    from imaginary_amd import _abi
    assert _abi.JPEG_SCAN_OPT_HEADER_BYTES == jpegeo_ref.HEADER_BYTES == 16 + 4 * 272
    for w, h in SIZES:
        for layout in (YCC_444, YCC_420):
            assert ia.jpeg_scan_opt_bytes(w, h, layout) == jpegeo_ref.jpeg_scan_opt_bytes(w, h, layout) \
                == 1104 + ia.jpegc_bytes(w, h, layout) == ia.jpeg_scan_bytes(w, h, layout) + 1088
    assert ia.jpeg_scan_opt_bytes(8, 8, YCC_444) == 1104 + 384
    assert ia.jpeg_scan_opt_bytes(0, 3, YCC_420) == 0 and ia.jpeg_scan_opt_bytes(3, -1, YCC_444) == 0
    assert ia.jpeg_scan_opt_bytes(3, 3, 2) == 0 and ia.jpeg_scan_opt_bytes(3, 3, -1) == 0


def test_workspace_formula():
    import imaginary_amd as ia
    f = ia.lib.mipx_op_workspace_bytes
    for n in (1, 3, 64):
        for w, h in SIZES:
            assert f(OP_JPEGE, n, w, h, 3, 1.0, 0.0) == jpegeo_ref.workspace_bytes(n, w, h), (n, w, h)
            assert f(OP_JPEGE, n, w, h, 3, 0.0, 0.0) == jpege_ref.workspace_bytes(n, w, h), (n, w, h)   # unchanged
    assert f(OP_JPEGE, 1, 8, 8, 3, 1.0, 0.0) == 2 * 512 + 6 * 256 + 8192
    assert f(OP_JPEGE, 0, 8, 8, 3, 1.0, 0.0) == 0
    p = _plan(ia, w=64, h=48)
    ia.plan_set_jpeg_scan_output(p, YCC_420, 75, optimize=True)
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= jpegeo_ref.workspace_bytes(2, 64, 48)
    q = _plan(ia, w=64, h=48)
    ia.plan_set_jpeg_scan_output(q, YCC_420, 75)
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) == ia.lib.mipx_workspace_bytes(C.byref(q), 2) + 2 * 8192


def test_abi_version_is_unchanged():
    from imaginary_amd import _abi
    assert _abi.lib.mipx_abi_version() == 6 and _abi.OP_JPEGE == OP_JPEGE


# ---------------------------------------------------------------- planner and plan validation
def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


def test_planner_entry_point_sets_the_flag_and_nothing_else():
    import imaginary_amd as ia
    a, b = _plan(ia, width=60, height=40, crop=1), _plan(ia, width=60, height=40, crop=1)
    before = a.describe()
    assert ia.plan_set_jpeg_scan_output(a, YCC_420, 80, optimize=True) is a
    ia.plan_set_jpeg_scan_output(b, YCC_420, 80)
    assert a.describe() == before + [("jpege", (YCC_420, 80, 1, 0, 0, 0, 0, 0), (0.0,) * 4, (60, 40, 3))]
    assert b.describe() == before + [("jpege", (YCC_420, 80, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (60, 40, 3))]   # planner-built: 0
    b.steps[b.n_steps - 1].a[2] = 1
    assert bytes(a) == bytes(b)
    assert ia.lib.mipx_workspace_bytes(C.byref(a), 2) > 0


def test_planner_entry_point_refusals():
    import imaginary_amd as ia
    L = ia.lib
    f = L.mipx_plan_set_jpeg_scan_output_optimized
    p = _plan(ia, width=60)
    assert f(C.byref(p), 2, 75) == EINVAL and f(C.byref(p), -1, 75) == EINVAL
    for q in (0, -5, 101, 1000):
        assert f(C.byref(p), YCC_420, q) == EINVAL
    assert f(None, YCC_420, 75) == EINVAL and p.n_steps == 1
    for bands in (1, 2, 4):
        q = _plan(ia, bands=bands, width=60)
        assert f(C.byref(q), YCC_420, 75) == EINVAL
    assert f(C.byref(p), YCC_420, 1) == 0
    assert f(C.byref(p), YCC_420, 1) == EINVAL and L.mipx_plan_set_jpeg_scan_output(C.byref(p), YCC_420, 1) == EINVAL
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_420, 75) == EINVAL
    assert L.mipx_plan_add_jpeg_roundtrip(C.byref(p), YCC_420, 75, 1) == EINVAL and p.n_steps == 2
    c = _plan(ia, width=60)
    ia.plan_set_jpegc_output(c, YCC_420, 75)
    assert f(C.byref(c), YCC_420, 75) == EINVAL
    # it composes as today's step does: a text mark lands in front of it
    d = _plan(ia, width=60)
    ia.plan_set_jpeg_scan_output(d, YCC_444, 90, optimize=True)
    ia.plan_add_textmark(d, 20, 8, 5, 0.5, (1, 2, 3))
    assert [s[0] for s in d.describe()] == ["reduce", "textmark", "jpege"] and d.steps[2].a[2] == 1


def _hand_plan(ia, ops, bands=3, w=16, h=12, flag=1):
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op in (16, OP_JPEGE):
            p.steps[i].a[0], p.steps[i].a[1] = YCC_420, 75
        if op == OP_JPEGE:
            p.steps[i].a[2] = flag
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_the_flag_is_zero_or_one_and_the_step_is_legal_where_todays_is():
    import imaginary_amd as ia
    L = ia.lib
    for flag in (0, 1):
        assert L.mipx_workspace_bytes(C.byref(_hand_plan(ia, [2, OP_JPEGE], flag=flag)), 1) > 0
    bad = [_hand_plan(ia, [2, OP_JPEGE], flag=flag) for flag in (2, -1, 3, 256, 1 << 30)]
    bad += [_hand_plan(ia, [OP_JPEGE, 2]), _hand_plan(ia, [OP_JPEGE, OP_JPEGE]), _hand_plan(ia, [2, OP_JPEGE, 2]),
            _hand_plan(ia, [2, OP_JPEGE], bands=4), _hand_plan(ia, [2, OP_JPEGE], bands=1), _hand_plan(ia, [16, OP_JPEGE]),
            _hand_plan(ia, [OP_JPEGE, 16]), _hand_plan(ia, [2, 16, OP_JPEGE])]
    for k, field in enumerate([7, 0, 101]):
        p = _hand_plan(ia, [2, OP_JPEGE])
        p.steps[1].a[0 if k == 0 else 1] = field
        bad.append(p)
    for p in bad:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == EINVAL


def test_a_scan_of_a_thousand_million_symbols_is_refused_for_this_variant_only():
    """64 x blocks >= 10^9: 15,625,000 blocks; 4:4:4 has 3 per 8 x 8 pixels."""
    import imaginary_amd as ia
    L = ia.lib
    w, h = 8 * 2500, 8 * 2084       # 5,210,000 MCUs: 15,630,000 blocks
    assert 64 * 3 * 2500 * 2084 >= 10 ** 9 > 64 * 3 * 2500 * 2083
    big, under = _hand_plan(ia, [OP_JPEGE], w=w, h=h), _hand_plan(ia, [OP_JPEGE], w=w, h=h - 8)
    big.steps[0].a[0] = under.steps[0].a[0] = YCC_444
    assert L.mipx_workspace_bytes(C.byref(big), 1) == 0 and L.mipx_workspace_bytes(C.byref(under), 1) > 0
    big.steps[0].a[2] = 0
    assert L.mipx_workspace_bytes(C.byref(big), 1) > 0
    p = _plan(ia, w=w, h=h)
    assert L.mipx_plan_set_jpeg_scan_output_optimized(C.byref(p), YCC_444, 75) == EINVAL
    assert L.mipx_plan_set_jpeg_scan_output_optimized(C.byref(p), YCC_420, 75) == 0     # half the blocks
    W = 4096
    assert L.mipx_op_jpegc_to_scan_optimized(1, 1, 1, w, h, YCC_444, W, None) == EINVAL
    assert L.mipx_op_rgb_to_jpeg_scan_optimized(1, 1, 1, w, h, YCC_444, 75, W, None) == EINVAL


def test_chain_keeps_the_flag():
    import imaginary_amd as ia
    s0 = _plan(ia, width=64)
    last = _plan(ia, w=s0.out_w, h=s0.out_h, width=32)
    ia.plan_set_jpeg_scan_output(last, YCC_420, 75, optimize=True)
    merged = ia.plan_chain([s0, last])
    assert [s[0] for s in merged.describe()] == ["reduce", "reduce", "jpege"]
    assert merged.describe()[-1][1][:3] == (YCC_420, 75, 1)
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    first = _plan(ia, width=64)
    ia.plan_set_jpeg_scan_output(first, YCC_420, 75, optimize=True)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain((ia.MipxPlan * 2)(first, _plan(ia, w=first.out_w, h=first.out_h, width=32)), 2, C.byref(out)) == EINVAL


def test_new_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    f, g = L.mipx_op_rgb_to_jpeg_scan_optimized, L.mipx_op_jpegc_to_scan_optimized
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
    for layout in (YCC_420, YCC_444):                                   # 2^32 bytes or more, as today's calls
        assert f(1, 1, 1, 40000, 40000, layout, 75, W, None) == -2
        assert g(1, 1, 1, 40000, 40000, layout, W, None) == -2

    # mipx_submit for an optimised scan plan: data = one slot of the larger size
    p = _plan(ia, w=16, h=12, width=8)
    ia.plan_set_jpeg_scan_output(p, YCC_420, 75, optimize=True)
    src = np.zeros((12, 16, 3), np.uint8)
    dst = np.zeros(jpegeo_ref.jpeg_scan_opt_bytes(p.out_w, p.out_h, YCC_420), np.uint8)
    img = MipxImg(src.ctypes.data, 16, 12, 3, 0)
    t = C.c_uint64()
    out = MipxImg(dst.ctypes.data, 8, 6, 3, 24)
    assert L.mipx_submit(-1, C.byref(p), C.byref(img), None, C.byref(out), C.byref(t)) == EINVAL   # a stride
    if ia.device_count() == 0:
        out = MipxImg(dst.ctypes.data, 8, 6, 3, 0)
        assert L.mipx_submit(-1, C.byref(p), C.byref(img), None, C.byref(out), C.byref(t)) == -7   # only the engine is missing


def test_scan_slot_reads_both_kinds_of_slot():
    import imaginary_amd as ia
    w, h, layout = 17, 9, YCC_420
    coefs = jpegc_ref(picture("noise", w, h)[None], layout, 75)[0]
    want = jpegeo_ref.slot_ref(coefs, w, h, layout)
    slot = np.zeros(jpegeo_ref.jpeg_scan_opt_bytes(w, h, layout), np.uint8)
    slot[:16] = want.header().view(np.uint8)
    for k, tc in enumerate(jpegeo_ref.SLOT_TABLES):
        slot[16 + 272 * k:16 + 272 * (k + 1)] = jpegeo_ref.table_bytes(want.tables[tc])
    slot[1104:1104 + want.length] = np.frombuffer(want.scan, np.uint8)
    jpegeo_ref.check_slot(slot, want, "the reference's own slot")
    assert ia.scan_slot(slot) == (0, want.bits, want.scan)
    assert ia.scan_slot(slot, tables=True) == (0, want.bits, want.scan, want.tables)
    plain = jpege_ref.slot_ref(coefs, w, h, layout)
    assert want.length <= plain.length and want.tables != ia.codec.HUFFMAN_TABLES
    old = np.zeros(jpege_ref.jpeg_scan_bytes(w, h, layout), np.uint8)
    old[:16] = plain.header().view(np.uint8)
    old[16:16 + plain.length] = np.frombuffer(plain.scan, np.uint8)
    assert ia.scan_slot(old, tables=True) == (0, plain.bits, plain.scan, None)
    slot[4] = 1
    assert ia.scan_slot(slot, tables=True) == (1, want.bits, b"", None) and ia.scan_slot(slot) == (1, want.bits, b"")
