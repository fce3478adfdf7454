"""Grey (one-component) JPEGs without a device: tests/jpeggrey_ref.py against Pillow's libjpeg-turbo
(mode "L": JCS_GRAYSCALE) at full size and at every shrink-on-load scale, the host readers' opt-in
(`grey=True`), the slots and the model of the entropy decoder on them, the host writers byte for
byte against Pillow's files, the geometry struct, and the C ABI: the layout's value, the sizes, the
one rule of the setters (grey goes with 1 band, the three-component layouts with 3) and the calls
that do not take the layout."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

import jpeggrey_ref as R
from conftest import ROOT
from jpegc_ref import YCC_420, YCC_444
from jpeggrey_ref import YCC_GREY

PIL = pytest.importorskip("PIL.Image")

YCC_422 = 3
SIZES = [(1, 1), (2, 3), (8, 8), (9, 17), (16, 8), (33, 17), (131, 37)]
QUALITIES = (30, 75, 92, 100)
CSRC = os.path.join(ROOT, "imaginary_amd", "csrc")


def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


# ---------------------------------------------------------------- 1. the restatement is libjpeg-turbo's
def test_the_decode_restatement_is_libjpeg_turbos_at_every_scale():
    from imaginary_amd import codec
    ran = {1: 0, 2: 0, 4: 0, 8: 0}
    for w, h in SIZES:
        for quality in QUALITIES:
            for px in (R.noise(w, h), R.smooth(w, h)):
                buf = R.pillow_jpeg(px, quality)
                payload, layout = codec.decode_jpeg_coefs(buf, grey=True)
                assert layout == YCC_GREY and payload.dtype == np.uint8 and payload.shape == (R.jpegd_bytes(w, h),)
                assert not payload[128:384].any()                      # zeros behind Y's table
                want = codec.decode(buf)
                assert want.shape == (h, w, 1)
                assert np.array_equal(R.jpegd_grey_ref(payload, w, h), want), (w, h, quality)
                ran[1] += 1
                for shrink in (2, 4, 8):
                    want = codec.decode(buf, shrink)
                    s = codec.decode_scale(w, h, shrink)               # the scale draft really delivers
                    assert want.shape == (-(-h // s), -(-w // s), 1), (w, h, shrink, s, want.shape)
                    assert np.array_equal(R.jpegd_grey_ref(payload, w, h, s), want), (w, h, quality, shrink, s)
                    ran[s] += 1
    assert all(ran.values()), ran


def test_the_decode_restatement_takes_optimised_tables_and_restart_intervals():
    """A restart interval of a one-component scan counts blocks: the host decoder must count so too."""
    from imaginary_amd import codec
    for w, h in [(9, 17), (131, 37), (264, 64)]:
        for kw in (dict(optimize=True), dict(restart_marker_blocks=1), dict(restart_marker_blocks=8),
                   dict(restart_marker_rows=1)):
            buf = R.pillow_jpeg(R.noise(w, h), 75, **kw)
            if "restart_marker_rows" in kw:                            # one block row: ceil(w / 8) blocks
                at = buf.index(b"\xff\xdd")
                assert int.from_bytes(buf[at + 4:at + 6], "big") == -(-w // 8)
            payload, layout = codec.decode_jpeg_coefs(buf, grey=True)
            assert layout == YCC_GREY
            assert np.array_equal(R.jpegd_grey_ref(payload, w, h), codec.decode(buf)), (w, h, kw)


def test_the_encode_restatement_and_the_writers_are_libjpeg_turbos_byte_for_byte():
    from imaginary_amd import codec
    for w, h in SIZES:
        for quality in (1,) + QUALITIES:
            for px in (R.noise(w, h), R.smooth(w, h), np.zeros((h, w, 1), np.uint8), np.full((h, w, 1), 255, np.uint8)):
                coefs = R.jpegc_grey_ref(px, quality)[0]
                assert coefs.shape == (R.jpegc_bytes(w, h) // 2,)
                # Annex K tables
                assert codec.encode_jpeg_coefs(coefs, w, h, YCC_GREY, quality) == R.pillow_jpeg(px, quality), (w, h, quality)
                # the image's own tables: whole files, the header included
                counts = codec.jpeg_symbol_counts(coefs, w, h, YCC_GREY)
                assert sorted(counts) == [0x00, 0x10]
                tables = {tc: codec.jpeg_optimal_table(f) for tc, f in counts.items()}
                want = R.pillow_jpeg(px, quality, optimize=True)
                assert codec.encode_jpeg_coefs(coefs, w, h, YCC_GREY, quality, tables=tables) == want, (w, h, quality)
                assert codec.encode_jpeg_coefs(coefs, w, h, YCC_GREY, quality, tables="optimal") == want


def test_the_header_is_libjpegs_for_jcs_grayscale():
    from imaginary_amd import codec
    hdr = codec.jpeg_header(37, 29, YCC_GREY, 75)
    markers, p = [], 2
    while p < len(hdr):
        markers.append((hdr[p + 1], hdr[p + 4:p + 2 + int.from_bytes(hdr[p + 2:p + 4], "big")]))
        p += 2 + int.from_bytes(hdr[p + 2:p + 4], "big")
    assert [m for m, _ in markers] == [0xE0, 0xDB, 0xC0, 0xC4, 0xC4, 0xDA]    # JFIF, one DQT, SOF0, DC 0, AC 0, SOS
    assert markers[1][1][0] == 0 and len(markers[1][1]) == 65
    assert markers[2][1] == bytes([8, 0, 29, 0, 37, 1, 1, 0x11, 0])           # one component: id 1, 1 x 1, table 0
    assert [b[0] for m, b in markers if m == 0xC4] == [0x00, 0x10]
    assert markers[5][1] == bytes([1, 1, 0x00, 0, 63, 0])
    scan = codec.jpeg_scan(R.jpegc_grey_ref(R.noise(37, 29), 75)[0], 37, 29, YCC_GREY)
    assert codec.jpeg_from_scan(scan, 37, 29, YCC_GREY, 75) == R.pillow_jpeg(R.noise(37, 29), 75)
    assert codec.jpeg_scan_bits(R.jpegc_grey_ref(R.noise(37, 29), 75)[0], 37, 29, YCC_GREY)[0] == scan


def test_the_sampling_factors_a_grey_file_declares_change_nothing_but_the_header():
    """libjpeg writes 2 x 2 for the one component when its caller asked for 4:2:0, as codec.encode
    does below Q 90: the scan is not interleaved, so blocks, payload and scan are the same."""
    from imaginary_amd import codec
    for w, h in [(9, 17), (33, 17), (131, 37)]:
        px = R.noise(w, h)
        plain = R.pillow_jpeg(px, 75)
        declared = R.pillow_jpeg(px, 75, subsampling=2)
        assert declared == codec.encode(px, "jpeg", 75) and declared != plain
        assert len(declared) == len(plain) and [i for i in range(len(plain)) if plain[i] != declared[i]] == [
            declared.index(b"\xff\xc0") + 11]                                  # the SOF's sampling byte alone
        assert declared[declared.index(b"\xff\xc0") + 11] == 0x22
        a, b = codec.decode_jpeg_coefs(plain, grey=True), codec.decode_jpeg_coefs(declared, grey=True)
        assert a[1] == b[1] == YCC_GREY and np.array_equal(a[0], b[0])
        assert codec.decode_jpeg_coefs(declared) is None
        coefs = R.jpegc_grey_ref(px, 75)[0]
        assert codec.encode_jpeg_coefs(coefs, w, h, YCC_GREY, 75, grey_sampling=2) == declared
        assert codec.encode_jpeg_coefs(coefs, w, h, YCC_GREY, 75, grey_sampling=1) == plain


# ---------------------------------------------------------------- 2. the host reader
def test_the_reader_takes_grey_only_when_asked_and_nothing_else_new():
    from imaginary_amd import codec
    grey = R.pillow_jpeg(R.noise(32, 24), 85)
    assert codec.decode_jpeg_coefs(grey) is None and codec.decode_jpeg_coefs(grey, grey=False) is None
    assert codec.decode_jpeg_coefs(grey, h2v1=True) is None
    assert codec.decode_jpeg_coefs(grey, grey=True)[1] == YCC_GREY
    assert codec.decode_jpeg_coefs(grey, h2v1=True, grey=True)[1] == YCC_GREY
    assert codec.decode_ycc(grey) is None
    for kw in (dict(), dict(restart=True)):
        assert codec.jpeg_huff_slot(grey, **kw) is None and codec.jpeg_huff_slot(grey, h2v1=True, **kw) is None
        assert codec.jpeg_huff_slot(grey, grey=True, **kw)[1] == YCC_GREY
    b = io.BytesIO()
    PIL.fromarray(R.noise(32, 24)[:, :, 0], "L").save(b, "JPEG", quality=85, progressive=True)
    assert codec.decode_jpeg_coefs(b.getvalue(), grey=True) is None
    assert codec.decode_jpeg_coefs(grey[:len(grey) // 2], grey=True) is None        # truncated
    rgb = PIL.fromarray(np.repeat(R.noise(32, 24), 3, axis=2))
    for sub, layout in ((0, YCC_444), (2, YCC_420)):       # what it took before, it takes unchanged
        b = io.BytesIO()
        rgb.save(b, "JPEG", quality=85, subsampling=sub)
        a, g = codec.decode_jpeg_coefs(b.getvalue()), codec.decode_jpeg_coefs(b.getvalue(), grey=True)
        assert a[1] == g[1] == layout and np.array_equal(a[0], g[0])
    b = io.BytesIO()
    rgb.save(b, "JPEG", quality=85, subsampling=1)
    assert codec.decode_jpeg_coefs(b.getvalue(), grey=True) is None                 # 4:2:2 keeps its own option


def test_jpeg_huff_slot_lays_the_grey_slot_out_as_documented_and_the_model_decodes_it():
    import jpegh_ref
    from imaginary_amd import codec
    for w, h in [(9, 17), (131, 37), (264, 64)]:
        blocks = R.scan_blocks(w, h)
        for kw, ri in ((dict(), 0), (dict(optimize=True), 0), (dict(restart_marker_blocks=1), 1),
                       (dict(restart_marker_blocks=8), 8), (dict(restart_marker_rows=1), -(-w // 8))):
            buf = R.pillow_jpeg(R.noise(w, h), 75, **kw)
            fw, fh, samp, qt, sel, dht, dri, scan = jpegh_ref.file_tables(buf)
            assert (fw, fh, dri) == (w, h, ri) and samp == [(1, 1)] and sel == [0, 0] and sorted(dht) == [0x00, 0x10]
            assert codec.jpeg_huff_slot(buf, restart=True) is None              # opt-in
            got = codec.jpeg_huff_slot(buf, restart=True, grey=True)
            assert got is not None and got[1] == YCC_GREY
            slot = got[0]
            assert slot.dtype == np.uint8 and slot.shape == (R.jpegh_bytes(w, h),) == (1504 + 128 * blocks,)
            p = buf.index(b"\xff\xda")
            p += 2 + int.from_bytes(buf[p + 2:p + 4], "big")
            whole = buf[p:-2]                                                   # restart markers included
            length, q, selectors, tables = jpegh_ref.parse_slot(slot)
            assert length == len(whole) and slot[1504:1504 + length].tobytes() == whole
            assert int(slot[4:8].view("<u4")[0]) == ri and not slot[8:16].any() and not slot[1504 + length:].any()
            assert q[0].tolist() == qt[0] and not q[1:].any()                   # Y's table, zeros behind it
            assert selectors == [0, 0, 0, 0, 0, 0]                              # bytes 400 and 403 are Y's
            for i, key in enumerate(jpegh_ref.TABLE_KEYS):                      # DC 0, DC 1, AC 0, AC 1
                if key in dht:
                    assert tables[i] == (dht[key][0], dht[key][1] + bytes(256 - len(dht[key][1])))
                else:
                    assert tables[i] == (bytes(16), bytes(256))                 # a table the file does not define
            plain = codec.jpeg_huff_slot(buf, grey=True)
            if ri == 0:
                assert np.array_equal(plain[0], slot) and plain[1] == YCC_GREY
            else:
                assert plain is None                                            # restart files stay opt-in of their own
            # the model of the decoder on the slot gives the host decoder's payload
            status, payload = R.decode_slot(slot, w, h)
            assert status == R.OK and np.array_equal(payload, codec.decode_jpeg_coefs(buf, grey=True)[0]), (w, h, kw)


def test_the_model_takes_table_1_and_reports_damage():
    """A file may define table 1 and use it: the slot then names it in bytes 400 and 403."""
    import jpegh_ref
    from imaginary_amd import codec
    w, h = 131, 37
    buf = R.pillow_jpeg(R.noise(w, h), 75, optimize=True)
    slot, _ = codec.jpeg_huff_slot(buf, grey=True)
    want = codec.decode_jpeg_coefs(buf, grey=True)[0]
    moved = slot.copy()                                   # DC 0 -> DC 1, AC 0 -> AC 1, and the selectors say so
    moved[416 + 272:416 + 2 * 272], moved[416 + 3 * 272:416 + 4 * 272] = slot[416:416 + 272], slot[416 + 2 * 272:416 + 3 * 272]
    moved[416:416 + 272] = 0
    moved[416 + 2 * 272:416 + 3 * 272] = 0
    moved[400], moved[403] = 1, 1
    assert jpegh_ref.parse_slot(moved)[2] == [1, 0, 0, 1, 0, 0]
    status, payload = R.decode_slot(moved, w, h)
    assert status == R.OK and np.array_equal(payload, want)
    ignored = slot.copy()
    ignored[401], ignored[402], ignored[404], ignored[405] = 7, 1, 200, 3          # the other four bytes
    status, payload = R.decode_slot(ignored, w, h)
    assert status == R.OK and np.array_equal(payload, want)
    for at, v in ((400, 2), (403, 5)):
        bad = slot.copy()
        bad[at] = v
        assert R.decode_slot(bad, w, h) == (R.BAD, None)
    cut = slot.copy()
    cut[:4] = np.frombuffer((int(slot[:4].view("<u4")[0]) // 2).to_bytes(4, "little"), np.uint8)
    assert R.decode_slot(cut, w, h)[0] == R.BAD


# ---------------------------------------------------------------- 3. the geometry struct
@pytest.fixture(scope="module")
def geom_lines(tmp_path_factory):
    out = tmp_path_factory.mktemp("jpeg_geom_grey") / "jpeg_geom_grey_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "jpeg_geom_grey_host.cpp"), "-o", str(out)], check=True)
    return subprocess.run([str(out)], capture_output=True, text=True, check=True).stdout.splitlines()


def test_the_struct_follows_the_one_component_rule(geom_lines):
    geom = [l for l in geom_lines if l.startswith("geom ")]
    assert len(geom) == 40 * 40 + 4 + 2
    seen = set()
    for l in geom:
        head, body = l.split(" : ")
        w, h = (int(v) for v in head.split()[1:])
        parts = [tuple(int(v) for v in p.split()) for p in body.split(" | ")]
        if w <= 0 or h <= 0:
            assert not any(parts[0]), l
            continue
        assert parts[0] == R.geom(w, h), (l, R.geom(w, h))
        assert parts[1:] == [R.planes(w, h, s) for s in (1, 2, 4, 8)], l
        seen.add((w, h))
    assert (1, 1) in seen and (9, 17) in seen and (3840, 2160) in seen and (65535, 65535) in seen


def test_the_predicates_and_the_workspace_maxima(geom_lines):
    layouts = {int(l.split()[1]): [int(v) for v in l.split(" : ")[1].split()] for l in geom_lines if l.startswith("layout ")}
    # three components: input, output; coefficient input, coefficient output; bands
    assert layouts[0] == [1, 1, 1, 1, 3] and layouts[1] == [1, 1, 1, 1, 3] and layouts[3] == [1, 0, 1, 0, 3]
    assert layouts[6] == [0, 0, 1, 1, 1]
    for none in (-1, 2, 4, 5, 7, 1 << 20):
        assert layouts[none][:4] == [0, 0, 0, 0]
    most = [l for l in geom_lines if l.startswith("max ")]
    assert len(most) == 40 * 40
    for l in most:
        own, out, inp = ([int(v) for v in p.split()] for p in l.split(" : ")[1].split(" | "))
        assert own[0] <= out[0] and own[1] <= out[1] and own[0] <= inp[0] and own[1] <= inp[1], l


# ---------------------------------------------------------------- 4. the ABI
def test_the_layout_is_6_and_the_abi_version_stays():
    import imaginary_amd as ia
    from imaginary_amd import _abi, codec
    assert _abi.YCC_GREY == codec.YCC_GREY == ia.YCC_GREY == YCC_GREY == 6
    assert _abi.lib.mipx_abi_version() == 6
    assert (ia.YCC_444, ia.YCC_420, ia.YCC_422) == (0, 1, 3)


def test_the_sizes():
    import imaginary_amd as ia
    for w in range(1, 41):
        for h in range(1, 41):
            blocks = -(-w // 8) * -(-h // 8)
            assert ia.ycc_bytes(w, h, YCC_GREY) == w * h
            assert ia.jpegc_bytes(w, h, YCC_GREY) == R.jpegc_bytes(w, h) == 128 * blocks
            assert ia.jpegd_bytes(w, h, YCC_GREY) == R.jpegd_bytes(w, h) == 384 + 128 * blocks
            assert ia.jpegh_bytes(w, h, YCC_GREY) == R.jpegh_bytes(w, h) == 1504 + 128 * blocks
            assert ia.jpeg_scan_bytes(w, h, YCC_GREY) == 16 + 128 * blocks
            assert ia.jpeg_scan_opt_bytes(w, h, YCC_GREY) == 1104 + 128 * blocks
    for fn in (ia.ycc_bytes, ia.jpegc_bytes, ia.jpegd_bytes, ia.jpegh_bytes, ia.jpeg_scan_bytes, ia.jpeg_scan_opt_bytes):
        assert fn(0, 8, YCC_GREY) == 0 and fn(8, -1, YCC_GREY) == 0
        for none in (2, 4, 5, 7, -1, 1 << 20):
            assert fn(8, 8, none) == 0


def test_grey_goes_with_one_band_and_the_other_layouts_with_three():
    import imaginary_amd as ia
    L = ia.lib
    W, H = 131, 37
    # coefficient input
    d = ia.plan_set_jpegd_input(_plan(ia, W, H, 1, width=60), YCC_GREY)
    assert d.describe()[0] == ("jpegd", (YCC_GREY, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (W, H, 1))
    assert (d.in_bands, d.out_bands) == (1, 1) and L.mipx_workspace_bytes(C.byref(d), 2) > 0      # the plan validates
    for s in (2, 4, 8):
        ow, oh = -(-W // s), -(-H // s)
        ds = ia.plan_set_jpegd_input_scaled(_plan(ia, ow, oh, 1, width=max(ow // 2, 1)), YCC_GREY, s, W, H)
        assert ds.describe()[0] == ("jpegd", (YCC_GREY, s, W, H, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 1))
        assert L.mipx_workspace_bytes(C.byref(ds), 1) > 0
    # coefficient output, of a 1-band plan and of a colour plan that ends in B_W
    c = ia.plan_set_jpegc_output(_plan(ia, W, H, 1, width=60), YCC_GREY, 75)
    assert c.describe()[-1] == ("jpegc", (YCC_GREY, 75, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (c.out_w, c.out_h, 1))
    assert L.mipx_workspace_bytes(C.byref(c), 2) > 0
    bw = _plan(ia, W, H, 3, width=60, interpretation=ia._abi.INTERPRETATION_BW)
    assert bw.out_bands == 1 and [s[0] for s in bw.describe()][-1] == "bw"
    ia.plan_set_jpegc_output(bw, YCC_GREY, 90)
    assert [s[0] for s in bw.describe()][-2:] == ["bw", "jpegc"] and L.mipx_workspace_bytes(C.byref(bw), 1) > 0
    # coefficients in, coefficients out, nothing between
    both = ia.plan_set_jpegd_input(ia.plan_set_jpegc_output(_plan(ia, W, H, 1), YCC_GREY, 75), YCC_GREY)
    assert [s[0] for s in both.describe()] == ["jpegd", "jpegc"] and L.mipx_workspace_bytes(C.byref(both), 1) > 0
    # the scan steps: the same steps with another op
    hp = ia.plan_set_jpegh_input(_plan(ia, W, H, 1, width=60), YCC_GREY)
    assert hp.describe() == [("jpegh",) + d.describe()[0][1:]] + d.describe()[1:]
    assert L.mipx_workspace_bytes(C.byref(hp), 2) > 0
    hs = ia.plan_set_jpegh_input_scaled(_plan(ia, -(-W // 4), -(-H // 4), 1), YCC_GREY, 4, W, H)
    assert hs.describe()[0] == ("jpegh", (YCC_GREY, 4, W, H, 0, 0, 0, 0), (0.0,) * 4, (-(-W // 4), -(-H // 4), 1))
    for optimize in (False, True):
        e = ia.plan_set_jpeg_scan_output(_plan(ia, W, H, 1, width=60), YCC_GREY, 75, optimize)
        assert e.describe()[-1] == ("jpege", (YCC_GREY, 75, int(optimize), 0, 0, 0, 0, 0), (0.0,) * 4, (e.out_w, e.out_h, 1))
        assert L.mipx_workspace_bytes(C.byref(e), 2) > 0
    through = ia.plan_set_jpegh_input(ia.plan_set_jpeg_scan_output(_plan(ia, W, H, 1), YCC_GREY, 75, True), YCC_GREY)
    assert [s[0] for s in through.describe()] == ["jpegh", "jpege"] and L.mipx_workspace_bytes(C.byref(through), 1) > 0
    # every other pairing is refused, and a refusal leaves the plan's bytes untouched
    setters = (lambda q, l: L.mipx_plan_set_jpegd_input(C.byref(q), l),
               lambda q, l: L.mipx_plan_set_jpegd_input_scaled(C.byref(q), l, 1, W, H),
               lambda q, l: L.mipx_plan_set_jpegc_output(C.byref(q), l, 75),
               lambda q, l: L.mipx_plan_set_jpegh_input(C.byref(q), l),
               lambda q, l: L.mipx_plan_set_jpegh_input_scaled(C.byref(q), l, 1, W, H),
               lambda q, l: L.mipx_plan_set_jpeg_scan_output(C.byref(q), l, 75),
               lambda q, l: L.mipx_plan_set_jpeg_scan_output_optimized(C.byref(q), l, 75))
    for bands, layouts in ((3, (YCC_GREY,)), (1, (YCC_444, YCC_420, YCC_422)), (2, (YCC_GREY, YCC_444)),
                           (4, (YCC_GREY, YCC_420))):
        for layout in layouts:
            for setter in setters:
                q = _plan(ia, W, H, bands)
                untouched = bytes(q)
                assert setter(q, layout) == -1, (bands, layout)
                assert bytes(q) == untouched
    for none in (2, 4, 5, 7, -1, 1 << 20):
        for setter in setters:
            q = _plan(ia, W, H, 1)
            untouched = bytes(q)
            assert setter(q, none) == -1 and bytes(q) == untouched


def test_the_calls_that_do_not_take_grey_refuse_it():
    """Planes and the round trip are three-component: on 1 band and on 3."""
    import imaginary_amd as ia
    L, big = ia.lib, 1 << 40
    for bands in (1, 3):
        p = _plan(ia, 64, 48, bands)
        untouched = bytes(p)
        assert L.mipx_plan_set_ycc_input(C.byref(p), YCC_GREY) == -1
        assert L.mipx_plan_add_jpeg_roundtrip(C.byref(p), YCC_GREY, 75, 1) == -1
        assert L.mipx_plan_add_jpeg_roundtrip(C.byref(p), YCC_GREY, 75, 2) == -1
        assert bytes(p) == untouched
    assert L.mipx_op_ycc_to_rgb(1, 1, 1, 64, 48, YCC_GREY, None) == -1
    assert L.mipx_op_jpeg_roundtrip(1, 1, 1, 64, 48, YCC_GREY, 75, 1, 1, big, None) == -1


def _hand_plan(ia, ops, layout, bands, w=16, h=12):
    """A plan of flips and coefficient steps written by hand (geometry consistent)."""
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, bands
    p.out_w, p.out_h, p.out_bands = w, h, bands
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        if op in (15, 16, 17, 18, 19, 20):
            p.steps[i].a[0] = layout
        if op in (16, 18, 19):
            p.steps[i].a[1] = 75
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, bands
    return p


def test_the_plan_validation_follows_the_same_rule():
    """Plans are ABI data: the re-derivation before any device work applies the pairing too."""
    import imaginary_amd as ia
    L = ia.lib
    for ok in (_hand_plan(ia, [17], YCC_GREY, 1), _hand_plan(ia, [17, 2], YCC_GREY, 1), _hand_plan(ia, [2, 16], YCC_GREY, 1),
               _hand_plan(ia, [17, 16], YCC_GREY, 1), _hand_plan(ia, [17, 16], YCC_420, 3), _hand_plan(ia, [20], YCC_GREY, 1),
               _hand_plan(ia, [2, 19], YCC_GREY, 1), _hand_plan(ia, [20, 19], YCC_GREY, 1)):
        assert L.mipx_workspace_bytes(C.byref(ok), 1) > 0
    bad = [_hand_plan(ia, [17], YCC_GREY, 3), _hand_plan(ia, [16], YCC_GREY, 3), _hand_plan(ia, [17], YCC_420, 1),
           _hand_plan(ia, [16], YCC_444, 1), _hand_plan(ia, [17], YCC_GREY, 2), _hand_plan(ia, [2, 17], YCC_GREY, 1),
           _hand_plan(ia, [16, 2], YCC_GREY, 1)]
    bad += [_hand_plan(ia, [op], YCC_GREY, bands) for op in (15, 18) for bands in (1, 3)]
    bad += [_hand_plan(ia, [op], YCC_GREY, 3) for op in (19, 20)] + [_hand_plan(ia, [op], YCC_420, 1) for op in (19, 20)]
    lying = _hand_plan(ia, [17], YCC_GREY, 1)             # a grey step that says it makes 3 bands
    lying.steps[0].out_bands = lying.out_bands = 3
    for p in bad + [lying]:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1


def test_the_chain_puts_the_steps_where_it_puts_the_colour_ones():
    import imaginary_amd as ia
    s0 = _plan(ia, 128, 96, 1, width=64)
    s1 = _plan(ia, s0.out_w, s0.out_h, 1, width=32)
    d0 = ia.plan_set_jpegd_input(_plan(ia, 128, 96, 1, width=64), YCC_GREY)
    c1 = ia.plan_set_jpegc_output(_plan(ia, s0.out_w, s0.out_h, 1, width=32), YCC_GREY, 75)
    merged = ia.plan_chain([d0, c1])
    assert [s[0] for s in merged.describe()] == ["jpegd", "reduce", "reduce", "jpegc"]
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    out = ia.MipxPlan()
    d1 = ia.plan_set_jpegd_input(_plan(ia, s0.out_w, s0.out_h, 1, width=32), YCC_GREY)
    assert ia.lib.mipx_plan_chain((ia.MipxPlan * 2)(s0, d1), 2, C.byref(out)) == -1     # coefficient input after stage 0
    c0 = ia.plan_set_jpegc_output(_plan(ia, 128, 96, 1, width=64), YCC_GREY, 75)
    assert ia.lib.mipx_plan_chain((ia.MipxPlan * 2)(c0, s1), 2, C.byref(out)) == -1     # coefficient output before the last


def test_the_op_calls_take_it_as_far_as_their_argument_checks():
    import imaginary_amd as ia
    L, big = ia.lib, 1 << 40
    # a layout the call takes gets past the layout check to the next one: the missing workspace
    assert L.mipx_op_jpegd_to_rgb(1, 1, 2, 37, 29, YCC_GREY, 1, 0, None) == -1
    assert "workspace" in L.mipx_last_error().decode()
    assert L.mipx_op_jpegd_to_rgb_scaled(1, 1, 2, 37, 29, YCC_GREY, 4, 1, 0, None) == -1
    assert "workspace" in L.mipx_last_error().decode()
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 40000, 40000, YCC_GREY, 1, big, None) == -2
    assert L.mipx_op_jpegh_to_rgb(1, 1, 4, 1, 37, 29, YCC_GREY, 16, 0, None) == -1
    assert "workspace" in L.mipx_last_error().decode()
    assert L.mipx_op_jpegh_to_jpegd(1, 1, 4, 1, 37, 29, YCC_GREY, 16, 0, None) == -1
    assert "workspace" in L.mipx_last_error().decode()
    for call in (lambda: L.mipx_op_rgb_to_jpeg_scan(1, 1, 1, 64, 48, YCC_GREY, 75, 17, None),        # ... the alignment
                 lambda: L.mipx_op_rgb_to_jpeg_scan_optimized(1, 1, 1, 64, 48, YCC_GREY, 75, 17, None),
                 lambda: L.mipx_op_jpegc_to_scan(1, 1, 1, 64, 48, YCC_GREY, 17, None),
                 lambda: L.mipx_op_jpegc_to_scan_optimized(1, 1, 1, 64, 48, YCC_GREY, 17, None),
                 lambda: L.mipx_op_jpegc_to_scan_packed(1, 1, 1, 64, 48, YCC_GREY, 17, None, 0, 8),
                 lambda: L.mipx_op_rgb_to_jpeg_scan_packed(1, 1, 1, 64, 48, YCC_GREY, 75, 17, None, 1, 8)):
        assert call() == -1 and "aligned" in L.mipx_last_error().decode()
    # the entropy decoder's and coder's workspaces, sized without the layout, are what grey is asked for
    for n, w, h in [(1, 1, 1), (3, 37, 29)]:
        for op, p0 in ((19, 0.0), (19, 1.0), (20, 0.0)):
            assert L.mipx_op_workspace_bytes(op, n, w, h, 1, p0, 0.0) == L.mipx_op_workspace_bytes(op, n, w, h, 3, p0, 0.0) > 0
    assert L.mipx_op_rgb_to_jpegc(1, 1, 1, 64, 48, YCC_GREY, 0, None) == -1            # ... the quality
    assert L.mipx_op_rgb_to_jpegc(None, 1, 1, 64, 48, YCC_GREY, 75, None) == -1
    # the workspace a 3-band call is told to bring stays what a grey call is asked for
    for n, w, h in [(1, 1, 1), (3, 37, 29), (64, 3840, 2160)]:
        assert L.mipx_op_workspace_bytes(17, n, w, h, 1, 0.0, 0.0) == L.mipx_op_workspace_bytes(17, n, w, h, 3, 0.0, 0.0) > 0


def test_the_wrappers_check_shapes_without_a_device():
    import imaginary_amd as ia
    with pytest.raises(ValueError):
        ia.rgb_to_jpegc(np.zeros((8, 8, 3), np.uint8), YCC_GREY, 75)       # 3 bands in the 1-band layout
    with pytest.raises(ValueError):
        ia.rgb_to_jpegc(np.zeros((8, 8, 1), np.uint8), YCC_420, 75)
    with pytest.raises(ValueError):
        ia.jpegd_to_rgb(np.zeros(R.jpegd_bytes(8, 8) + 1, np.uint8), 8, 8, YCC_GREY)
