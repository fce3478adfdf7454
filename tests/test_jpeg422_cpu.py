"""4:2:2 (h2v1) JPEG input without a device: tests/jpeg422_ref.py against Pillow's libjpeg-turbo at
full size and at every shrink-on-load scale, the host readers' opt-in (`h2v1=True`), and the C ABI:
the layout's value, the sizes, the input setters that take it and the output calls that do not."""
import ctypes as C
import io

import numpy as np
import pytest

import jpeg422_ref as R
import jpegh_ref
from jpeg422_ref import YCC_422
from jpegc_ref import YCC_420, YCC_444

PIL = pytest.importorskip("PIL.Image")

SIZES = [(1, 1), (2, 3), (4, 5), (8, 16), (16, 8), (17, 9), (33, 17), (131, 37)]
ABI_SIZES = [(1, 1), (8, 16), (17, 9), (37, 29), (3840, 2160)]


def _plan(ia, w=128, h=96, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


# ---------------------------------------------------------------- 1. the restatement is libjpeg-turbo's
def test_the_restatement_is_libjpeg_turbos_at_every_scale():
    from imaginary_amd import codec
    ran = {1: 0, 2: 0, 4: 0, 8: 0}
    for w, h in SIZES:
        for quality in (30, 75, 92):
            for px in (R.noise(w, h), R.smooth(w, h)):
                buf = R.pillow_jpeg(px, quality)
                payload, layout = codec.decode_jpeg_coefs(buf, h2v1=True)
                assert layout == YCC_422 and payload.shape == (R.jpegd_bytes(w, h),)
                want = np.asarray(PIL.open(io.BytesIO(buf)).convert("RGB"))
                assert np.array_equal(R.jpegd422_ref(payload, w, h), want), (w, h, quality)
                ran[1] += 1
                for shrink in (2, 4, 8):
                    im = PIL.open(io.BytesIO(buf))
                    im.draft("RGB", (-(-w // shrink), -(-h // shrink)))
                    want = np.asarray(im.convert("RGB"))
                    s = codec.decode_scale(w, h, shrink)      # the scale draft really delivers
                    assert want.shape == (-(-h // s), -(-w // s), 3), (w, h, shrink, s, want.shape)
                    assert np.array_equal(R.jpegd422_ref(payload, w, h, s), want), (w, h, quality, shrink, s)
                    ran[s] += 1
    assert all(ran.values()), ran                              # 131 x 37 and 33 x 17 between them deliver every scale


def test_the_upsample_known_answers():
    c = np.array([[0, 100, 200]], np.uint8)
    # (3 a + b + 1) >> 2 on even x, (3 a + b + 2) >> 2 on odd x, the neighbours clamped
    assert R.upsample_422(c, 6).tolist() == [[0, 25, 75, 125, 175, 200]]
    assert R.upsample_422(c, 5).tolist() == [[0, 25, 75, 125, 175]]
    assert R.upsample_422(c, 6, fancy=False).tolist() == [[0, 0, 100, 100, 200, 200]]
    assert R.upsample_422(c[:, :2], 4).tolist() == [[0, 0, 100, 100]]          # cw <= 2: replication
    assert R.upsample_422(np.array([[3, 4, 4]], np.uint8), 6).tolist() == [[3, 3, 4, 4, 4, 4]]   # the two biases


# ---------------------------------------------------------------- 2. the host readers
def test_decode_jpeg_coefs_places_the_blocks_as_the_model_does():
    from imaginary_amd import codec
    for w, h in [(8, 16), (17, 9), (33, 17), (131, 37)]:
        for optimize in (False, True):
            buf = R.pillow_jpeg(R.noise(w, h), 75, optimize)
            payload, layout = codec.decode_jpeg_coefs(buf, h2v1=True)
            slot, l2 = codec.jpeg_huff_slot(buf, h2v1=True)
            assert layout == l2 == YCC_422
            blocks = R.scan_coefs(slot, w, h)          # the model's own walk of the scan, 4 blocks per MCU
            assert blocks is not None and blocks.shape == (R.scan_blocks(w, h), 64)
            tables = payload[:384].view("<u2").reshape(3, 64)
            assert np.array_equal(R.payload_from_blocks(tables, blocks, w, h), payload), (w, h, optimize)


def test_jpeg_huff_slot_lays_the_slot_out_as_documented():
    from imaginary_amd import codec
    for w, h in [(8, 16), (17, 9), (131, 37)]:
        for kw, ri in ((dict(), 0), (dict(restart_marker_blocks=3), 3), (dict(restart_marker_rows=1), -(-w // 16))):
            buf = R.pillow_jpeg(R.noise(w, h), 75, **kw)
            fw, fh, samp, qt, sel, dht, dri, scan = jpegh_ref.file_tables(buf)
            assert (fw, fh, dri) == (w, h, ri) and samp == [(2, 1), (1, 1), (1, 1)]
            got = codec.jpeg_huff_slot(buf, restart=True, h2v1=True)
            assert got is not None and got[1] == YCC_422
            slot = got[0]
            assert slot.dtype == np.uint8 and slot.shape == (R.jpegh_bytes(w, h),)
            p = buf.index(b"\xff\xda")
            p += 2 + int.from_bytes(buf[p + 2:p + 4], "big")
            whole = buf[p:-2]                              # restart markers included
            length, q, selectors, tables = jpegh_ref.parse_slot(slot)
            assert length == len(whole) and slot[1504:1504 + length].tobytes() == whole
            assert int(slot[4:8].view("<u4")[0]) == ri and not slot[8:16].any() and not slot[1504 + length:].any()
            assert q.tolist() == qt and selectors == sel
            for i, key in enumerate(jpegh_ref.TABLE_KEYS):
                assert tables[i] == (dht[key][0], dht[key][1] + bytes(256 - len(dht[key][1])))
            plain = codec.jpeg_huff_slot(buf, h2v1=True)
            if ri == 0:
                assert np.array_equal(plain[0], slot) and plain[1] == YCC_422
            else:
                assert plain is None                       # restart files stay opt-in of their own


def test_the_readers_take_422_only_when_asked_and_nothing_else_new():
    from imaginary_amd import codec
    rgb = PIL.fromarray(R.noise(32, 24))

    def save(**kw):
        b = io.BytesIO()
        rgb.save(b, "JPEG", quality=85, **kw)
        return b.getvalue()

    readers = (lambda b, **kw: codec.decode_jpeg_coefs(b, **kw), lambda b, **kw: codec.jpeg_huff_slot(b, **kw),
               lambda b, **kw: codec.jpeg_huff_slot(b, restart=True, **kw))
    f422 = save(subsampling=1)
    for read in readers:
        assert read(f422) is None and read(f422, h2v1=False) is None
        assert read(f422, h2v1=True)[1] == YCC_422
        assert read(save(subsampling=1, progressive=True), h2v1=True) is None
        for sub, layout in ((0, YCC_444), (2, YCC_420)):   # what they took before, they take unchanged
            a, b = read(save(subsampling=sub)), read(save(subsampling=sub), h2v1=True)
            assert a[1] == b[1] == layout and np.array_equal(a[0], b[0])
    assert codec.decode_ycc(f422) is None
    try:
        f440 = save(subsampling="4:4:0")
    except (TypeError, ValueError, KeyError, OSError):
        f440 = None
    if f440 is not None and jpegh_ref.file_tables(f440)[2] == [(1, 2), (1, 1), (1, 1)]:
        for read in readers:
            assert read(f440, h2v1=True) is None


# ---------------------------------------------------------------- 3. the ABI
def test_the_layout_is_3_and_the_abi_version_stays():
    import imaginary_amd as ia
    from imaginary_amd import _abi, codec
    assert _abi.YCC_422 == codec.YCC_422 == ia.YCC_422 == YCC_422 == 3
    assert _abi.lib.mipx_abi_version() == 6
    assert (ia.YCC_444, ia.YCC_420) == (0, 1)


def test_the_sizes():
    import imaginary_amd as ia
    for w, h in ABI_SIZES:
        assert ia.ycc_bytes(w, h, YCC_422) == R.ycc_bytes(w, h) == w * h + 2 * ((w + 1) // 2) * h
        assert ia.jpegc_bytes(w, h, YCC_422) == R.jpegc_bytes(w, h)
        assert ia.jpegd_bytes(w, h, YCC_422) == R.jpegd_bytes(w, h) == 384 + R.jpegc_bytes(w, h)
        assert ia.jpegh_bytes(w, h, YCC_422) == R.jpegh_bytes(w, h) == 1504 + R.jpegc_bytes(w, h)
        # an output slot is never 4:2:2
        assert ia.jpeg_scan_bytes(w, h, YCC_422) == 0 and ia.jpeg_scan_opt_bytes(w, h, YCC_422) == 0
        assert ia.jpeg_scan_bytes(w, h, YCC_420) > 0 and ia.jpeg_scan_opt_bytes(w, h, YCC_444) > 0
    assert ia.jpegc_bytes(17, 9, YCC_422) == 128 * (3 * 2 + 2 * 2 * 2)
    assert ia.jpegc_bytes(8, 16, YCC_422) == 128 * (2 + 2 * 2)
    for fn in (ia.ycc_bytes, ia.jpegc_bytes, ia.jpegd_bytes, ia.jpegh_bytes):
        assert fn(0, 8, YCC_422) == 0 and fn(8, -1, YCC_422) == 0 and fn(8, 8, 2) == 0 and fn(8, 8, 4) == 0


def test_the_decoders_workspace_holds_a_422_scan():
    """8 x 16 and 5 x 32 have 8 and 16 blocks in 4:2:2 where the other layouts have 6 and 12: the
    workspace, sized without the layout, must hold a DC difference per block of those."""
    import imaginary_amd as ia
    for w, h, blocks in [(8, 16, 8), (5, 32, 16)]:
        assert R.scan_blocks(w, h) == blocks
        assert blocks > max(jpegh_ref.scan_blocks(w, h, YCC_444), jpegh_ref.scan_blocks(w, h, YCC_420))
        for n in (1, 3, 64):
            got = ia.lib.mipx_op_workspace_bytes(20, n, w, h, 3, 0.0, 0.0)
            assert got >= R.workspace_bytes(n, w, h) >= jpegh_ref.workspace_bytes(n, w, h), (n, w, h)
    # 64 images of 5 x 32: 16 blocks need 4096 bytes of differences where 12 needed 3072
    assert R.workspace_bytes(64, 5, 32) == jpegh_ref.workspace_bytes(64, 5, 32) + 1024
    for w, h in [(1, 1), (17, 9), (37, 29), (3840, 2160)]:       # elsewhere nothing moved
        assert R.workspace_bytes(3, w, h) == jpegh_ref.workspace_bytes(3, w, h)
        assert ia.lib.mipx_op_workspace_bytes(20, 3, w, h, 3, 0.0, 0.0) == jpegh_ref.workspace_bytes(3, w, h)


def test_the_input_setters_take_it():
    import imaginary_amd as ia
    W, H = 131, 37
    p = ia.plan_set_ycc_input(_plan(ia, W, H, width=60), YCC_422)
    assert p.describe()[0] == ("ycc", (YCC_422, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (W, H, 3))
    assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) > 0                      # the plan validates
    d = ia.plan_set_jpegd_input(_plan(ia, W, H, width=60), YCC_422)
    assert d.describe()[0] == ("jpegd", (YCC_422, 0, 0, 0, 0, 0, 0, 0), (0.0,) * 4, (W, H, 3))
    assert ia.lib.mipx_workspace_bytes(C.byref(d), 2) >= 2 * R.ycc_bytes(W, H)
    hp = ia.plan_set_jpegh_input(_plan(ia, W, H, width=60), YCC_422)
    assert hp.describe() == [("jpegh",) + d.describe()[0][1:]] + d.describe()[1:]
    assert ia.lib.mipx_workspace_bytes(C.byref(hp), 2) >= 256 + R.workspace_bytes(2, W, H)
    for s in (2, 4, 8):
        ow, oh = -(-W // s), -(-H // s)
        ds = ia.plan_set_jpegd_input_scaled(_plan(ia, ow, oh, width=max(ow // 2, 1)), YCC_422, s, W, H)
        hs = ia.plan_set_jpegh_input_scaled(_plan(ia, ow, oh, width=max(ow // 2, 1)), YCC_422, s, W, H)
        assert ds.describe()[0] == ("jpegd", (YCC_422, s, W, H, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 3))
        assert hs.describe()[0] == ("jpegh", (YCC_422, s, W, H, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 3))
        assert ia.lib.mipx_workspace_bytes(C.byref(ds), 1) > 0 and ia.lib.mipx_workspace_bytes(C.byref(hs), 1) > 0
    # 2 stays unknown, and so does everything past 3
    for bad in (2, 4, 7, -1):
        q = _plan(ia, W, H, width=60)
        untouched = bytes(q)
        assert ia.lib.mipx_plan_set_ycc_input(C.byref(q), bad) == -1
        assert ia.lib.mipx_plan_set_jpegd_input(C.byref(q), bad) == -1
        assert ia.lib.mipx_plan_set_jpegh_input(C.byref(q), bad) == -1
        assert bytes(q) == untouched


def test_the_op_calls_take_it_as_far_as_their_argument_checks():
    import imaginary_amd as ia
    L, big = ia.lib, 1 << 40
    # a layout the call takes gets past the layout check to the next one: the missing workspace
    assert L.mipx_op_jpegd_to_rgb(1, 1, 2, 37, 29, YCC_422, 1, 0, None) == -1
    assert "workspace" in ia.lib.mipx_last_error().decode()
    assert L.mipx_op_jpegd_to_rgb_scaled(1, 1, 2, 37, 29, YCC_422, 4, 1, 0, None) == -1
    assert "workspace" in ia.lib.mipx_last_error().decode()
    assert L.mipx_op_jpegh_to_rgb(1, 1, 4, 1, 37, 29, YCC_422, 16, 0, None) == -1
    assert "workspace" in ia.lib.mipx_last_error().decode()
    assert L.mipx_op_jpegd_to_rgb(1, 1, 1, 40000, 40000, YCC_422, 1, big, None) == -2


def test_every_output_call_refuses_it():
    import imaginary_amd as ia
    L, big = ia.lib, 1 << 40
    p = _plan(ia, width=60)
    untouched = bytes(p)
    assert L.mipx_plan_set_jpegc_output(C.byref(p), YCC_422, 75) == -1
    assert L.mipx_plan_set_jpeg_scan_output(C.byref(p), YCC_422, 75) == -1
    assert L.mipx_plan_set_jpeg_scan_output_optimized(C.byref(p), YCC_422, 75) == -1
    assert L.mipx_plan_add_jpeg_roundtrip(C.byref(p), YCC_422, 75, 1) == -1
    assert bytes(p) == untouched
    assert L.mipx_jpeg_scan_bytes(64, 48, YCC_422) == 0 and L.mipx_jpeg_scan_opt_bytes(64, 48, YCC_422) == 0
    assert L.mipx_op_rgb_to_jpegc(1, 1, 1, 64, 48, YCC_422, 75, None) == -1
    assert L.mipx_op_rgb_to_jpeg_scan(1, 1, 1, 64, 48, YCC_422, 75, 16, None) == -1
    assert L.mipx_op_rgb_to_jpeg_scan_optimized(1, 1, 1, 64, 48, YCC_422, 75, 16, None) == -1
    assert L.mipx_op_rgb_to_jpeg_scan_packed(1, 1, 1, 64, 48, YCC_422, 75, 16, None, 0, 8) == -1
    assert L.mipx_op_jpegc_to_scan(1, 1, 1, 64, 48, YCC_422, 16, None) == -1
    assert L.mipx_op_jpegc_to_scan_optimized(1, 1, 1, 64, 48, YCC_422, 16, None) == -1
    assert L.mipx_op_jpegc_to_scan_packed(1, 1, 1, 64, 48, YCC_422, 16, None, 0, 8) == -1
    assert L.mipx_op_jpeg_roundtrip(1, 1, 1, 64, 48, YCC_422, 75, 1, 1, big, None) == -1
    # the steps themselves: a plan that names the layout in an output step does not validate
    for setter, at in ((lambda q: ia.plan_set_jpegc_output(q, YCC_420, 75), -1),
                       (lambda q: ia.plan_set_jpeg_scan_output(q, YCC_420, 75), -1),
                       (lambda q: ia.plan_add_jpeg_roundtrip(q, YCC_420, 75, 1), -1)):
        q = _plan(ia, width=60)
        setter(q)
        assert ia.lib.mipx_workspace_bytes(C.byref(q), 1) > 0
        q.steps[q.n_steps + at].a[0] = YCC_422
        assert ia.lib.mipx_workspace_bytes(C.byref(q), 1) == 0
