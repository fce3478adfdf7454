"""Entropy-coded JPEG input without a device: codec.jpeg_huff_slot against a marker walk of the test's
own, the model of tests/jpegh_ref.py against codec.decode_jpeg_coefs, the sizes, the plan calls and
their refusals, what the files are that the slot builder declines, and what the inputs are that
tests/test_jpegh_gpu.py relies on."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import jpegh_ref
from conftest import GOLDEN
from jpegc_ref import YCC_420, YCC_444, jpegc_bytes
from jpegh_ref import BAD, HEADER_BYTES, OK, ROUNDS, SEQ, SEQ_BYTES, SUB, UNSYNCED, jpegd_bytes, jpegh_bytes
from test_jpegh_gpu import _damaged, dense_slot, files, pillow_jpeg, pixels, several_sequences_size

PIL = pytest.importorskip("PIL.Image")
W, H = 128, 96


def _plan(ia, w=W, h=H, bands=3, **opts):
    return ia.plan_make(ia.make_opts(**opts), ia.make_input(w, h, bands, "png"))


# ---------------------------------------------------------------- the slot
@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimized"])
@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
def test_the_slot_holds_the_files_tables_and_scan(layout, optimize):
    from imaginary_amd import codec
    for w, h in [(1, 1), (17, 9), (37, 29), (129, 67)]:
        for quality in (1, 75, 100):
            for buf, slot, payload in files(w, h, layout, quality, optimize):
                fw, fh, samp, qt, sel, dht, dri, scan = jpegh_ref.file_tables(buf)
                assert (fw, fh, dri) == (w, h, 0) and samp == ([(1, 1)] * 3 if layout == YCC_444 else [(2, 2), (1, 1), (1, 1)])
                length, q, selectors, tables = jpegh_ref.parse_slot(slot)
                assert slot.dtype == np.uint8 and slot.shape == (jpegh_bytes(w, h, layout),)
                assert length == len(scan) and slot[HEADER_BYTES:HEADER_BYTES + length].tobytes() == scan
                assert not slot[HEADER_BYTES + length:].any() and not slot[4:16].any() and not slot[406:416].any()
                assert q.tolist() == qt and selectors == sel
                for i, key in enumerate(jpegh_ref.TABLE_KEYS):
                    counts, symbols = dht[key]
                    assert tables[i] == (counts, symbols + bytes(256 - len(symbols)))
                # built again from its parts by the reference's own builder
                again = jpegh_ref.build_slot(w, h, layout, scan, qt, sel, dht)
                assert np.array_equal(again, slot)
                if optimize and quality == 75 and (w, h) == (129, 67):
                    assert dht[0x10] != codec.HUFFMAN_TABLES[0x10]      # the tables are not Annex K's


@pytest.mark.parametrize("layout", [YCC_444, YCC_420], ids=["444", "420"])
def test_the_model_decodes_to_what_the_host_decoder_gives(layout):
    for w, h in [(1, 1), (8, 8), (17, 9), (33, 17), (129, 67)]:
        for quality in (1, 50, 100):
            for optimize in (False, True):
                for _, slot, payload in files(w, h, layout, quality, optimize):
                    status, got = jpegh_ref.decode_slot(slot, w, h, layout)
                    assert status == OK and np.array_equal(got, payload), (w, h, quality, optimize)


def test_the_model_on_a_photograph():
    from imaginary_amd import codec
    buf = open(os.path.join(GOLDEN, "testdata", "imaginary.jpg"), "rb").read()
    (slot, layout), (payload, _) = codec.jpeg_huff_slot(buf), codec.decode_jpeg_coefs(buf)
    hd = codec.header(buf)
    status, got = jpegh_ref.decode_slot(slot, hd.w, hd.h, layout)
    assert status == OK and np.array_equal(got, payload)
    assert int(slot[:4].view("<u4")[0]) > 3 * SEQ_BYTES     # four sequences: a photograph locks at once


def test_the_model_declines_what_the_host_decoder_declines():
    from imaginary_amd import codec
    w, h = 129, 67
    for layout in (YCC_444, YCC_420):
        buf = files(w, h, layout, 90)[0][0]
        at = buf.index(bytes(files(w, h, layout, 90)[0][1][HEADER_BYTES:HEADER_BYTES + 16]))
        for name, slot in _damaged(w, h, layout).items():
            status, payload = jpegh_ref.decode_slot(slot, w, h, layout)
            assert status in (OK, BAD), name            # one sequence: never UNSYNCED
            if name in ("length 0", "length past the capacity", "counts summing to 300", "table index 2"):
                assert status == BAD
                continue
            length = int(slot[:4].view("<u4")[0])
            host = codec.decode_jpeg_coefs(buf[:at] + slot[HEADER_BYTES:HEADER_BYTES + length].tobytes() + b"\xff\xd9")
            assert (host is None) == (status == BAD), name
            if host is not None:
                assert np.array_equal(host[0], payload), name


# ---------------------------------------------------------------- files without a slot
def _save(im, **kw):
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    return b.getvalue()


def test_jpeg_huff_slot_declines_everything_else():
    from imaginary_amd import codec
    rgb = PIL.fromarray(pixels(32, 24)[0])
    whole = _save(rgb, quality=92)
    assert codec.jpeg_huff_slot(whole) is not None
    assert codec.jpeg_huff_slot(_save(rgb, quality=92, progressive=True)) is None
    assert codec.jpeg_huff_slot(_save(rgb.convert("L"), quality=92)) is None                  # grey
    assert codec.jpeg_huff_slot(_save(rgb, quality=92, subsampling=1)) is None                # 4:2:2
    assert codec.jpeg_huff_slot(_save(rgb.convert("CMYK"), quality=92)) is None
    restart = _save(rgb, quality=92, restart_marker_blocks=2)
    assert b"\xff\xdd" in restart and b"\xff\xd0" in restart                                   # DRI and a restart marker
    assert codec.decode_jpeg_coefs(restart) is not None and codec.jpeg_huff_slot(restart) is None
    scan = whole.index(b"\xff\xda")
    for cut in (scan + 14 + (len(whole) - scan - 14) // 2, len(whole) - 2, scan + 4):
        assert codec.jpeg_huff_slot(whole[:cut]) is None                                      # truncated
    b = io.BytesIO()
    rgb.save(b, "PNG")
    for buf in (b.getvalue(), b"", b"\xff\xd8\xff not a jpeg", open(os.path.join(GOLDEN, "testdata", "test.webp"), "rb").read(),
                np.random.default_rng(9).integers(0, 256, 4096, dtype=np.uint8).tobytes()):
        assert codec.jpeg_huff_slot(buf) is None
    # Huffman tables 2 and 3 in the chroma's place: the host decoder takes them, the slot has no room
    moved = bytearray(whole)
    p = 2
    while moved[p + 1] != 0xDA:
        size = int.from_bytes(moved[p + 2:p + 4], "big")
        if moved[p + 1] == 0xC4 and moved[p + 4] in (0x01, 0x11):
            moved[p + 4] += 1
        p += 2 + size
    assert bytes(moved[p + 4:p + 11]) == bytes([3, 1, 0x00, 2, 0x11, 3, 0x11])
    moved[p + 8] = moved[p + 10] = 0x22
    assert codec.decode_jpeg_coefs(bytes(moved))[0].tobytes() == codec.decode_jpeg_coefs(whole)[0].tobytes()
    assert codec.jpeg_huff_slot(bytes(moved)) is None
    # a scan longer than the coefficients it codes: every AC +-1023, 26 bits for 16
    c = np.where(np.arange(3 * 4 * 64) % 2 == 0, 1023, -1023).astype(np.int16)
    c[::64] = 0
    long_scan = codec.encode_jpeg_coefs(c, 16, 16, YCC_444, 90)
    assert len(long_scan) > jpegc_bytes(16, 16, YCC_444) and codec.decode_jpeg_coefs(long_scan) is not None
    assert codec.jpeg_huff_slot(long_scan) is None
    # damaged files: whatever it returns, it does not raise
    rng = np.random.default_rng(11)
    for _ in range(40):
        bad = bytearray(whole)
        for at in rng.integers(2, len(whole), 3):
            bad[at] = rng.integers(0, 256)
        got = codec.jpeg_huff_slot(bytes(bad))
        assert got is None or (got[0].dtype == np.uint8 and got[0].ndim == 1 and got[1] in (YCC_444, YCC_420))


# ---------------------------------------------------------------- sizes
def test_sizes():
    import imaginary_amd as ia
    from imaginary_amd import _abi
    assert _abi.lib.mipx_abi_version() == 6 and _abi.OP_JPEGH == 20 and _abi.MIPX_EDATA == -10
    assert (_abi.JPEGH_HEADER_BYTES, _abi.JPEGH_OK, _abi.JPEGH_UNSYNCED, _abi.JPEGH_BAD) == (HEADER_BYTES, OK, UNSYNCED, BAD)
    assert b"not decodable" in _abi.lib.mipx_strerror(-10)
    for w, h in [(1, 1), (2, 2), (5, 3), (17, 9), (64, 48), (37, 29), (197, 117), (3840, 2160)]:
        for layout in (YCC_444, YCC_420):
            assert ia.jpegh_bytes(w, h, layout) == jpegh_bytes(w, h, layout) == 1504 + jpegc_bytes(w, h, layout)
        for n in (1, 3, 64):
            assert ia.lib.mipx_op_workspace_bytes(20, n, w, h, 3, 0.0, 0.0) == jpegh_ref.workspace_bytes(n, w, h), (n, w, h)
    for w, h, layout in [(0, 8, YCC_444), (8, 0, YCC_420), (-1, 8, YCC_444), (8, 8, 2), (8, 8, -1)]:
        assert ia.jpegh_bytes(w, h, layout) == 0
    assert ia.lib.mipx_op_workspace_bytes(20, 0, 8, 8, 3, 0.0, 0.0) == 0


# ---------------------------------------------------------------- planner
def test_setters_put_the_step_first_with_the_coefficient_steps_arguments():
    import imaginary_amd as ia
    for opts in (dict(), dict(width=60), dict(width=40, height=30, crop=1)):
        for layout in (YCC_444, YCC_420):
            d = ia.plan_set_jpegd_input(_plan(ia, **opts), layout)
            p = ia.plan_set_jpegh_input(_plan(ia, **opts), layout)
            assert p.describe() == [("jpegh",) + d.describe()[0][1:]] + d.describe()[1:]
            b = _plan(ia, **opts)
            assert ia.plan_set_jpegh_input_scaled(b, layout, 1, W, H) is b and bytes(b) == bytes(p)
            # the workspace: the statuses at the head, then the decoder's
            assert ia.lib.mipx_workspace_bytes(C.byref(p), 3) >= 256 + jpegh_ref.workspace_bytes(3, W, H)
    for s in (2, 4, 8):
        ow, oh = -(-W // s), -(-H // s)
        d = ia.plan_set_jpegd_input_scaled(_plan(ia, ow, oh, width=max(ow // 2, 1)), YCC_420, s, W, H)
        p = ia.plan_set_jpegh_input_scaled(_plan(ia, ow, oh, width=max(ow // 2, 1)), YCC_420, s, W, H)
        assert p.describe()[0] == ("jpegh", (YCC_420, s, W, H, 0, 0, 0, 0), (0.0,) * 4, (ow, oh, 3))
        assert p.describe()[1:] == d.describe()[1:]
        # sized by the file, not by what it decodes to
        assert ia.lib.mipx_workspace_bytes(C.byref(p), 2) >= 256 + jpegh_ref.workspace_bytes(2, W, H)


def test_setters_compose_with_the_text_watermark_and_the_jpeg_outputs():
    import imaginary_amd as ia
    a = _plan(ia, width=20)
    ia.plan_add_textmark(a, 10, 4, 3, 0.5, (1, 2, 3))
    ia.plan_set_jpeg_scan_output(a, YCC_420, 75)
    ia.plan_set_jpegh_input(a, YCC_420)
    b = _plan(ia, width=20)
    ia.plan_set_jpegh_input(b, YCC_420)
    ia.plan_set_jpeg_scan_output(b, YCC_420, 75)
    ia.plan_add_textmark(b, 10, 4, 3, 0.5, (1, 2, 3))
    names = [st[0] for st in a.describe()]
    assert names[0] == "jpegh" and names[-2:] == ["textmark", "jpege"] and names.count("jpegh") == 1
    assert bytes(a) == bytes(b) and ia.lib.mipx_workspace_bytes(C.byref(a), 1) > 0
    d = ia.plan_set_jpegh_input(ia.plan_set_jpegc_output(_plan(ia), YCC_444, 90), YCC_420)
    assert [st[0] for st in d.describe()] == ["jpegh", "jpegc"] and ia.lib.mipx_workspace_bytes(C.byref(d), 1) > 0


def test_setter_refusals_leave_the_plan_untouched():
    import imaginary_amd as ia
    L = ia.lib
    s = 2
    ow, oh = -(-W // s), -(-H // s)
    p = _plan(ia, ow, oh, width=30)
    untouched = bytes(p)
    set_ = L.mipx_plan_set_jpegh_input_scaled
    assert set_(C.byref(p), 2, s, W, H) == -1 and set_(C.byref(p), -1, s, W, H) == -1      # unknown layout
    assert set_(None, YCC_420, s, W, H) == -1 and L.mipx_plan_set_jpegh_input(None, YCC_420) == -1
    assert L.mipx_plan_set_jpegh_input(C.byref(p), 2) == -1
    for shrink in (0, 3, 5, 6, 7, 16, -2):
        assert set_(C.byref(p), YCC_420, shrink, W, H) == -1, shrink
    for fw, fh, shrink in [(W + 2, H, s), (W, H + 2, s), (W, H, 4), (W, H, 1), (0, H, s), (W, 0, s), (-W, -H, s),
                           (ow, oh, s), (2 ** 31 - 1, H, s)]:
        assert set_(C.byref(p), YCC_420, shrink, fw, fh) == -1, (fw, fh, shrink)
    assert bytes(p) == untouched
    for bands in (1, 2, 4):
        q = _plan(ia, ow, oh, bands=bands, width=30)
        before = bytes(q)
        assert set_(C.byref(q), YCC_420, s, W, H) == -1 and L.mipx_plan_set_jpegh_input(C.byref(q), YCC_420) == -1
        assert bytes(q) == before
    # the input calls refuse each other
    setters = [lambda q: L.mipx_plan_set_jpegh_input_scaled(C.byref(q), YCC_420, s, W, H),
               lambda q: L.mipx_plan_set_jpegd_input_scaled(C.byref(q), YCC_420, s, W, H),
               lambda q: L.mipx_plan_set_jpegh_input(C.byref(q), YCC_420),
               lambda q: L.mipx_plan_set_jpegd_input(C.byref(q), YCC_420),
               lambda q: L.mipx_plan_set_ycc_input(C.byref(q), YCC_420)]
    for first in (0, 1, 4):
        q = _plan(ia, ow, oh, width=30)
        assert setters[first](q) == 0
        taken = bytes(q)
        for other in setters:
            assert other(q) == -1
        assert bytes(q) == taken
    full = _plan(ia, ow, oh)
    full.n_steps = 64   # MIPX_MAX_STEPS
    for i in range(full.n_steps):
        full.steps[i].op = 2
        full.steps[i].out_w, full.steps[i].out_h, full.steps[i].out_bands = ow, oh, 3
    taken = bytes(full)
    assert set_(C.byref(full), YCC_420, s, W, H) == -1 and bytes(full) == taken


def test_chain_takes_the_step_in_stage_zero_only():
    import imaginary_amd as ia
    s0 = ia.plan_set_jpegh_input(_plan(ia, width=32), YCC_420)
    s1 = _plan(ia, s0.out_w, s0.out_h, width=16)
    merged = ia.plan_chain([s0, s1])
    names = [st[0] for st in merged.describe()]
    assert names[0] == "jpegh" and names.count("jpegh") == 1 and names.count("reduce") == 2
    assert ia.lib.mipx_workspace_bytes(C.byref(merged), 1) > 0
    h1 = ia.plan_set_jpegh_input(_plan(ia, s0.out_w, s0.out_h, width=16), YCC_420)
    arr = (ia.MipxPlan * 2)(_plan(ia, width=32), h1)
    out = ia.MipxPlan()
    assert ia.lib.mipx_plan_chain(arr, 2, C.byref(out)) == -1


def _hand_plan(ia, a, w, h, ops=(20,)):
    p = ia.MipxPlan()
    p.load_shrink = 1
    p.in_w, p.in_h, p.in_bands = w, h, 3
    p.out_w, p.out_h, p.out_bands = w, h, 3
    p.n_steps = len(ops)
    for i, op in enumerate(ops):
        p.steps[i].op = op
        p.steps[i].out_w, p.steps[i].out_h, p.steps[i].out_bands = w, h, 3
    for k, v in enumerate(a):
        p.steps[0].a[k] = v
    return p


def test_hand_written_steps_are_validated_before_any_device_work():
    import imaginary_amd as ia
    from imaginary_amd._abi import MipxImg
    L = ia.lib
    good = [_hand_plan(ia, (YCC_420, 2, 33, 17), 17, 9), _hand_plan(ia, (YCC_444, 4, 33, 17), 9, 5, ops=(20, 2)),
            _hand_plan(ia, (YCC_420, 8, 40, 24), 5, 3), _hand_plan(ia, (YCC_420, 1, 0, 0), 33, 17),
            _hand_plan(ia, (YCC_420, 0, 0, 0), 33, 17)]
    for p in good:
        assert L.mipx_workspace_bytes(C.byref(p), 1) > 0
    assert bytes(ia.plan_set_jpegh_input_scaled(_plan(ia, 17, 9), YCC_420, 2, 33, 17)) == bytes(good[0])
    bad = [_hand_plan(ia, (YCC_420, 3, 33, 17), 11, 6), _hand_plan(ia, (YCC_420, 2, 33, 17), 16, 9),
           _hand_plan(ia, (YCC_420, 2, 0, 17), 17, 9), _hand_plan(ia, (7, 2, 33, 17), 17, 9),
           _hand_plan(ia, (YCC_420, 0, 0, 0), 33, 17, ops=(2, 20)),        # behind another step
           _hand_plan(ia, (YCC_420, 0, 0, 0), 33, 17, ops=(20, 17)),       # beside the coefficient step
           _hand_plan(ia, (YCC_420, 0, 0, 0), 33, 17, ops=(20, 15)),       # beside the planar step
           _hand_plan(ia, (YCC_444, 0, 0, 0), 12000, 12000)]               # a scan of 2^32 bits or more
    assert jpegc_bytes(12000, 12000, YCC_444) >= 2 ** 29
    for p in bad:
        assert L.mipx_workspace_bytes(C.byref(p), 1) == 0
        assert L.mipx_execute_dev(C.byref(p), 1, 4096, 8192, None, 12288, 1 << 20, None) == -1
    # submit: the image is described as the decode, without a stride; a length past the capacity is refused on the host
    p = ia.plan_set_jpegh_input_scaled(_plan(ia, 17, 9, width=8), YCC_420, 2, 33, 17)
    data = np.zeros(jpegh_bytes(33, 17, YCC_420), np.uint8)
    dst = np.zeros((p.out_h, p.out_w, 3), np.uint8)
    out = MipxImg(dst.ctypes.data, p.out_w, p.out_h, 3, 0)
    t = C.c_uint64()

    def submit(w, h, bands, stride, ptr=data.ctypes.data):
        src = MipxImg(ptr, w, h, bands, stride)
        return L.mipx_submit(-1, C.byref(p), C.byref(src), None, C.byref(out), C.byref(t))

    assert submit(33, 17, 3, 0) == -1 and submit(17, 9, 3, 51) == -1 and submit(17, 9, 1, 0) == -1
    assert submit(17, 9, 3, 0, None) == -1
    data[:4] = np.array([jpegc_bytes(33, 17, YCC_420) + 1], "<u4").view(np.uint8)
    assert submit(17, 9, 3, 0) == -1 and b"capacity" in L.mipx_last_error()
    data[:4] = 0
    if ia.device_count() == 0:
        assert submit(17, 9, 3, 0) == -7          # well-formed: only the engine is missing


def test_entry_points_reject_bad_arguments_without_touching_the_device():
    import imaginary_amd as ia
    L = ia.lib
    big = 1 << 40
    calls = [lambda *a: L.mipx_op_jpegh_to_jpegd(*a), lambda *a: L.mipx_op_jpegh_to_rgb(*a),
             lambda a, b, c, n, w, h, layout, ws, wsb, st: L.mipx_op_jpegh_to_rgb_scaled(a, b, c, n, w, h, layout, 2, ws, wsb, st)]
    for f in calls:
        assert f(None, 256, 256, 1, 8, 8, YCC_420, 256, big, None) == -1
        assert f(256, None, 256, 1, 8, 8, YCC_420, 256, big, None) == -1
        assert f(256, 256, None, 1, 8, 8, YCC_420, 256, big, None) == -1
        assert f(256, 256, 256, 1, 8, 8, YCC_420, None, big, None) == -1
        assert f(256, 256, 256, 0, 8, 8, YCC_420, 256, big, None) == -1
        assert f(256, 256, 256, 1, 0, 8, YCC_420, 256, big, None) == -1
        assert f(256, 256, 256, 1, 8, -1, YCC_444, 256, big, None) == -1
        assert f(256, 256, 256, 1, 8, 8, 2, 256, big, None) == -1
        assert f(256, 256, 256, 1, 8, 8, YCC_420, 264, big, None) == -1      # the workspace on 8 bytes
        assert f(256, 256, 258, 1, 8, 8, YCC_420, 256, big, None) == -1      # the statuses on 2
        need = L.mipx_op_workspace_bytes(20, 2, 37, 29, 3, 0.0, 0.0)
        assert f(256, 256, 256, 2, 37, 29, YCC_420, 256, need - 1, None) == -1
        assert f(256, 256, 256, 1, 12000, 12000, YCC_444, 256, big, None) == -2
    for s in (3, 5, 16, -1):
        assert L.mipx_op_jpegh_to_rgb_scaled(256, 256, 256, 1, 8, 8, YCC_420, s, 256, big, None) == -1
    with pytest.raises(ValueError):
        ia.jpegh_to_jpegd(np.zeros(jpegh_bytes(16, 16, YCC_444) - 1, np.uint8), 16, 16, YCC_444)
    with pytest.raises(ValueError):
        ia.jpegh_to_rgb_scaled(np.zeros(jpegh_bytes(16, 16, YCC_444), np.uint8), 16, 16, YCC_444, 3)
    p = ia.plan_set_jpegh_input_scaled(_plan(ia, 17, 9), YCC_420, 2, 33, 17)
    with pytest.raises(ValueError):     # execute reads the file's size from the step
        ia.execute(p, np.zeros((2, jpegh_bytes(17, 9, YCC_420)), np.uint8))


# ---------------------------------------------------------------- what the inputs of the GPU tests are
def _passes(slot, w, h, layout):
    """(subsequences, passes of entry[i + 1] = F_i(entry[i]) over all of them until nothing changes),
    every decoder but the first starting with the guess."""
    length, _, sel, tables = jpegh_ref.parse_slot(slot)
    data, marker = jpegh_ref.unstuff(slot[HEADER_BYTES:HEADER_BYTES + length].tobytes())
    s = jpegh_ref.Stream(data, [jpegh_ref.lookup16(c, sy) for c, sy in tables], sel, layout, jpegh_ref.scan_blocks(w, h, layout))
    entry = [(8 * SUB * i, 0, 0) for i in range(s.nsub + 1)]      # the last one is the scan's exit state
    passes = 0
    while True:
        passes += 1
        exits = [s.run(*entry[i], min(8 * SUB * (i + 1), s.total))[:3] for i in range(s.nsub)]
        new = [entry[0]] + exits
        if new == entry:
            return s.nsub, passes
        entry = new


def test_the_dense_scans_never_synchronise():
    """Every block DC 0 and 63 ACs of 1: 191 bits a block, no end-of-block code anywhere, so the decoders
    agree only as far as the truth has walked: one pass per subsequence, and one to see it."""
    from imaginary_amd import codec
    for side, want in [(64, 36), (80, 56)]:
        slot, payload = dense_slot(side)
        assert int(slot[:4].view("<u4")[0]) == -(-3 * (side // 8) ** 2 * 191 // 8)     # no 0xFF byte in it
        nsub, passes = _passes(slot, side, side, YCC_444)
        assert (nsub, passes) == (want, want + 1)
        assert (payload[384:].view("<i2").reshape(-1, 64)[:, 1:] == 1).all() and not payload[384:].view("<i2")[::64].any()
    slot, _ = dense_slot(128)
    length = int(slot[:4].view("<u4")[0])
    assert -(-length // SUB) == 144 and length < SEQ_BYTES         # 144 lanes of one sequence
    assert jpegh_ref.decode_slot(slot, 128, 128, YCC_444)[0] == OK
    # the truth walks one sequence per launch: ROUNDS sequences are decoded, one more is not
    for sequences, want in [(ROUNDS - 1, OK), (ROUNDS, UNSYNCED), (ROUNDS + 1, UNSYNCED)]:
        side = jpegh_ref.dense_size(sequences)
        slot, _ = dense_slot(side)
        length = int(slot[:4].view("<u4")[0])
        assert sequences * SEQ_BYTES < length <= (sequences + 1) * SEQ_BYTES, (side, length)
        assert jpegh_ref.decode_slot(slot, side, side, YCC_444)[0] == want, sequences
    # a photograph of as many subsequences locks in a few passes
    buf = open(os.path.join(GOLDEN, "testdata", "smart-crop.jpg"), "rb").read()
    hd = codec.header(buf)
    slot, layout = codec.jpeg_huff_slot(buf)
    nsub, passes = _passes(slot, hd.w, hd.h, layout)
    assert nsub > 600 and passes <= 12


def test_the_noise_scan_spans_enough_sequences():
    w, h = several_sequences_size()
    assert (w, h) == (205, 117)
    for _, slot, _ in files(w, h, YCC_444, 100):
        assert int(slot[:4].view("<u4")[0]) > (ROUNDS + 1) * SEQ_BYTES
        assert jpegh_ref.decode_slot(slot, w, h, YCC_444)[0] == OK
    assert SEQ_BYTES == SUB * SEQ == 32768
