"""4:2:2 (h2v1) JPEG input on the device (MIPX_YCC_422): k_ycc422 against tests/jpeg422_ref.py on
random planes, the coefficient decode at every scale on Pillow-written files and on coefficients no
encoder writes, the entropy decoder against codec.decode_jpeg_coefs on ordinary and restart files,
then plans, the request path and process_bytes.  Every comparison is exact; the guard bands of
every buffer are live.

The shapes are the smallest at which a specific thing can go wrong:
  1x1, 3x2, 4x5   cw <= 2: replication, the pixel path
  5x3, 6x1        cw = 3: the smallest fancy case, every lane an edge lane
  8x16            the workspace bound: 8 scan blocks where the other layouts have 6
  17x9            odd w, a partial MCU in both directions, dummy Y and chroma blocks
  261x19          more than one wave per row: an interior lane, an edge lane, a short last lane; w h odd
  1027x13         several workgroups across, unaligned rows
  520x40          k_jpegd / k_jpegds runs: 65 Y blocks across, so a second, partial run"""
import functools
import io

import numpy as np
import pytest

import jpeg422_ref as R
import jpegh_ref
from footprint import FILL, guarded  # noqa: F401
from jpeg422_ref import YCC_422
from jpegh_ref import BAD, OK

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 2), (4, 5), (5, 3), (6, 1), (8, 16), (17, 9), (261, 19), (1027, 13), (520, 40)]
FILE_SHAPES = [(8, 16), (17, 9), (261, 19), (520, 40)]
SKEWS = [(0, 0), (1, 3), (2, 1), (3, 2)]
RESTARTS = [dict(), dict(restart_marker_blocks=1), dict(restart_marker_blocks=3), dict(restart_marker_rows=1)]


def _under(skew_in, skew_out, call):
    from imaginary_amd import engine
    prev = engine.set_guard(FILL, skew_in, skew_out)
    try:
        before = engine.guarded_calls()
        out = call()
        assert engine.guarded_calls() > before, "the guard was not live"
        return out
    finally:
        engine.set_guard(*prev)


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        d = np.flatnonzero(got.ravel() != want.ravel())
        at = int(d[0])
        raise AssertionError(f"{what}: {d.size} of {got.size} bytes differ, the first at {at}: "
                             f"got {got.ravel()[at:at + 8].tolist()} want {want.ravel()[at:at + 8].tolist()}")


@functools.lru_cache(maxsize=None)
def planes(w, h, n=3):
    """Random packed 4:2:2 planes and the reference's RGB; read-only."""
    p = np.random.default_rng(4220 + 31 * w + h).integers(0, 256, (n, R.ycc_bytes(w, h)), dtype=np.uint8)
    rgb = R.ycc422_ref(p, w, h)
    p.setflags(write=False), rgb.setflags(write=False)
    return p, rgb


@functools.lru_cache(maxsize=None)
def files(w, h, quality=75, optimize=False, restart=0, n=3):
    """n files of w x h noise (RESTARTS[restart]) with their slots and the host decoder's payloads; read-only."""
    from imaginary_amd import codec
    out = []
    for i in range(n):
        buf = R.pillow_jpeg(R.noise(w, h, i), quality, optimize, **RESTARTS[restart])
        (slot, l1), (payload, l2) = codec.jpeg_huff_slot(buf, restart=True, h2v1=True), codec.decode_jpeg_coefs(buf, h2v1=True)
        assert l1 == l2 == YCC_422 and slot.size == R.jpegh_bytes(w, h) and payload.size == R.jpegd_bytes(w, h)
        slot.setflags(write=False), payload.setflags(write=False)
        out.append((buf, slot, payload))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def decoded(w, h, s):
    """The reference's RGB at 1 / s of files(w, h)'s payloads; read-only."""
    rgb = R.jpegd422_ref(np.stack([p for _, _, p in files(w, h)]), w, h, s)
    rgb.setflags(write=False)
    return rgb


def _copy(gpu, p):
    import ctypes as C
    q = gpu.MipxPlan()
    C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
    return q


def _base(gpu, w, h, **opts):
    return gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png"))


# ---------------------------------------------------------------- 1. planes to RGB
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_ycc422_equals_the_reference(gpu, shape):
    w, h = shape
    p, want = planes(w, h)
    for si, so in SKEWS:
        got = _under(si, so, lambda: gpu.ycc_to_rgb(p, w, h, YCC_422))
        _same(got, want, f"ycc_to_rgb 3x{h}x{w} skew {si},{so}")
    one = gpu.ycc_to_rgb(p[1], w, h, YCC_422)
    _same(one[0], want[1], f"ycc_to_rgb {h}x{w}, one image")


@pytest.mark.parametrize("shape", [(17, 9), (261, 19), (520, 40)], ids=lambda s: "%dx%d" % s)
def test_a_plan_takes_422_planes(gpu, shape):
    w, h = shape
    p, rgb = planes(w, h)
    base = _base(gpu, w, h, width=max(w // 3, 1))
    q = gpu.plan_set_ycc_input(_copy(gpu, base), YCC_422)
    assert q.describe()[0][0] == "ycc" and q.describe()[0][1][0] == YCC_422
    want = gpu.execute(base, rgb, junk=0x3C)
    got = _under(1, 3, lambda: gpu.execute(q, p, junk=0x3C))
    _same(got, want, f"resize of {h}x{w} planes")


# ---------------------------------------------------------------- 2. coefficients to RGB
@pytest.mark.parametrize("shrink", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", FILE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_coefficient_decode_equals_the_reference(gpu, shape, shrink):
    pytest.importorskip("PIL.Image")
    w, h = shape
    p = np.stack([pl for _, _, pl in files(w, h)])
    want = decoded(w, h, shrink)
    for si, so in SKEWS[:2] if shrink > 1 else SKEWS:
        if shrink == 1:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb(p, w, h, YCC_422))
        else:
            got = _under(si, so, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, YCC_422, shrink))
        _same(got, want, f"jpegd 3x{h}x{w} at 1/{shrink} skew {si},{so}")


def test_the_coefficient_rule_is_total(gpu):
    """Coefficients no encoder writes: full-range random int16 with random tables, where pass 1
    saturates and the dequantisation wraps.  The reference alone is the yardstick here."""
    rng = np.random.default_rng(422)
    w, h = 261, 19
    coefs = rng.integers(-32768, 32768, (3, R.jpegc_bytes(w, h) // 2), dtype=np.int16)
    p = np.stack([np.concatenate([rng.integers(1, 256, 192).astype("<u2").view(np.uint8), c.view(np.uint8)]) for c in coefs])
    for shrink in (1, 2, 4, 8):
        trace = {}
        want = R.jpegd422_ref(p, w, h, shrink, trace)
        assert shrink == 8 or trace["saturated"] > 0          # the saturation really fires
        got = _under(2, 1, lambda: gpu.jpegd_to_rgb_scaled(p, w, h, YCC_422, shrink))
        _same(got, want, f"random coefficients {h}x{w} at 1/{shrink}")


# ---------------------------------------------------------------- 3. the scan to coefficients and RGB
def _decode(gpu, slots, w, h, skews=(0, 0)):
    payloads, status = _under(*skews, lambda: gpu.jpegh_to_jpegd(np.stack(slots), w, h, YCC_422))
    assert payloads.shape == (len(slots), R.jpegd_bytes(w, h)) and status.shape == (len(slots),)
    return payloads, status.tolist()


@pytest.mark.parametrize("optimize", [False, True], ids=["annexk", "optimized"])
@pytest.mark.parametrize("restart", range(4), ids=["plain", "ri1", "ri3", "row"])
@pytest.mark.parametrize("shape", FILE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_decoder_equals_the_host_decoder(gpu, shape, restart, optimize):
    pytest.importorskip("PIL.Image")
    w, h = shape
    f = files(w, h, 75, optimize, restart)
    mw, mh = R.mcus(w, h)
    ri = [0, 1, 3, mw][restart]
    for _, slot, _ in f:
        assert int(slot[4:8].view("<u4")[0]) == ri
    for n in (1, 3):
        skews = SKEWS[(restart + n) % 4]
        got, status = _decode(gpu, [s for _, s, _ in f[:n]], w, h, skews)
        assert status == [OK] * n, (shape, restart, optimize, status)
        for i in range(n):
            _same(got[i], f[i][2], f"{h}x{w} restart {ri} optimize {optimize} skew {skews}, image {i} of {n}")


@pytest.mark.parametrize("shape", FILE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_the_scan_decodes_to_pixels_at_every_scale(gpu, shape):
    pytest.importorskip("PIL.Image")
    w, h = shape
    for restart in (0, 2):
        f = files(w, h, 75, False, restart)
        slots = np.stack([s for _, s, _ in f])
        for k, shrink in enumerate((1, 2, 4, 8)):
            if shrink == 1:
                got, status = _under(*SKEWS[k], lambda: gpu.jpegh_to_rgb(slots, w, h, YCC_422))
            else:
                got, status = _under(*SKEWS[k], lambda: gpu.jpegh_to_rgb_scaled(slots, w, h, YCC_422, shrink))
            assert status.tolist() == [OK] * 3
            want = decoded(w, h, shrink) if restart == 0 else R.jpegd422_ref(np.stack([p for _, _, p in f]), w, h, shrink)
            _same(got, want, f"jpegh to rgb {h}x{w} restart {restart} at 1/{shrink}")


def _flipped(slot):
    """An ordinary slot with one scan byte's bits flipped: a 00 that no FF precedes and no 00 follows
    becomes an FF that no 00 follows, which include/mipx.h says is BAD."""
    length = int(slot[:4].view("<u4")[0])
    scan = slot[1504:1504 + length]
    at = [i for i in range(1, length - 1) if scan[i] == 0 and scan[i - 1] != 0xFF and scan[i + 1] != 0]
    assert at, "no such byte in this scan"
    out = slot.copy()
    out[1504 + at[len(at) // 2]] ^= 0xFF
    return out


def _wrong_marker(slot):
    """A restart slot whose second marker carries another number."""
    length = int(slot[:4].view("<u4")[0])
    scan = slot[1504:1504 + length].tobytes()
    at = scan.index(b"\xff\xd1")
    out = slot.copy()
    out[1504 + at + 1] = 0xD3
    return out


def test_a_batch_mixes_ordinary_and_restart_slots_and_damaged_ones_are_bad(gpu):
    pytest.importorskip("PIL.Image")
    w, h = 261, 19
    plain, one, three = files(w, h, 75, False, 0), files(w, h, 75, False, 1), files(w, h, 75, True, 2)
    slots = [plain[0][1], three[1][1], _flipped(plain[1][1]), one[2][1], _wrong_marker(three[0][1]), plain[2][1]]
    good = {0: plain[0][2], 1: three[1][2], 3: one[2][2], 5: plain[2][2]}
    for skews in (SKEWS[1], SKEWS[2]):
        got, status = _decode(gpu, slots, w, h, skews)
        assert status == [OK, OK, BAD, OK, BAD, OK], status
        for i, want in good.items():
            _same(got[i], want, f"slot {i} skew {skews}")


def test_a_scan_that_crosses_a_sequence_boundary(gpu):
    pytest.importorskip("PIL.Image")
    w, h = 200, 150
    f = files(w, h, 95, False, 0, 1)
    sync, unstuffed = R.synchronised(f[0][1], w, h)
    assert sync and jpegh_ref.SEQ_BYTES < unstuffed < 2 * jpegh_ref.SEQ_BYTES     # the model: two sequences that lock
    got, status = _decode(gpu, [f[0][1]], w, h, SKEWS[3])
    assert status == [OK]
    _same(got[0], f[0][2], "a scan of two sequences")


# ---------------------------------------------------------------- 4. plans and the request path
def _plan_pair(gpu, w, h, shrink, **opts):
    ow, oh = -(-w // shrink), -(-h // shrink)
    base = _base(gpu, ow, oh, **opts)
    if shrink == 1:
        return base, gpu.plan_set_jpegd_input(_copy(gpu, base), YCC_422), gpu.plan_set_jpegh_input(_copy(gpu, base), YCC_422)
    return (base, gpu.plan_set_jpegd_input_scaled(_copy(gpu, base), YCC_422, shrink, w, h),
            gpu.plan_set_jpegh_input_scaled(_copy(gpu, base), YCC_422, shrink, w, h))


@pytest.mark.parametrize("shrink", [1, 2, 8])
def test_plans_on_coefficients_and_on_the_scan(gpu, shrink):
    pytest.importorskip("PIL.Image")
    w, h = 261, 19
    f = files(w, h)
    slots, payloads = np.stack([s for _, s, _ in f]), np.stack([p for _, _, p in f])
    base, pd, ph = _plan_pair(gpu, w, h, shrink, width=24)
    assert pd.steps[0].op == 17 and ph.steps[0].op == 20 and pd.steps[0].a[0] == ph.steps[0].a[0] == YCC_422
    want = gpu.execute(base, decoded(w, h, shrink), junk=0x3C)
    _same(_under(1, 3, lambda: gpu.execute(pd, payloads, junk=0x3C)), want, f"a plan on coefficients at 1/{shrink}")
    got = _under(2, 1, lambda: gpu.execute(ph, slots, junk=0x3C))
    assert gpu.execute_status().tolist() == [OK] * 3
    _same(got, want, f"a plan on the scan at 1/{shrink}")


def test_the_request_path_batches_422_requests(gpu):
    pytest.importorskip("PIL.Image")
    w, h = 261, 19
    plain, restart = files(w, h), files(w, h, 75, False, 2)
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8, batch_wait_us=2000)
    try:
        for shrink in (1, 2):
            _, pd, ph = _plan_pair(gpu, w, h, shrink, width=24)
            want = gpu.execute(pd, np.stack([p for _, _, p in plain]))      # the op-level result
            reqs = [(plain, restart)[i % 2][i % 3] for i in range(6)]
            for plan, pick in ((pd, 2), (ph, 1)):
                outs = [np.full((plan.out_h, plan.out_w, 3), 0x5A, np.uint8) for _ in reqs]
                tickets = [eng.submit(plan, r[pick], out=o)[0] for r, o in zip(reqs, outs)]
                for t in tickets:
                    eng.wait(t)          # MIPX_EDATA would raise
                for i in range(6):
                    _same(outs[i], want[i % 3], f"{'scan' if pick == 1 else 'coefficient'} request {i} at 1/{shrink}")
    finally:
        eng.shutdown()


# ---------------------------------------------------------------- 5. end to end over bytes
@pytest.mark.parametrize("restart", [False, True], ids=["plain", "restart"])
def test_process_bytes_takes_a_422_file_on_the_engine(gpu, monkeypatch, restart):
    pytest.importorskip("PIL.Image")
    from PIL import Image
    from imaginary_amd import codec, imaginary
    w, h = 261, 147
    y, x = np.mgrid[0:h, 0:w]
    px = np.stack([(x * 255) // (w - 1), (y * 255) // (h - 1), ((x * y) % 256)], axis=-1).astype(np.uint8)
    px = (px.astype(int) + R.noise(w, h) // 8).clip(0, 255).astype(np.uint8)
    b = io.BytesIO()
    Image.fromarray(px).save(b, "JPEG", quality=85, subsampling=1, **(dict(restart_marker_blocks=4) if restart else {}))
    buf = b.getvalue()
    assert codec.jpeg_huff_slot(buf, restart=True) is None and codec.decode_jpeg_coefs(buf) is None
    assert codec.jpeg_huff_slot(buf, restart=True, h2v1=True)[1] == YCC_422
    flags = dict(jpeg_huff=True, jpeg_dct=True, jpeg_dct_shrink=True, jpeg_huff_restart=True)
    calls = []
    real_decode, real_coefs = codec.decode, codec.decode_jpeg_coefs
    for opts in (dict(width=w - 8), dict(width=40)):               # full size; a thumbnail that shrinks on load
        want = imaginary.process_bytes(buf, dict(opts))
        monkeypatch.setattr(codec, "decode", lambda *a, **k: calls.append("decode") or real_decode(*a, **k))
        monkeypatch.setattr(codec, "decode_jpeg_coefs", lambda *a, **k: calls.append("coefs") or real_coefs(*a, **k))
        got = imaginary.process_bytes(buf, dict(opts), jpeg_422=True, **flags)
        assert got.mime == want.mime and got.body == want.body, opts
        assert calls == [], f"the host decoded ({calls}): the engine did not take the scan"
        # by the coefficients alone: the host entropy-decodes, the engine does the rest
        again = imaginary.process_bytes(buf, dict(opts), jpeg_dct=True, jpeg_dct_shrink=True, jpeg_422=True)
        assert again.body == want.body and calls == ["coefs"]
        del calls[:]
        # without the flag: today's path, the host's RGB decode
        off = imaginary.process_bytes(buf, dict(opts), **flags)
        assert off.body == want.body and "decode" in calls
        del calls[:]
        monkeypatch.setattr(codec, "decode", real_decode)
        monkeypatch.setattr(codec, "decode_jpeg_coefs", real_coefs)
