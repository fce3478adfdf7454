"""What a kernel does OUTSIDE its buffers, where the guard mode inherited by the other
GPU modules (tests/footprint.py) cannot reach:

 a. the detector itself detects (one stray byte right before / right after a payload);
 b. every op at the smallest shapes whose row ends and image ends fall off the 4- and
    16-byte grids, under two complementary fills (0xA5 / 0x5A): both outputs equal the
    oracle byte for byte and every guard is clean, so no out-of-payload byte reaches a
    result and no unwritten output byte hides behind a coincidence with the fill;
 c. input and output base pointers 1-3 bytes off a dword (include/mipx.h: any alignment,
    except rot / embed of 4-band images, which must refuse with MIPX_EINVAL);
 d. a workspace of exactly the advertised size is enough, one byte less is refused
    before anything is launched;
 e. the request path writes only the caller's output view.

Every deliberate stray byte in (a) lies inside the test's own allocation.
"""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from footprint import guarded  # noqa: F401

pytestmark = pytest.mark.gpu

FILLS = (0xA5, 0x5A)
SHAPES = [(1, 1), (1, 7), (2, 5), (3, 23), (17, 21), (16, 64), (33, 67), (9, 130)]
NS = (1, 3)
BG = (200, 17, 90)
WM_PAIRS = [(3, 3), (3, 4), (4, 4), (4, 3), (1, 2), (2, 2)]   # test_watermark_matches_oracle's


def _round(v):  # vips rounding of a positive size
    return int(math.floor(v + 0.5))


def rejected(op, p, h, w, b):
    """The explicit rule for a geometry the op itself refuses (libvips' size rules, as
    the oracle applies them); None when the case runs."""
    if op in ("reduce", "reducev", "reduceh"):
        hs, vs = p.get("hshrink", 1.0), p.get("vshrink", 1.0)
        if (hs != 1.0 and _round(w / hs) < 1) or (vs != 1.0 and _round(h / vs) < 1):
            return "reduce would make an empty image"
    if op == "extract" and w < 2:
        return "no window with an odd left in a one-pixel row"
    return None


def resolve(op, p, h, w, b):
    """run_op keyword arguments of a case: the parameters that depend on the shape."""
    if op == "extract":
        # left odd; a window whose rows are off a dword where the band count allows one
        ow = next((c for c in (w - 1, w - 2, w - 3) if c >= 1 and (c * b) % 4), w - 1)
        top = 1 if h > 1 else 0
        return dict(left=1, top=top, width=ow, height=h - top)
    if op == "embed":  # negative origin, larger canvas: border on every side the mode fills
        return dict(x=-2, y=-1, width=w + 7, height=h + 4, extend=p["extend"], background=(12, 200, 77))
    if op == "watermark":  # the mark touches the right and bottom edges
        mh, mw = (h + 1) // 2, (w + 1) // 2
        wm = np.random.default_rng(h * 131 + w).integers(0, 256, (mh, mw, p["wb"]), dtype=np.uint8)
        return dict(wm=wm, left=w - mw, top=h - mh, opacity=0.5)
    return dict(p)


def oracle_op(oracle, op, kw, img):
    if op == "reduce":
        return oracle.reduce(img, kw["hshrink"], kw["vshrink"])
    if op == "reducev":
        return oracle.reducev(img, kw["vshrink"])
    if op == "reduceh":
        return oracle.reduceh(img, kw["hshrink"])
    if op == "shrink":
        return oracle.shrink(img, kw["hshrink"], kw["vshrink"])
    if op == "gaussblur":
        return oracle.gaussblur(img, kw["sigma"], kw["min_ampl"])
    if op == "embed":
        return oracle.embed(img, kw["x"], kw["y"], kw["width"], kw["height"], kw["extend"], kw["background"])
    if op == "extract":
        return oracle.extract(img, kw["left"], kw["top"], kw["width"], kw["height"])
    if op == "rot":
        return oracle.rot(img, kw["angle"])
    if op == "flip":
        return oracle.flip(img, kw["vertical"])
    if op == "zoom":
        return oracle.zoom(img, kw["xfac"], kw["yfac"])
    if op == "flatten":
        return oracle.flatten(img, kw["background"])
    if op == "bw":
        return oracle.bw(img)
    if op == "watermark":
        return oracle.watermark(img, kw["wm"], kw["left"], kw["top"], kw["opacity"])
    if op == "affine":
        return oracle.affine(img, kw["xscale"], kw["yscale"], kw["extend"])
    raise ValueError(op)


# ---------------------------------------------------------------- (b) the case list
GENERATED = 0
SKIPPED = 0


def _group(op, p, bands, shapes=None, ns=NS):
    """One pytest case per (op, parameters, band count): every shape x batch size the op
    accepts.  Counts what the rule in rejected() leaves out."""
    global GENERATED, SKIPPED
    out = []
    for b in bands:
        cases = []
        for (h, w) in (shapes or SHAPES):
            for n in ns:
                GENERATED += 1
                if rejected(op, p, h, w, b):
                    SKIPPED += 1
                    continue
                cases.append((h, w, b, n))
        if cases:
            tag = ",".join(f"{k}={v}" for k, v in p.items())
            out.append(pytest.param(op, p, cases, id=f"{op}[{tag}]-b{b}"))
    return out


ALL = (1, 2, 3, 4)
REDUCE_GROUPS = []
for _hs, _vs in ((2.0, 2.0), (1.6, 1.6), (1.0, 2.5), (2.5, 1.0), (3.7, 1.2)):
    REDUCE_GROUPS += _group("reduce", dict(hshrink=_hs, vshrink=_vs), ALL)
# the fused 2 x 2 kernels' smallest sizes
REDUCE_GROUPS += _group("reduce", dict(hshrink=2.0, vshrink=2.0), (4,), shapes=[(8, 8)])
REDUCE_GROUPS += _group("reduce", dict(hshrink=2.0, vshrink=2.0), (3,), shapes=[(9, 12)])
# k_rcol's specialised and generic builds; the gather fallback of the horizontal pass
REDUCE_GROUPS += _group("reduce", dict(hshrink=1.6, vshrink=1.6), (3,), shapes=[(37, 1028)])
REDUCE_GROUPS += _group("reduce", dict(hshrink=1.6, vshrink=1.6), (4,), shapes=[(19, 333)])
REDUCE_GROUPS += _group("reduce", dict(hshrink=20.0, vshrink=3.0), (4,), shapes=[(40, 700)])

OP_GROUPS = []
for _s in (1.6, 3.3):
    OP_GROUPS += _group("reducev", dict(vshrink=_s), ALL)
    OP_GROUPS += _group("reduceh", dict(hshrink=_s), ALL)
for _hs, _vs in ((2, 2), (3, 5), (4, 4), (7, 7), (9, 2)):
    OP_GROUPS += _group("shrink", dict(hshrink=_hs, vshrink=_vs), ALL)
for _sigma in (0.3, 1.0, 5.0, 12.5):
    OP_GROUPS += _group("gaussblur", dict(sigma=_sigma, min_ampl=0.2), ALL)
for _e in range(7):
    OP_GROUPS += _group("embed", dict(extend=_e), ALL)
OP_GROUPS += _group("extract", dict(), ALL)
for _a in (90, 180, 270):
    OP_GROUPS += _group("rot", dict(angle=_a), ALL)
    OP_GROUPS += _group("rot", dict(angle=_a), (4,), shapes=[(64, 96)])   # the tiled rotates
    OP_GROUPS += _group("rot", dict(angle=_a), (2,), shapes=[(70, 71)])
for _v in (0, 1):
    OP_GROUPS += _group("flip", dict(vertical=_v), ALL)
OP_GROUPS += _group("zoom", dict(xfac=2, yfac=3), ALL)
OP_GROUPS += _group("flatten", dict(background=BG), ALL)
OP_GROUPS += _group("bw", dict(), ALL)
for _bb, _wb in WM_PAIRS:
    OP_GROUPS += _group("watermark", dict(wb=_wb), (_bb,))
for _scale in (2.0, 3.004291845493562):
    for _e in (0, 1, 4):
        OP_GROUPS += _group("affine", dict(xscale=_scale, yscale=_scale, extend=_e), ALL)

# at most 10 % of the generated cases may fall to the rule in rejected()
assert GENERATED > 2000 and SKIPPED * 10 <= GENERATED, (SKIPPED, GENERATED)


@functools.lru_cache(maxsize=None)
def _inputs(h, w, b, n):
    a = np.random.default_rng(((h * 1009 + w) * 5 + b) * 7 + n).integers(0, 256, (n, h, w, b), dtype=np.uint8)
    a.setflags(write=False)
    return a


_WANT = {}


def _want(oracle, key, op, kw, imgs):
    """The oracle's result of a case, computed once and shared (read-only)."""
    if key not in _WANT:
        r = np.stack([oracle_op(oracle, op, kw, im) for im in imgs])
        r.setflags(write=False)
        _WANT[key] = r
    return _WANT[key]


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(d)} bytes differ, first at {d[0].tolist()} "
                             f"got {got[tuple(d[0])]} want {want[tuple(d[0])]}")


def _engine():
    from imaginary_amd import engine
    return engine


def _under_fills(call, what, skew_in=0, skew_out=0):
    """call() under each fill (guards checked inside run_op / execute / smartcrop_origins);
    the two results must be the same bytes."""
    engine = _engine()
    outs = []
    for fill in FILLS:
        prev = engine.set_guard(fill, skew_in, skew_out)
        try:
            before = engine.guarded_calls()
            outs.append(call())
            assert engine.guarded_calls() > before, f"{what}: the guard was not live"
        finally:
            engine.set_guard(*prev)
    _same(outs[1], outs[0], f"{what}: fill 0x5A against fill 0xA5")
    return outs[0]


def needs_aligned_pointers(op, b):
    """include/mipx.h: rot and embed of 4-band images take dword-aligned image pointers
    only and refuse others with MIPX_EINVAL (so does flip, above 2 GiB or 65535 rows)."""
    return b == 4 and op in ("rot", "embed")


def _run_cases(gpu, oracle, op, p, cases, tag="", skew_in=0, skew_out=0):
    for h, w, b, n in cases:
        imgs = _inputs(h, w, b, n)
        kw = resolve(op, p, h, w, b)
        what = f"{op} {p} {n}x{h}x{w}x{b} {tag}".strip()
        if (skew_in % 4 or skew_out % 4) and needs_aligned_pointers(op, b):
            prev = _engine().set_guard(FILLS[0], skew_in, skew_out)
            try:
                with pytest.raises(gpu.MipxError) as e:   # refused with an error code, never wrong bytes
                    gpu.run_op(op, imgs, **kw)
            finally:
                _engine().set_guard(*prev)
            assert e.value.code == gpu.MIPX_EINVAL, f"{what}: {e.value}"
            continue
        got = _under_fills(lambda: gpu.run_op(op, imgs, **kw), what, skew_in, skew_out)
        key = (op, tuple(sorted((k, str(v)) for k, v in p.items())), h, w, b, n, tag if op == "reduce" else "")
        _same(got, _want(oracle, key, op, kw, imgs), what)


@pytest.mark.parametrize("op,p,cases", REDUCE_GROUPS)
def test_reduce_footprint(gpu, oracle, convention, op, p, cases):
    _run_cases(gpu, oracle, op, p, cases, tag=convention)


@pytest.mark.parametrize("op,p,cases", OP_GROUPS)
def test_op_footprint(gpu, oracle, op, p, cases):
    _run_cases(gpu, oracle, op, p, cases)


def test_affine_enlm_footprint(gpu, oracle, monkeypatch):
    """k_enlm at its smallest accepted tile (a 1 x 1 RGBA image at 2 x; MIPX_ENLM=2 makes
    anything but k_enlm an error), and a shape it declines (1.2 x 1.1: too close to 1)
    on the kernels behind it."""
    monkeypatch.setenv("MIPX_ENLM", "2")
    _run_cases(gpu, oracle, "affine", dict(xscale=2.0, yscale=2.0, extend=1), [(1, 1, 4, 1), (1, 1, 4, 3)], tag="enlm")
    monkeypatch.delenv("MIPX_ENLM")
    _run_cases(gpu, oracle, "affine", dict(xscale=1.2, yscale=1.1, extend=1), [(40, 50, 3, 1), (40, 50, 3, 3)])


def test_smartcrop_footprint(gpu, oracle):
    h, w, cw, ch = 240, 180, 100, 100
    r = np.random.default_rng(5)
    y, x = np.mgrid[0:h, 0:w]
    smooth = np.stack([(127.5 + 127.5 * np.sin(x * 0.05 + c) * np.cos(y * 0.08 - c)).astype(np.uint8)
                       for c in range(3)], -1)
    imgs = np.stack([smooth, r.integers(0, 256, (h, w, 3), dtype=np.uint8), smooth[::-1, ::-1]])
    got = _under_fills(lambda: gpu.smartcrop_origins(imgs, cw, ch), "smartcrop")
    for i in range(3):
        assert tuple(got[i]) == oracle.smartcrop_origin(imgs[i], cw, ch), f"smartcrop img{i}"


# ---------------------------------------------------------------- (a) the detector detects
@pytest.mark.parametrize("where", ["after", "before"])
def test_detector_reports_one_stray_byte(gpu, where):
    engine = _engine()
    nbytes = 3 * 23 * 3
    buf = engine.GuardedBuffer(nbytes, 0xA5, row_bytes=23 * 3, skew=0, name="out", op="mipx_op_probe")
    assert buf.guard == 4096 and buf.damage() is None
    buf.check()
    off = nbytes if where == "after" else -1
    engine.check(gpu.lib.mipx_memset_dev(buf.ptr + off, 0x3C, 1), "mipx_memset_dev")  # inside buf's own allocation
    gpu.synchronize()
    assert buf.damage() == (off, off, 1)
    with pytest.raises(AssertionError) as e:
        buf.check()
    msg = str(e.value)
    assert "'out'" in msg and "mipx_op_probe" in msg and "1 byte(s)" in msg, msg
    assert f"first at payload offset {off}, last at {off} " in msg, msg
    buf.close()


def test_guard_is_live_in_this_suite(gpu):
    """The autouse fixture switched the guard on, and a run_op advances the call counter:
    a green run of the modules that import it did check footprints."""
    engine = _engine()
    assert engine.guard_setting() == (0xA5, 0, 0)
    before = engine.guarded_calls()
    gpu.run_op("rot", _inputs(3, 23, 3, 1), angle=90)
    assert engine.guarded_calls() == before + 1 > 0


# ---------------------------------------------------------------- (c) skewed base pointers
SKEWS = [(i, o) for i in range(4) for o in range(4) if (i, o) != (0, 0)]
SKEW_CASES = [(17, 21, 3, 2), (16, 64, 4, 2), (33, 67, 1, 2)]
SKEW_OPS = [("reduce", dict(hshrink=2.0, vshrink=2.0)), ("reduce", dict(hshrink=1.6, vshrink=1.6)),
            ("shrink", dict(hshrink=2, vshrink=2)), ("gaussblur", dict(sigma=1.0, min_ampl=0.2)),
            ("rot", dict(angle=90)), ("extract", dict()), ("embed", dict(extend=1)),
            ("affine", dict(xscale=2.0, yscale=2.0, extend=1)), ("bw", dict())]


@pytest.mark.parametrize("skew_in,skew_out", SKEWS)
@pytest.mark.parametrize("op,p", SKEW_OPS, ids=[f"{o}{i}" for i, (o, _) in enumerate(SKEW_OPS)])
def test_skewed_base_pointers(gpu, oracle, op, p, skew_in, skew_out):
    """Input and output bases 1-3 bytes off a dword, independently: the oracle's bytes and
    clean guards, or (4-band rot / embed, as include/mipx.h states) MIPX_EINVAL."""
    assert gpu.reduce_sampling() == "corner" and oracle.get_switch("reduce_centre") == 0
    _run_cases(gpu, oracle, op, p, SKEW_CASES, tag="corner", skew_in=skew_in, skew_out=skew_out)


# ---------------------------------------------------------------- (d) workspace honesty
def _guarded_call(what, x, onb, wsb, call, short, out_name):
    """One direct entry-point call on guarded buffers: call(din, dout, ws_ptr, ws_bytes) -> code,
    with the advertised workspace (short=0) or one a byte smaller (short=1).  Returns
    (code, output payload); every guard is checked."""
    engine = _engine()
    fill = 0xA5
    n, h, w, b = x.shape
    din = engine.GuardedBuffer(x.nbytes, fill, w * b, 0, "in", what).upload(x)
    dout = engine.GuardedBuffer(onb, fill, 0, 0, out_name, what)
    ws = engine.GuardedBuffer(wsb - short, fill, 0, 0, "ws", what)
    code = call(din, dout, ws.ptr, wsb - short)
    engine.synchronize()
    for buf in (din, dout, ws):
        buf.check()
    got = dout.download(onb)
    for buf in (din, dout, ws):
        buf.close()
    return code, got


def _honest(what, x, wsb, call, want, out_name="out"):
    assert wsb > 1, f"{what}: the case needs a workspace"
    want = np.ascontiguousarray(want)
    code, got = _guarded_call(what, x, want.nbytes, wsb, call, 0, out_name)
    assert code == 0, f"{what}: the advertised workspace ({wsb} bytes) was refused: {code}"
    _same(got, want.view(np.uint8).ravel(), what)
    code, got = _guarded_call(what, x, want.nbytes, wsb, call, 1, out_name)
    assert code < 0, f"{what}: a workspace of {wsb - 1} bytes ({wsb} advertised) was accepted"
    assert np.all(got == 0xA5), f"{what}: output written although the workspace was refused"


def test_workspace_honesty_reduce(gpu, oracle, monkeypatch):
    """mipx_op_reduce on the route that uses its workspace (the two separable passes; the
    one-launch kernels need none and are switched off)."""
    from imaginary_amd._abi import sync_tuning
    for k in ("MIPX_RCOL", "MIPX_RMFMA", "MIPX_RSTRIP", "MIPX_FUSED_REDUCE"):
        monkeypatch.setenv(k, "0")
    sync_tuning()
    n, h, w, b, hs, vs = 3, 33, 67, 3, 1.6, 2.4
    x = _inputs(h, w, b, n)
    want = np.stack([oracle.reduce(im, hs, vs) for im in x])
    wsb = gpu.lib.mipx_op_workspace_bytes(4, n, w, h, b, hs, vs)
    _honest("mipx_op_reduce", x, wsb,
            lambda i, o, wp, wb: gpu.lib.mipx_op_reduce(i.ptr, o.ptr, n, w, h, b, hs, vs, wp, wb, None), want)


def test_workspace_honesty_gaussblur(gpu, oracle, monkeypatch):
    """mipx_op_gaussblur on the route that uses its workspace (the two separable passes)."""
    from imaginary_amd._abi import sync_tuning
    for k in ("MIPX_BCOL", "MIPX_BLUR2D"):
        monkeypatch.setenv(k, "0")
    sync_tuning()
    n, h, w, b, sigma = 3, 33, 67, 3, 2.2
    x = _inputs(h, w, b, n)
    want = np.stack([oracle.gaussblur(im, sigma, 0.2) for im in x])
    wsb = gpu.lib.mipx_op_workspace_bytes(8, n, w, h, b, sigma, 0.2)
    _honest("mipx_op_gaussblur", x, wsb,
            lambda i, o, wp, wb: gpu.lib.mipx_op_gaussblur(i.ptr, o.ptr, n, w, h, b, sigma, 0.2, wp, wb, None), want)


def test_workspace_honesty_smartcrop(gpu, oracle):
    from imaginary_amd._abi import sync_tuning
    sync_tuning()
    n, h, w, b, cw, ch = 2, 120, 90, 3, 50, 50
    x = _inputs(h, w, b, n)
    want = np.array([oracle.smartcrop_origin(im, cw, ch) for im in x], dtype=np.int32)
    wsb = gpu.lib.mipx_op_workspace_bytes(7, n, w, h, b, cw, ch)
    _honest("mipx_op_smartcrop_origin", x, wsb,
            lambda i, o, wp, wb: gpu.lib.mipx_op_smartcrop_origin(i.ptr, o.ptr, n, w, h, b, cw, ch, wp, wb, None),
            want, out_name="origins")


def _chain(gpu, w, h, b, opts2):
    p1 = gpu.plan_make(gpu.make_opts(width=w // 2, embed=1), gpu.make_input(w, h, b, "png"))
    p2 = gpu.plan_make(gpu.make_opts(**opts2), gpu.make_input(p1.out_w, p1.out_h, b, "png"))
    return p1, p2, gpu.plan_chain([p1, p2])


PLAN_CASES = ["chain", "thumbnail+watermark", "window-g0", "window-g3", "enlarge"]


@pytest.mark.parametrize("kind", PLAN_CASES)
def test_workspace_honesty_execute(gpu, oracle, kind):
    """mipx_execute_dev with exactly mipx_workspace_bytes, and with one byte less."""
    from imaginary_amd._abi import sync_tuning
    sync_tuning()
    n, wm = 2, None
    if kind == "chain":        # the C3 chain (2 x 2 resize, then resize) at a small size
        w, h, b = 132, 90, 4
        p1, p2, plan = _chain(gpu, w, h, b, dict(width=40, height=27, embed=1))
        d1, d2 = p1.describe()[0][2], p2.describe()[0][2]
        assert [s[0] for s in p2.describe()] == ["reduce"], p2.describe()
        ref = lambda im: oracle.reduce(oracle.reduce(im, d1[0], d1[1]), d2[0], d2[1])  # noqa: E731
    else:
        if kind == "thumbnail+watermark":
            w, h, b = 100, 75, 3
            opts = dict(width=64, height=48, wm_enable=1, wm_left=4, wm_top=4, wm_opacity=0.5)
            wm = np.random.default_rng(3).integers(0, 256, (32, 32, 4), dtype=np.uint8)
            hdr = dict(wm_w=32, wm_h=32, wm_bands=4)
        elif kind.startswith("window"):
            w, h, b = 120, 101, 3   # reduce -> extract: the reduce computes the crop window only
            opts, hdr = dict(width=63, height=25, crop=1, gravity=int(kind[-1])), {}
        else:
            w, h, b = 50, 40, 3
            opts, hdr = dict(width=100, height=100, enlarge=1, crop=1), {}   # affine 2.5 x, then the crop
        plan = gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, b, "png", **hdr))
        e, rp = oracle.plan(opts, dict(w=w, h=h, bands=b, type=3, **hdr))
        assert e == 0
        ref = lambda im: oracle.execute(rp, im, wm)  # noqa: E731
    x = _inputs(h, w, b, n)
    want = np.stack([ref(im) for im in x])
    assert want.shape == (n, plan.out_h, plan.out_w, plan.out_bands)
    wsb = gpu.lib.mipx_workspace_bytes(C.byref(plan), n)
    engine = _engine()
    dwm = engine.GuardedBuffer(wm.nbytes, 0xA5, 32 * 4, 0, "wm", kind).upload(wm) if wm is not None else None
    _honest(f"mipx_execute_dev {kind}", x, wsb,
            lambda i, o, wp, wb: gpu.lib.mipx_execute_dev(C.byref(plan), n, i.ptr, o.ptr, dwm.ptr if dwm else None,
                                                          wp, wb, None), want)
    if dwm:
        dwm.check()
        dwm.close()


# ---------------------------------------------------------------- (e) host side of the request path
def test_request_path_writes_only_its_output_view(gpu, oracle):
    """mipx_submit / mipx_wait with `out` carved from the middle of a larger host array:
    the bytes around the view stay as they were."""
    opts = dict(width=160, height=120, embed=1)
    img = _inputs(240, 320, 3, 1)[0]
    gpu.lib.mipx_shutdown()  # mipx_init refuses another configuration while one runs
    eng = gpu.Engine(max_batch=8)
    try:
        p = gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(320, 240, 3, "png"))
        e, rp = oracle.plan(opts, dict(w=320, h=240, bands=3, type=3))
        assert e == 0
        nbytes = p.out_h * p.out_w * p.out_bands
        pad = 4096 + 3   # the view starts and ends off every grid
        host = np.full(pad + nbytes + pad, 0x5A, np.uint8)
        view = host[pad:pad + nbytes].reshape(p.out_h, p.out_w, p.out_bands)
        t, out = eng.submit(p, img, out=view)
        eng.wait(t)
        assert out is view
        _same(view, oracle.execute(rp, img), "request path into a view")
        assert np.all(host[:pad] == 0x5A) and np.all(host[pad + nbytes:] == 0x5A), "bytes around the view changed"
    finally:
        eng.shutdown()
