"""k_smartcrop_score pinned by its one observable, the crop origin.

Every comparison is an exact (left, top) against the CPU oracle; where the float64
reference of tests/smartcrop_ref.py decides (gap > M) the origin is compared with the
reference too, so a misreading shared by oracle and kernel cannot pass.  The inputs are
the sets tests/test_smartcrop_cpu.py shows to be sensitive: exact ties (the argmax's
"first in raster order" rule, within a thread, across the lanes of a wave and across
the four waves), ties decided by one float rounding, origins clipped at each side, full
width / height and one-pixel crops, every resize route under both sampling conventions,
RGBA, the refusals, and per-image device origins inside a batched plan.
"""
import numpy as np
import pytest

from footprint import guarded  # noqa: F401
import smartcrop_ref as ref
from smartcrop_ref import M
from test_configs_gpu import structured_img

pytestmark = pytest.mark.gpu


def _check(gpu, oracle, imgs, cw, ch, what, rgb=None):
    """One batched call; each origin against the oracle's (on `rgb[i]` if given: the
    3-band twin of a 4-band image) and, where it decides, the reference's."""
    imgs = np.ascontiguousarray(imgs)
    got = gpu.smartcrop_origins(imgs, cw, ch)
    assert got.shape == (len(imgs), 2)
    decided = 0
    for i, img in enumerate(imgs):
        g = (int(got[i][0]), int(got[i][1]))
        want = oracle.smartcrop_origin(img, cw, ch)
        assert g == want, f"{what} img{i} crop {cw}x{ch}: engine {g}, oracle {want}"
        if rgb is not None:
            want3 = oracle.smartcrop_origin(rgb[i], cw, ch)
            assert g == want3, f"{what} img{i} crop {cw}x{ch}: engine on 4 bands {g}, oracle on 3 bands {want3}"
        r, gp = ref.reference_origin(oracle, img, cw, ch)
        if gp > M:
            decided += 1
            assert g == r, f"{what} img{i} crop {cw}x{ch}: engine {g}, reference {r} at gap {gp}"
    return got, decided


# ---------------------------------------------------------------- ties and near-ties
@pytest.mark.parametrize("name", list(ref.TIE_SETS))
def test_ties(gpu, oracle, name):
    cases = ref.tie_set(name)
    for (cw, ch), idx in ref.by_crop(cases).items():
        _check(gpu, oracle, np.stack([cases[k][0] for k in idx]), cw, ch, f"{name} twins {idx[0]}..")


def test_regression_transposed_twin_161(gpu, oracle):
    """Transposed twin 161 at crop 2 x 2: the two peaks are the same float in libvips'
    pipeline, so the earlier one, at (10, 8), wins and the origin is (9, 7).  With the
    cube-root look-up built by cbrtf (one ulp off in 11,553 entries) the engine's two peaks
    differed and it returned the later twin's origin, (7, 22)."""
    img, (cw, ch) = ref.tie_set("transposed")[161]
    assert (cw, ch) == (2, 2) and oracle.smartcrop_origin(img, cw, ch) == (9, 7)
    got, _ = _check(gpu, oracle, img[None], cw, ch, "transposed twin 161")
    assert tuple(got[0]) == (9, 7)


def test_constants_and_mixed_batch(gpu, oracle):
    consts = [ref.constant(v) for v in (0, 128, 255)]
    mixed = [consts[0], ref.tie_set("transposed")[3][0], ref.tie_set("periodic")[0][0], consts[2],
             ref.tie_set("translated")[0][0], ref.tie_set("perturbed")[5][0], consts[1],
             ref.tie_set("transposed")[42][0]]
    for cw, ch in ((2, 2), (5, 3), (12, 11)):
        got, _ = _check(gpu, oracle, np.stack(consts), cw, ch, "constants")
        assert not got.any()
        _check(gpu, oracle, np.stack(mixed), cw, ch, "mixed")


# ---------------------------------------------------------------- geometry
def test_origins_clip_at_each_side(gpu, oracle):
    corners = ref.corner_features()
    for cw, ch in ref.CORNER_CROPS:
        got, decided = _check(gpu, oracle, np.stack(list(corners.values())), cw, ch, "corners")
        assert decided == len(corners)
        for (name, _), (left, top) in zip(corners.items(), got):
            parts = name.split("_")
            assert ("left" not in parts or left == 0) and ("right" not in parts or left == 32 - cw), (name, left)
            assert ("top" not in parts or top == 0) and ("bottom" not in parts or top == 32 - ch), (name, top)


@pytest.mark.parametrize("cw,ch", [(32, 5), (7, 32), (32, 32), (1, 1), (2, 2), (3, 3), (31, 17), (6, 9)])
def test_full_width_height_and_tiny_crops(gpu, oracle, cw, ch):
    rng = np.random.default_rng(ref.SEED + 11)
    corners = ref.corner_features()
    imgs = [ref.uniform_noise(rng), ref.jittered_blocks(rng), corners["bottom_right"], corners["top"],
            ref.tie_set("translated")[7][0], ref.low_contrast_noise(rng), ref.feature_at(rng, 13, 17)]
    got, _ = _check(gpu, oracle, np.stack(imgs), cw, ch, "32 px")
    if cw == 32:
        assert not got[:, 0].any()
    if ch == 32:
        assert not got[:, 1].any()
    # the same on a resized route: cw == w, ch == h scaled to 64 x 48
    big = np.stack([ref.enlarge(im, 64, 48) for im in imgs[:3]])
    _check(gpu, oracle, big, cw * 2 if cw > 1 else 1, max(1, ch * 3 // 2), "64 x 48")


# ---------------------------------------------------------------- resize routes
@pytest.mark.parametrize("w,h", ref.ROUTES)
def test_resize_routes(gpu, oracle, convention, w, h):
    decided = 0
    for imgs, (cw, ch) in ref.route_batches(w, h, structured_img):
        decided += _check(gpu, oracle, imgs, cw, ch, f"{w}x{h} {convention}")[1]
    assert decided >= 2, f"{w}x{h}: the reference decides {decided} of 6"


# ---------------------------------------------------------------- RGBA
@pytest.mark.parametrize("w,h", ref.ROUTES)
def test_rgba_routes(gpu, oracle, w, h):
    rng = np.random.default_rng(ref.SEED + 13 + w)
    for imgs, (cw, ch) in ref.route_batches(w, h, structured_img):
        _check(gpu, oracle, ref.with_alpha(rng, imgs), cw, ch, f"{w}x{h} rgba", rgb=imgs)


def test_rgba_transposed_twins(gpu, oracle):
    rng = np.random.default_rng(ref.SEED + 14)
    cases = ref.tie_set("transposed")
    for (cw, ch), idx in ref.by_crop(cases).items():
        imgs = np.stack([cases[k][0] for k in idx])
        _check(gpu, oracle, ref.with_alpha(rng, imgs), cw, ch, "transposed twins rgba", rgb=imgs)


# ---------------------------------------------------------------- refusals
def _refused(gpu, x, cw, ch):
    """mipx_op_smartcrop_origin on guarded buffers: (code, origins payload); the guards of
    every buffer are checked."""
    from imaginary_amd import engine
    what = "mipx_op_smartcrop_origin"
    n, h, w, b = x.shape
    wsb = max(16, gpu.lib.mipx_op_workspace_bytes(7, n, w, h, b, max(cw, 1), max(ch, 1)))
    din = engine.GuardedBuffer(x.nbytes, 0xA5, w * b, 0, "in", what).upload(x)
    org = engine.GuardedBuffer(8 * n, 0xA5, 0, 0, "origins", what)
    ws = engine.GuardedBuffer(wsb, 0xA5, 0, 0, "ws", what)
    code = gpu.lib.mipx_op_smartcrop_origin(din.ptr, org.ptr, n, w, h, b, cw, ch, ws.ptr, wsb, None)
    engine.synchronize()
    for buf in (din, org, ws):
        buf.check()
    got, scratch = org.download(8 * n), ws.download(wsb)
    for buf in (din, org, ws):
        buf.close()
    assert np.all(scratch == 0xA5), f"{w}x{h} crop {cw}x{ch}: workspace written by a refused call"
    return code, got


@pytest.mark.parametrize("w,h,cw,ch,code", [
    (31, 64, 8, 8, "MIPX_EUNSUPPORTED"), (64, 31, 8, 8, "MIPX_EUNSUPPORTED"),
    (40, 50, 41, 10, "MIPX_EINVAL"), (40, 50, 10, 51, "MIPX_EINVAL"), (40, 50, 0, 10, "MIPX_EINVAL"),
    (40, 50, 10, 0, "MIPX_EINVAL"), (40, 50, -3, 10, "MIPX_EINVAL")])
def test_refusals(gpu, oracle, w, h, cw, ch, code):
    x = np.random.default_rng(ref.SEED + w).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    with pytest.raises(oracle.OracleError) as e:
        oracle.smartcrop_origin(x[0], cw, ch)
    assert e.value.code == {"MIPX_EUNSUPPORTED": -2, "MIPX_EINVAL": -1}[code]      # REF_EUNSUPPORTED / REF_EINVAL
    got_code, origins = _refused(gpu, x, cw, ch)
    assert got_code == getattr(gpu, code), (got_code, code)
    assert np.all(origins == 0xA5), "origins written by a refused call"
    with pytest.raises(gpu.MipxError) as ge:
        gpu.smartcrop_origins(x, cw, ch)
    assert ge.value.code == getattr(gpu, code)


# ---------------------------------------------------------------- plans
def _plans(gpu, oracle, w, h, bands, ow, oh):
    opts = dict(width=ow, height=oh, crop=1, gravity=5)
    p = gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, bands, "png", 0))
    e, rp = oracle.plan(opts, dict(w=w, h=h, bands=bands, type=3))
    assert e == 0
    ops = [s[0] for s in p.describe()]
    assert ops.count("smartcrop") == 1 and (p.out_w, p.out_h) == (ow, oh), ops
    head = type(rp).from_buffer_copy(rp)       # the oracle's plan up to the smartcrop step
    head.n_steps = ops.index("smartcrop")
    return p, rp, head


def _plan_origins(oracle, head, imgs, ow, oh):
    out = []
    for img in imgs:
        pre = oracle.execute(head, img)
        out.append(oracle.smartcrop_origin(pre, ow, oh))
        r, g = ref.reference_origin(oracle, pre, ow, oh)
        assert g <= M or r == out[-1], (r, out[-1], g)
    return out


def _same_images(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(d)} bytes differ, first at {d[0].tolist()}")


@pytest.mark.parametrize("bands", [3, 4])
@pytest.mark.parametrize("w,h,ow,oh", [(200, 150, 64, 64), (96, 160, 40, 40)])
def test_plan_origins_per_image(gpu, oracle, w, h, ow, oh, bands):
    """A smartcrop plan on a batch: every image is cut at its own device origin."""
    rng = np.random.default_rng(ref.SEED + 17 + w + bands)
    p, rp, head = _plans(gpu, oracle, w, h, bands, ow, oh)
    places = ((24, 5), (17, 12), (11, 17), (4, 24))
    imgs = np.stack([ref.enlarge(ref.feature_at(rng, y, x), w, h) for y, x in places])
    twins = np.stack([ref.enlarge(ref.transposed_twins(rng, k), w, h) for k in range(4)])
    if bands == 4:
        imgs, twins = ref.with_alpha(rng, imgs), ref.with_alpha(rng, twins)
    origins = _plan_origins(oracle, head, imgs, ow, oh)
    assert len(set(origins)) == len(origins), f"the batch's origins do not all differ: {origins}"
    _plan_origins(oracle, head, twins, ow, oh)
    for batch, what in ((imgs, "features"), (twins, "transposed twins")):
        got = gpu.execute(p, batch)
        assert len(got) == len(batch)
        for i in range(len(batch)):
            _same_images(got[i], oracle.execute(rp, batch[i]), f"{w}x{h}x{bands} -> {ow}x{oh} {what} img{i}")
