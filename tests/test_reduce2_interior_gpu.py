"""k_reduce2x2 on the tiles that touch no image edge (reduce2_tile_interior of
csrc/reduce2_geom.h) and on their neighbours, against the oracle, byte for byte, at the corner
sampling convention.  The kernel computes both kinds with one body today (a straight-line body
for the interior ones measured no faster, profiles/r18); these shapes are where such a body and
the general one would meet.

A tile is interior when its 24 rows need no input row outside the image (band 1 of an h-row image
needs row 99, so h >= 100), its strip no pixel outside it (strip 1 needs pixel 643 RGB / 483 RGBA)
and every store of the walk is a whole aligned item (ow * 3 a multiple of 4, ow * 4 of 8).  The
shapes are the smallest that put an interior tile beside each kind of tile that is not; the
existing small shapes (tests/test_reduce2_hpass_gpu.py) hold none.  tests/test_reduce2_geom_host.py
pins the number of interior tiles of each shape here.

  648 x 100 x 3   one interior tile (strip 1, band 1), dword-aligned output pitch
  644 x 100 x 3   the same tile but ow * 3 = 966: its stores start off a dword
  648 x 99 x 3    one input row short of interior
  642 x 100 x 3   one pixel short; its rows are not dword aligned, so the generic reduce runs it
  640 x 100 x 3   the nearest narrower width k_reduce2x2 takes: strip 1 replicates its right edge
  484 x 100 x 4   RGBA, one interior tile; 482 x 100 and 484 x 99 are one short of it
  1288 x 200 x 3  3 x 3 interior tiles inside a frame of edge and partial tiles (968 x 200 x 4 in
                  the window test)

Every batch holds 3 images, so the last image ends at the end of the guard-banded buffers
(footprint.py)."""
import ctypes as C

import numpy as np
import pytest

from footprint import FILL, guarded  # noqa: F401

pytestmark = pytest.mark.gpu

SHAPES = {
    3: [(648, 100), (644, 100), (648, 99), (642, 100), (640, 100), (1288, 200)],
    4: [(484, 100), (482, 100), (484, 99)],
}
CASES = [(b, w, h) for b in (3, 4) for w, h in SHAPES[b]]
N = 3


@pytest.fixture(scope="module")
def corner(gpu, oracle):
    prev_engine, prev_oracle = gpu.reduce_sampling(), oracle.get_switch("reduce_centre")
    gpu.set_reduce_sampling("corner")
    oracle.set_switch("reduce_centre", 0)
    yield
    gpu.set_reduce_sampling(prev_engine)
    oracle.set_switch("reduce_centre", prev_oracle)


_batches = {}


def _batch(oracle, w, h, b):
    """[(kind, images (3, h, w, b), oracle outputs)], computed once per shape; read-only."""
    key = (w, h, b)
    if key not in _batches:
        r = np.random.default_rng(9000 * w + 10 * h + b)
        checker = ((np.indices((h, w)).sum(0) % 2) * 255).astype(np.uint8)[..., None].repeat(b, 2)
        out = []
        for kind, imgs in (("random", r.integers(0, 256, (N, h, w, b), dtype=np.uint8)),
                           ("zeros", np.zeros((N, h, w, b), np.uint8)),
                           ("255", np.full((N, h, w, b), 255, np.uint8)),
                           ("checker", np.stack([checker] * N))):
            if kind == "random":
                want = np.stack([oracle.reduce(imgs[i], 2.0, 2.0) for i in range(N)])
            else:
                want = np.stack([oracle.reduce(imgs[0], 2.0, 2.0)] * N)
            imgs.setflags(write=False)
            want.setflags(write=False)
            out.append((kind, imgs, want))
        _batches[key] = out
    return _batches[key]


@pytest.mark.parametrize("b,w,h", CASES, ids=[f"{w}x{h}x{b}" for b, w, h in CASES])
def test_interior_and_its_neighbours_exact(gpu, oracle, corner, b, w, h):
    for kind, imgs, want in _batch(oracle, w, h, b):
        got = gpu.run_op("reduce", imgs, hshrink=2.0, vshrink=2.0)
        assert got.shape == want.shape, (kind, got.shape, want.shape)
        d = np.argwhere(got != want)
        assert len(d) == 0, (f"{w}x{h}x{b} {kind}: {len(d)} bytes differ, first at "
                             f"{d[0].tolist()} got {got[tuple(d[0])]} want {want[tuple(d[0])]}")


# mipx::reduce2_window_launch(in, out, n, w, h, b, x0, y0, x1, y1, stream), by its C++ name
_WINDOW_LAUNCH = "_ZN4mipx21reduce2_window_launchEPKhPhiiiiiiiiP12ihipStream_t"
_STRIP = {3: 160, 4: 120}   # output pixels per strip (Reduce2Geom<B>::TW, reduce2_geom.h)
_ITEM = {3: 4, 4: 2}        # output pixels per horizontal item: a window's right edge rounds to it
_SIZE = {3: (1288, 200), 4: (968, 200)}   # interior strips 1..3, interior bands 1..3 (rows 24..95)

# (x0, y0, x1, y1) per band count; None = the image's edge
WINDOWS = {
    # bands start at rows 12, 36, 60, 84: off the full launch's 24-row grid, bands 0..2 interior
    "y0_12": {3: (0, 12, None, None), 4: (0, 12, None, None)},
    # x1 ends inside strip 2, which would be interior: its tile clips items, strip 1's does not
    "x1_inside": {3: (0, 0, 402, None), 4: (0, 0, 301, None)},
    # wholly inside interior tiles: strips 1..2, rows 24..71
    "inside": {3: (160, 24, 480, 72), 4: (120, 24, 360, 72)},
}


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("window", list(WINDOWS))
def test_demand_windows_exact_and_nothing_else_written(gpu, oracle, corner, b, window):
    """As the window test of tests/test_reduce2_hpass_gpu.py: the launcher computes the window
    rounded out to whole strips on the left, to a multiple of 12 rows at the top and to a whole
    item on the right, and clips exactly at the bottom; every byte it computes equals the oracle
    and every other byte of the output keeps the poison, guard bands included."""
    from imaginary_amd._abi import check, sync_tuning
    from imaginary_amd.engine import GuardedBuffer
    w, h = _SIZE[b]
    ow, oh = w // 2, h // 2
    x0, y0, x1, y1 = WINDOWS[window][b]
    x1 = ow if x1 is None else x1
    y1 = oh if y1 is None else y1
    _kind, imgs, want = _batch(oracle, w, h, b)[0]
    fn = getattr(gpu.lib, _WINDOW_LAUNCH)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int] * 8 + [C.c_void_p]
    sync_tuning()
    din = GuardedBuffer(imgs.nbytes, FILL, w * b, name="in").upload(imgs)
    dout = GuardedBuffer(N * oh * ow * b, FILL, ow * b, name="out")
    try:
        check(fn(din.ptr, dout.ptr, N, w, h, b, x0, y0, x1, y1, None), "reduce2_window_launch")
        check(gpu.lib.mipx_device_sync(), "mipx_device_sync")
        got = dout.download((N, oh, ow, b))
        din.check("window")
        dout.check("window")
    finally:
        din.close()
        dout.close()
    assert y0 % 12 == 0
    xl = x0 // _STRIP[b] * _STRIP[b]
    xr = min(-(-x1 // _ITEM[b]) * _ITEM[b], ow)
    assert np.array_equal(got[:, y0:y1, xl:xr], want[:, y0:y1, xl:xr]), f"{window} x{b}"
    outside = np.ones(got.shape, bool)
    outside[:, y0:y1, xl:xr] = False
    assert np.all(got[outside] == FILL), f"{window} x{b}: wrote outside the window"
