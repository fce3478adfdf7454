"""k_reduce2x2 (k_reduce.hip) against the oracle, byte for byte, at the corner sampling
convention.  A tile is one load burst, one vertical pass over 24 rows, one barrier and one
horizontal pass.

The shapes are the places a 24-row, one-barrier tile can go wrong: a partial chunk,
exactly one chunk (the 12-row vertical pass), 12 rows plus 1 (the 24-row pass with its
second half almost empty), exactly one tile, a second tile of one row, a full tile plus
a partial one, the right edge fill inside a partial tile, and three strips of which one
is interior.  Every batch holds 3 images, so the last image ends at the end of the
guard-banded buffers (footprint.py)."""
import ctypes as C

import numpy as np
import pytest

from footprint import FILL, guarded  # noqa: F401

pytestmark = pytest.mark.gpu

# input (w, h) -> output (w / 2, h / 2)
SHAPES = [(8, 8), (40, 24), (40, 26), (40, 48), (40, 50), (40, 74), (324, 50), (644, 98)]
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
    """[(kind, images (3, h, w, b), oracle outputs)], computed once per shape and shared
    by the tests; read-only."""
    key = (w, h, b)
    if key not in _batches:
        r = np.random.default_rng(1000 * w + 10 * h + b)
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


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_onepass_exact(gpu, oracle, corner, w, h, b):
    for kind, imgs, want in _batch(oracle, w, h, b):
        got = gpu.run_op("reduce", imgs, hshrink=2.0, vshrink=2.0)
        assert got.shape == want.shape, (kind, got.shape, want.shape)
        d = np.argwhere(got != want)
        assert len(d) == 0, (f"{w}x{h}x{b} {kind}: {len(d)} bytes differ, first at "
                             f"{d[0].tolist()} got {got[tuple(d[0])]} want {want[tuple(d[0])]}")


# mipx::reduce2_window_launch(in, out, n, w, h, b, x0, y0, x1, y1, stream): the launcher the
# demand-driven plans call; it is not part of the C ABI, so it is looked up by its C++ name
_WINDOW_LAUNCH = "_ZN4mipx21reduce2_window_launchEPKhPhiiiiiiiiP12ihipStream_t"
_STRIP = {3: 160, 4: 120}   # output pixels per strip (Reduce2Geom<B>::TW, reduce2_geom.h)
_ITEM = {3: 4, 4: 2}        # output pixels per horizontal item (Reduce2Geom<B>::K)


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("window", ["rows", "cols"])
def test_demand_windows_exact_and_nothing_else_written(gpu, oracle, corner, b, window):
    """Rows [12, 30) and columns [150, 170) of the 322 x 49 output of 644 x 98.  The
    launcher computes the window rounded out to whole strips on the left, to a multiple of
    12 rows at the top (12 is one) and to a whole horizontal item (4 pixels RGB, 2 RGBA)
    on the right, and clips exactly at the bottom; every byte it computes equals the
    oracle and every other byte of the output keeps the poison, guard bands included."""
    from imaginary_amd._abi import check, sync_tuning
    from imaginary_amd.engine import GuardedBuffer
    w, h = 644, 98
    ow, oh = w // 2, h // 2
    x0, y0, x1, y1 = (0, 12, ow, 30) if window == "rows" else (150, 0, 170, oh)
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
    xl = x0 // _STRIP[b] * _STRIP[b]
    xr = min(-(-x1 // _ITEM[b]) * _ITEM[b], ow)
    assert np.array_equal(got[:, y0:y1, xl:xr], want[:, y0:y1, xl:xr]), f"{window} x{b}"
    outside = np.ones(got.shape, bool)
    outside[:, y0:y1, xl:xr] = False
    assert np.all(got[outside] == FILL), f"{window} x{b}: wrote outside the window"
