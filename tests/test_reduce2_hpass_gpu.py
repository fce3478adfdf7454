"""The k_reduce2x2 tile's horizontal pass (reduce2_hwalk, k_reduce.hip) against the
oracle, byte for byte, at the corner sampling convention.

A lane takes one item column (4 pixels RGB, 2 RGBA) and walks down it 6 / 4 rows at a time
with an LDS address and an output pointer that advance by constants.  The shapes were
chosen for a walk of 8- / 4-pixel items stored as two halves over 12 / 8 rows a step (which
measured slower and is not what the kernel does), and hold for the 4- / 2-pixel walk too:
a strip narrower than a wave's items, a partial last item, output rows that start off a
dword (RGB, ow not a multiple of 4), a last walk step of one row, one row short of a
12-row step, exactly one strip and one tile, a second strip of a single item beside a
second tile of one row, and three strips.  Every batch holds 3 images, so the last image
ends at the end of the guard-banded buffers (footprint.py)."""
import ctypes as C

import numpy as np
import pytest

from footprint import FILL, guarded  # noqa: F401

pytestmark = pytest.mark.gpu

# input (w, h) -> output (w / 2, h / 2)
SHAPES = {
    3: [(8, 8), (12, 8), (20, 24), (28, 26), (320, 48), (328, 50), (332, 22), (336, 24), (644, 98)],
    4: [(8, 8), (10, 14), (14, 16), (18, 18), (240, 34), (246, 50)],
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
        r = np.random.default_rng(7000 * w + 10 * h + b)
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
def test_hwalk_exact(gpu, oracle, corner, b, w, h):
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
_ITEM = {3: 4, 4: 2}        # output pixels per horizontal item: a window's right edge rounds to it

# (x0, y0, x1, y1) in the 322 x 49 output of 644 x 98; None = the image's edge
WINDOWS = {
    "cols_174": (150, 0, 174, None),  # RGB: ends inside item [172, 176), the second of an aligned pair
    "cols_162": (150, 0, 162, None),  # RGB: ends inside item [160, 164), the first item of strip 1
    "rows": (0, 12, None, 30),
}


@pytest.mark.parametrize("b", [3, 4])
@pytest.mark.parametrize("window", list(WINDOWS))
def test_demand_windows_exact_and_nothing_else_written(gpu, oracle, corner, b, window):
    """The launcher computes the window rounded out to whole strips on the left, to a multiple
    of 12 rows at the top and to a whole horizontal item (4 pixels RGB, 2 RGBA) on the right, and
    clips exactly at the bottom; every byte it computes equals the oracle and every other
    byte of the output keeps the poison, guard bands included."""
    from imaginary_amd._abi import check, sync_tuning
    from imaginary_amd.engine import GuardedBuffer
    w, h = 644, 98
    ow, oh = w // 2, h // 2
    x0, y0, x1, y1 = WINDOWS[window]
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
