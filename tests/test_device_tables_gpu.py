"""The device table cache's two paths nothing else walks (mipx_device_tables.cpp): a
growable table replaced by a larger one while the old one stays readable, and every table
freed by mipx_shutdown and uploaded again afterwards (a new generation).  k_rcol's vertical
plan and k_enlm's axis records are the growable kinds: cap 1024 rows, then 2048."""
import numpy as np
import pytest

from footprint import guarded  # noqa: F401
from test_parity_gpu import assert_same, rand_img, smooth_img

pytestmark = pytest.mark.gpu


def _restart(gpu):
    """An engine up and down again: mipx_shutdown frees every device table."""
    gpu.lib.mipx_shutdown()   # mipx_init keeps a running engine's configuration
    gpu.Engine(devices=[0], max_batch=4).shutdown()


def test_vplan_grows_and_is_rebuilt_after_shutdown(gpu, oracle, rng, convention):
    hs = vs = 1.6
    small = np.stack([rand_img(rng, 120, 40, 3), smooth_img(rng, 120, 40, 3)])      # 75 output rows: cap 1024
    tall = np.stack([rand_img(rng, 1800, 40, 3), smooth_img(rng, 1800, 40, 3)])     # 1125 output rows: cap 2048
    want_small = [oracle.reduce(im, hs, vs) for im in small]
    want_tall = [oracle.reduce(im, hs, vs) for im in tall]
    _restart(gpu)
    first = gpu.run_op("reduce", small, hshrink=hs, vshrink=vs)
    grown = gpu.run_op("reduce", tall, hshrink=hs, vshrink=vs)
    again = gpu.run_op("reduce", small, hshrink=hs, vshrink=vs)
    assert grown.shape[1] == 1125
    for i in range(2):
        assert_same(first[i], want_small[i], f"{convention} plan at 1024 rows img{i}")
        assert_same(grown[i], want_tall[i], f"{convention} plan grown to 2048 rows img{i}")
        assert_same(again[i], want_small[i], f"{convention} small image on the grown plan img{i}")
    _restart(gpu)
    after = gpu.run_op("reduce", small, hshrink=hs, vshrink=vs)
    assert_same(after, first, f"{convention} tables uploaded again after shutdown")


def test_enlm_axis_grows_and_is_rebuilt_after_shutdown(gpu, oracle, rng, monkeypatch):
    monkeypatch.setenv("MIPX_ENLM", "2")   # k_enlm or an error, never the VALU kernels
    short = np.stack([rand_img(rng, 300, 16, 3), smooth_img(rng, 300, 16, 3)])      # 600 output rows: cap 1024
    tall = np.stack([rand_img(rng, 700, 16, 3), smooth_img(rng, 700, 16, 3)])       # 1400 output rows: cap 2048
    want_short = [oracle.affine(im, 2.0, 2.0, 1) for im in short]
    want_tall = [oracle.affine(im, 2.0, 2.0, 1) for im in tall]
    _restart(gpu)
    first = gpu.run_op("affine", short, xscale=2.0, yscale=2.0, extend=1)
    grown = gpu.run_op("affine", tall, xscale=2.0, yscale=2.0, extend=1)
    again = gpu.run_op("affine", short, xscale=2.0, yscale=2.0, extend=1)
    assert grown.shape[1] == 1400
    for i in range(2):
        assert_same(first[i], want_short[i], f"axis at 1024 positions img{i}")
        assert_same(grown[i], want_tall[i], f"axis grown to 2048 positions img{i}")
        assert_same(again[i], want_short[i], f"short image on the grown axis img{i}")
    _restart(gpu)
    after = gpu.run_op("affine", short, xscale=2.0, yscale=2.0, extend=1)
    assert_same(after, first, "axis uploaded again after shutdown")
