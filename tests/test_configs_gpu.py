"""BASELINE.json configs C4 and C5 at their workload geometry, GPU against the
oracle bit for bit.

  C4: 4000x3000 and 3000x4000 RGB through the SmartCrop 256^2 plan (reference
      image.go:236-245: shrink 8 -> reduce 1.4648 -> smartcrop) and the Thumbnail
      256^2 + 128^2 RGBA watermark at (16, 16), opacity 0.5 (:279-284, :343-370).
  C5: every plan group of the seed-5 mixed stream (workloads.c5_requests, the
      same requests bench_configs.py times), one true-size image per group.

Each case runs mipx_plan_make's plan through mipx_execute_dev and the oracle
planner's plan through ref_execute on the same image.
"""
import numpy as np
import pytest

from footprint import guarded  # noqa: F401
import workloads

pytestmark = pytest.mark.gpu


def structured_img(rng, h, w, b):
    """Smooth gradients, a few saturated / skin-toned blobs and noise: gives the
    smartcrop scorer edges, saturation and skin to rank (uniform noise would not)."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    img = np.empty((h, w, b), np.float32)
    for c in range(b):
        f = rng.uniform(0.002, 0.02, 2)
        img[..., c] = 110 + 60 * np.sin(x * f[0] + c) * np.cos(y * f[1] - c)
    for _ in range(6):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(0.03, 0.12) * min(w, h)
        m = ((x - cx) ** 2 + (y - cy) ** 2) < r * r
        img[m] = rng.choice([[224, 172, 140], [250, 20, 30], [20, 200, 40]])[:b]
    img += rng.normal(0, 6, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def run_case(gpu, oracle, opts, w, h, img, wm=None):
    hdr = dict(w=w, h=h, bands=3, type=3)
    kw = {}
    if wm is not None:
        kw = dict(wm_w=wm.shape[1], wm_h=wm.shape[0], wm_bands=wm.shape[2])
        hdr.update(kw)
    p = gpu.plan_make(gpu.make_opts(**opts), gpu.make_input(w, h, 3, "png", 0, **kw))
    e, rp = oracle.plan(opts, hdr)
    assert e == 0
    got = gpu.execute(p, img, wm)[0]
    want = oracle.execute(rp, img, wm)
    assert got.shape == want.shape, (opts, got.shape, want.shape)
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError(f"{opts} {w}x{h} {p.describe()}: {len(d)} bytes differ, first at {d[0].tolist()}")
    return p


@pytest.mark.parametrize("w,h", workloads.C4_SIZES)
@pytest.mark.parametrize("kind", ["smartcrop", "thumbnail_watermark"])
def test_c4_at_12mp(gpu, oracle, w, h, kind):
    rng = np.random.default_rng(4 + w)
    img = structured_img(rng, h, w, 3)
    if kind == "smartcrop":
        p = run_case(gpu, oracle, workloads.C4_OPTS[0], w, h, img)
        ops = [s[0] for s in p.describe()]
        assert ops[:3] == ["shrink", "reduce", "smartcrop"], ops    # the C4 chain, 12 MP decoded input
        assert (p.out_w, p.out_h) == (256, 256)
    else:
        p = run_case(gpu, oracle, workloads.C4_OPTS[1], w, h, img, workloads.c4_watermark())
        ops = [s[0] for s in p.describe()]
        assert ops[0] == "shrink" and ops[-1] == "watermark", ops
        assert p.out_bands == 4


def test_c4_smartcrop_on_noise(gpu, oracle):
    """Uniform noise (the bench's C4 input) through the same plan."""
    rng = np.random.default_rng(44)
    img = rng.integers(0, 256, (3000, 4000, 3), dtype=np.uint8)
    run_case(gpu, oracle, workloads.C4_OPTS[0], 4000, 3000, img)


def _c5_groups():
    import imaginary_amd as ia
    return workloads.c5_groups(workloads.c5_requests(512, 5, ia.fit_dimension))


C5_GROUPS = _c5_groups()


@pytest.mark.parametrize("k", range(len(C5_GROUPS)),
                         ids=[f"{w}x{h}-" + "-".join(f"{a}{v}" for a, v in sorted(o.items()))
                              for (w, h), o, _ in C5_GROUPS])
def test_c5_plan_group(gpu, oracle, k):
    (w, h), opts, _ = C5_GROUPS[k]
    rng = np.random.default_rng(500 + k)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8) if k % 2 else structured_img(rng, h, w, 3)
    run_case(gpu, oracle, opts, w, h, img)


def test_c5_covers_every_request_kind():
    kinds = set()
    for (w, h), o, _ in C5_GROUPS:
        kinds.add("rotate" if "rotate" in o else "blur" if "sigma" in o else
                  "embed" if "extend" in o else "resize" if "height" not in o else "fit")
    assert kinds == {"rotate", "blur", "embed", "resize", "fit"}
    assert {(w, h) for (w, h), _, _ in C5_GROUPS} == {(1920, 1080), (3840, 2160), (4000, 3000)}
