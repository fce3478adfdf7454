"""The smartcrop reference and inputs of tests/smartcrop_ref.py, checked without a GPU.

 1. The float64 reference against the CPU oracle: wherever the reference's argmax is
    decided by more than rounding (gap > M) the two origins are the same, on 3 200
    seeded 32 x 32 images and on the larger sizes of the resize routes; and the share of
    noise images the reference leaves undecided is capped, so the check cannot quietly
    lose its cases.
 2. The twin sets are what they claim: exact ties where they should be exact, ties to
    1e-9 where libvips' float rounding decides, and on those the oracle picks both sides.
 3. Mutants: a numpy float32 restatement of the oracle's pipeline follows the oracle's
    origins on the committed inputs; six wrong variants of it (the mistakes a kernel could
    make) each change at least one origin there, so the GPU comparison in
    tests/test_smartcrop_gpu.py can fail.

The measured figures are printed (pytest -s) and recorded in smartcrop_ref's docstring.
"""
import numpy as np
import pytest

import smartcrop_ref as ref
from smartcrop_ref import M

F = np.float32
D = np.float64


# ------------------------------------------------------------------ float32 model
def _tables():
    f = (np.arange(256).astype(F) / F(255)).astype(D)
    v2y = np.where(f <= 0.04045, f / 12.92, ((f + 0.055) / 1.055) ** 2.4).astype(F)
    q = (np.arange(100000) / 100000.0).astype(F).astype(D)
    cb = np.where(q < 0.008856, 7.787 * q + 16.0 / 116.0, np.cbrt(q)).astype(F)
    return v2y, cb


V2Y, CBRT = _tables()


def _lab_cbrt(v, white):
    n = ((F(100000) * v).astype(D) / white).astype(F)
    i = np.clip(n.astype(np.int64), 0, len(CBRT) - 2)
    f = n - i.astype(F)
    return CBRT[i] + f * (CBRT[i + 1] - CBRT[i])


def _conv(a, mask, scale, axis, mode, acc):
    """One pass of the float convolution: the sum in `acc`, taps in mask order."""
    r = len(mask) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode=mode).astype(acc)
    n = a.shape[axis]
    s = np.zeros(a.shape, acc)
    for t, m in enumerate(mask):
        s = s + acc(m) * (p[t:t + n, :] if axis == 0 else p[:, t:t + n])
    return (s / acc(scale) + acc(0)).astype(F)


MUTANTS = {
    "a": "blur sums kept in float32",
    "b": "the last maximum in place of the first",
    "c": "wrapped edges in place of clamped edges",
    "d": "sat and skin not masked by Y > 5",
    "e": "cw / 2 taken as a float division",
    "f": "hblur and vblur swapped",
}


def model(small, cw, ch, in_w, in_h, mutant=None):
    """The oracle's float / double pipeline in numpy, one rounding per C operation.
    Returns ((left, top), map)."""
    mode = "wrap" if mutant == "c" else "edge"
    px = np.asarray(small)[..., :3]
    R, G, B = (V2Y[px[..., c]] * F(100) for c in range(3))
    Rd, Gd, Bd = R.astype(D), G.astype(D), B.astype(D)
    X = (0.4124 * Rd + 0.3576 * Gd + 0.1805 * Bd).astype(F)
    Y = (0.2126 * Rd + 0.7152 * Gd + 0.0722 * Bd).astype(F)
    Z = (0.0193 * Rd + 0.1192 * Gd + 0.9505 * Bd).astype(F)
    p = np.pad(Y, 1, mode=mode).astype(D)
    acc = np.zeros(Y.shape, D)
    for w, s in ((-1.0, p[:-2, 1:-1]), (-1.0, p[1:-1, :-2]), (4.0, p[1:-1, 1:-1]), (-1.0, p[1:-1, 2:]),
                 (-1.0, p[2:, 1:-1])):
        acc = acc + w * s
    edge = np.abs(F(5) * (acc / 1.0 + 0.0).astype(F) + F(0))
    sq = X * X
    sq = sq + Y * Y
    sq = sq + Z * Z
    mag = np.sqrt(sq.astype(D)).astype(F)
    safe = np.where(mag == 0, F(1), mag)
    nx, ny, nz = (np.where(mag == 0, F(0), c / safe) for c in (X, Y, Z))
    dx, dy, dz = nx + F(-0.78), ny + F(-0.57), nz + F(-0.44)
    d2 = dx * dx
    d2 = d2 + dy * dy
    d2 = d2 + dz * dz
    dist = np.sqrt(d2.astype(D)).astype(F)
    skin = F(-100) * dist + F(100)
    sat = (500.0 * (_lab_cbrt(X, 95.047) - _lab_cbrt(Y, 100.0)).astype(D)).astype(F)
    if mutant != "d":
        bright = Y.astype(D) > 5.0
        skin = np.where(bright, skin, F(0))
        sat = np.where(bright, sat, F(0))
    score = (edge + skin) + sat
    assert score.dtype == F
    mask, scale = ref.gaussmat(ref.sigma_of(cw, ch, in_w, in_h))
    acc_t = F if mutant == "a" else D
    first, second = (0, 1) if mutant == "f" else (1, 0)
    m = _conv(_conv(score, mask, scale, first, mode, acc_t), mask, scale, second, mode, acc_t)
    flat = m.ravel()
    best = len(flat) - 1 - int(np.argmax(flat[::-1])) if mutant == "b" else int(np.argmax(flat))
    yp, xp = divmod(best, m.shape[1])
    hw, hh = (cw / 2, ch / 2) if mutant == "e" else (cw // 2, ch // 2)
    left = min(max(xp / (32.0 / in_w) - hw, 0.0), float(in_w - cw))
    top = min(max(yp / (32.0 / in_h) - hh, 0.0), float(in_h - ch))
    return (int(left), int(top)), m


def test_engine_colour_tables_are_the_formulas(tmp_path):
    """The two look-ups the kernel reads, as csrc/mipx_planner.cpp builds them, bit for bit
    against the tables of the float32 restatement (which follows the oracle everywhere).
    Regression: the cube-root table was built with std::cbrt(float), which is cbrtf, where
    libvips' C calls the double cbrt and rounds once; 11,553 of the 100,000 entries were one
    ulp off, and the engine picked the later of two tied twins on transposed twin 161."""
    import os
    import subprocess
    from conftest import ROOT
    csrc = os.path.join(ROOT, "imaginary_amd", "csrc")
    exe = tmp_path / "colour_tables_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", csrc,
                    os.path.join(ROOT, "tests", "c", "colour_tables_host.cpp"), os.path.join(csrc, "mipx_tables.cpp"),
                    os.path.join(csrc, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    raw = np.frombuffer(subprocess.run([str(exe)], capture_output=True, check=True).stdout, F)
    assert raw.size == 256 + len(CBRT)
    assert np.array_equal(raw[:256].view(np.uint32), V2Y.view(np.uint32))
    bad = np.flatnonzero(raw[256:].view(np.uint32) != CBRT.view(np.uint32))
    assert bad.size == 0, f"{bad.size} cube-root entries differ, first at {bad[0]}"


# ------------------------------------------------------------------ 1. reference against oracle
PER_KIND = 800
KINDS = ref.NOISE_KINDS + (ref.perturbed_twins,)


@pytest.fixture(scope="module")
def survey(oracle):
    """Every 32 x 32 survey image once: (kind, gap, reference origin, oracle origin,
    largest |float32 model - float64 map|)."""
    rng = np.random.default_rng(ref.SEED)
    rows = []
    for k in range(PER_KIND * len(KINDS)):
        kind = KINDS[k % len(KINDS)]
        img = kind(rng)
        cw, ch = ref.REF_CROPS[(k // len(KINDS)) % len(ref.REF_CROPS)]
        m = ref.score_map(img, cw, ch, 32, 32)
        _, m32 = model(img, cw, ch, 32, 32)
        rows.append((kind.__name__, ref.gap(m), ref.origin(m, cw, ch, 32, 32), oracle.smartcrop_origin(img, cw, ch),
                     float(np.abs(m32.astype(D) - m).max())))
    return rows


def test_gaussmat_is_the_oracles(oracle):
    for sigma in (1.0, 1.2, 1.5, 1.7, 2.0, 2.63, 3.3, 4.53):
        mask, scale = ref.gaussmat(sigma)
        want, wscale = oracle.gaussmat(sigma, 0.2)
        assert [int(v) for v in mask] == want and int(scale) == wscale, sigma
    sizes = {len(ref.gaussmat(ref.sigma_of(cw, ch, 32, 32))[0]) for cw, ch in ref.SMALL_CROPS}
    assert sizes == {3, 5, 7}, sizes      # the small crops cover three mask widths


def test_reference_agrees_with_oracle(survey):
    assert len(survey) >= 3000
    worst = max((g for _, g, r, o, _ in survey if r != o), default=0.0)
    differ = [(k, g) for k, g, r, o, _ in survey if r != o]
    model_err = max(e for *_, e in survey)
    print(f"\nsurvey of {len(survey)}: float32 model against float64 map, largest difference {model_err:.3g}; "
          f"{len(differ)} origins differ ({sorted({k for k, _ in differ})}), {sum(g == 0.0 for _, g in differ)} at "
          f"gap 0.0, largest gap among them {worst:.3g}")
    for kind, g, r, o, _ in survey:
        if g > M:
            assert r == o, f"{kind}: reference {r}, oracle {o} at gap {g}"
    # float32 rounding must stay far under M for "gap > M" to mean "decided by the
    # arithmetic", and a disagreement above M / 10 is not rounding
    assert model_err < M / 10, model_err
    assert worst <= M / 10, worst


def test_undecided_share_is_capped(survey):
    noise = [g for k, g, *_ in survey if k != "perturbed_twins"]
    assert len(noise) == PER_KIND * len(ref.NOISE_KINDS)
    under = sum(g <= M for g in noise)
    print(f"\n{under} of {len(noise)} noise images undecided ({100.0 * under / len(noise):.2f} %)")
    assert under <= 0.02 * len(noise), (under, len(noise))


def test_reference_agrees_with_oracle_through_the_resize(oracle):
    """The larger sizes: the oracle's own resamplers under a restated vips_resize schedule,
    then the reference scorer and the origin mapping at hscale != 1."""
    from test_configs_gpu import structured_img
    decided = 0
    for w, h in ref.ROUTES:
        small = ref.downsample(oracle, np.zeros((h, w, 3), np.uint8))
        assert small.shape == (32, 32, 3), (w, h, small.shape)
        for imgs, (cw, ch) in ref.route_batches(w, h, structured_img):
            for i, img in enumerate(imgs):
                got, g = ref.reference_origin(oracle, img, cw, ch)
                if g > M:
                    decided += 1
                    assert got == oracle.smartcrop_origin(img, cw, ch), (w, h, i, cw, ch, g)
    assert decided >= 3 * len(ref.ROUTES), decided     # at least half of the 42 are decided


def test_downsample_refuses_an_upsize(oracle):
    for w, h in ((31, 64), (64, 31)):
        with pytest.raises(ValueError):
            ref.downsample(oracle, np.zeros((h, w, 3), np.uint8))
        with pytest.raises(oracle.OracleError) as e:
            oracle.smartcrop_origin(np.zeros((h, w, 3), np.uint8), 8, 8)
        assert e.value.code == -2


# ------------------------------------------------------------------ 2. the twin sets
def _twin_peaks(m, cw, ch):
    """Origins of the best place in the upper half (A) and in the lower half (B)."""
    ya, xa = ref.peak(m[:16])
    yb, xb = ref.peak(m[16:])
    return ref.origin_of(ya, xa, cw, ch, 32, 32), ref.origin_of(yb + 16, xb, cw, ch, 32, 32), (ya, xa), (yb + 16, xb)


def test_translated_twins_tie_exactly(oracle):
    rng = np.random.default_rng(ref.SEED + 2)
    waves = set()
    for k, (img, (cw, ch)) in enumerate(ref.tie_set("translated")):
        _, a, b = ref.translated_twins(rng, k % 4, places=True)      # the set's own generator, replayed
        m = ref.score_map(img, cw, ch, 32, 32)
        assert ref.gap(m) == 0.0, k
        oa, ob, pa, pb = _twin_peaks(m, cw, ch)
        assert m[pa] == m[pb] == m.max(), k
        # the two peaks are the same place of the two patches, inside or next to them
        assert (pb[0] - pa[0], pb[1] - pa[1]) == (b[0] - a[0], b[1] - a[1]), k
        assert -3 <= pa[0] - a[0] < 7 and -3 <= pa[1] - a[1] < 7, k
        assert oa != ob and ref.origin(m, cw, ch, 32, 32) == oa
        assert oracle.smartcrop_origin(img, cw, ch) == oa, f"translated twin {k}: the oracle left the earlier peak"
        ia, ib = pa[0] * 32 + pa[1], pb[0] * 32 + pb[1]
        waves.add(("same thread" if ia % 256 == ib % 256 else "same wave" if ia % 256 // 64 == ib % 256 // 64
                   else "other wave"))
    assert waves == {"same thread", "same wave", "other wave"}, waves


def test_periodic_ties_exactly(oracle):
    for k, (img, (cw, ch)) in enumerate(ref.tie_set("periodic")):
        m = ref.score_map(img, cw, ch, 32, 32)
        assert ref.gap(m) == 0.0, k
        assert int((m == m.max()).sum()) >= 2
        assert oracle.smartcrop_origin(img, cw, ch) == ref.origin(m, cw, ch, 32, 32), f"periodic {k}"


def test_transposed_twins_tie_to_rounding_and_split(oracle):
    cases = ref.tie_set("transposed")
    assert len(cases) == 200 and all(2 <= c <= 12 for _, crop in cases for c in crop)
    worst, earlier, later = 0.0, 0, 0
    for k, (img, (cw, ch)) in enumerate(cases):
        m = ref.score_map(img, cw, ch, 32, 32)
        worst = max(worst, ref.gap(m))
        oa, ob, pa, pb = _twin_peaks(m, cw, ch)
        assert abs(m[pa] - m[pb]) < 1e-9 and oa != ob, k
        got = oracle.smartcrop_origin(img, cw, ch)
        assert got in (oa, ob), (k, got, oa, ob)
        earlier += got == oa
        later += got == ob
    print(f"\ntransposed twins: largest float64 gap {worst:.3g}; oracle picks the earlier twin on {earlier}, "
          f"the later on {later} of {len(cases)}")
    assert worst < 1e-9, worst
    assert later >= 0.05 * len(cases) and earlier >= 0.5 * len(cases), (earlier, later)


def test_constants_and_corners(oracle):
    for v in (0, 128, 255):
        for cw, ch in ref.SMALL_CROPS[:3]:
            m = ref.score_map(ref.constant(v), cw, ch, 32, 32)
            assert ref.gap(m) == 0.0 and ref.origin(m, cw, ch, 32, 32) == (0, 0)
            assert oracle.smartcrop_origin(ref.constant(v), cw, ch) == (0, 0)
    sides = {"left": (0, None), "right": (1, None), "top": (None, 0), "bottom": (None, 1)}
    for name, img in ref.corner_features().items():
        for cw, ch in ref.CORNER_CROPS:
            m = ref.score_map(img, cw, ch, 32, 32)
            assert ref.gap(m) > M, (name, cw, ch)
            got = ref.origin(m, cw, ch, 32, 32)
            assert got == oracle.smartcrop_origin(img, cw, ch), (name, cw, ch)
            yp, xp = ref.peak(m)
            for side, (cx, cy) in sides.items():
                if side in name.split("_"):       # the unclipped crop would leave the image on that side
                    if cx is not None:
                        assert (xp - cw // 2 < 0, xp - cw // 2 > 32 - cw)[cx], (name, cw, ch, xp)
                        assert got[0] == (0, 32 - cw)[cx]
                    else:
                        assert (yp - ch // 2 < 0, yp - ch // 2 > 32 - ch)[cy], (name, cw, ch, yp)
                        assert got[1] == (0, 32 - ch)[cy]


# ------------------------------------------------------------------ 3. mutants
def _committed_cases():
    """Every 32 x 32 (image, crop) the GPU tests compare by origin."""
    cases = []
    for name in ref.TIE_SETS:
        cases += ref.tie_set(name)
    for img in ref.corner_features().values():
        cases += [(img, c) for c in ref.CORNER_CROPS]
    rng = np.random.default_rng(ref.SEED + 5)
    for k in range(60):
        cases.append((ref.NOISE_KINDS[k % 3](rng), ref.SMALL_CROPS[k % len(ref.SMALL_CROPS)]))
    return cases


def test_every_mutant_changes_an_origin(oracle):
    cases = _committed_cases()
    want = [oracle.smartcrop_origin(img, cw, ch) for img, (cw, ch) in cases]
    faithful = [model(img, cw, ch, 32, 32)[0] for img, (cw, ch) in cases]
    match = [k for k in range(len(cases)) if faithful[k] == want[k]]
    print(f"\nthe float32 restatement gives the oracle's origin on {len(match)} of {len(cases)} committed cases")
    # one rounding per C operation, the same order: the restatement is the oracle
    assert len(match) == len(cases), [k for k in range(len(cases)) if faithful[k] != want[k]]
    for mutant, what in MUTANTS.items():
        changed = sum(model(cases[k][0], *cases[k][1], 32, 32, mutant)[0] != want[k] for k in match)
        print(f"mutant ({mutant}) {what}: {changed} origins change")
        assert changed >= 1, f"mutant ({mutant}) {what}: no committed input notices it"
