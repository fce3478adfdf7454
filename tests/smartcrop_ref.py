"""A plain float64 reference of the smartcrop attention scorer, and the inputs that
make its one observable -- the crop origin -- as sensitive as a byte comparison.

The scorer (libvips vips_smartcrop, INTERESTING_ATTENTION) works on the ~32 px
downsample of the image:

    linear = sRGB^-1(v / 255) * 100            piecewise formula
    XYZ    = M * linear                        the sRGB / D65 matrix
    edge   = |5 * Laplacian(Y)|                COPY edges
    skin   = 100 - 100 * |XYZ / |XYZ| - (0.78, 0.57, 0.44)|   where Y > 5, else 0
    sat    = 500 * (f(X / 95.047) - f(Y / 100))               where Y > 5, else 0
             f(t) = 7.787 t + 16 / 116 below 0.008856, cbrt(t) above
    map    = gaussblur(edge + skin + sat)      integer mask, min_ampl 0.2, COPY edges,
             sigma = max(1, sqrt((cw * 32 / in_w)^2 + (ch * 32 / in_h)^2) / 10)
    origin = first maximum in raster order, scaled back, centred, clipped

Everything here is numpy float64 written from these formulas: no table, no float
rounding between the steps, no operation order to keep.  The engine's kernel and the
CPU oracle both restate libvips' float / double pipeline step by step from one
reading of smartcrop.c; this file shares none of that code, so where the argmax is
decided by more than rounding (gap(map) > M) an origin that all three agree on is
not a shared misreading.  Where it is decided by rounding (the twin sets below), the
oracle alone is the reference and the test is a bit-level one.

Measured with this file (tests/test_smartcrop_cpu.py repeats every measurement and
asserts the bounds next to them), seed 20250613:

  * float32 model of the libvips pipeline (tests/test_smartcrop_cpu.py model(), which
    gives the oracle's origin on all 504 committed tie, corner and noise cases) against
    this float64 map, largest absolute difference over 3 200 32 x 32 images (800 each
    of uniform noise, low-contrast noise, jittered blocks, perturbed twins, crops
    cycling through REF_CROPS): 1.36e-4.
  * largest gap at which this reference and the oracle give different origins, over
    the same 3 200 images: 1.44e-5 (one image, a perturbed twin), under M / 10 = 1e-3.
    On the 42 larger images of ROUTES every decided origin agrees.
  * undecided share (gap <= M = 1e-2) on the 2 400 noise images: 25, 1.04 %.
  * transposed twins, 200 images (seed 20250613 + 1), crops 2..12: largest float64
    gap 3.41e-13; the oracle picks the earlier twin on 179 (89.5 %) and the later on
    21 (10.5 %), read off the oracle's origin against the two origins this reference
    gives for the best place of the upper and of the lower half.  On 155 of the 200
    the two peaks are the same float and the tie rule alone decides.
  * mutants of the float32 model, origins changed among the 504 committed cases:
    float32 blur sums 56, last maximum 330, wrapped edges 25, no Y > 5 mask 37,
    cw / 2 as a float 279, blur passes swapped 45.

What the sets found: the engine built Lab's cube-root look-up with cbrtf where libvips'
C calls the double cbrt; 11,553 of its 100,000 entries were one ulp off, which moved
the origin of transposed twin 161 (crop 2 x 2) from (9, 7) to the later twin's (7, 22)
and of none of the images the suite had before.
"""
import numpy as np

M = 1e-2           # a gap above this is decided by the arithmetic, not by rounding
SEED = 20250613
SMALL = 32         # the scorer's working size


# ------------------------------------------------------------------ the scorer
def _linear(v):
    f = np.asarray(v, np.float64) / 255.0
    return np.where(f <= 0.04045, f / 12.92, ((f + 0.055) / 1.055) ** 2.4)


def _lab_f(t):
    return np.where(t < 0.008856, 7.787 * t + 16.0 / 116.0, np.cbrt(t))


def sigma_of(cw, ch, in_w, in_h):
    return max(1.0, np.hypot(cw * 32.0 / in_w, ch * 32.0 / in_h) / 10.0)


def gaussmat(sigma, min_ampl=0.2):
    """The integer gaussian mask: rint(20 exp(-x^2 / 2 sigma^2)) out to the last x whose
    amplitude is still at least min_ampl.  Returns (mask, sum)."""
    r = 0
    while np.exp(-((r + 1) ** 2) / (2.0 * sigma * sigma)) >= min_ampl:
        r += 1
    x = np.arange(-r, r + 1, dtype=np.float64)
    m = np.rint(20.0 * np.exp(-(x * x) / (2.0 * sigma * sigma)))
    return m, m.sum()


def _blur_axis(a, mask, axis):
    r = len(mask) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    out = np.zeros_like(a)
    for t, m in enumerate(mask):
        out += m * (p[t:t + n, :] if axis == 0 else p[:, t:t + n])
    return out


def score_map(small, cw, ch, in_w, in_h):
    """The blurred attention map of the ~32 px image `small` (H x W x >= 3, uint8) for a
    crop of cw x ch out of the in_w x in_h original."""
    lin = _linear(np.asarray(small)[..., :3]) * 100.0
    R, G, B = lin[..., 0], lin[..., 1], lin[..., 2]
    X = 0.4124 * R + 0.3576 * G + 0.1805 * B
    Y = 0.2126 * R + 0.7152 * G + 0.0722 * B
    Z = 0.0193 * R + 0.1192 * G + 0.9505 * B
    p = np.pad(Y, 1, mode="edge")
    edge = np.abs(5.0 * (4.0 * Y - p[:-2, 1:-1] - p[2:, 1:-1] - p[1:-1, :-2] - p[1:-1, 2:]))
    mag = np.sqrt(X * X + Y * Y + Z * Z)
    safe = np.where(mag == 0.0, 1.0, mag)
    nx, ny, nz = (np.where(mag == 0.0, 0.0, c / safe) for c in (X, Y, Z))
    dist = np.sqrt((nx - 0.78) ** 2 + (ny - 0.57) ** 2 + (nz - 0.44) ** 2)
    bright = Y > 5.0
    skin = np.where(bright, 100.0 - 100.0 * dist, 0.0)
    sat = np.where(bright, 500.0 * (_lab_f(X / 95.047) - _lab_f(Y / 100.0)), 0.0)
    mask, total = gaussmat(sigma_of(cw, ch, in_w, in_h))
    score = edge + skin + sat
    return _blur_axis(_blur_axis(score, mask, 1) / total, mask, 0) / total


def peak(m):
    """(row, column) of the first maximum in raster order."""
    i = int(np.argmax(m))          # numpy: the first occurrence
    return i // m.shape[1], i % m.shape[1]


def origin_of(yp, xp, cw, ch, in_w, in_h):
    left = min(max(xp / (32.0 / in_w) - cw // 2, 0.0), float(in_w - cw))
    top = min(max(yp / (32.0 / in_h) - ch // 2, 0.0), float(in_h - ch))
    return int(left), int(top)


def origin(m, cw, ch, in_w, in_h):
    """(left, top) of the crop centred on the map's first maximum, clipped to the image."""
    yp, xp = peak(m)
    return origin_of(yp, xp, cw, ch, in_w, in_h)


def gap(m):
    """Best minus second-best value of the map (0.0 where the maximum is shared)."""
    v = np.partition(np.asarray(m, np.float64).ravel(), -2)
    return float(v[-1] - v[-2])


def downsample(oracle, img):
    """vips_resize(32 / w, vscale = 32 / h) as a schedule over the oracle's resamplers:
    box shrink by floor(1 / (2 scale)), reducev of the residual, then reduceh."""
    cur = np.ascontiguousarray(img)
    h, w = cur.shape[:2]
    hscale, vscale = 32.0 / w, 32.0 / h
    if hscale > 1.0 or vscale > 1.0:
        raise ValueError(f"{w}x{h}: smaller than {SMALL} px, not a downsize")
    sh, sv = (max(1, int(np.floor(1.0 / (2.0 * s)))) for s in (hscale, vscale))
    if sh > 1 or sv > 1:
        cur = oracle.shrink(cur, sh, sv)
        hscale, vscale = hscale * sh, vscale * sv
    if vscale < 1.0:
        cur = oracle.reducev(cur, 1.0 / vscale)
    if hscale < 1.0:
        cur = oracle.reduceh(cur, 1.0 / hscale)
    return cur


def reference_origin(oracle, img, cw, ch):
    """(origin, gap) of the reference for an image of any accepted size."""
    h, w = img.shape[:2]
    m = score_map(img if (h, w) == (SMALL, SMALL) else downsample(oracle, img), cw, ch, w, h)
    return origin(m, cw, ch, w, h), gap(m)


# ------------------------------------------------------------------ the inputs
PATCH = 4


def _ground(rng):
    """A flat ground dull enough that a random patch out-scores it."""
    img = np.empty((SMALL, SMALL, 3), np.uint8)
    img[:] = rng.integers(60, 140, 3, dtype=np.uint8)
    return img


def _twin_places(rng, variant):
    """Top-left corners (ay, ax), (by, bx) of the two 4 x 4 patches: A in rows 3-12, B in
    rows 18-25, both at least 4 px from every edge.  Raster index i of a 32-wide map is
    handled by thread i % 256 of the scorer, wave (y % 8) // 2:
      variant 0  B 16 rows below A, same column: the two peaks meet in one thread
      variant 1  B 16 rows below A, another column: same wave, other lane
      variant 2  the row distance is 2..6 mod 8: the peaks lie in different waves
      variant 3  anything"""
    ax, bx = (int(v) for v in rng.integers(4, SMALL - 4 - PATCH + 1, 2))
    if variant in (0, 1):
        ay = int(rng.integers(3, 7))
        by = ay + 16
        if variant == 0:
            bx = ax
        elif bx == ax:
            bx = ax + 5 if ax + 5 <= SMALL - 4 - PATCH else ax - 5
    else:
        while True:
            ay, by = int(rng.integers(3, 10)), int(rng.integers(18, 23))
            if variant == 3 or 2 <= (by - ay) % 8 <= 6:
                break
    return (ay, ax), (by, bx)


def _twins(rng, variant, transpose):
    variant = int(rng.integers(0, 4)) if variant is None else variant
    img = _ground(rng)
    f = rng.integers(0, 256, (PATCH, PATCH, 3), dtype=np.uint8)
    (ay, ax), (by, bx) = _twin_places(rng, variant)
    img[ay:ay + PATCH, ax:ax + PATCH] = f
    img[by:by + PATCH, bx:bx + PATCH] = f.transpose(1, 0, 2) if transpose else f
    return img, (ay, ax), (by, bx)


def translated_twins(rng, variant=None, places=False):
    """A flat ground with one random 4 x 4 patch at A and the same patch at B: exact ties
    in any faithful pipeline, the earlier one (A) wins."""
    img, a, b = _twins(rng, variant, False)
    return (img, a, b) if places else img


def transposed_twins(rng, variant=None, places=False):
    """As translated_twins, but B holds the patch transposed.  A and B tie in exact
    arithmetic; libvips rounds the horizontal pass to float before the vertical one, so
    there they differ by an ulp or so, and either can win."""
    img, a, b = _twins(rng, variant, True)
    return (img, a, b) if places else img


def perturbed_twins(rng, variant=None):
    """Translated twins with one to three ground pixels, each within 2 px of one of the
    patches, moved by one grey level: the tie is broken by a little, or not at all."""
    img, a, b = _twins(rng, variant, False)
    for _ in range(int(rng.integers(1, 4))):
        py, px = a if rng.integers(0, 2) else b
        while True:
            y = py + int(rng.integers(-2, PATCH + 2))
            x = px + int(rng.integers(-2, PATCH + 2))
            if not (py <= y < py + PATCH and px <= x < px + PATCH):
                break
        c = int(rng.integers(0, 3))
        img[y, x, c] = int(img[y, x, c]) + (1 if rng.integers(0, 2) else -1)     # the ground is 60..139
    return img


CORNER_PLACES = {"top_left": (0, 0), "top": (0, 14), "top_right": (0, 28), "right": (14, 28),
                 "bottom_right": (28, 28), "bottom": (28, 14), "bottom_left": (28, 0), "left": (14, 0)}
CORNER_CROPS = ((12, 12), (11, 13), (20, 9))


def corner_features(seed=SEED + 7):
    """name -> image: one random patch in each corner and at the middle of each side.
    With any of CORNER_CROPS the crop centred on the patch clips at that side."""
    rng = np.random.default_rng(seed)
    return {name: feature_at(rng, y, x) for name, (y, x) in CORNER_PLACES.items()}


def feature_at(rng, y, x):
    """A flat ground with one random patch whose top-left corner is (y, x)."""
    img = _ground(rng)
    img[y:y + PATCH, x:x + PATCH] = rng.integers(0, 256, (PATCH, PATCH, 3), dtype=np.uint8)
    return img


def periodic(rng):
    """An 8 x 8 tile repeated 4 x 4: every interior repeat of the best place ties."""
    return np.tile(rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), (4, 4, 1))


def constant(v):
    return np.full((SMALL, SMALL, 3), v, np.uint8)


def uniform_noise(rng):
    return rng.integers(0, 256, (SMALL, SMALL, 3), dtype=np.uint8)


def low_contrast_noise(rng):
    base = rng.integers(20, 220, 3)
    return (base + rng.integers(0, 17, (SMALL, SMALL, 3))).astype(np.uint8)


def jittered_blocks(rng):
    """4 x 4 blocks of random colour with +-3 of noise on top."""
    blocks = rng.integers(0, 256, (8, 8, 3))
    img = np.kron(blocks, np.ones((4, 4, 1), np.int64)) + rng.integers(-3, 4, (SMALL, SMALL, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


NOISE_KINDS = (uniform_noise, low_contrast_noise, jittered_blocks)


def enlarge(img, w, h):
    """Pixel replication of a 32 x 32 image to w x h, so its downsample keeps the
    competing peaks."""
    ys = (np.arange(h) * img.shape[0]) // h
    xs = (np.arange(w) * img.shape[1]) // w
    return np.ascontiguousarray(img[ys][:, xs])


def with_alpha(rng, img):
    a = rng.integers(0, 256, img.shape[:-1] + (1,), dtype=np.uint8)
    return np.ascontiguousarray(np.concatenate([img[..., :3], a], -1))


# crops for the 32 px sets: small, odd, and (for the reference only) full width / height
SMALL_CROPS = ((2, 2), (3, 5), (4, 4), (5, 3), (7, 7), (8, 6), (9, 12), (12, 12), (11, 2), (6, 11))
REF_CROPS = SMALL_CROPS + ((32, 5), (7, 32), (32, 32), (1, 1), (31, 17))

# the resize routes of the scorer: (w, h)
ROUTES = ((32, 32), (33, 40), (64, 64), (48, 200), (36, 1000), (257, 95), (240, 180))

TIE_SETS = {"transposed": (transposed_twins, 200, 1), "translated": (translated_twins, 100, 2),
            "perturbed": (perturbed_twins, 100, 3), "periodic": (periodic, 20, 4)}
_CACHE = {}


def tie_set(name):
    """The committed tie and near-tie cases of a kind: a list of (image, (cw, ch)), image k
    built as twin variant k % 4 and cropped by SMALL_CROPS[(k // 4) % 10].  Built once,
    read-only."""
    if name not in _CACHE:
        build, count, salt = TIE_SETS[name]
        rng = np.random.default_rng(SEED + salt)
        out = []
        for k in range(count):
            img = build(rng) if build is periodic else build(rng, k % 4)
            img.setflags(write=False)
            out.append((img, SMALL_CROPS[(k // 4) % len(SMALL_CROPS)]))
        _CACHE[name] = out
    return _CACHE[name]


def by_crop(cases):
    """{(cw, ch): [index into cases]}: the batches a list of (image, crop) runs as."""
    groups = {}
    for k, (_, crop) in enumerate(cases):
        groups.setdefault(crop, []).append(k)
    return groups


def route_batches(w, h, structured_img):
    """Two batches of three w x h images for a resize route: enlarged twins and corner
    features (the downsample still holds competing peaks) and structured_img content.
    Returns [(images (3, h, w, 3), (cw, ch))]: one even crop, one odd."""
    key = ("route", w, h)
    if key not in _CACHE:
        rng = np.random.default_rng(SEED + w * 1009 + h)
        corners = corner_features()
        a = np.stack([enlarge(transposed_twins(rng, 2), w, h), enlarge(corners["right"], w, h),
                      structured_img(rng, h, w, 3)])
        b = np.stack([enlarge(translated_twins(rng, 0), w, h), enlarge(corners["bottom_left"], w, h),
                      enlarge(perturbed_twins(rng, 1), w, h)])
        for x in (a, b):
            x.setflags(write=False)
        even = (max(2, (w * 6 // 32) & ~1), max(2, (h * 6 // 32) & ~1))
        odd = (max(1, w * 9 // 32) | 1, max(1, h * 5 // 32) | 1)
        _CACHE[key] = [(a, even), (b, odd)]
    return _CACHE[key]
