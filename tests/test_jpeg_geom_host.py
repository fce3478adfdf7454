"""The JPEG geometry (csrc/jpeg_geom.h) on the host, no GPU.  tests/c/jpeg_geom_host.cpp links
mipx_planner.cpp only and has two parts.  `pin`: every size the engine reports of (w, h, layout),
hashed: the six mipx_*_bytes functions (bad layouts and sizes included), jpeg_opt_in_range and every
field of JpegeWork and JpeghWork, over w, h in 1..40 and the sizes either side of each limit;
tests/golden/jpeg_geom_host.txt is what the commit before jpeg_geom.h printed.  `geom`: the struct's
own fields, which are compared here with libjpeg's general rule for sampling factors (hs, vs):
a component is ceil(size * samp / max) samples and ceil(that / 8) blocks, the MCU grid is
ceil(size / (8 max)), and at 1/s a component's inverse DCT is N = 8 / s, doubled up to 8 where both
of its sampling ratios allow (jdmaster.c), its plane ceil(size * samp * N / (max * 8))."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "imaginary_amd", "csrc")
FACTORS = {0: (1, 1), 1: (2, 2), 3: (2, 1)}   # MIPX_YCC_444, _420, _422: Y's sampling factors


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("jpeg_geom") / "jpeg_geom_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    # as tests/test_tables_host.py: mipx_planner.cpp reaches the HIP headers for declarations only
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "jpeg_geom_host.cpp"), os.path.join(CSRC, "mipx_planner.cpp"),
                    "-o", str(out)], check=True)
    return str(out)


def test_sizes_match_the_recorded_ones(exe):
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "jpeg_geom_host.txt")).read().splitlines()
    assert len(want) > 200 and len(set(l.split(" : ")[1] for l in want)) > 200   # not trivially short, rows differ
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]
    assert len(got) == len(want)


def _cd(a, b):
    return -(-a // b)


def _expected(layout, w, h):
    """The geom line's numbers from (hs, vs) alone."""
    hs, vs = FACTORS[layout]
    size = [(w, h), (_cd(w, hs), _cd(h, vs))]                   # ceil(size * samp / max): chroma's samp is 1
    blocks = [(_cd(cw, 8), _cd(ch, 8)) for cw, ch in size]
    coef = [128 * blocks[0][0] * blocks[0][1], 128 * blocks[1][0] * blocks[1][1]]
    plane = [size[0][0] * size[0][1], size[1][0] * size[1][1]]
    mw, mh = _cd(w, 8 * hs), _cd(h, 8 * vs)
    per_mcu = hs * vs + 2
    full = [size[0][0], size[0][1], blocks[0][0], blocks[0][1], size[1][0], size[1][1], blocks[1][0], blocks[1][1],
            0, coef[0], coef[0] + coef[1], 0, plane[0], plane[0] + plane[1], coef[0] + 2 * coef[1],
            plane[0] + 2 * plane[1], mw, mh, per_mcu, mw * mh * per_mcu]
    scaled = []
    for s in (1, 2, 4, 8):
        ny = nc = 8 // s
        while nc < 8 and (hs * ny) % (2 * nc) == 0 and (vs * ny) % (2 * nc) == 0:   # jdmaster.c: both ratios allow
            nc *= 2
        pw = [_cd(w * hs * ny, hs * 8), _cd(w * nc, hs * 8)]
        ph = [_cd(h * vs * ny, vs * 8), _cd(h * nc, vs * 8)]
        scaled.append([ny, nc, pw[0], ph[0], pw[1], ph[1], 0, pw[0] * ph[0], pw[0] * ph[0] + pw[1] * ph[1],
                       pw[0] * ph[0] + 2 * pw[1] * ph[1]])
    return full, scaled


def test_struct_follows_libjpegs_sampling_rule(exe):
    lines = subprocess.run([exe, "geom"], capture_output=True, text=True, check=True).stdout.splitlines()
    geom = [l for l in lines if l.startswith("geom ")]
    most = [l for l in lines if l.startswith("max ")]
    assert len(geom) == 3 * 40 * 40 + 3 * 4 and len(most) == 40 * 40
    seen = set()
    for l in geom:
        head, body = l.split(" : ")
        layout, w, h = (int(v) for v in head.split()[1:])
        parts = [[int(v) for v in p.split()] for p in body.split(" | ")]
        full, scaled = _expected(layout, w, h)
        assert parts[0] == full, (l, full)
        assert parts[1:] == scaled, (l, scaled)
        seen.add((layout, w, h))
    assert (3, 8, 16) in seen and (3, 3840, 2160) in seen   # 4:2:2's one block across, even blocks down
    for l in most:
        head, body = l.split(" : ")
        w, h = (int(v) for v in head.split()[1:])
        out, inp = ([int(v) for v in p.split()] for p in body.split(" | "))
        # the structs' maxima are what the two workspaces report ...
        assert out[:2] == out[2:] and inp[:2] == inp[2:], l
        # ... and are the most of the layouts each serves
        cap = {k: _expected(k, w, h)[0][14] for k in FACTORS}
        blk = {k: _expected(k, w, h)[0][19] for k in FACTORS}
        assert out[:2] == [max(cap[0], cap[1]), max(blk[0], blk[1])], l
        assert inp[:2] == [max(cap.values()), max(blk.values())], l
