"""k_reduce2x2's launch geometry, and which of its tiles touch no edge (csrc/reduce2_geom.h), on
the host, no GPU.  tests/c/reduce2_geom_host.cpp includes the header only.  It first checks the
launch the launcher takes from the header against a table of launches worked out by hand (C2's
12 x 45 tiles, the demand windows and the one- and two-chunk shapes of the GPU tests, rejected
windows).  Then it restates the tile's walk; over w 8..1400 (every residue mod 8), h 8..220, RGB and RGBA, the full image
and demand windows whose y0 is a multiple of 12, and output bases on and off the store alignment, it
demands for every tile that the predicate is true exactly when a brute-force walk of the tile finds
no row or pixel index outside the image, no item past x_end and every store offset aligned.  The
counts pin what the kernel's records rely on: C2 (3840 x 2160 x 3) has 10 x 43 interior tiles per
image, the existing small GPU shapes (644 x 98) have none, and the shapes of
tests/test_reduce2_interior_gpu.py have the tiles that file says they have."""
import os
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "imaginary_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "c", "reduce2_geom_host.cpp")


def _build(out, *flags):
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, SRC, "-o", str(out)],
                   check=True)
    return str(out)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("reduce2_geom") / "reduce2_geom_host")


def test_predicate_equals_the_brute_force_walk(exe):
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert lines[-1] == "ok"
    counts = dict(zip(lines[-2].split()[::2], (int(v) for v in lines[-2].split()[1::2])))
    # not trivially satisfied: thousands of launches, and tiles of both kinds among them
    assert counts["launches"] > 5000 and counts["interior"] > 5000 and counts["other"] > 5000, counts


def _count(exe, w, h, b):
    return int(subprocess.run([exe, "count", str(w), str(h), str(b)], capture_output=True, text=True,
                              check=True).stdout)


def test_c2_has_10_by_43_interior_tiles_and_the_small_shapes_none(exe):
    assert _count(exe, 3840, 2160, 3) == 10 * 43
    assert _count(exe, 644, 98, 3) == 0
    assert _count(exe, 246, 50, 4) == 0


@pytest.mark.parametrize("w,h,b,n", [(648, 100, 3, 1), (644, 100, 3, 0), (648, 99, 3, 0), (640, 100, 3, 0),
                                     (484, 100, 4, 1), (482, 100, 4, 0), (484, 99, 4, 0),
                                     (1288, 200, 3, 3 * 3), (968, 200, 4, 3 * 3)])
def test_the_gpu_tests_shapes_hold_the_tiles_they_name(exe, w, h, b, n):
    assert _count(exe, w, h, b) == n


def test_the_program_is_clean_under_the_host_sanitizers(tmp_path):
    """The same stand-alone program with -fsanitize=address,undefined, run directly."""
    san = _build(tmp_path / "reduce2_geom_host_san", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=undefined")
    out = subprocess.run([san], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "ok", out.stdout[-1000:] + out.stderr[-3000:]
