"""The host table builders (csrc/mipx_tables.cpp) build byte for byte what the engine
uploaded before they were split from the runtime: tests/c/tables_host.cpp runs every
builder over a fixed parameter list (no HIP call, no GPU) and prints one hash per table;
tests/golden/tables_host.txt holds those hashes as computed by the device_* functions of
the commit before the split, compiled for the host with the four HIP calls they make
replaced by malloc / memcpy / free.  One line has changed since: colour_tables, when the
cube-root look-up went from cbrtf to the double cbrt that libvips calls
(tests/test_smartcrop_cpu.py compares that table with the formula entry by entry)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "imaginary_amd", "csrc")


def test_host_builders_match_the_recorded_tables(tmp_path):
    exe = tmp_path / "tables_host"
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    # -ffp-contract=off as the Makefile's %.cpp.o rule; mipx_planner.cpp reaches the HIP
    # headers through mipx_internal.h (declarations only: nothing of HIP is linked)
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
                    "-I", os.path.join(rocm, "include"), "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                    os.path.join(ROOT, "tests", "c", "tables_host.cpp"), os.path.join(CSRC, "mipx_tables.cpp"),
                    os.path.join(CSRC, "mipx_planner.cpp"), "-o", str(exe)], check=True)
    got = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    want = open(os.path.join(ROOT, "tests", "golden", "tables_host.txt")).read().splitlines()
    assert len(want) > 800 and sum(l.endswith(": none") for l in want) > 100   # the refusals are pinned too
    diff = [(g, w) for g, w in zip(got, want) if g != w]
    assert not diff, diff[:5]
    assert len(got) == len(want)
