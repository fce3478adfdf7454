#!/usr/bin/env python3
"""Request rate of a JPEG scan answer from C (tests/c/mipx_e2e_scan.c), the variants alternating in
one session: the scan answer with the trimmed download (MIPX_SCAN_TRIM=1) and with whole slots (=0,
the yardstick), the coefficient answer and the RGB answer, on two inputs: uniform noise, and
tests/golden/testdata/large.jpg's pixels scaled to 3840 x 2160.  One JSON line per run on stdout.

    python scripts/e2e_scan_ab.py [--rounds 4] [--requests 256] [--threads 16] [--inflight 2] [--max-batch 8]
"""
import argparse
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--requests", type=int, default=256, help="per caller thread and run")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--queues", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--max-batch", type=int, default=8)
    a = ap.parse_args()
    import numpy as np
    from PIL import Image
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "mipx_e2e_scan")
    lib = os.path.join(ROOT, "imaginary_amd")
    subprocess.run(["gcc", "-O2", "-std=c11", "-D_DEFAULT_SOURCE", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "mipx_e2e_scan.c"), "-L", lib, "-lmipx", "-lpthread",
                    "-Wl,-rpath," + lib, "-o", exe], check=True)
    raw = {"noise": os.path.join(tmp, "noise.rgb"), "large": os.path.join(tmp, "large.rgb")}
    np.random.default_rng(14).integers(0, 256, (2160, 3840, 3), dtype=np.uint8).tofile(raw["noise"])
    photo = Image.open(os.path.join(ROOT, "tests", "golden", "testdata", "large.jpg")).convert("RGB")
    np.asarray(photo.resize((3840, 2160), Image.BICUBIC), dtype=np.uint8).tofile(raw["large"])
    for _ in range(a.rounds):
        for name, path in raw.items():
            for trim, answer in (("1", "scan"), ("0", "scan"), ("1", "coefs"), ("1", "rgb")):
                r = subprocess.run([exe, answer, str(a.threads), str(a.requests), str(a.queues), str(a.inflight),
                                    str(a.max_batch), path], env=dict(os.environ, MIPX_SCAN_TRIM=trim),
                                   capture_output=True, text=True, timeout=300)
                if r.returncode:   # an engine error or a slot that is not OK: nothing further is started
                    sys.exit(f"mipx_e2e_scan {answer} on {name}: exit {r.returncode}: {r.stderr[-500:]}")
                print(r.stdout.strip().replace('"input": "file"', f'"input": "{name}"'), flush=True)


if __name__ == "__main__":
    main()
