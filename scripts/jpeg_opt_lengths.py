#!/usr/bin/env python3
"""Scan bytes of one picture with the Annex K Huffman tables and with optimised ones
(mipx_op_rgb_to_jpeg_scan / mipx_op_rgb_to_jpeg_scan_optimized), one JSON line per setting:

    python scripts/jpeg_opt_lengths.py tests/golden/testdata/large.jpg

The picture's decoded pixels are coded at Q 75 in 4:2:0 and at Q 92 in 4:4:4.  Each line also says
whether header + tables + scan + EOI is the file the host writer makes of the same coefficients
(codec.encode_jpeg_coefs(..., tables="optimal")).  Needs a GPU.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import imaginary_amd as ia  # noqa: E402
from imaginary_amd import codec  # noqa: E402


def main():
    path = sys.argv[1]
    px = np.ascontiguousarray(codec.decode(open(path, "rb").read())[:, :, :3])
    h, w = px.shape[:2]
    for layout, q in ((codec.YCC_420, 75), (codec.YCC_444, 92)):
        plain = ia.rgb_to_jpeg_scan(px, layout, q)[0]
        opt = ia.rgb_to_jpeg_scan(px, layout, q, optimize=True)[0]
        a, b = plain[:16].view("<u4"), opt[:16].view("<u4")
        _, _, scan, tables = ia.scan_slot(opt, tables=True)
        body = codec.jpeg_from_scan(scan, w, h, layout, q, tables)
        coefs = ia.rgb_to_jpegc(px, layout, q)[0]
        same = body == codec.encode_jpeg_coefs(coefs, w, h, layout, q, tables="optimal")
        print(json.dumps({"image": os.path.basename(path), "w": w, "h": h, "layout": layout, "q": q,
                          "annex_k_length": int(a[0]), "optimized_length": int(b[0]), "statuses": [int(a[1]), int(b[1])],
                          "ratio": round(int(b[0]) / int(a[0]), 4), "file_equals_host_writer": same}), flush=True)


if __name__ == "__main__":
    main()
