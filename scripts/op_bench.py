#!/usr/bin/env python3
"""Time one libmipx op on a device-resident batch (HIP events on its stream) so
rocprofv3 passes see that kernel alone.

    python scripts/op_bench.py reducev --w 1024 --h 1024 --b 4 --n 512 --s 1.3333333333333333
    python scripts/op_bench.py textmark --w 3840 --h 2160 --b 3 --n 64
    python scripts/op_bench.py ycc420 --w 3840 --h 2160 --n 64
    python scripts/op_bench.py jpegc420 --w 3840 --h 2160 --n 64 --q 75
    python scripts/op_bench.py jpegd420 --w 3840 --h 2160 --n 64 --q 75
    python scripts/op_bench.py jpegds420 --w 3840 --h 2160 --n 64 --q 75 --shrink 4
    python scripts/op_bench.py jpegrt420 --w 3840 --h 2160 --n 64 --q 75
    python scripts/op_bench.py jpege420 --w 3840 --h 2160 --n 64 --q 75     (RGB -> entropy-coded scan)
    python scripts/op_bench.py jpegcs420 --w 3840 --h 2160 --n 64 --q 75    (the entropy coder alone)
    python scripts/op_bench.py jpege420 --w 3840 --h 2160 --n 64 --q 75 --optimize   (with optimised Huffman tables)
    python scripts/op_bench.py jpege420 --w 3840 --h 2160 --n 64 --q 75 --packed     (the slots packed back to back)
    python scripts/op_bench.py jpegh420 --w 3840 --h 2160 --n 64 --q 75     (entropy-coded scan -> RGB)
    python scripts/op_bench.py jpeghd420 --w 3840 --h 2160 --n 64 --q 75    (the entropy decoder alone)
    python scripts/op_bench.py jpegh420 --file tests/golden/testdata/large.jpg --n 64   (a photograph's scan)
    python scripts/op_bench.py jpeghd420 --w 3840 --h 2160 --n 64 --q 75 --restart 8    (a restart interval of 8 MCUs)
    python scripts/op_bench.py jpeghd420 --file tests/golden/testdata/large.jpg --n 64 --restart r1   (of one MCU row)
    python scripts/op_bench.py ycc422 --w 3840 --h 2160 --n 64              (4:2:2 planes -> RGB)
    python scripts/op_bench.py jpegds422 --w 3840 --h 2160 --n 64 --q 75 --shrink 4
    python scripts/op_bench.py jpeghd422 --w 3840 --h 2160 --n 64 --q 75 --restart 0   (4:2:2 scans are Pillow's: --restart)
    ops: reduce reducev reduceh shrink blur embed rot flip extract affine zoom textmark watermark ycc420 ycc444
         jpegc420 jpegc444 jpegd420 jpegd444 jpegds420 jpegds444 jpegrt420 jpegrt444
         jpege420 jpege444 jpegcs420 jpegcs444 jpegh420 jpegh444 jpeghd420 jpeghd444
         ycc422 jpegd422 jpegds422 jpegh422 jpeghd422 (input only; jpegh422 / jpeghd422 need --restart)
         jpegcgrey jpegdgrey jpegdsgrey jpegegrey jpegcsgrey jpeghgrey jpeghdgrey (MIPX_YCC_GREY: 1-band pixels)
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from imaginary_amd._abi import check, lib  # noqa: E402


def vips_round(v):
    import math
    return int(math.floor(v + 0.5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("op")
    ap.add_argument("--w", type=int, default=1024)
    ap.add_argument("--h", type=int, default=1024)
    ap.add_argument("--b", type=int, default=4)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--s", type=float, default=2.0, help="shrink / sigma / angle")
    ap.add_argument("--s2", type=float, default=0.0, help="vertical shrink (reduce/shrink); 0 = same")
    ap.add_argument("--ow", type=int, default=0)
    ap.add_argument("--oh", type=int, default=0)
    ap.add_argument("--extend", type=int, default=1)
    ap.add_argument("--mw", type=int, default=0, help="textmark / watermark: mask or watermark width (0 = w / 6)")
    ap.add_argument("--mh", type=int, default=0, help="textmark / watermark: mask or watermark height (0 = mw / 5)")
    ap.add_argument("--margin", type=int, default=-1, help="textmark: margin (-1 = the mask width, bimg's default)")
    ap.add_argument("--opacity", type=float, default=0.25)
    ap.add_argument("--q", type=int, default=75, help="jpegc420 / jpegc444 / jpegd* / jpegrt* : JPEG quality")
    ap.add_argument("--shrink", type=int, default=0, choices=[0, 1, 2, 4, 8],
                    help="jpegds420 / jpegds444: decode the w x h file's coefficients at 1/shrink (0 = 2); "
                         "jpegrt420 / jpegrt444: the round trip's decode at 1/shrink (0 = 1)")
    ap.add_argument("--file", default="", help="jpegh* / jpeghd*: n copies of this JPEG's scan instead of the coder's "
                                               "output on noise (sets w, h and the layout)")
    ap.add_argument("--restart", default=None,
                    help="jpegh* / jpeghd*: n copies of one file that Pillow writes at --q of the pixels (of --file, else "
                         "noise) with a restart interval of N MCUs, or of R MCU rows as rR; 0: the same file without "
                         "restart markers, the twin to compare with")
    ap.add_argument("--optimize", action="store_true",
                    help="jpege* / jpegcs*: optimised Huffman tables (the *_optimized calls; the slots carry the tables)")
    ap.add_argument("--packed", action="store_true",
                    help="jpege* / jpegcs*: the slots packed back to back behind a directory (the *_packed calls)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--ab", default="", help="KNOB=v1,v2,...: same-process A/B of a MIPX_* knob")
    ap.add_argument("--warm-ms", type=float, default=200.0, help="device-time warm-up; 0: none, one group (PMC runs)")
    ap.add_argument("--sampling", choices=["corner", "centre"], default=None,
                    help="reduce sampling convention (mipx_set_reduce_sampling); default: the library's")
    a = ap.parse_args()
    a.shrink = a.shrink or (1 if a.op.startswith("jpegrt") else 2)
    dev = torch.device("cuda", 0)
    check(lib.mipx_set_device(0))
    if a.sampling:
        check(lib.mipx_set_reduce_sampling({"corner": 0, "centre": 1}[a.sampling]))
    w, h, b, n = a.w, a.h, a.b, a.n
    s2 = a.s2 or a.s
    if a.op in ("reduce", "reducev", "reduceh"):
        ow = vips_round(w / a.s) if a.op != "reducev" else w
        oh = vips_round(h / s2) if a.op != "reduceh" else h
    elif a.op == "shrink":
        ow, oh = max(1, vips_round(w / a.s)), max(1, vips_round(h / s2))
    elif a.op == "affine":
        import math
        ow, oh = math.ceil(w * a.s), math.ceil(h * s2)
    elif a.op == "zoom":
        ow, oh = w * int(a.s), h * int(s2)
    elif a.op == "rot":
        ow, oh = (h, w) if int(a.s) % 180 == 90 else (w, h)
    elif a.op in ("embed", "extract"):
        ow, oh = a.ow or w, a.oh or h
    else:
        ow, oh = w, h
    ob = b
    mw = a.mw or max(1, w // 6)
    mh = a.mh or max(1, mw // 5)
    if a.op == "textmark":      # a text-like mask: a third of it covered, the rest 0
        ob = 3
        g = torch.Generator(device="cpu").manual_seed(1)
        m = torch.randint(0, 256, (mh * mw,), dtype=torch.uint8, generator=g)
        m[torch.rand(mh * mw, generator=g) > 0.35] = 0
        mask = m.to(dev)
    elif a.op == "watermark":   # an RGBA watermark image at (100, 100)
        ob = b if b in (2, 4) else b + 1
        mask = torch.randint(0, 256, (mh * mw * 4,), dtype=torch.uint8, device=dev)
    in_img = w * h * b          # input bytes of one image
    LAYOUT = {"420": 1, "444": 0, "422": 3, "rey": 6}   # MIPX_YCC_*, by the op's last three characters (grey)
    grey = a.op.endswith("grey")
    pb = 1 if grey else 3       # bands of the pixels beside a JPEG of the op's layout
    if a.op in ("ycc420", "ycc444", "ycc422"):   # packed JPEG planes in, RGB out
        b = ob = 3
        layout = LAYOUT[a.op[-3:]]
        in_img = lib.mipx_ycc_bytes(w, h, layout)
    out_img = ow * oh * ob      # output bytes of one image
    if a.op in ("jpegc420", "jpegc444", "jpegcgrey"):   # RGB in, quantised DCT coefficients out
        b = ob = pb             # "out" names the image the step consumes; its bytes are out_img
        layout = LAYOUT[a.op[-3:]]
        in_img, out_img = w * h * pb, lib.mipx_jpegc_bytes(w, h, layout)
    JPEGD = ("jpegd420", "jpegd444", "jpegd422", "jpegdgrey", "jpegds420", "jpegds444", "jpegds422", "jpegdsgrey")
    if a.op in JPEGD:   # quantisation tables + quantised DCT coefficients in, RGB out
        b = ob = pb
        layout = LAYOUT[a.op[-3:]]
        in_img = lib.mipx_jpegd_bytes(w, h, layout)
        if grey:
            out_img = ow * oh
        if a.op.startswith("jpegds"):   # ... at 1/shrink: the same payload, RGB at the decoded size
            ow, oh = -(-w // a.shrink), -(-h // a.shrink)
            out_img = ow * oh * pb
    if a.op in ("jpegrt420", "jpegrt444"):   # RGB in, RGB out at 1/shrink; the planes in between are not credited
        b = ob = 3
        layout = 1 if a.op == "jpegrt420" else 0
        ow, oh = -(-w // a.shrink), -(-h // a.shrink)
        in_img, out_img = w * h * 3, ow * oh * 3
    JPEGE = ("jpege420", "jpege444", "jpegegrey", "jpegcs420", "jpegcs444", "jpegcsgrey")
    if a.op in JPEGE:   # RGB (jpege*) or the encoder's coefficients (jpegcs*) in, one slot per image out
        b = ob = pb
        layout = LAYOUT[a.op[-3:]]
        in_img = w * h * pb if a.op.startswith("jpege") else lib.mipx_jpegc_bytes(w, h, layout)
        out_img = (lib.mipx_jpeg_scan_opt_bytes if a.optimize else lib.mipx_jpeg_scan_bytes)(w, h, layout)
    JPEGH = ("jpegh420", "jpegh444", "jpegh422", "jpeghgrey", "jpeghd420", "jpeghd444", "jpeghd422", "jpeghdgrey")
    file_slot = None
    if a.op in JPEGH:   # one input slot per image in; RGB (jpegh*) or MIPX_OP_JPEGD's payload (jpeghd*) out
        b = ob = pb
        layout = LAYOUT[a.op[-3:]]
        if layout == 3 and a.restart is None:
            raise SystemExit("4:2:2 scans are Pillow's: give --restart (0 for a file without markers)")
        if a.restart is not None:
            import io
            import numpy as np
            from PIL import Image, ImageFile
            from imaginary_amd import codec
            if a.file:
                px = codec.decode(open(a.file, "rb").read())[:, :, :3]
            else:
                px = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
            if grey:
                px = px[:, :, 1]
            kw = {}
            if a.restart.startswith("r"):
                kw = dict(restart_marker_rows=int(a.restart[1:]))
            elif int(a.restart):
                kw = dict(restart_marker_blocks=int(a.restart))
            ImageFile.MAXBLOCK = max(ImageFile.MAXBLOCK, 1 << 26)   # noise at a high quality is a long scan
            out = io.BytesIO()
            if grey:
                Image.fromarray(np.ascontiguousarray(px), "L").save(out, "JPEG", quality=a.q, **kw)
            else:
                Image.fromarray(np.ascontiguousarray(px)).save(out, "JPEG", quality=a.q, subsampling={0: 0, 1: 2, 3: 1}[layout], **kw)
            file_slot, layout = codec.jpeg_huff_slot(out.getvalue(), restart=True, h2v1=layout == 3, grey=grey)
            w, h = px.shape[1], px.shape[0]
            ow, oh = w, h
        elif a.file:
            from imaginary_amd import codec
            buf = open(a.file, "rb").read()
            hd = codec.header(buf)
            file_slot, layout = codec.jpeg_huff_slot(buf, grey=grey)
            w, h, ow, oh = hd.w, hd.h, hd.w, hd.h
        in_img = lib.mipx_jpegh_bytes(w, h, layout)
        out_img = lib.mipx_jpegd_bytes(w, h, layout) if a.op.startswith("jpeghd") else w * h * pb
    margin = mw if a.margin < 0 else a.margin
    colour = (C.c_int32 * 3)(255, 128, 0)
    x = torch.randint(0, 256, (n * in_img,), dtype=torch.uint8, device=dev)
    y = torch.empty((n * out_img,), dtype=torch.uint8, device=dev)
    ws = torch.empty((n * max(w * h, ow * oh) * (3 if grey else b) + 4096,), dtype=torch.uint8, device=dev)   # grey: what a 3-band call brings
    if a.op in JPEGE:
        ws = torch.empty((lib.mipx_op_workspace_bytes(19, n, w, h, 3, 1.0 if a.optimize else 0.0, 0.0),), dtype=torch.uint8,
                         device=dev)
        directory = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    if a.op in JPEGH:
        import numpy as np
        ws = torch.empty((lib.mipx_op_workspace_bytes(20, n, w, h, 3, 0.0, 0.0),), dtype=torch.uint8, device=dev)
        status = torch.zeros((n,), dtype=torch.int32, device=dev)
        xv = x.view(n, in_img)
        if file_slot is not None:
            xv[:] = torch.from_numpy(file_slot).to(dev)
        else:
            # what the engine's own coder makes of random pixels at --q, behind that quality's tables and
            # the Annex K Huffman tables
            from imaginary_amd import codec
            lum, chrom = codec.jpeg_qtables(a.q)
            head = np.zeros(1504, np.uint8)
            if grey:   # Y's table and zeros behind it; bytes 400 and 403 name tables 0
                head[16:144] = np.array(lum, "<u2").view(np.uint8)
            else:
                head[16:400] = np.array([lum, chrom, chrom], "<u2").ravel().view(np.uint8)
                head[400:406] = [0, 1, 1, 0, 1, 1]
            for i, key in enumerate((0x00, 0x01, 0x10, 0x11)):
                counts, symbols = codec.HUFFMAN_TABLES[key]
                head[416 + 272 * i:432 + 272 * i] = list(counts)
                head[432 + 272 * i:432 + 272 * i + len(symbols)] = list(symbols)
            px = torch.randint(0, 256, (n * w * h * pb,), dtype=torch.uint8, device=dev)
            scans = torch.empty((n, in_img - 1504 + 16), dtype=torch.uint8, device=dev)
            ews = torch.empty((lib.mipx_op_workspace_bytes(19, n, w, h, 3, 0.0, 0.0),), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            assert lib.mipx_op_rgb_to_jpeg_scan(px.data_ptr(), scans.data_ptr(), n, w, h, layout, a.q, ews.data_ptr(), None) == 0
            check(lib.mipx_device_sync())
            assert int(scans[:, 4:8].max()) == 0, "a scan did not fit its slot"
            xv[:, :1504] = torch.from_numpy(head).to(dev)
            xv[:, :4] = scans[:, :4]
            xv[:, 1504:] = scans[:, 16:]
            del px, scans, ews
        torch.cuda.synchronize(dev)
    if a.op in ("jpegcs420", "jpegcs444", "jpegcsgrey"):
        # the coefficients the engine's own encoder makes of random pixels at --q, as for jpegd*
        px = torch.randint(0, 256, (n * w * h * pb,), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        assert lib.mipx_op_rgb_to_jpegc(px.data_ptr(), x.data_ptr(), n, w, h, layout, a.q, None) == 0
        check(lib.mipx_device_sync())
        del px
    if a.op in JPEGD:
        # what a decoder hands over: the coefficients the engine's own encoder makes of random pixels
        # at --q (zero runs and small values, not noise), behind that quality's tables
        import numpy as np
        lum, chrom = (C.c_uint8 * 64)(), (C.c_uint8 * 64)()
        assert lib.mipx_jpeg_qtables(a.q, lum, chrom) == 0
        head = np.concatenate([np.array(t, dtype="<u2") for t in (lum, chrom, chrom)]).view(np.uint8)
        if grey:
            head[128:] = 0      # Y's table alone
        px = torch.randint(0, 256, (n * w * h * pb,), dtype=torch.uint8, device=dev)
        coefs = torch.empty((n * (in_img - 384),), dtype=torch.uint8, device=dev)
        assert coefs.numel() == n * lib.mipx_jpegc_bytes(w, h, layout)
        torch.cuda.synchronize(dev)
        if layout == 3:
            # the engine writes no 4:2:2: the 4:4:4 coefficients of the same pixels, Y whole and of each chroma
            # component the left ceil(ceil(w / 2) / 8) block columns (an encoder's blocks of noise all the same)
            ywb, yhb, cwb = (w + 7) // 8, (h + 7) // 8, ((w + 1) // 2 + 7) // 8
            full = torch.empty((n, 3, yhb, ywb, 128), dtype=torch.uint8, device=dev)
            assert lib.mipx_op_rgb_to_jpegc(px.data_ptr(), full.data_ptr(), n, w, h, 0, a.q, None) == 0
            check(lib.mipx_device_sync())
            cv = coefs.view(n, in_img - 384)
            cv[:, :yhb * ywb * 128] = full[:, 0].reshape(n, -1)
            cv[:, yhb * ywb * 128:] = full[:, 1:, :, :cwb].reshape(n, -1)
            del full
        else:
            assert lib.mipx_op_rgb_to_jpegc(px.data_ptr(), coefs.data_ptr(), n, w, h, layout, a.q, None) == 0
            check(lib.mipx_device_sync())
        xv = x.view(n, in_img)
        xv[:, 384:] = coefs.view(n, in_img - 384)
        xv[:, :384] = torch.from_numpy(head).to(dev)
        torch.cuda.synchronize(dev)
        del px, coefs
    st = torch.cuda.current_stream(dev)
    sp = C.c_void_p(st.cuda_stream)
    X, Y, WS, WSB = x.data_ptr(), y.data_ptr(), ws.data_ptr(), ws.numel()
    bg = (C.c_int32 * 3)(10, 20, 30)

    def run():
        if a.op == "reduce":
            return lib.mipx_op_reduce(X, Y, n, w, h, b, a.s, s2, WS, WSB, sp)
        if a.op == "reducev":
            return lib.mipx_op_reducev(X, Y, n, w, h, b, s2, sp)
        if a.op == "reduceh":
            return lib.mipx_op_reduceh(X, Y, n, w, h, b, a.s, sp)
        if a.op == "shrink":
            return lib.mipx_op_shrink(X, Y, n, w, h, b, int(a.s), int(s2), sp)
        if a.op == "blur":
            return lib.mipx_op_gaussblur(X, Y, n, w, h, b, a.s, 0.2, WS, WSB, sp)
        if a.op == "embed":
            return lib.mipx_op_embed(X, Y, n, w, h, b, (ow - w) // 2, (oh - h) // 2, ow, oh, a.extend, bg, sp)
        if a.op == "extract":
            return lib.mipx_op_extract(X, Y, n, w, h, b, (w - ow) // 2, (h - oh) // 2, ow, oh, sp)
        if a.op == "rot":
            return lib.mipx_op_rot(X, Y, n, w, h, b, int(a.s), sp)
        if a.op == "flip":
            return lib.mipx_op_flip(X, Y, n, w, h, b, int(a.s), sp)
        if a.op == "affine":
            return lib.mipx_op_affine(X, Y, n, w, h, b, a.s, s2, a.extend, sp)
        if a.op == "zoom":
            return lib.mipx_op_zoom(X, Y, n, w, h, b, int(a.s), int(s2), sp)
        if a.op == "textmark":
            return lib.mipx_op_text_watermark(X, mask.data_ptr(), Y, n, w, h, b, mw, mh, margin, a.opacity, colour, sp)
        if a.op == "watermark":
            return lib.mipx_op_watermark(X, mask.data_ptr(), Y, n, w, h, b, mw, mh, 4, 100, 100, a.opacity, sp)
        if a.op in ("ycc420", "ycc444", "ycc422"):
            return lib.mipx_op_ycc_to_rgb(X, Y, n, w, h, layout, sp)
        if a.op in ("jpegc420", "jpegc444", "jpegcgrey"):
            return lib.mipx_op_rgb_to_jpegc(X, Y, n, w, h, layout, a.q, sp)
        if a.op in ("jpegd420", "jpegd444", "jpegd422", "jpegdgrey"):
            return lib.mipx_op_jpegd_to_rgb(X, Y, n, w, h, layout, WS, WSB, sp)
        if a.op in ("jpegds420", "jpegds444", "jpegds422", "jpegdsgrey"):
            return lib.mipx_op_jpegd_to_rgb_scaled(X, Y, n, w, h, layout, a.shrink, WS, WSB, sp)
        if a.op in ("jpegrt420", "jpegrt444"):
            return lib.mipx_op_jpeg_roundtrip(X, Y, n, w, h, layout, a.q, a.shrink, WS, WSB, sp)
        if a.op in ("jpege420", "jpege444", "jpegegrey") and a.packed:
            return lib.mipx_op_rgb_to_jpeg_scan_packed(X, Y, n, w, h, layout, a.q, WS, sp, int(a.optimize), directory.data_ptr())
        if a.op in ("jpegcs420", "jpegcs444", "jpegcsgrey") and a.packed:
            return lib.mipx_op_jpegc_to_scan_packed(X, Y, n, w, h, layout, WS, sp, int(a.optimize), directory.data_ptr())
        if a.op in ("jpege420", "jpege444", "jpegegrey"):
            if a.optimize:
                return lib.mipx_op_rgb_to_jpeg_scan_optimized(X, Y, n, w, h, layout, a.q, WS, sp)
            return lib.mipx_op_rgb_to_jpeg_scan(X, Y, n, w, h, layout, a.q, WS, sp)
        if a.op in ("jpegcs420", "jpegcs444", "jpegcsgrey"):
            if a.optimize:
                return lib.mipx_op_jpegc_to_scan_optimized(X, Y, n, w, h, layout, WS, sp)
            return lib.mipx_op_jpegc_to_scan(X, Y, n, w, h, layout, WS, sp)
        if a.op in ("jpegh420", "jpegh444", "jpegh422", "jpeghgrey"):
            return lib.mipx_op_jpegh_to_rgb(X, Y, status.data_ptr(), n, w, h, layout, WS, WSB, sp)
        if a.op in ("jpeghd420", "jpeghd444", "jpeghd422", "jpeghdgrey"):
            return lib.mipx_op_jpegh_to_jpegd(X, Y, status.data_ptr(), n, w, h, layout, WS, WSB, sp)
        raise SystemExit(a.op)

    # warm-up of >= 200 ms of device time first: a fresh process's first milliseconds run
    # below the sustained clock (r03: a 20-launch run of a 0.2 ms kernel read 15-20 % slow
    # against the same kernel in a long same-process A/B); then the median of 5 groups
    def measure():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        check(run(), a.op)
        torch.cuda.synchronize()
        warm = 0.0
        while warm < a.warm_ms:
            e0.record(st)
            for _ in range(10):
                check(run(), a.op)
            e1.record(st)
            torch.cuda.synchronize()
            warm += e0.elapsed_time(e1)
        groups = []
        for _ in range(5 if a.warm_ms > 0 else 1):
            e0.record(st)
            for _ in range(a.iters):
                check(run(), a.op)
            e1.record(st)
            torch.cuda.synchronize()
            groups.append(e0.elapsed_time(e1) / a.iters)
        return sorted(groups)[len(groups) // 2]

    alg = n * (in_img + out_img)   # bytes = input + output
    line = {"op": a.op, "w": w, "h": h, "b": b, "n": n, "s": a.s, "s2": s2, "out": [ow, oh, ob],
            "sampling": ["corner", "centre"][lib.mipx_reduce_sampling()]}
    if a.op.startswith(("jpegds", "jpegrt")):
        line["shrink"] = a.shrink
    if not a.ab:
        ms = measure()
        if a.op in JPEGE and a.packed:   # what the directory says: the bytes a caller downloads of the n slots' bytes
            offs = directory.cpu().tolist()
            heads = [y[o:o + 16].cpu().numpy().view("<u4") for o in offs[:-1]]
            line.update(q=a.q, optimize=a.optimize, packed=True, packed_bytes=offs[-1], slots_bytes=n * out_img,
                        mean_length=round(sum(int(hd[0]) for hd in heads) / n, 1), statuses=sorted({int(hd[1]) for hd in heads}))
        elif a.op in JPEGE:   # what the slots say: the scans' mean length against the slot's capacity
            head = y.view(n, out_img)[:, :16].cpu().numpy().view("<u4")
            line.update(q=a.q, optimize=a.optimize, capacity=out_img - (1104 if a.optimize else 16), mean_length=round(float(head[:, 0].mean()), 1),
                        statuses=sorted(set(head[:, 1].tolist())))
        if a.op in JPEGH:   # the statuses, and what a request uploads next to its RGB
            lengths = x.view(n, in_img)[:, :4].cpu().numpy().view("<u4")
            if a.restart is not None:
                line.update(restart=a.restart, restart_mcus=int(x.view(n, in_img)[0, 4:8].cpu().numpy().view("<u4")[0]))
            line.update(q=a.q, file=os.path.basename(a.file), capacity=in_img - 1504,
                        mean_length=round(float(lengths.mean()), 1), upload_bytes=round(1504 + float(lengths.mean()), 1),
                        rgb_bytes=w * h * pb, statuses=sorted(set(status.cpu().tolist())))
        print(json.dumps({**line, "ms": round(ms, 4), "alg_GBps": round(alg / ms / 1e6, 1)}))
        return
    # same-process A/B: --ab KNOB=v1,v2,... interleaved over 2 rounds, output checked equal
    knob, vals = a.ab.split("=", 1)
    first = None
    for rnd in range(2):
        for v in vals.split(","):
            os.environ[knob] = v
            lib.mipx_tuning_reload()  # the library snapshots MIPX_* knobs
            ms = measure()
            same = None
            if rnd == 0:
                y.zero_()
                check(run(), a.op)
                torch.cuda.synchronize()
                if first is None:
                    first = y.clone()
                same = bool(torch.equal(y, first))
            print(json.dumps({**line, knob: v, "round": rnd, "ms": round(ms, 4), "alg_GBps": round(alg / ms / 1e6, 1),
                              "same_as_first": same}), flush=True)

if __name__ == "__main__":
    main()
