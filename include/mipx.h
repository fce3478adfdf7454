/*
 * mipx.h — C-ABI of the MI355X pixel-transform engine (libmipx.so).
 *
 * Drop-in for the pixel work inside imaginary's Process() (reference
 * image.go:81-113): today Process calls bimg.Resize(buf, opts) (image.go:96),
 * which decodes, runs the libvips pixel ops and encodes in one call.  With the
 * engine, the host keeps libvips decode/encode and hands DECODED pixels plus a
 * plan (built from the same bimg.Options fields that options.go:128-172 and the
 * image.go operation wrappers set) to this library.  A Go shim binds these
 * entry points through cgo.
 *
 * Conventions
 *  - Every entry point returns 0 (MIPX_OK) or a negative MIPX_E* code; nothing
 *    aborts or throws across the ABI.  MIPX_EUNSUPPORTED means "the plan needs
 *    an op the engine does not implement": the caller falls back to
 *    bimg.Resize for that request (SURVEY.md §5 failure handling).
 *  - Images are interleaved uchar, `bands` 1..4, rows `stride` bytes apart
 *    (stride 0 = w * bands).
 *  - mipx_submit copies the input into pinned staging before it returns (cgo
 *    pointer rule: no Go pointer is retained); the output buffer must stay
 *    valid until mipx_wait returns a FINAL status for the ticket (anything but
 *    MIPX_ETIMEOUT) or mipx_cancel returns for it.  After MIPX_ETIMEOUT the
 *    request is still queued or running and will still write the output: wait
 *    again, or call mipx_cancel before freeing the buffer.
 *  - Plans are validated before use: every step's out_w/out_h/out_bands must be
 *    what its op makes from the previous step's geometry (MIPX_EINVAL otherwise),
 *    and a watermark image (or rendered text mask) must have the watermark step's geometry.
 *  - All mipx_op_* / mipx_execute_dev entry points take DEVICE pointers to a
 *    batch of n equally sized images packed back to back, and a hipStream_t
 *    passed as void* (NULL = the device's default engine stream).  They only
 *    enqueue work; they never synchronise or allocate.
 *  - Footprint of those entry points (pinned by tests/test_footprint_gpu.py): they
 *    read only the n * w * h * bands input bytes and the watermark image, and write
 *    only the output bytes and the first mipx_[op_]workspace_bytes() bytes of the
 *    workspace.  The image pointers may have any byte alignment, with one exception:
 *    on 4-band images mipx_op_rot and mipx_op_embed (and mipx_op_flip on images of
 *    2 GiB or more, or more than 65535 rows), per op or as a plan step, take 4-byte
 *    aligned input and output pointers only and return MIPX_EINVAL for others.
 *    A plan that starts with MIPX_OP_YCC, and mipx_op_ycc_to_rgb, read n * mipx_ycc_bytes()
 *    input bytes instead (packed JPEG planes, see MIPX_YCC_*), at any alignment.
 *    A plan that ends with MIPX_OP_JPEGC, and mipx_op_rgb_to_jpegc, write n * mipx_jpegc_bytes()
 *    output bytes instead (JPEG coefficients), at any alignment.
 *    A plan that ends with MIPX_OP_JPEGE, mipx_op_rgb_to_jpeg_scan and mipx_op_jpegc_to_scan write
 *    n * mipx_jpeg_scan_bytes() output bytes instead (entropy-coded scans), at any alignment; the _packed
 *    calls write, inside the same n slots' bytes, only each slot's header and scan at its directory offset.
 *    A plan that starts with MIPX_OP_JPEGD, and mipx_op_jpegd_to_rgb, read n * mipx_jpegd_bytes()
 *    input bytes instead (quantisation tables + JPEG coefficients), at any alignment.
 *    A plan that starts with MIPX_OP_JPEGH, and mipx_op_jpegh_to_*, read n slots of
 *    mipx_jpegh_bytes() instead (tables + a JPEG's entropy-coded scan), at any alignment, and of
 *    each slot only the header and the scan's `length` bytes.
 *  - Thread-safe: mipx_submit / mipx_wait / mipx_process may be called from
 *    many threads (one goroutine per HTTP request).
 */
#ifndef MIPX_H
#define MIPX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPX_ABI_VERSION 6

/* ---- error codes ---- */
#define MIPX_OK 0
#define MIPX_EINVAL (-1)         /* bad argument / geometry (libvips "bad extract area" etc.) */
#define MIPX_EUNSUPPORTED (-2)   /* op not implemented by the engine: fall back to bimg.Resize */
#define MIPX_ENOMEM (-3)
#define MIPX_ENODEV (-4)         /* no usable gfx950 device */
#define MIPX_EDEVICE (-5)        /* HIP runtime error (details: mipx_last_error()) */
#define MIPX_ETIMEOUT (-6)
#define MIPX_ENOTINIT (-7)
#define MIPX_ESTALE (-8)         /* unknown or already-waited ticket */
#define MIPX_EBUSY (-9)          /* refused while requests are queued or running */
#define MIPX_EDATA (-10)         /* input not decodable on the device (MIPX_OP_JPEGH: status not MIPX_JPEGH_OK) */

/* ---- bimg enums (bimg v1.1.9 options.go / type.go) ---- */
enum { MIPX_GRAVITY_CENTRE = 0, MIPX_GRAVITY_NORTH, MIPX_GRAVITY_EAST, MIPX_GRAVITY_SOUTH,
       MIPX_GRAVITY_WEST, MIPX_GRAVITY_SMART };
enum { MIPX_EXTEND_BLACK = 0, MIPX_EXTEND_COPY, MIPX_EXTEND_REPEAT, MIPX_EXTEND_MIRROR,
       MIPX_EXTEND_WHITE, MIPX_EXTEND_BACKGROUND, MIPX_EXTEND_LAST };
enum { MIPX_TYPE_UNKNOWN = 0, MIPX_TYPE_JPEG, MIPX_TYPE_WEBP, MIPX_TYPE_PNG, MIPX_TYPE_TIFF,
       MIPX_TYPE_GIF, MIPX_TYPE_PDF, MIPX_TYPE_SVG, MIPX_TYPE_MAGICK, MIPX_TYPE_HEIF,
       MIPX_TYPE_AVIF };

/* Mirror of the bimg.Options subset set by options.go:128-172 (BimgOptions) and
 * the image.go wrappers (Resize 115, Fit 139, Enlarge 202, Extract 213, Crop 226,
 * SmartCrop 236, Rotate 247, Flip 267, Flop 273, Thumbnail 279, Zoom 286,
 * WatermarkImage 343, GaussianBlur 372).  Booleans are 0/1. */
typedef struct mipx_opts {
    int32_t width, height;          /* bimg Width/Height */
    int32_t area_width, area_height;/* bimg AreaWidth/AreaHeight (Extract, Zoom) */
    int32_t top, left;              /* bimg Top/Left */
    int32_t crop, embed, enlarge, force;
    int32_t no_auto_rotate;         /* bimg NoAutoRotate (options.go:137) */
    int32_t rotate;                 /* bimg Rotate: bimg.Angle(o.Rotate) (options.go:145) */
    int32_t flip, flop;
    int32_t gravity;                /* MIPX_GRAVITY_* */
    int32_t extend;                 /* MIPX_EXTEND_*; imaginary default ExtendCopy (params.go:342,356) */
    int32_t background[3];          /* options.go:151-153 */
    int32_t zoom;                   /* bimg Zoom (image.go:308) */
    double sigma, min_ampl;         /* bimg GaussianBlur (options.go:164-169) */
    int32_t smart_crop;             /* bimg SmartCrop */
    int32_t wm_enable;              /* WatermarkImage present (image.go:364-367) */
    int32_t wm_left, wm_top;
    float wm_opacity;               /* 0 -> 1.0 as bimg does */
    int32_t interpretation;         /* bimg Interpretation at save (options.go:142): 0 or
                                       sRGB = keep, MIPX_INTERPRETATION_BW = vips_colourspace B_W */
} mipx_opts;

#define MIPX_INTERPRETATION_SRGB 22 /* VIPS_INTERPRETATION_sRGB */
#define MIPX_INTERPRETATION_BW 26   /* VIPS_INTERPRETATION_B_W (params.go:392 colorspace=bw) */

/* What the host codec knows about the encoded input. */
typedef struct mipx_input {
    int32_t w, h, bands;            /* header size and bands of the encoded image */
    int32_t type;                   /* MIPX_TYPE_*; JPEG/WEBP allow shrink-on-load */
    int32_t orientation;            /* EXIF orientation 0..8 */
    int32_t decoded_w, decoded_h;   /* size the codec produced at plan.load_shrink (0 = ceil) */
    int32_t wm_w, wm_h, wm_bands;   /* decoded watermark image, when opts.wm_enable */
} mipx_input;

/* Plan steps: the libvips ops bimg would run, in order. */
enum {
    MIPX_OP_ROT = 1,     /* a[0] = angle 0/90/180/270 clockwise              (vips_rot) */
    MIPX_OP_FLIP,        /* a[0] = 0 horizontal mirror, 1 vertical           (vips_flip) */
    MIPX_OP_SHRINK,      /* a[0] = hshrink, a[1] = vshrink (integer box)     (vips_shrink) */
    MIPX_OP_REDUCE,      /* d[0] = hshrink, d[1] = vshrink, Lanczos3; a[7] = MIPX_SAMPLE_*  (vips_reduce) */
    MIPX_OP_EXTRACT,     /* a[0..3] = left, top, width, height               (vips_extract_area) */
    MIPX_OP_EMBED,       /* a[0..3] = x, y, w, h; a[4] = extend; a[5..7] bg  (vips_embed) */
    MIPX_OP_SMARTCROP,   /* a[0..1] = width, height, attention; a[7] = MIPX_SAMPLE_*  (vips_smartcrop) */
    MIPX_OP_BLUR,        /* d[0] = sigma, d[1] = min_ampl                    (vips_gaussblur) */
    MIPX_OP_WATERMARK,   /* a[0..1] = left, top; d[0] = opacity  (bimg vips_watermark_image) */
    MIPX_OP_AFFINE,      /* d[0] = xscale, d[1] = yscale, a[0] = extend; bicubic  (vips_affine) */
    MIPX_OP_ZOOM,        /* a[0] = xfac, a[1] = yfac                         (vips_zoom) */
    MIPX_OP_FLATTEN,     /* a[0..2] = background rgb                         (vips_flatten) */
    MIPX_OP_BW,          /* sRGB -> B_W                                      (vips_colourspace) */
    MIPX_OP_TEXTMARK,    /* a[0..1] = mask w, h; a[2] = margin; a[3..5] = colour; d[0] = opacity after
                            defaulting; out_bands = 3; the rendered text mask travels as the request's
                            watermark image (a[0] x a[1] x 1)              (bimg vips_watermark) */
    MIPX_OP_YCC,         /* a[0] = MIPX_YCC_*; out_bands = 3; only as step 0 of a 3-band plan, whose input
                            buffer is then the packed planes (mipx_plan_set_ycc_input)
                                                     (libjpeg upsample + colour conversion) */
    MIPX_OP_JPEGC,       /* a[0] = MIPX_YCC_*, a[1] = quality 1..100; out_w/out_h/out_bands = the image it
                            consumes (w, h, 3); only as the LAST step of a plan whose image there has 3
                            bands (MIPX_YCC_GREY: 1 band, and out_bands = 1); the output buffer is then
                            the quantised coefficients
                            (mipx_plan_set_jpegc_output)
                                  (libjpeg colour conversion, downsample, forward DCT, quantisation) */
    MIPX_OP_JPEGD,       /* a[0] = MIPX_YCC_*; out_bands = 3; only as step 0 of a 3-band plan (MIPX_YCC_GREY:
                            out_bands = 1, of a 1-band plan), never together with MIPX_OP_YCC; the input buffer is then the file's quantisation tables and
                            quantised coefficients (mipx_plan_set_jpegd_input)
                                  (libjpeg dequantisation, inverse DCT, upsample, colour conversion)
                            a[1] = shrink: 0 or 1 decode at full size; 2, 4, 8 decode at that fraction
                            (libjpeg's shrink-on-load), and then a[2], a[3] = the file's width and height,
                            the payload is that file's, and the plan's in_w x in_h must be
                            ceil(a[2] / a[1]) x ceil(a[3] / a[1]) (mipx_plan_set_jpegd_input_scaled);
                            any other a[1] is MIPX_EINVAL */
    MIPX_OP_JPEGRT,      /* = 18, the JPEG round trip: a[0] = MIPX_YCC_*, a[1] = quality 1..100, a[2] = shrink
                            (0 or 1 full size; 2, 4, 8); on a 3-band image at any index of a plan; out =
                            ceil(w / shrink) x ceil(h / shrink) x 3: the pixels the JPEG of the image at that
                            quality decodes to at that scale (mipx_plan_add_jpeg_roundtrip)
                                  (MIPX_OP_JPEGC's rule, then MIPX_OP_JPEGD's with the same tables) */
    MIPX_OP_JPEGE,       /* = 19, the entropy-coded scan: a[0] = MIPX_YCC_*, a[1] = quality 1..100, a[2] = 0 for
                            the Annex K Huffman tables or 1 for the image's own optimised ones (any other value
                            is MIPX_EINVAL: this tightens a word that was ignored); out_w/out_h/
                            out_bands = the image it consumes (w, h, 3); only as the LAST step of a plan whose
                            image there has 3 bands (MIPX_YCC_GREY: 1 band, and out_bands = 1), never
                            together with MIPX_OP_JPEGC; the output buffer is
                            then one slot per image (mipx_plan_set_jpeg_scan_output)
                                  (MIPX_OP_JPEGC's rule, then libjpeg's baseline Huffman coder) */
    MIPX_OP_JPEGH        /* = 20, entropy-coded JPEG input (see MIPX_JPEGH_HEADER_BYTES): a[] exactly as
                            MIPX_OP_JPEGD (layout; shrink 0 or 1, or 2, 4, 8 with the file's size in a[2], a[3]);
                            only as step 0, never beside MIPX_OP_YCC or MIPX_OP_JPEGD, in a chain in stage 0
                            only; the input buffer is then one slot per image (mipx_plan_set_jpegh_input)
                                  (libjpeg's baseline Huffman decoder, then MIPX_OP_JPEGD's rule) */
};

/* Planar YCbCr input, as a JPEG decoder has it before its upsample and colour conversion
 * (libjpeg jpeg_read_raw_data, TurboJPEG tjDecompressToYUVPlanes).  One image is Y, h rows
 * of w bytes, then Cb, then Cr, ch rows of cw bytes each: no row, plane or image padding, so
 * planes and images start on any byte.  MIPX_YCC_444: cw = w, ch = h.  MIPX_YCC_420:
 * cw = ceil(w / 2), ch = ceil(h / 2).  MIPX_YCC_422 (libjpeg's h2v1, what most cameras write):
 * cw = ceil(w / 2), ch = h.  The engine upsamples 4:2:0 chroma as libjpeg's default "fancy"
 * h2v2 upsampler does and 4:2:2 chroma as its h2v1 one does (both plain replication when
 * cw <= 2) and converts with libjpeg's integer YCbCr -> RGB, bit for bit
 * (PARITY_ASSUMPTIONS.md rows 16 and 25).  MIPX_YCC_422 is an input layout only: every call
 * and plan step that writes a JPEG (MIPX_OP_JPEGC, MIPX_OP_JPEGE, MIPX_OP_JPEGRT) rejects it.
 * The value 2 is deliberately unused: it has always been an unknown layout and stays one.
 *    MIPX_YCC_GREY is a one-component (greyscale) JPEG: its single plane is the 1-band image, so
 * there is nothing to upsample or convert, and MIPX_OP_YCC and MIPX_OP_JPEGRT reject it.  The steps
 * that read or write a file take it (MIPX_OP_JPEGD, MIPX_OP_JPEGH, MIPX_OP_JPEGC, MIPX_OP_JPEGE),
 * on 1 band only, and their out_bands is then 1: grey goes with 1 band and the other layouts with
 * 3, every other pairing is MIPX_EINVAL (PARITY_ASSUMPTIONS.md row 26).  Its value is 6 because
 * -1, 2, 4, 5, 7 and 1 << 20 have always been unknown layouts and stay so. */
enum { MIPX_YCC_444 = 0, MIPX_YCC_420 = 1, MIPX_YCC_422 = 3, MIPX_YCC_GREY = 6 };

/* JPEG coefficient output (MIPX_OP_JPEGC): what a JPEG encoder has in front of its entropy
 * coder, so the host only Huffman-codes (libjpeg jpeg_write_coefficients).  The same two
 * layouts name the file's sampling.  One image is the quantised DCT coefficients of the real
 * blocks only, int16 little-endian: component Y, then Cb, then Cr; each component hb x wb
 * blocks in raster order; each block 64 coefficients in natural (row-major) order, i.e.
 * libjpeg's coefficient arrays.  Y (and 4:4:4 chroma): wb = ceil(w / 8), hb = ceil(h / 8).
 * 4:2:0 chroma: wb = ceil(ceil(w / 2) / 8), hb = ceil(ceil(h / 2) / 8).  4:2:2 chroma (input
 * only; mipx_jpegc_bytes sizes it because the input payloads are made of it):
 * wb = ceil(ceil(w / 2) / 8), hb = ceil(h / 8).  The blocks that pad a partial MCU in 4:2:0
 * and 4:2:2 (zero AC, DC copied) are the entropy coder's and are not emitted.  The
 * engine computes libjpeg's integer RGB -> YCbCr, its h2v2 downsample, the "islow" forward DCT
 * and the quantisation with the tables of jpeg_set_quality(quality, TRUE), bit for bit
 * (PARITY_ASSUMPTIONS.md row 17); images and both pointers start on any byte.
 *    MIPX_YCC_GREY (libjpeg's JCS_GRAYSCALE): the input is 1-band pixels, w * h bytes per image, and
 * the output is Y's blocks alone, 128 * ceil(w / 8) * ceil(h / 8) bytes: sample - 128 with the last
 * column and row repeated, the same forward DCT, the luminance table (PARITY_ASSUMPTIONS.md row 26).
 * Grey goes with 1 band and the other layouts with 3: every other pairing is MIPX_EINVAL. */
/* JPEG coefficient input (MIPX_OP_JPEGD): what a JPEG decoder has behind its entropy decoder
 * (libjpeg jpeg_read_coefficients), so the host only Huffman-decodes.  One image is a 384-byte
 * header followed by the coefficients.  The header is the file's quantisation tables of Y, Cb and
 * Cr, each 64 little-endian uint16 values in natural (row-major) order, of which 1..255 are legal
 * (8-bit tables); they travel with the image because they are the file's own, so requests with
 * the same plan and different tables still batch.  The coefficients are exactly what
 * MIPX_OP_JPEGC writes, mipx_jpegc_bytes(w, h, layout) bytes: int16 little-endian, the real
 * blocks only (the shim drops the blocks that pad a partial MCU), Y then Cb then Cr, blocks in
 * raster order, natural order inside a block.  The engine dequantises (the low 16 bits of
 * coefficient * divisor, signed), runs libjpeg's "islow" inverse DCT (jidctint.c; pass 1 down the
 * columns saturated to int16, pass 2 along the rows, + 128, clamped to 0..255) and then upsamples
 * and converts as MIPX_OP_YCC does.  The result is libjpeg-turbo's for every file an encoder
 * writes; where a sum saturates or wraps (corrupt or hand-made coefficients) it is the rule's,
 * which tests/jpegd_ref.py restates, not the library's (PARITY_ASSUMPTIONS.md row 18).  Images
 * and both pointers start on any byte.
 *    The same payload decodes at 1/2, 1/4 and 1/8 as libjpeg's scaled decode does (jdmaster.c,
 * jidctred.c; what jpeg_read_coefficients gives does not depend on the scale).  The output is
 * ceil(w / s) x ceil(h / s).  Y and 4:4:4 chroma blocks get the 4 x 4, 2 x 2 or 1 x 1 inverse
 * DCT; 4:2:0 chroma blocks get the next larger one (8 x 8, 4 x 4, 2 x 2), so chroma comes out at
 * the output size and nothing is upsampled; the conversion is the 4:4:4 one.  4:2:2 chroma
 * blocks get the same inverse DCT as Y (jdmaster.c enlarges a component's only when both of
 * its sampling ratios allow it), so chroma comes out ceil(h / s) high and ceil(ceil(w / s) / 2)
 * wide, the MIPX_YCC_422 planes of the decoded size, and is upsampled as MIPX_OP_YCC does at
 * that size; at 1 / 8 by plain replication at every width, as libjpeg switches the fancy
 * upsampler off there.  Bit for bit libjpeg-turbo's on files an encoder writes,
 * tests/jpegds_ref.py's rule elsewhere (PARITY_ASSUMPTIONS.md rows 19 and 25).
 *    MIPX_YCC_GREY: the 384-byte header stays; only its first 128 bytes (Y's table) are read and the
 * host writes zeros behind them.  Then Y's coefficients: hb x wb blocks in raster order, natural order
 * inside a block.  The step is step 0 of a 1-band plan and its out_bands is 1: the decoded plane,
 * ceil(w / s) x ceil(h / s) from the 8 / s point inverse DCT, is the image, written straight to the
 * step's output (at 1 / 8 it is the block grid's DC terms).  The op calls write n * ow * oh bytes.
 * The workspace a 3-band call needs stays sufficient and is still asked for (row 26). */
/* JPEG round trip (MIPX_OP_JPEGRT): what re-encoding an image as a JPEG and decoding that file
 * does to its pixels, as imaginary's /pipeline does between stages and bimg does before a rotated
 * JPEG shrinks on load, without the file: exactly MIPX_OP_JPEGC's rule at (layout, quality), then
 * exactly MIPX_OP_JPEGD's rule on those coefficients at scale 1 / shrink with the tables of
 * jpeg_set_quality(quality, TRUE).  Blocks are independent, so the coefficients stay on the chip.
 * Bit for bit libjpeg-turbo's encode -> decode (PARITY_ASSUMPTIONS.md row 20). */
/* Entropy-coded JPEG output (MIPX_OP_JPEGE): the finished scan of a baseline JPEG, so the host only
 * writes the header in front (SOI to SOS: a function of w, h, layout and quality) and FF D9 behind.
 * The engine codes exactly MIPX_OP_JPEGC's coefficients (PARITY_ASSUMPTIONS.md row 21): one
 * interleaved scan without restart markers; the four Huffman tables of Annex K.3, Y with tables
 * 0/0, Cb and Cr with 1/1; MCU order Y Cb Cr (4:4:4) or Y00 Y01 Y10 Y11 Cb Cr (4:2:0) over
 * ceil(w / 16) x ceil(h / 16) MCUs; libjpeg's dummy blocks where the Y blocks do not fill the
 * MCUs (zero AC; the DC of the block to the left or, in a wholly dummy block row, of the last block
 * of the same MCU's row above); bits packed most significant first, the last byte padded with
 * 1-bits, every 0xFF byte followed by 0x00.
 *    One image's output is a slot of mipx_jpeg_scan_bytes(w, h, layout) = 16 +
 * mipx_jpegc_bytes(w, h, layout) bytes: four little-endian uint32 (length, status, bits, 0), then
 * `length` scan bytes; the slot's bytes behind them are unspecified.  bits is the scan's length in
 * bits before padding and stuffing (saturating at 2^32 - 1).  status MIPX_JPEG_SCAN_OK: the scan is
 * there.  MIPX_JPEG_SCAN_OVERFLOW: it does not fit the slot; length is then ceil(bits / 8), a lower
 * bound of the need, the data bytes are unspecified, and the caller asks for coefficients instead
 * (a coefficient can cost 26 bits and stuffing can double them, so no capacity short of about 416
 * bytes per block excludes this; the slot keeps the size of the coefficients it replaces).
 * MIPX_JPEG_SCAN_UNCODABLE: a coefficient has no Annex K code (an AC magnitude above 1023 or a DC
 * difference above 2047 in magnitude, which MIPX_OP_JPEGC never makes of 8-bit pixels); length is 0;
 * it wins over OVERFLOW.  Nothing outside the slot is ever written; slots and both pointers start
 * on any byte.
 *    With optimised tables (a[2] = 1, mipx_plan_set_jpeg_scan_output_optimized, the _optimized op
 * calls; PARITY_ASSUMPTIONS.md row 24) the scan is coded with the four tables libjpeg's
 * optimize_coding makes of the image's own symbol counts (jpeg_gen_optimal_table, tie-breaks
 * included; Y counts into DC 0 / AC 0, Cb and Cr together into DC 1 / AC 1), and the slot carries
 * them: mipx_jpeg_scan_opt_bytes(w, h, layout) = MIPX_JPEG_SCAN_OPT_HEADER_BYTES +
 * mipx_jpegc_bytes(w, h, layout) bytes.  The first 16 bytes are (length, status, bits, 1); at byte 16
 * stand four tables of 272 bytes, DC 0, DC 1, AC 0, AC 1, each the DHT's 16 counts and then the
 * symbols, zero-padded: the layout of a MIPX_OP_JPEGH slot at byte 416, so one copies into the
 * other; the scan starts at byte 1104.  The statuses mean what they mean above (a value without an
 * Annex K code has no code here either); when the status is not OK the tables are unspecified.
 * A scan of 64 x blocks >= 10^9 (libjpeg's search starts there) is MIPX_EINVAL for this variant.
 *    MIPX_YCC_GREY: the input is 1-band pixels (n * w * h bytes) or Y's coefficients alone, and the scan
 * is the one libjpeg writes for JCS_GRAYSCALE: not interleaved, ceil(w / 8) x ceil(h / 8) MCUs of one
 * block each in raster order, no dummy blocks, tables 0/0.  The 16- and 1104-byte headers stay; with
 * optimised tables DC 0 and AC 0 stand at their places and the places of DC 1 and AC 1 are all zero,
 * which is "a table the file does not define" in a MIPX_OP_JPEGH slot, so one still copies into the
 * other.  The host writes one DQT, an SOF0 and an SOS of one component, and DHT DC 0 and AC 0 only.
 *    Packed slots (mipx_op_rgb_to_jpeg_scan_packed, mipx_op_jpegc_to_scan_packed; what the request path
 * downloads): the same slots back to back in the same output buffer, each rounded up to 16 bytes, behind a
 * directory of n + 1 uint64 byte offsets; a slot is then its header (and tables) and its `length` bytes, a
 * slot that is not OK its header alone, and no other byte of the buffer is written.  mipx_jpeg_scan_unpack
 * takes one slot out of a downloaded buffer on the host. */
#define MIPX_JPEG_SCAN_HEADER_BYTES 16
#define MIPX_JPEG_SCAN_OPT_HEADER_BYTES 1104
enum { MIPX_JPEG_SCAN_OK = 0, MIPX_JPEG_SCAN_OVERFLOW = 1, MIPX_JPEG_SCAN_UNCODABLE = 2 };
#define MIPX_JPEGD_HEADER_BYTES 384
/* Entropy-coded JPEG input (mipx_op_jpegh_*): the file's scan bytes instead of its coefficients, a
 * fifth to a third of their size, so the host only reads markers.  The engine decodes a baseline
 * (or extended sequential) Huffman scan of three components, one interleaved scan with or without
 * restart intervals, into exactly MIPX_OP_JPEGD's payload (PARITY_ASSUMPTIONS.md rows 22 and 23).
 *    One image's input is a slot of mipx_jpegh_bytes(w, h, layout) = MIPX_JPEGH_HEADER_BYTES +
 * mipx_jpegc_bytes(w, h, layout) bytes, all fields little-endian, starting on any byte:
 *      0  uint32 length: bytes of entropy-coded data behind the header, exactly as in the file
 *         between the SOS segment and FF D9 (stuffed, restart markers included)
 *      4  uint32 restart: the file's DRI value Ri in MCUs, 0 for a file without one; then two uint32
 *         zeros.  With M the scan's MCUs (ceil(w/8) ceil(h/8) for 4:4:4, ceil(w/16) ceil(h/16) for
 *         4:2:0, ceil(w/16) ceil(h/8) for 4:2:2, whose MCU is Y left, Y right, Cb, Cr) and
 *         K = ceil(M / Ri): Ri = 0, or Ri <= 65535 with K = 1, is an ordinary scan
 *         without a marker.  Ri <= 65535 with K >= 2: the scan is K intervals with K - 1 two-byte
 *         markers between them, marker k (from 0) FF D0 + (k & 7); interval k holds the MCUs k Ri ..
 *         min((k + 1) Ri, M) - 1, starts on a byte boundary with the DC predictors 0, and is decoded
 *         by a decoder of its own: the bits behind its last block are ignored
 *     16  384 bytes: the quantisation tables of Y, Cb, Cr, as in MIPX_OP_JPEGD's payload
 *    400  6 bytes: DC table index of Y, Cb, Cr, then AC table index of Y, Cb, Cr (0 or 1); 10 zeros
 *    416  four tables of 272 bytes, DC 0, DC 1, AC 0, AC 1: the DHT's 16 counts, then up to 256
 *         symbols, zero-padded; a table the file does not define is all zero
 *   1504  the scan
 * Bytes of the slot past `length` are never read.  Per image a status comes back:
 * MIPX_JPEGH_OK: the payload holds what jpeg_read_coefficients gives for the file.
 * MIPX_JPEGH_UNSYNCED: the decoders, started at every 128th byte of the unstuffed scan, did not
 * agree on the codeword boundaries within the fixed number of launches (scans of more than 64
 * KiB almost without end-of-block codes); the caller decodes on the host instead.  Never reported
 * for a scan of K >= 2 restart intervals, whose boundaries are its markers.
 * MIPX_JPEGH_BAD: not decodable: length above the capacity; restart above 65535; in an ordinary
 * scan an FF that no 00 follows (a marker, a restart marker, a fill byte, the last byte); in a scan
 * of K >= 2 intervals an FF that neither 00 nor D0..D7 follows (the last byte included), a number
 * of markers other than K - 1, marker k with another value than D0 + (k & 7), an interval that ends
 * before its last block (an empty one too); code counts that sum past 256 or overflow a length;
 * a table index above 1; a code that is in no table; a run and value that pass coefficient 63; a
 * DC symbol above 15; a scan that ends before its last block; a DC outside int16.  (A run of 16
 * zeros that passes coefficient 63 ends the block, as in libjpeg.)  Bits behind the last block are
 * ignored.  The payload of an image whose status is not OK is unspecified, but every write stays
 * inside it.
 *    MIPX_YCC_GREY: a scan of one component, which is not interleaved.  The 1504-byte header stays:
 * Y's quantisation table at byte 16 with zeros behind it; byte 400 is Y's DC table index and byte
 * 403 its AC index, and the other four bytes are ignored; all four table places may be filled,
 * because a file may define table 1 and use it.  M = ceil(w / 8) ceil(h / 8) MCUs of one block each
 * in raster order, no dummy blocks; a restart interval counts blocks; the DC predictor is the one
 * component's.  Every status and every BAD condition keeps its meaning.  The payload is
 * MIPX_OP_JPEGD's for the layout, and the op calls that go on to pixels write n * ow * oh bytes. */
#define MIPX_JPEGH_HEADER_BYTES 1504
enum { MIPX_JPEGH_OK = 0, MIPX_JPEGH_UNSYNCED = 1, MIPX_JPEGH_BAD = 2 };

#define MIPX_MAX_STEPS 64   /* room for a merged /pipeline chain (mipx_plan_chain) */
typedef struct mipx_step {
    int32_t op;
    int32_t a[8];
    double d[4];
    int32_t out_w, out_h, out_bands;
} mipx_step;

typedef struct mipx_plan {
    int32_t load_shrink;            /* codec shrink-on-load the HOST applies (1,2,4,8) */
    int32_t in_w, in_h, in_bands;   /* decoded image the engine receives */
    int32_t out_w, out_h, out_bands;
    int32_t n_steps;
    mipx_step steps[MIPX_MAX_STEPS];
} mipx_plan;

typedef struct mipx_img {
    uint8_t *data;
    int32_t w, h, bands;
    int64_t stride;                 /* bytes between rows; 0 = w * bands */
} mipx_img;

typedef struct mipx_cfg {
    int32_t n_devices;              /* 0 = every visible device */
    int32_t device_ids[16];
    int64_t staging_bytes;          /* pinned staging kept cached for reuse; 0 = default (1 GiB) */
    int32_t max_batch;              /* requests fused into one launch; 0 = default (64) */
    int32_t batch_wait_us;          /* bounded wait for more requests; 0 = none */
    int32_t queues_per_device;      /* request queues (worker + 3 streams each) per device; 0 = 1 */
} mipx_cfg;

/* ---- library / devices ---- */
const char *mipx_version(void);
/* Build identity: the first 16 hex digits of the SHA-256 of the engine sources this
 * library was compiled from (imaginary_amd/csrc/ + include/mipx.h; imaginary_amd/srchash.py). */
const char *mipx_build_id(void);
int mipx_abi_version(void);
const char *mipx_strerror(int code);
const char *mipx_last_error(void);      /* thread-local detail of the last failure */
/* NULL = defaults.  Already up: MIPX_OK for NULL or the running configuration,
 * MIPX_EINVAL (with mipx_last_error) for a different one — mipx_shutdown first. */
int mipx_init(const mipx_cfg *cfg);
void mipx_shutdown(void);
int mipx_device_count(void);

/* ---- host planner (bimg resizer.go restated; callable without a GPU) ---- */
int mipx_plan_make(const mipx_opts *opts, const mipx_input *in, mipx_plan *plan);
/* /pipeline GPU-resident fusion (image.go:379-410 Pipeline): concatenate the plans of
 * a pipeline's stages (stage k planned on stage k-1's output, decoded intermediates)
 * into one plan, so the request path runs the chain with one upload, device-resident
 * intermediates and one download.  Stage k > 0 must take stage k-1's output geometry
 * and have load_shrink 1; at most one stage may carry a watermark step (WATERMARK or
 * TEXTMARK: a request has one watermark image).  A stage whose file the reference would
 * write as a JPEG ends with MIPX_OP_JPEGRT (mipx_plan_add_jpeg_roundtrip), which also does
 * the next stage's shrink-on-load.
 * MIPX_EUNSUPPORTED when the chain exceeds MIPX_MAX_STEPS or has two watermark stages
 * (the caller then runs the stages one by one). */
int mipx_plan_chain(const mipx_plan *stages, int32_t n_stages, mipx_plan *out);
/* Text watermark (imaginary image.go:322-341 Watermark, bimg watermarkImageWithText): the
 * host renders the text (vips_text) and the engine tiles and blends the 1-band mask
 * (MIPX_OP_TEXTMARK).  The step sits after the blur and before the watermark image,
 * flatten and B_W steps of a mipx_plan_make plan.  Both calls work without a GPU.
 * mipx_plan_textmark_geometry: the image at that insertion point, so the host can apply
 * bimg's text width default (floor(w / 6)) before it renders.
 * mipx_plan_add_textmark: inserts the step (opacity 0 -> 0.25, above 1 -> 1, as bimg).
 * MIPX_EINVAL for a non-positive mask size, a negative margin, a colour outside 0..255 or a
 * full plan; MIPX_EUNSUPPORTED (the caller falls back to bimg) when no_replicate is set,
 * when the image there has 2 or 4 bands (libvips refuses the 3-band colour against it),
 * when the plan already has a WATERMARK or TEXTMARK step (one watermark slot per request),
 * or when a 1-band image (which leaves the step with 3 bands) has steps after it. */
int mipx_plan_textmark_geometry(const mipx_plan *plan, int32_t *w, int32_t *h, int32_t *bands);
int mipx_plan_add_textmark(mipx_plan *plan, int32_t mask_w, int32_t mask_h, int32_t margin, float opacity,
                           const int32_t *colour3, int32_t no_replicate);
/* Planar JPEG input (MIPX_YCC_*).  Both calls work without a GPU.
 * mipx_ycc_bytes: bytes of one w x h image's packed planes, w * h + 2 * cw * ch; 0 for a
 * non-positive size or an unknown layout.
 * mipx_plan_set_ycc_input: inserts the MIPX_OP_YCC step at index 0 of a 3-band plan (the other
 * steps move up).  The plan's geometry (in_w, in_h, in_bands, out_*) is unchanged; what
 * changes is the input buffer, which is then mipx_ycc_bytes(in_w, in_h, layout) bytes per
 * image for mipx_execute_dev, and for mipx_submit a mipx_img of w = in_w, h = in_h, bands = 3,
 * stride = 0 whose data is the packed planes (anything else is MIPX_EINVAL).  Use it on plans
 * with load_shrink 1 (the planes are the full-size decode).  In a mipx_plan_chain the step may
 * appear in stage 0 only.  MIPX_EINVAL for an unknown layout, in_bands != 3, a plan that
 * already starts with the step, or a full plan. */
size_t mipx_ycc_bytes(int32_t w, int32_t h, int32_t layout);
int mipx_plan_set_ycc_input(mipx_plan *plan, int32_t layout);
/* JPEG coefficient output (MIPX_OP_JPEGC, see MIPX_YCC_*).  The three calls work without a GPU.
 * mipx_jpegc_bytes: bytes of one w x h image's coefficients, 128 * its real blocks; 0 for a
 * non-positive size or an unknown layout.
 * mipx_plan_set_jpegc_output: appends the MIPX_OP_JPEGC step to a plan whose output has 3
 * bands.  The plan's geometry (in_*, out_w, out_h, out_bands) is unchanged; what changes is
 * the output buffer, which is then mipx_jpegc_bytes(out_w, out_h, layout) bytes per image for
 * mipx_execute_dev, and for mipx_submit a mipx_img of w = out_w, h = out_h, bands = 3,
 * stride = 0 whose data has that many bytes (anything else is MIPX_EINVAL).  The step is
 * legal only as a plan's last one; in a mipx_plan_chain it may appear in the last stage only.
 * MIPX_EINVAL for an unknown layout, a quality outside 1..100, out_bands != 3, a plan that
 * already ends with the step, or a full plan.
 * mipx_jpeg_qtables: the quantisation tables the coefficients of `quality` were made with, 64
 * values each in natural order (a DQT segment wants them in zigzag order); MIPX_EINVAL for
 * a quality outside 1..100 or a NULL table. */
size_t mipx_jpegc_bytes(int32_t w, int32_t h, int32_t layout);
int mipx_plan_set_jpegc_output(mipx_plan *plan, int32_t layout, int32_t quality);
int mipx_jpeg_qtables(int32_t quality, uint8_t lum[64], uint8_t chr[64]);
/* Entropy-coded JPEG output (MIPX_OP_JPEGE, see MIPX_JPEG_SCAN_HEADER_BYTES).  Both calls work
 * without a GPU.
 * mipx_jpeg_scan_bytes: bytes of one w x h image's output slot, 16 + mipx_jpegc_bytes(w, h,
 * layout); 0 for a non-positive size or an unknown layout.
 * mipx_plan_set_jpeg_scan_output: appends the MIPX_OP_JPEGE step to a plan whose output has 3
 * bands.  The plan's geometry is unchanged; the output buffer is then mipx_jpeg_scan_bytes(out_w,
 * out_h, layout) bytes per image for mipx_execute_dev, and for mipx_submit a mipx_img of w = out_w,
 * h = out_h, bands = 3, stride = 0 whose data has that many bytes (anything else is MIPX_EINVAL).
 * Composition rules and MIPX_EINVAL cases are mipx_plan_set_jpegc_output's: last step only, last
 * chain stage only, after planar or coefficient input, a text watermark and a round trip in either
 * call order; and MIPX_EINVAL for a plan that already ends with MIPX_OP_JPEGC or MIPX_OP_JPEGE
 * (mipx_plan_set_jpegc_output and mipx_plan_add_jpeg_roundtrip likewise refuse a plan that ends
 * with MIPX_OP_JPEGE).  The request path downloads each slot's header (and tables) and `length` bytes only,
 * and writes only those into the caller's buffer (MIPX_SCAN_TRIM=0 at mipx_init: whole slots).
 * mipx_jpeg_scan_opt_bytes and mipx_plan_set_jpeg_scan_output_optimized: the same for the step with
 * optimised Huffman tables (a[2] = 1), whose slots are MIPX_JPEG_SCAN_OPT_HEADER_BYTES +
 * mipx_jpegc_bytes(w, h, layout) bytes; also MIPX_EINVAL for an image of 10^9 / 64 scan blocks or more. */
size_t mipx_jpeg_scan_bytes(int32_t w, int32_t h, int32_t layout);
int mipx_plan_set_jpeg_scan_output(mipx_plan *plan, int32_t layout, int32_t quality);
size_t mipx_jpeg_scan_opt_bytes(int32_t w, int32_t h, int32_t layout);
int mipx_plan_set_jpeg_scan_output_optimized(mipx_plan *plan, int32_t layout, int32_t quality);
/* JPEG coefficient input (MIPX_OP_JPEGD, see MIPX_JPEGD_HEADER_BYTES).  Both calls work without a GPU.
 * mipx_jpegd_bytes: bytes of one w x h image's payload, 384 + mipx_jpegc_bytes(w, h, layout); 0
 * for a non-positive size or an unknown layout.
 * mipx_plan_set_jpegd_input: inserts the MIPX_OP_JPEGD step at index 0 of a 3-band plan (the
 * other steps move up).  The plan's geometry is unchanged; what changes is the input buffer,
 * which is then mipx_jpegd_bytes(in_w, in_h, layout) bytes per image for mipx_execute_dev, and
 * for mipx_submit a mipx_img of w = in_w, h = in_h, bands = 3, stride = 0 whose data is the
 * payload (anything else is MIPX_EINVAL).  Use it on plans with load_shrink 1
 * (mipx_plan_set_jpegd_input_scaled serves the others).  In a
 * mipx_plan_chain the step may appear in stage 0 only.  It composes with
 * mipx_plan_add_textmark and mipx_plan_set_jpegc_output in either call order.  MIPX_EINVAL,
 * with the plan untouched, for an unknown layout, in_bands != 3, a plan that already starts
 * with this step or with MIPX_OP_YCC, or a full plan (mipx_plan_set_ycc_input likewise refuses
 * a plan that starts with this step). */
size_t mipx_jpegd_bytes(int32_t w, int32_t h, int32_t layout);
int mipx_plan_set_jpegd_input(mipx_plan *plan, int32_t layout);
/* mipx_plan_set_jpegd_input for a file decoded at 1/shrink (libjpeg's shrink-on-load; works
 * without a GPU).  Plan as usual on the decoded size, in_w x in_h = ceil(file_w / shrink) x
 * ceil(file_h / shrink), then call this: the step at index 0 carries shrink and the file's size,
 * and the input buffer is the unchanged payload of the full-size file,
 * mipx_jpegd_bytes(file_w, file_h, layout) bytes per image (for mipx_submit a mipx_img of
 * w = in_w, h = in_h, bands = 3, stride = 0 with that payload as data).  shrink 1 gives exactly
 * the plan mipx_plan_set_jpegd_input gives.  Same composition rules and refusals as
 * mipx_plan_set_jpegd_input; also MIPX_EINVAL, with the plan untouched, for a shrink other than
 * 1, 2, 4, 8 and for a file size that does not give in_w x in_h at that shrink. */
int mipx_plan_set_jpegd_input_scaled(mipx_plan *plan, int32_t layout, int32_t shrink, int32_t file_w,
                                     int32_t file_h);
/* JPEG round trip (MIPX_OP_JPEGRT); works without a GPU.  Appends the step to a plan whose output
 * has 3 bands; out_w x out_h become ceil(out_w / shrink) x ceil(out_h / shrink) (shrink 0 or 1:
 * unchanged).  Input and output buffers stay pixels.  The step is legal at any index of a plan and
 * in any stage of a mipx_plan_chain: a caller whose next stage shrinks on load puts that shrink
 * into the step and plans the stage on the decoded size with load_shrink 1.
 * mipx_plan_add_textmark on a plan that ends with the step inserts before it (the file is made of
 * the marked image), and mipx_plan_set_jpegc_output may follow it.  MIPX_EINVAL, with the plan
 * untouched, for an unknown layout, a quality outside 1..100, a shrink other than 0, 1, 2, 4, 8,
 * out_bands != 3, an image whose coefficients or RGB are 2^32 bytes or more, a plan that ends with
 * MIPX_OP_JPEGC, or a full plan. */
int mipx_plan_add_jpeg_roundtrip(mipx_plan *plan, int32_t layout, int32_t quality, int32_t shrink);
/* imaginary image.go:190 calculateDestinationFitDimension */
int mipx_fit_dimension(int32_t image_w, int32_t image_h, int32_t fit_w, int32_t fit_h,
                       int32_t *out_w, int32_t *out_h);

/* ---- request API (host buffers; pinned staging, per-device queues, batching) ---- */
int mipx_submit(int device, const mipx_plan *plan, const mipx_img *in, const mipx_img *wm,
                mipx_img *out, uint64_t *ticket);   /* device < 0 = least loaded */
int mipx_wait(uint64_t ticket, int timeout_ms);      /* timeout < 0 = forever */
/* Detach a submitted request's output: once this returns, the engine never writes
 * the caller's output buffer for `ticket` (a copy already under way completes
 * first) and the ticket is released.  MIPX_ESTALE for an unknown ticket. */
int mipx_cancel(uint64_t ticket);
int mipx_process(const mipx_plan *plan, const mipx_img *in, const mipx_img *wm,
                 mipx_img *out);                     /* submit + wait */
/* Batches launched and requests retired so far on `device`, summed over its
 * queues (batching telemetry).  mipx_submit(device >= 0) picks the least-loaded
 * queue of that device; device < 0 the least-loaded queue of all. */
int mipx_stats(int device, uint64_t *batches, uint64_t *requests);
int mipx_queue_count(void);                           /* 0 before mipx_init */
/* The dispatch rule of mipx_submit, callable without a GPU: the queue (index into
 * the n_queues arrays) with the fewest pending bytes among those of `device`
 * (device < 0: among all), first on ties; MIPX_EINVAL when none qualifies. */
int mipx_pick_queue(int32_t device, const int32_t *queue_device, const int64_t *pending_bytes,
                    int32_t n_queues);
int mipx_queue_stats(int queue, int32_t *device, uint64_t *batches, uint64_t *requests,
                     int64_t *pending_bytes);         /* pending = queued input bytes */
/* What crosses the host link: the bytes the request path has enqueued in each direction on `queue`
 * since mipx_init, every copy counted (inputs, watermarks, outputs, MIPX_OP_JPEGH statuses, packed-scan
 * directories).  Either pointer may be NULL.  MIPX_ENOTINIT before mipx_init, MIPX_EINVAL for a queue
 * that does not exist. */
int mipx_transfer_stats(int queue, uint64_t *h2d_bytes, uint64_t *d2h_bytes);

/* ---- device-resident batch API ---- */
size_t mipx_workspace_bytes(const mipx_plan *plan, int32_t n);
int mipx_execute_dev(const mipx_plan *plan, int32_t n, const uint8_t *d_in, uint8_t *d_out,
                     const uint8_t *d_wm, void *d_workspace, size_t workspace_bytes,
                     void *stream);

/* Per-op kernels (each replaces one libvips operation).  n images of w x h x bands
 * packed back to back in and out; output geometry follows the libvips rule. */
int mipx_op_reduce(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                   int32_t bands, double hshrink, double vshrink, void *d_workspace,
                   size_t workspace_bytes, void *stream);
int mipx_op_reducev(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                    int32_t bands, double vshrink, void *stream);
int mipx_op_reduceh(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                    int32_t bands, double hshrink, void *stream);
int mipx_op_shrink(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                   int32_t bands, int32_t hshrink, int32_t vshrink, void *stream);
int mipx_op_embed(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                  int32_t bands, int32_t x, int32_t y, int32_t out_w, int32_t out_h,
                  int32_t extend, const int32_t *background3, void *stream);
int mipx_op_extract(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                    int32_t bands, int32_t left, int32_t top, int32_t out_w, int32_t out_h,
                    void *stream);
int mipx_op_rot(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                int32_t bands, int32_t angle, void *stream);
int mipx_op_flip(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                 int32_t bands, int32_t vertical, void *stream);
int mipx_op_gaussblur(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                      int32_t bands, double sigma, double min_ampl, void *d_workspace,
                      size_t workspace_bytes, void *stream);
int mipx_op_watermark(const uint8_t *d_base, const uint8_t *d_wm, uint8_t *d_out, int32_t n,
                      int32_t w, int32_t h, int32_t bands, int32_t wm_w, int32_t wm_h,
                      int32_t wm_bands, int32_t left, int32_t top, float opacity, void *stream);
/* The text watermark after rendering: d_mask is the rendered text, mask_w x mask_h x 1;
 * the output has 3 bands (a 1-band image is up-banded against the colour).
 * MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0, non-positive sizes, a
 * negative margin or a colour outside 0..255; MIPX_EUNSUPPORTED for 2 or 4 bands. */
int mipx_op_text_watermark(const uint8_t *d_in, const uint8_t *d_mask, uint8_t *d_out, int32_t n,
                           int32_t w, int32_t h, int32_t bands, int32_t mask_w, int32_t mask_h,
                           int32_t margin, float opacity, const int32_t *colour3, void *stream);
/* n images of packed planes (n * mipx_ycc_bytes(w, h, layout) bytes) -> n x h x w x 3 RGB; both
 * pointers at any alignment.  MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0, a
 * non-positive size or an unknown layout; MIPX_EUNSUPPORTED for an image of 2^32 / 3 pixels
 * or more (the kernel's byte offsets inside an image are 32-bit).  No workspace. */
int mipx_op_ycc_to_rgb(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                       int32_t layout, void *stream);
/* n x h x w x 3 RGB -> n images of JPEG coefficients (n * mipx_jpegc_bytes(w, h, layout) bytes);
 * both pointers at any alignment.  MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0,
 * a non-positive size, an unknown layout or a quality outside 1..100; MIPX_EUNSUPPORTED for an
 * image whose input or output is 2^32 bytes or more (the kernel's byte offsets inside an image
 * are 32-bit).  No workspace. */
int mipx_op_rgb_to_jpegc(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                         int32_t layout, int32_t quality, void *stream);
/* The entropy coder (MIPX_OP_JPEGE): n images of JPEG coefficients, as mipx_op_rgb_to_jpegc writes
 * them, -> n slots (n * mipx_jpeg_scan_bytes(w, h, layout) bytes); any int16 values are legal input
 * (see MIPX_JPEG_SCAN_UNCODABLE).  mipx_op_rgb_to_jpeg_scan runs mipx_op_rgb_to_jpegc into the
 * workspace first.  Input and output pointers at any alignment.  d_work: 16-byte aligned device
 * memory of mipx_op_workspace_bytes(MIPX_OP_JPEGE, n, w, h, 3, 0, 0) bytes (the coefficients, the scan
 * before stuffing, bit counts per block and their sums: about 12.3 bytes per pixel, sized for 4:4:4).  A call is a
 * memset and six launches; every dependency between workgroups is a launch boundary.  MIPX_EINVAL,
 * before any HIP call, for NULL pointers, n <= 0, a non-positive size, an unknown layout, a quality
 * outside 1..100 or a misaligned workspace; MIPX_EUNSUPPORTED for an image whose payload or RGB is
 * 2^32 bytes or more, as for mipx_op_jpegd_to_rgb. */
int mipx_op_jpegc_to_scan(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                          int32_t layout, void *d_work, void *stream);
int mipx_op_rgb_to_jpeg_scan(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                             int32_t layout, int32_t quality, void *d_work, void *stream);
/* The same two with optimised Huffman tables: n slots of mipx_jpeg_scan_opt_bytes(w, h, layout) bytes,
 * d_work of mipx_op_workspace_bytes(MIPX_OP_JPEGE, n, w, h, 3, 1.0, 0) bytes (8 KiB per image more: the
 * symbol counts and the codes), two more launches in front (the histogram, the tables).  Also
 * MIPX_EINVAL for an image of 10^9 / 64 scan blocks or more. */
int mipx_op_jpegc_to_scan_optimized(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                    int32_t layout, void *d_work, void *stream);
int mipx_op_rgb_to_jpeg_scan_optimized(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                       int32_t layout, int32_t quality, void *d_work, void *stream);
/* The same coder with its slots packed back to back, so that a caller downloads the scans and not the
 * capacity: the arguments of the unpacked calls, then optimize (0: Annex K tables, 1: optimised; any other
 * value is MIPX_EINVAL) and d_dir, device memory for n + 1 little-endian uint64 byte offsets
 * (mipx_jpeg_scan_packed_dir_bytes(n) = 8 (n + 1) bytes; 8-byte aligned, else MIPX_EINVAL).  d_out and
 * d_work have the sizes of the unpacked calls.  With head = 16, or 1104 with optimised tables:
 *   off[0] = 0,  off[i + 1] = off[i] + align16(head + (status_i == MIPX_JPEG_SCAN_OK ? length_i : 0))
 * Slot i stands at d_out + off[i] and is what the unpacked call writes, up to its `length`: the header
 * (the tables) and the scan.  A slot that is OVERFLOW or UNCODABLE is its header alone (an OVERFLOW
 * header's length is above the capacity and means no bytes).  Only [off[i], off[i] + head + length_i) is
 * written: not the pad bytes up to off[i + 1], nothing at or past off[n]; off[n] <= n slots' bytes.  One
 * launch of one workgroup more than the unpacked call; nothing is moved twice.
 * mipx_jpeg_scan_unpack, on the host and without a GPU: checks a downloaded directory (off[0] = 0,
 * non-decreasing, every step a multiple of 16 and >= head, off[n] <= packed_bytes), reads slot i's header
 * and copies head + (status == OK ? length : 0) bytes to `slot`, after checking that amount against
 * off[i + 1] - off[i] and slot_bytes.  MIPX_EINVAL for NULL pointers, n <= 0, i outside 0..n-1 or a head
 * that is neither size; MIPX_EDATA, with nothing written, for anything inconsistent. */
int mipx_op_jpegc_to_scan_packed(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                 int32_t layout, void *d_work, void *stream, int32_t optimize, uint64_t *d_dir);
int mipx_op_rgb_to_jpeg_scan_packed(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                    int32_t layout, int32_t quality, void *d_work, void *stream, int32_t optimize,
                                    uint64_t *d_dir);
size_t mipx_jpeg_scan_packed_dir_bytes(int32_t n);
int mipx_jpeg_scan_unpack(const uint64_t *dir, int32_t n, const uint8_t *packed, size_t packed_bytes, int32_t i,
                          size_t head, uint8_t *slot, size_t slot_bytes);
/* The entropy decoder (see MIPX_JPEGH_HEADER_BYTES): n slots (n * mipx_jpegh_bytes(w, h, layout)
 * bytes) -> n payloads of MIPX_OP_JPEGD (n * mipx_jpegd_bytes(w, h, layout) bytes) and n uint32
 * statuses (MIPX_JPEGH_*).  mipx_jpegh_bytes works without a GPU: MIPX_JPEGH_HEADER_BYTES +
 * mipx_jpegc_bytes(w, h, layout), 0 where that is 0.  Slots, payloads and pixels at any alignment;
 * d_status 4-byte aligned; d_ws 16-byte aligned device memory of at least
 * mipx_op_workspace_bytes(MIPX_OP_JPEGH, n, w, h, 3, 0, 0) bytes (one size for the three calls and
 * both layouts: the unstuffed scans, the decoders' states, the DC differences, and for the calls
 * that go on to pixels the payloads and MIPX_OP_JPEGD's planes; w, h the file's size).
 * mipx_op_jpegh_to_rgb[_scaled] run the decoder and then mipx_op_jpegd_to_rgb[_scaled]; the pixels
 * of an image whose status is not OK are unspecified, the other images are unaffected.  A call is
 * three memsets and 11 launches (13 to pixels); every dependency between workgroups is a launch
 * boundary, nothing is read back.  MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0, a
 * non-positive size, an unknown layout or shrink, a misaligned or short workspace, a misaligned
 * d_status; MIPX_EUNSUPPORTED for an image whose coefficients are 2^29 bytes or more (bit offsets
 * are 32-bit) or whose RGB is 2^32 bytes or more. */
size_t mipx_jpegh_bytes(int32_t w, int32_t h, int32_t layout);
/* Entropy-coded JPEG input of a plan (MIPX_OP_JPEGH).  Both calls work without a GPU; they are
 * mipx_plan_set_jpegd_input[_scaled] with the slot in the payload's place: the same composition
 * rules and MIPX_EINVAL cases, and the four calls (and mipx_plan_set_ycc_input) refuse a plan that
 * one of them already changed.  The input buffer is mipx_jpegh_bytes(file_w, file_h, layout) bytes
 * per image.  mipx_execute_dev leaves the n statuses (uint32, MIPX_JPEGH_*) in the first 4 n
 * bytes of its workspace; the pixels of an image whose status is not MIPX_JPEGH_OK are
 * unspecified, the other images of the batch are unaffected.  mipx_submit takes a mipx_img of
 * w = in_w, h = in_h, bands = 3, stride = 0 whose data is the slot; it reads `length` on the host
 * (above the capacity: MIPX_EINVAL), stages and uploads only the header and `length` bytes, and
 * counts only those as the queue's pending bytes.  A request whose status is not MIPX_JPEGH_OK
 * completes with MIPX_EDATA from mipx_wait / mipx_process, its output is not written, and its
 * batch neighbours complete normally. */
int mipx_plan_set_jpegh_input(mipx_plan *plan, int32_t layout);
int mipx_plan_set_jpegh_input_scaled(mipx_plan *plan, int32_t layout, int32_t shrink, int32_t file_w, int32_t file_h);
int mipx_op_jpegh_to_jpegd(const uint8_t *d_slots, uint8_t *d_payloads, uint32_t *d_status, int32_t n, int32_t w,
                           int32_t h, int32_t layout, void *d_ws, size_t ws_bytes, void *stream);
int mipx_op_jpegh_to_rgb(const uint8_t *d_slots, uint8_t *d_out, uint32_t *d_status, int32_t n, int32_t w, int32_t h,
                         int32_t layout, void *d_ws, size_t ws_bytes, void *stream);
int mipx_op_jpegh_to_rgb_scaled(const uint8_t *d_slots, uint8_t *d_out, uint32_t *d_status, int32_t n, int32_t file_w,
                                int32_t file_h, int32_t layout, int32_t shrink, void *d_ws, size_t ws_bytes,
                                void *stream);
/* n payloads (n * mipx_jpegd_bytes(w, h, layout) bytes) -> n x h x w x 3 RGB; both pointers at any
 * alignment.  The workspace takes the decoded planes between the two launches (inverse DCT, then
 * the MIPX_OP_YCC kernels): mipx_op_workspace_bytes(MIPX_OP_JPEGD, n, w, h, 3, 0, 0) bytes.
 * MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0, a non-positive size, an unknown
 * layout or a workspace that is NULL or too small; MIPX_EUNSUPPORTED for an image whose payload
 * or RGB is 2^32 bytes or more (the kernels' byte offsets inside an image are 32-bit). */
int mipx_op_jpegd_to_rgb(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                         int32_t layout, void *d_workspace, size_t workspace_bytes, void *stream);
/* The same n payloads of file_w x file_h files decoded at 1/shrink -> n x oh x ow x 3 RGB with
 * ow = ceil(file_w / shrink), oh = ceil(file_h / shrink); shrink 1 forwards to
 * mipx_op_jpegd_to_rgb.  The workspace takes three ow x oh planes:
 * mipx_op_workspace_bytes(MIPX_OP_JPEGD, n, ow, oh, 3, 0, 0) bytes.  MIPX_EINVAL and
 * MIPX_EUNSUPPORTED as for mipx_op_jpegd_to_rgb (the RGB bound is on the output size), and
 * MIPX_EINVAL for a shrink other than 1, 2, 4, 8. */
int mipx_op_jpegd_to_rgb_scaled(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t file_w, int32_t file_h,
                                int32_t layout, int32_t shrink, void *d_workspace, size_t workspace_bytes,
                                void *stream);
/* n x h x w x 3 RGB -> n x oh x ow x 3 RGB with ow = ceil(w / shrink), oh = ceil(h / shrink)
 * (shrink 0 = 1): the JPEG round trip (MIPX_OP_JPEGRT); both pointers at any alignment.  One launch
 * makes the decoder's planes in the workspace, the MIPX_OP_YCC kernels make RGB of them:
 * mipx_op_workspace_bytes(MIPX_OP_JPEGRT, n, w, h, 3, shrink, 0) bytes, the planes', at most 3 per
 * input pixel.  MIPX_EINVAL, before any HIP call, for NULL pointers, n <= 0, a non-positive size,
 * an unknown layout, a quality outside 1..100, a shrink other than 0, 1, 2, 4, 8 or a workspace
 * that is NULL or too small; MIPX_EUNSUPPORTED for an image whose coefficients or RGB are 2^32
 * bytes or more (the kernels' byte offsets inside an image are 32-bit). */
int mipx_op_jpeg_roundtrip(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                           int32_t layout, int32_t quality, int32_t shrink, void *d_workspace,
                           size_t workspace_bytes, void *stream);
int mipx_op_affine(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                   int32_t bands, double xscale, double yscale, int32_t extend, void *stream);
int mipx_op_zoom(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                 int32_t bands, int32_t xfac, int32_t yfac, void *stream);
int mipx_op_flatten(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                    int32_t bands, const int32_t *background3, void *stream);
int mipx_op_colourspace_bw(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                           int32_t bands, void *stream);
/* writes n (left, top) int32 pairs to d_origins */
int mipx_op_smartcrop_origin(const uint8_t *d_in, int32_t *d_origins, int32_t n, int32_t w,
                             int32_t h, int32_t bands, int32_t crop_w, int32_t crop_h,
                             void *d_workspace, size_t workspace_bytes, void *stream);
size_t mipx_op_workspace_bytes(int32_t op, int32_t n, int32_t w, int32_t h, int32_t bands,
                               double p0, double p1);

/* ---- parity settings (PARITY_ASSUMPTIONS.md) ----
 * The sampling convention of libvips' Lanczos3 reduce (reducev.cpp / reduceh.cpp;
 * PARITY_ASSUMPTIONS.md row 1): MIPX_SAMPLE_CORNER, output o samples X = o * shrink,
 * or MIPX_SAMPLE_CENTRE, X = (o + 0.5) * shrink - 0.5.  Output sizes do not depend on it.
 * ABI v6: mipx_plan_make records the process setting in every REDUCE and SMARTCROP step
 * (a[7]), and a plan always executes under the convention it recorded (a cached plan
 * keeps its convention when the setting changes later; a zeroed a[7] is the corner
 * convention, any value but 0 / 1 is MIPX_EINVAL).  The per-op entry points
 * (mipx_op_reduce, _reducev, _reduceh, _smartcrop_origin) read the setting once per call.
 * The setter returns MIPX_EINVAL for a value other than the two; it also returns
 * MIPX_EBUSY when it sees mipx_submit requests queued or running.  That refusal is
 * advisory, not a guarantee: it counts mipx_submit work only (not mipx_execute_dev or the
 * per-op calls on a caller's stream) and a submit may land just after the check.  Nothing
 * depends on it: a plan's own a[7] decides its convention.  Set the convention once at
 * start-up. */
#define MIPX_SAMPLE_CORNER 0
#define MIPX_SAMPLE_CENTRE 1
int mipx_set_reduce_sampling(int32_t convention);
int mipx_reduce_sampling(void);

/* ---- engine tuning (tests and benchmarks) ----
 * Kernel-selection knobs (MIPX_* environment variables, e.g. MIPX_RCOL=0 for the
 * previous generic reduce) are read once, on first use.  Every knob only chooses
 * among kernels that give identical bytes; none changes a result.
 * mipx_tuning_reload() re-reads them; call it only between launches (A/B scripts,
 * tests). */
int mipx_tuning_reload(void);

/* ---- device memory helpers (so a binding needs no other HIP wrapper) ---- */
int mipx_set_device(int device);
int mipx_dev_malloc(void **ptr, size_t bytes);
int mipx_dev_free(void *ptr);
int mipx_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int mipx_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);
int mipx_memset_dev(void *d_dst, int value, size_t bytes);
int mipx_stream_sync(void *stream);
int mipx_device_sync(void);
int mipx_stream_create(void **stream);
int mipx_stream_destroy(void *stream);
/* HIP events, for timing on the engine's stream */
int mipx_event_create(void **event);
int mipx_event_destroy(void *event);
int mipx_event_record(void *event, void *stream);
int mipx_event_elapsed_ms(void *start, void *stop, float *ms);

#ifdef __cplusplus
}
#endif
#endif /* MIPX_H */
