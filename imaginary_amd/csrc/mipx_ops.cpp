// mipx_ops.cpp — C-ABI per-op entry points (include/mipx.h mipx_op_*): argument
// checks, workspace accounting and dispatch to the kernel launchers.  Each
// entry point replaces one libvips operation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "device_common.h"
#include "mipx_internal.h"

namespace mipx {

size_t op_workspace_bytes(int op, int n, int w, int h, int bands, double p0, double p1) {
    if (n <= 0 || w <= 0 || h <= 0 || bands <= 0) return 0;
    switch (op) {
        case MIPX_OP_REDUCE: {  // generic path: reducev intermediate
            if (!(p1 > 1.0) || !(p0 > 1.0)) return 0;
            const int oh = out_size_reduce(h, p1);
            return align_up(static_cast<size_t>(n) * w * oh * bands);
        }
        case MIPX_OP_BLUR: return align_up(static_cast<size_t>(n) * w * h * bands);
        case MIPX_OP_SMARTCROP: return smartcrop_workspace_bytes(n, w, h, bands);
        // the decoded planes between the inverse DCT and the upsample + conversion, packed as
        // mipx_ycc_bytes; sized by the 4:4:4 bound, which needs no layout
        case MIPX_OP_JPEGD: return align_up(static_cast<size_t>(n) * w * h * 3);
        // the round trip's planes between its two launches: p0 = shrink (0 or 1: full size), three
        // planes of the decoded size at most
        case MIPX_OP_JPEGRT: {
            const size_t s = p0 > 1.0 ? static_cast<size_t>(p0) : 1;
            return align_up(static_cast<size_t>(n) * ((w + s - 1) / s) * ((h + s - 1) / s) * 3);
        }
        // the entropy coder's: the coefficients, the scan before stuffing, the per-block and
        // per-tile bit counts and their scans (JpegeWork); sized without the layout.  p0 = 1: with
        // optimised tables, the symbol counts and the codes per image too
        case MIPX_OP_JPEGE: return JpegeWork(n, w, h, p0 == 1.0).total;
        // the entropy decoder's: the unstuffed scans, the decoders' states and block counts, the DC
        // differences, and what the coefficient step behind it needs (JpeghWork); sized without the layout
        case MIPX_OP_JPEGH: return JpeghWork(n, w, h).total;
        default: return 0;
    }
}

}  // namespace mipx

using namespace mipx;

extern "C" {

size_t mipx_op_workspace_bytes(int32_t op, int32_t n, int32_t w, int32_t h, int32_t bands, double p0, double p1) {
    return op_workspace_bytes(op, n, w, h, bands, p0, p1);
}

int mipx_op_reducev(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                    double vshrink, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || !(vshrink >= 1.0)) return MIPX_EINVAL;
    const SamplingScope sampling;  // one convention for the whole call
    if (vshrink == 1.0) {
        return device_copy(d_out, d_in, static_cast<size_t>(n) * w * h * bands, as_stream(stream));
    }
    return reducev_launch(d_in, d_out, n, w, h, bands, vshrink, as_stream(stream));
}

int mipx_op_reduceh(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                    double hshrink, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || !(hshrink >= 1.0)) return MIPX_EINVAL;
    const SamplingScope sampling;  // one convention for the whole call
    if (hshrink == 1.0) {
        return device_copy(d_out, d_in, static_cast<size_t>(n) * w * h * bands, as_stream(stream));
    }
    return reduceh_launch(d_in, d_out, n, w, h, bands, hshrink, as_stream(stream));
}

int mipx_op_reduce(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                   double hshrink, double vshrink, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || !(hshrink >= 1.0) || !(vshrink >= 1.0))
        return MIPX_EINVAL;
    const SamplingScope sampling;  // one convention for the whole call (the enclosing plan step's, if any)
    hipStream_t st = as_stream(stream);
    if (reduce2_eligible(d_in, w, h, bands, hshrink, vshrink)) return reduce2_launch(d_in, d_out, n, w, h, bands, st);
    if (vshrink == 1.0) return mipx_op_reduceh(d_in, d_out, n, w, h, bands, hshrink, stream);
    if (hshrink == 1.0) return mipx_op_reducev(d_in, d_out, n, w, h, bands, vshrink, stream);
    {  // both axes: one fused launch, intermediate in LDS
        const int e = reduce_one_launch(d_in, d_out, n, w, h, bands, hshrink, vshrink, 0, 0,
                                        out_size_reduce(w, hshrink), out_size_reduce(h, vshrink), st);
        if (e != MIPX_EUNSUPPORTED) return e;
    }
    const size_t need = op_workspace_bytes(MIPX_OP_REDUCE, n, w, h, bands, hshrink, vshrink);
    if (!d_ws || ws_bytes < need) return MIPX_EINVAL;
    uint8_t *t = static_cast<uint8_t *>(d_ws);
    int e = reducev_launch(d_in, t, n, w, h, bands, vshrink, st);
    if (e) return e;
    return reduceh_launch(t, d_out, n, w, out_size_reduce(h, vshrink), bands, hshrink, st);
}

int mipx_op_shrink(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                   int32_t hshrink, int32_t vshrink, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || hshrink < 1 || vshrink < 1) return MIPX_EINVAL;
    return shrink_launch(d_in, d_out, n, w, h, bands, hshrink, vshrink, as_stream(stream));
}

int mipx_op_embed(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands, int32_t x,
                  int32_t y, int32_t ow, int32_t oh, int32_t extend, const int32_t *bg, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || ow <= 0 || oh <= 0) return MIPX_EINVAL;
    int b3[3] = {0, 0, 0};
    if (bg) b3[0] = bg[0], b3[1] = bg[1], b3[2] = bg[2];
    return embed_launch(d_in, d_out, n, w, h, bands, x, y, ow, oh, extend, b3, nullptr, as_stream(stream));
}

int mipx_op_extract(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                    int32_t left, int32_t top, int32_t ow, int32_t oh, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    if (left < 0 || top < 0 || ow <= 0 || oh <= 0 || left + ow > w || top + oh > h) {
        set_error("bad extract area %d,%d %dx%d of %dx%d", left, top, ow, oh, w, h);
        return MIPX_EINVAL;
    }
    return extract_launch(d_in, d_out, n, w, h, bands, left, top, ow, oh, as_stream(stream));
}

int mipx_op_rot(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands, int32_t angle,
                void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    return rot_launch(d_in, d_out, n, w, h, bands, angle, as_stream(stream));
}

int mipx_op_flip(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                 int32_t vertical, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    return flip_launch(d_in, d_out, n, w, h, bands, vertical, as_stream(stream));
}

int mipx_op_gaussblur(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                      double sigma, double min_ampl, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    return blur_launch(d_in, d_out, n, w, h, bands, sigma, min_ampl, d_ws, ws_bytes, as_stream(stream));
}

int mipx_op_watermark(const uint8_t *d_base, const uint8_t *d_wm, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                      int32_t bands, int32_t ww, int32_t wh, int32_t wb, int32_t left, int32_t top, float opacity,
                      void *stream) {
    if (!d_base || !d_wm || !d_out || !geom_ok(n, w, h, bands) || ww <= 0 || wh <= 0 || wb < 1 || wb > 4)
        return MIPX_EINVAL;
    return watermark_launch(d_base, d_wm, d_out, n, w, h, bands, ww, wh, wb, left, top, opacity, as_stream(stream));
}

int mipx_op_text_watermark(const uint8_t *d_in, const uint8_t *d_mask, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                           int32_t bands, int32_t mask_w, int32_t mask_h, int32_t margin, float opacity,
                           const int32_t *colour3, void *stream) {
    if (!d_in || !d_mask || !d_out || !colour3 || !geom_ok(n, w, h, bands) || mask_w <= 0 || mask_h <= 0 || margin < 0)
        return MIPX_EINVAL;
    for (int z = 0; z < 3; ++z)
        if (colour3[z] < 0 || colour3[z] > 255) return MIPX_EINVAL;
    return textmark_launch(d_in, d_mask, d_out, n, w, h, bands, mask_w, mask_h, margin, opacity, colour3,
                           as_stream(stream));
}

int mipx_op_ycc_to_rgb(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                       void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, 3) || !ycc_input_layout(layout)) return MIPX_EINVAL;
    return ycc_launch(d_in, d_out, n, w, h, layout, as_stream(stream));
}

int mipx_op_rgb_to_jpegc(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                         int32_t quality, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, 3) || !jpeg_output_layout(layout) || !jpeg_quality_ok(quality))
        return MIPX_EINVAL;
    return jpegc_launch(d_in, d_out, n, w, h, layout, quality, as_stream(stream));
}

// The checks the four entropy-coder calls share.
static int jpege_check(const char *what, const void *d_in, const void *d_out, const void *d_work, int32_t n, int32_t w,
                       int32_t h, int32_t layout, bool optimise) {
    if (!d_in || !d_out || !d_work || !geom_ok(n, w, h, 3) || !jpeg_output_layout(layout)) return MIPX_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_work) & 15u) {
        set_error("%s: the workspace is not 16-byte aligned", what);
        return MIPX_EINVAL;
    }
    // byte offsets inside an image are 32-bit in the kernels
    if (!jpeg_fits_32(JpegGeom(w, h, layout), w, h)) {
        set_error("%s: image %dx%d too large (an image's bytes >= 2^32)", what, w, h);
        return MIPX_EUNSUPPORTED;
    }
    if (optimise && !jpeg_opt_in_range(w, h, layout)) {
        set_error("%s: a %dx%d scan has 10^9 / 64 blocks or more", what, w, h);
        return MIPX_EINVAL;
    }
    return MIPX_OK;
}

// d_dir: nullptr for whole slots, else the packed slots' directory (device memory, 8-byte aligned)
static int jpegc_to_scan(const char *what, const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                         int32_t layout, bool optimise, void *d_work, void *stream, uint64_t *d_dir = nullptr) {
    const int e = jpege_check(what, d_coefs, d_out, d_work, n, w, h, layout, optimise);
    if (e) return e;
    return jpege_launch(d_coefs, d_out, n, w, h, layout, optimise, static_cast<uint8_t *>(d_work), as_stream(stream),
                        reinterpret_cast<unsigned long long *>(d_dir));
}

static int rgb_to_jpeg_scan(const char *what, const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                            int32_t layout, int32_t quality, bool optimise, void *d_work, void *stream,
                            uint64_t *d_dir = nullptr) {
    if (!jpeg_quality_ok(quality)) return MIPX_EINVAL;
    int e = jpege_check(what, d_in, d_out, d_work, n, w, h, layout, optimise);
    if (e) return e;
    uint8_t *work = static_cast<uint8_t *>(d_work);
    uint8_t *coefs = work + JpegeWork(n, w, h, optimise).coefs;  // packed as mipx_jpegc_bytes per image
    e = jpegc_launch(d_in, coefs, n, w, h, layout, quality, as_stream(stream));
    if (e) return e;
    return jpege_launch(coefs, d_out, n, w, h, layout, optimise, work, as_stream(stream),
                        reinterpret_cast<unsigned long long *>(d_dir));
}

// What the two packed calls check of their own arguments.
static int packed_check(const char *what, int32_t optimize, const uint64_t *d_dir) {
    if (!d_dir || (optimize != 0 && optimize != 1)) return MIPX_EINVAL;
    if (reinterpret_cast<uintptr_t>(d_dir) & 7u) {
        set_error("%s: the directory is not 8-byte aligned", what);
        return MIPX_EINVAL;
    }
    return MIPX_OK;
}

int mipx_op_jpegc_to_scan(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                          void *d_work, void *stream) {
    return jpegc_to_scan("jpeg coefficients to scan", d_coefs, d_out, n, w, h, layout, false, d_work, stream);
}

int mipx_op_jpegc_to_scan_optimized(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                    int32_t layout, void *d_work, void *stream) {
    return jpegc_to_scan("jpeg coefficients to optimised scan", d_coefs, d_out, n, w, h, layout, true, d_work, stream);
}

int mipx_op_rgb_to_jpeg_scan(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                             int32_t quality, void *d_work, void *stream) {
    return rgb_to_jpeg_scan("rgb to jpeg scan", d_in, d_out, n, w, h, layout, quality, false, d_work, stream);
}

int mipx_op_rgb_to_jpeg_scan_optimized(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                       int32_t layout, int32_t quality, void *d_work, void *stream) {
    return rgb_to_jpeg_scan("rgb to optimised jpeg scan", d_in, d_out, n, w, h, layout, quality, true, d_work, stream);
}

int mipx_op_jpegc_to_scan_packed(const uint8_t *d_coefs, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                 int32_t layout, void *d_work, void *stream, int32_t optimize, uint64_t *d_dir) {
    const char *what = "jpeg coefficients to packed scans";
    const int e = packed_check(what, optimize, d_dir);
    if (e) return e;
    return jpegc_to_scan(what, d_coefs, d_out, n, w, h, layout, optimize == 1, d_work, stream, d_dir);
}

int mipx_op_rgb_to_jpeg_scan_packed(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h,
                                    int32_t layout, int32_t quality, void *d_work, void *stream, int32_t optimize,
                                    uint64_t *d_dir) {
    const char *what = "rgb to packed jpeg scans";
    const int e = packed_check(what, optimize, d_dir);
    if (e) return e;
    return rgb_to_jpeg_scan(what, d_in, d_out, n, w, h, layout, quality, optimize == 1, d_work, stream, d_dir);
}

// The checks the three entropy-decoder calls share; *work: the workspace.
static int jpegh_check(const char *what, const void *d_slots, const void *d_out, const uint32_t *d_status, int32_t n,
                       int32_t w, int32_t h, int32_t layout, void *d_ws, size_t ws_bytes) {
    if (!d_slots || !d_out || !d_status || !d_ws || !geom_ok(n, w, h, 3) || !jpeg_input_layout(layout))
        return MIPX_EINVAL;
    if ((reinterpret_cast<uintptr_t>(d_ws) & 15u) || (reinterpret_cast<uintptr_t>(d_status) & 3u)) {
        set_error("%s: the workspace is not 16-byte aligned, or the statuses are not 4-byte aligned", what);
        return MIPX_EINVAL;
    }
    // bit offsets inside a scan are 32-bit in the kernels
    if (!jpeg_scan_fits_decoder(JpegGeom(w, h, layout)) || 3ull * w * h > 0xffffffffull) {
        set_error("%s: image %dx%d too large (a scan of 2^32 bits or more)", what, w, h);
        return MIPX_EUNSUPPORTED;
    }
    if (ws_bytes < op_workspace_bytes(MIPX_OP_JPEGH, n, w, h, 3, 0, 0)) {
        set_error("%s: workspace %zu < %zu bytes", what, ws_bytes, op_workspace_bytes(MIPX_OP_JPEGH, n, w, h, 3, 0, 0));
        return MIPX_EINVAL;
    }
    return MIPX_OK;
}

int mipx_op_jpegh_to_jpegd(const uint8_t *d_slots, uint8_t *d_payloads, uint32_t *d_status, int32_t n, int32_t w,
                           int32_t h, int32_t layout, void *d_ws, size_t ws_bytes, void *stream) {
    const int e = jpegh_check("jpeg scan to coefficients", d_slots, d_payloads, d_status, n, w, h, layout, d_ws, ws_bytes);
    if (e) return e;
    return jpegh_launch(d_slots, d_payloads, d_status, n, w, h, layout, static_cast<uint8_t *>(d_ws), as_stream(stream));
}

int mipx_op_jpegh_to_rgb_scaled(const uint8_t *d_slots, uint8_t *d_out, uint32_t *d_status, int32_t n, int32_t file_w,
                                int32_t file_h, int32_t layout, int32_t shrink, void *d_ws, size_t ws_bytes,
                                void *stream) {
    shrink = jpeg_scale(shrink);
    if (!jpeg_scale_ok(shrink)) return MIPX_EINVAL;
    int e = jpegh_check("jpeg scan to rgb", d_slots, d_out, d_status, n, file_w, file_h, layout, d_ws, ws_bytes);
    if (e) return e;
    const JpeghWork W(n, file_w, file_h);
    uint8_t *work = static_cast<uint8_t *>(d_ws);
    e = jpegh_launch(d_slots, work + W.payload, d_status, n, file_w, file_h, layout, work, as_stream(stream));
    if (e) return e;
    return mipx_op_jpegd_to_rgb_scaled(work + W.payload, d_out, n, file_w, file_h, layout, shrink, work + W.planes,
                                       W.total - W.planes, stream);
}

int mipx_op_jpegh_to_rgb(const uint8_t *d_slots, uint8_t *d_out, uint32_t *d_status, int32_t n, int32_t w, int32_t h,
                         int32_t layout, void *d_ws, size_t ws_bytes, void *stream) {
    return mipx_op_jpegh_to_rgb_scaled(d_slots, d_out, d_status, n, w, h, layout, 1, d_ws, ws_bytes, stream);
}

int mipx_op_jpegd_to_rgb(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                         void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, 3) || !jpeg_input_layout(layout)) return MIPX_EINVAL;
    // byte offsets inside an image are 32-bit in both kernels
    if (!jpeg_fits_32(JpegGeom(w, h, layout), w, h)) {
        set_error("jpeg coefficients to rgb: image %dx%d too large (an image's bytes >= 2^32)", w, h);
        return MIPX_EUNSUPPORTED;
    }
    if (!d_ws || ws_bytes < op_workspace_bytes(MIPX_OP_JPEGD, n, w, h, 3, 0, 0)) {
        set_error("jpeg coefficients to rgb: workspace %zu < %zu bytes", ws_bytes,
                  op_workspace_bytes(MIPX_OP_JPEGD, n, w, h, 3, 0, 0));
        return MIPX_EINVAL;
    }
    // grey: Y's plane is the 1-band image; nothing is upsampled or converted, the workspace stays idle
    if (layout == MIPX_YCC_GREY) return jpegd_launch(d_in, d_out, n, w, h, layout, as_stream(stream));
    uint8_t *planes = static_cast<uint8_t *>(d_ws);
    const int e = jpegd_launch(d_in, planes, n, w, h, layout, as_stream(stream));
    if (e) return e;
    return ycc_launch(planes, d_out, n, w, h, layout, as_stream(stream));
}

int mipx_op_jpegd_to_rgb_scaled(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t file_w, int32_t file_h,
                                int32_t layout, int32_t shrink, void *d_ws, size_t ws_bytes, void *stream) {
    if (shrink == 1) return mipx_op_jpegd_to_rgb(d_in, d_out, n, file_w, file_h, layout, d_ws, ws_bytes, stream);
    if (!d_in || !d_out || !geom_ok(n, file_w, file_h, 3) || !jpeg_input_layout(layout) || !jpeg_scale_ok(shrink))
        return MIPX_EINVAL;
    const int ow = static_cast<int>((static_cast<long long>(file_w) + shrink - 1) / shrink);
    const int oh = static_cast<int>((static_cast<long long>(file_h) + shrink - 1) / shrink);
    // byte offsets inside an image are 32-bit in both kernels
    if (!jpeg_fits_32(JpegGeom(file_w, file_h, layout), ow, oh)) {
        set_error("jpeg coefficients to rgb at 1/%d: image %dx%d too large (an image's bytes >= 2^32)", shrink, file_w,
                  file_h);
        return MIPX_EUNSUPPORTED;
    }
    if (!d_ws || ws_bytes < op_workspace_bytes(MIPX_OP_JPEGD, n, ow, oh, 3, 0, 0)) {
        set_error("jpeg coefficients to rgb at 1/%d: workspace %zu < %zu bytes", shrink, ws_bytes,
                  op_workspace_bytes(MIPX_OP_JPEGD, n, ow, oh, 3, 0, 0));
        return MIPX_EINVAL;
    }
    // three ow x oh planes: no upsampling at these scales; but of a 4:2:2 file its planes at the decoded
    // size, whose chroma libjpeg replicates at 1 / 8 whatever its width
    if (layout == MIPX_YCC_GREY)  // the one plane of ow x oh is the image
        return jpegds_launch(d_in, d_out, n, file_w, file_h, layout, shrink, as_stream(stream));
    uint8_t *planes = static_cast<uint8_t *>(d_ws);
    const int e = jpegds_launch(d_in, planes, n, file_w, file_h, layout, shrink, as_stream(stream));
    if (e) return e;
    if (layout == MIPX_YCC_422) return ycc_launch(planes, d_out, n, ow, oh, MIPX_YCC_422, as_stream(stream), shrink == 8);
    return ycc_launch(planes, d_out, n, ow, oh, MIPX_YCC_444, as_stream(stream));
}

int mipx_op_jpeg_roundtrip(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t layout,
                           int32_t quality, int32_t shrink, void *d_ws, size_t ws_bytes, void *stream) {
    shrink = jpeg_scale(shrink);
    if (!d_in || !d_out || !geom_ok(n, w, h, 3) || !ycc_output_layout(layout) || !jpeg_quality_ok(quality) ||
        !jpeg_scale_ok(shrink))
        return MIPX_EINVAL;
    // byte offsets inside an image are 32-bit in both kernels
    if (!jpeg_fits_32(JpegGeom(w, h, layout), w, h)) {
        set_error("jpeg round trip: image %dx%d too large (an image's bytes >= 2^32)", w, h);
        return MIPX_EUNSUPPORTED;
    }
    const size_t need = op_workspace_bytes(MIPX_OP_JPEGRT, n, w, h, 3, shrink, 0);
    if (!d_ws || ws_bytes < need) {
        set_error("jpeg round trip: workspace %zu < %zu bytes", ws_bytes, need);
        return MIPX_EINVAL;
    }
    uint8_t *planes = static_cast<uint8_t *>(d_ws);
    const int e = jpegrt_launch(d_in, planes, n, w, h, layout, quality, shrink, as_stream(stream));
    if (e) return e;
    // full-size 4:2:0 keeps its half-size chroma planes for the fancy upsample; every other case made
    // three equal planes of the decoded size
    if (shrink == 1) return ycc_launch(planes, d_out, n, w, h, layout, as_stream(stream));
    return ycc_launch(planes, d_out, n, (w + shrink - 1) / shrink, (h + shrink - 1) / shrink, MIPX_YCC_444,
                      as_stream(stream));
}

int mipx_op_affine(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands, double xscale,
                   double yscale, int32_t extend, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || !(xscale > 0) || !(yscale > 0)) return MIPX_EINVAL;
    return affine_launch(d_in, d_out, n, w, h, bands, xscale, yscale, extend, as_stream(stream));
}

int mipx_op_zoom(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands, int32_t xfac,
                 int32_t yfac, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands) || xfac < 1 || yfac < 1) return MIPX_EINVAL;
    return zoom_launch(d_in, d_out, n, w, h, bands, xfac, yfac, as_stream(stream));
}

int mipx_op_flatten(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                    const int32_t *bg, void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    int b3[3] = {0, 0, 0};
    if (bg) b3[0] = bg[0], b3[1] = bg[1], b3[2] = bg[2];
    return flatten_launch(d_in, d_out, n, w, h, bands, b3, as_stream(stream));
}

int mipx_op_colourspace_bw(const uint8_t *d_in, uint8_t *d_out, int32_t n, int32_t w, int32_t h, int32_t bands,
                           void *stream) {
    if (!d_in || !d_out || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    return bw_launch(d_in, d_out, n, w, h, bands, as_stream(stream));
}

int mipx_op_smartcrop_origin(const uint8_t *d_in, int32_t *d_origins, int32_t n, int32_t w, int32_t h, int32_t bands,
                             int32_t cw, int32_t ch, void *d_ws, size_t ws_bytes, void *stream) {
    if (!d_in || !d_origins || !geom_ok(n, w, h, bands)) return MIPX_EINVAL;
    const SamplingScope sampling;  // one convention for the whole call
    return smartcrop_origins(d_in, d_origins, n, w, h, bands, cw, ch, d_ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
