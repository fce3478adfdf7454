// jpeg_geom.h — the one place that knows the JPEG layouts (MIPX_YCC_*): what (w, h, layout) means in
// planes, blocks, MCUs and bytes, at full size and decoded at 1/2, 1/4, 1/8; which layouts, qualities
// and scales are legal; and the size limits of the kernels.  The planner's mipx_*_bytes functions, the
// coder's and decoder's workspaces, the launchers' kernel arguments and every argument check read it.
// A new layout starts here.  No HIP, host only, 64-bit arithmetic throughout: a launcher narrows to
// the 32 bits of its kernel arguments after its size check.
#pragma once

#include <cstddef>
#include <cstdint>

#include "mipx.h"

namespace mipx {

// the layouts the engine reads (planes, coefficients, scans), and those it writes a JPEG in
inline bool ycc_input_layout(int layout) {
    return layout == MIPX_YCC_444 || layout == MIPX_YCC_420 || layout == MIPX_YCC_422;
}
inline bool ycc_output_layout(int layout) { return layout == MIPX_YCC_444 || layout == MIPX_YCC_420; }
// Those are the three-component ones: what MIPX_OP_YCC and MIPX_OP_JPEGRT take.  The steps that read
// or write a file (MIPX_OP_JPEGD, MIPX_OP_JPEGH; MIPX_OP_JPEGC, MIPX_OP_JPEGE) take the one-component
// layout too: its plane already is the image, of 1 band where the others make 3.
inline bool jpeg_input_layout(int layout) { return ycc_input_layout(layout) || layout == MIPX_YCC_GREY; }
inline bool jpeg_output_layout(int layout) { return ycc_output_layout(layout) || layout == MIPX_YCC_GREY; }
inline int jpeg_layout_bands(int layout) { return layout == MIPX_YCC_GREY ? 1 : 3; }
inline bool jpeg_quality_ok(int quality) { return quality >= 1 && quality <= 100; }
// a decoding scale; where a caller takes 0 for 1 it passes jpeg_scale(s)
inline bool jpeg_scale_ok(int s) { return s == 1 || s == 2 || s == 4 || s == 8; }
inline int jpeg_scale(int s) { return s == 0 ? 1 : s; }

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

struct JpegComp {       // one class of components
    uint64_t w, h;      // the plane in samples
    uint64_t wb, hb;    // its real 8 x 8 blocks across and down
};

// The planes a decoder has at 1/s (k_jpegds, k_jpegrt); [0]: Y, [1]: Cb and Cr
struct JpegPlanes {
    uint32_t n[2];      // the inverse DCT's size: a block gives n x n samples
    uint64_t w[2], h[2];
    uint64_t off[3];    // byte offset of each component's plane
    uint64_t bytes;     // per image
};

struct JpegGeom {
    uint64_t hs = 0, vs = 0;          // Y's sampling factors; chroma's are 1
    JpegComp y{}, c{};                // Y; Cb and Cr (all zero in MIPX_YCC_GREY, which has none)
    uint64_t coef_off[3] = {};        // byte offset of each component's coefficients, 128 bytes per real block
    uint64_t plane_off[3] = {};       // ... and of its plane
    uint64_t coef_bytes = 0, plane_bytes = 0;  // per image
    uint64_t mw = 0, mh = 0;          // the MCU grid: the chroma block grid
    uint64_t per_mcu = 0;             // blocks of an MCU: hs vs of Y, Cb, Cr
    uint64_t blocks = 0;              // of the scan, the dummy ones included

    // every field stays 0 for a size that is not positive or a layout that is none
    JpegGeom(int w, int h, int layout) {
        if (w <= 0 || h <= 0 || !jpeg_input_layout(layout)) return;
        if (layout == MIPX_YCC_GREY) {  // one component: the non-interleaved scan, an MCU is a block
            hs = vs = 1, y = comp(w, h);
            coef_off[1] = coef_off[2] = coef_bytes = 128 * y.wb * y.hb;
            plane_off[1] = plane_off[2] = plane_bytes = y.w * y.h;
            mw = y.wb, mh = y.hb, per_mcu = 1, blocks = mw * mh;
            return;
        }
        hs = layout == MIPX_YCC_444 ? 1 : 2, vs = layout == MIPX_YCC_420 ? 2 : 1;
        y = comp(w, h), c = comp(ceil_div(w, hs), ceil_div(h, vs));
        coef_off[1] = 128 * y.wb * y.hb, coef_off[2] = coef_off[1] + 128 * c.wb * c.hb;
        coef_bytes = coef_off[2] + 128 * c.wb * c.hb;
        plane_off[1] = y.w * y.h, plane_off[2] = plane_off[1] + c.w * c.h;
        plane_bytes = plane_off[2] + c.w * c.h;
        mw = c.wb, mh = c.hb, per_mcu = hs * vs + 2;
        blocks = mw * mh * per_mcu;
    }

    // libjpeg's shrink-on-load (jdmaster.c): Y takes N = 8 / s; chroma takes twice that, up to 8, where
    // both of its ratios are 2 (4:2:0: three equal planes below full size); 4:2:2 keeps N and so its
    // half-width chroma at every scale.  s = 1 gives the full-size planes above.  Grey: its one plane.
    JpegPlanes planes(int s) const {
        JpegPlanes p{};
        if (c.wb == 0) {
            p.n[0] = p.n[1] = 8u / static_cast<uint32_t>(s);
            p.w[0] = ceil_div(y.w, s), p.h[0] = ceil_div(y.h, s);
            p.off[1] = p.off[2] = p.bytes = p.w[0] * p.h[0];
            return p;
        }
        const uint64_t both = hs < vs ? hs : vs;
        p.n[0] = 8u / static_cast<uint32_t>(s);
        p.n[1] = p.n[0] * both > 8 ? 8u : static_cast<uint32_t>(p.n[0] * both);
        p.w[0] = ceil_div(y.w, s), p.h[0] = ceil_div(y.h, s);
        p.w[1] = ceil_div(p.w[0] * p.n[1], p.n[0] * hs), p.h[1] = ceil_div(p.h[0] * p.n[1], p.n[0] * vs);
        p.off[1] = p.w[0] * p.h[0], p.off[2] = p.off[1] + p.w[1] * p.h[1];
        p.bytes = p.off[2] + p.w[1] * p.h[1];
        return p;
    }

    const JpegComp &of(int cls) const { return cls ? c : y; }  // 0: Y, 1: Cb and Cr

   private:
    static JpegComp comp(uint64_t w, uint64_t h) { return JpegComp{w, h, ceil_div(w, 8), ceil_div(h, 8)}; }
};

// The most over the layouts a workspace serves (it is sized without the layout): the output layouts,
// or with `input` the input ones.  cap is 4:4:4's; 4:2:2's blocks pass the others' where the image is
// one block across and an even number down.
struct JpegMax {
    uint64_t cap, blocks;
};
inline JpegMax jpeg_max(int w, int h, bool input) {
    JpegMax m{0, 0};
    const int layouts[] = {MIPX_YCC_444, MIPX_YCC_420, MIPX_YCC_422};
    for (int layout : layouts) {
        if (!(input ? ycc_input_layout(layout) : ycc_output_layout(layout))) continue;
        const JpegGeom g(w, h, layout);
        if (g.coef_bytes > m.cap) m.cap = g.coef_bytes;
        if (g.blocks > m.blocks) m.blocks = g.blocks;
    }
    return m;
}

// ---- the kernels' limits ------------------------------------------------------------------
// Byte offsets inside an image are 32-bit in the kernels: the coefficient payload of the file and the
// RGB of the rgb_w x rgb_h image beside it (the file's size, or what it decodes to) stay below 2^32
inline bool jpeg_fits_32(const JpegGeom &file, int rgb_w, int rgb_h) {
    const uint64_t payload = file.coef_bytes ? MIPX_JPEGD_HEADER_BYTES + file.coef_bytes : 0;
    return !(payload > 0xffffffffull || 3ull * rgb_w * rgb_h > 0xffffffffull);
}
// Bit offsets inside a scan are 32-bit in the entropy decoder: the scan's coefficients below 2^29 bytes
inline bool jpeg_scan_fits_decoder(const JpegGeom &g) { return !(g.coef_bytes >= (1ull << 29)); }
// libjpeg's search for the least frequency starts at 10^9: a scan that could count that many symbols
// into one table (64 per block at most) is outside the optimised tables' rule
inline bool jpeg_blocks_fit_opt(uint64_t blocks) { return 64ull * blocks < 1000000000ull; }

// ---- layout dispatch ----------------------------------------------------------------------
// f(JpegLayout<L>()) with the layout as a compile-time constant; the output form instantiates nothing
// for 4:2:2.  The caller has checked the layout.  Both have the one-component arm: a caller that does
// not take it (k_jpegrt.hip) leaves that arm of its own empty.
template <int L>
struct JpegLayout {
    static constexpr int value = L;
};
template <class F>
inline void with_output_layout(int layout, F &&f) {
    if (layout == MIPX_YCC_420) f(JpegLayout<MIPX_YCC_420>());
    else if (layout == MIPX_YCC_GREY) f(JpegLayout<MIPX_YCC_GREY>());
    else f(JpegLayout<MIPX_YCC_444>());
}
template <class F>
inline void with_input_layout(int layout, F &&f) {
    if (layout == MIPX_YCC_420) f(JpegLayout<MIPX_YCC_420>());
    else if (layout == MIPX_YCC_422) f(JpegLayout<MIPX_YCC_422>());
    else if (layout == MIPX_YCC_GREY) f(JpegLayout<MIPX_YCC_GREY>());
    else f(JpegLayout<MIPX_YCC_444>());
}

}  // namespace mipx
