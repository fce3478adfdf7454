// k_ycc.hip — a JPEG decoder's output stage on gfx950 (PARITY_ASSUMPTIONS.md row 16): planar
// YCbCr in, interleaved RGB out, as libjpeg computes it with its default settings.
//   4:2:0 chroma (jdsample.c h2v2_fancy_upsample, chosen when cw > 2), C a ch x cw plane:
//     cy = y >> 1, cx = x >> 1; ny = cy - 1 for even y, cy + 1 for odd y, nx alike, clamped
//     s(c) = 3 C[cy][c] + C[ny][c];  c(x, y) = (3 s(cx) + s(nx) + (x even ? 8 : 7)) >> 4
//     cw <= 2: plain replication, c(x, y) = C[cy][cx] (the same expression with ny = cy, nx = cx)
//   4:2:2 chroma (jdsample.c h2v1_fancy_upsample, chosen when cw > 2), C an h x cw plane, no
//   vertical term (PARITY_ASSUMPTIONS.md row 25):
//     cx = x >> 1; nx = cx - 1 for even x, cx + 1 for odd x, clamped
//     c(x, y) = (3 C[y][cx] + C[y][nx] + (x even ? 1 : 2)) >> 2
//     cw <= 2, and at every width behind a 1 / 8 decode (the launch's `replicate`): c(x, y) = C[y][cx]
//   conversion (jdcolor.c), int32, arithmetic shifts, cb = Cb - 128, cr = Cr - 128:
//     R = clamp(Y + ((91881 cr + 32768) >> 16))
//     G = clamp(Y + ((-22554 cb - 46802 cr + 32768) >> 16))
//     B = clamp(Y + ((116130 cb + 32768) >> 16))
// Per image the input is Y (h x w), Cb, Cr (ch x cw each) back to back without padding, the
// output h x w x 3.  Bit-exact.
//
// Pure streaming (1.5 or 3 bytes in, 3 out per pixel), no LDS.  A lane makes 4 output pixels
// of a row from dwords: the Y dword, and per chroma plane the dword of columns cx0 - 1 ..
// cx0 + 2, which is exactly the neighbourhood of 4 pixels; it writes them as one 12-byte
// store, so a wave reads 256 and writes 768 contiguous bytes per row.  In 4:2:0 a lane does
// output rows 2j - 1 and 2j, which read the same two chroma rows j - 1 and j (weights 3 : 1
// and 1 : 3), so the four chroma dwords serve 8 pixels; it walks a few such row pairs, keeping
// chroma row j for the next one and loading ahead of the arithmetic.  4:2:2 is the same lane
// without the row pairing: one Y dword and one dword per chroma plane make the 4 pixels of one
// row, and a lane walks a few rows with the next row's loads ahead.  All accesses are plain
// unaligned dword ones: rows, planes and images start on any byte (w * h may be odd), and when
// they happen to be dword-aligned (any w that is a multiple of 4) so is every access.  A row's
// first and last lanes gather the same four chroma columns byte by byte with clamped indices
// (one counter run: with a per-pixel path there, the 2 edge waves of a 4K row's 15 issued a
// quarter of the kernel's instructions); only images with cw <= 2 go pixel by pixel.  The
// multiplies have 24-bit operands (v_mad_i32_i24, full rate).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.h"

namespace mipx {
namespace {

using namespace dev;

struct YccArgs {
    const u8 *in;
    u8 *out;
    long long in_img, out_img;  // bytes per image
    uint32_t w, h, cw, ch;
    uint32_t npix, cpix;        // w * h, cw * ch
    uint32_t gx;                // 4:2:0, 4:2:2: blocks across one image
    int rep;                    // 4:2:0, 4:2:2: chroma replicated (cw <= 2; 4:2:2 also on request)
};

__device__ __forceinline__ uint32_t ld32(const u8 *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);  // any alignment: one global_load_dword
    return v;
}
__device__ __forceinline__ int byte_of(uint32_t v, int k) { return static_cast<int>((v >> (8 * k)) & 255u); }

// a * k + c with 24-bit a and k: the full-rate v_mad_i32_i24.  Spelled out because the compiler
// loses the operands' range behind the upsample's shift and picks the quarter-rate v_mul_lo_u32.
__device__ __forceinline__ int mad24(int a, int k, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(c));
    return r;
}

// jdcolor.c with the - 128 folded into the rounding constants; cb, cr in 0..255
__device__ __forceinline__ void ycc_rgb(int y, int cb, int cr, int *r, int *g, int *b) {
    *r = clampi(y + (mad24(cr, 91881, 32768 - 128 * 91881) >> 16), 0, 255);
    *g = clampi(y + (mad24(cb, -22554, mad24(cr, -46802, 32768 + 128 * (22554 + 46802))) >> 16), 0, 255);
    *b = clampi(y + (mad24(cb, 116130, 32768 - 128 * 116130) >> 16), 0, 255);
}

// 4 pixels: Y in the bytes of yw, chroma already at full size; their 12 output bytes in d
__device__ __forceinline__ void ycc_rgb4(uint32_t yw, const int cb[4], const int cr[4], uint32_t d[3]) {
    int v[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) ycc_rgb(byte_of(yw, k), cb[k], cr[k], &v[3 * k], &v[3 * k + 1], &v[3 * k + 2]);
#pragma unroll
    for (int q = 0; q < 3; ++q)
        d[q] = static_cast<uint32_t>(v[4 * q]) | static_cast<uint32_t>(v[4 * q + 1]) << 8 |
               static_cast<uint32_t>(v[4 * q + 2]) << 16 | static_cast<uint32_t>(v[4 * q + 3]) << 24;
}
// the first `bytes` (12: one global_store_dwordx3, any alignment; fewer: the row's last lane) of d
__device__ __forceinline__ void ycc_store(u8 *o, const uint32_t d[3], uint32_t bytes) {
    if (bytes == 12u) {
        __builtin_memcpy(o, d, 12);
        return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (i < static_cast<int>(bytes)) o[i] = static_cast<u8>(d[i >> 2] >> (8 * (i & 3)));
}
__device__ __forceinline__ void ycc_emit4(u8 *o, uint32_t yw, const int cb[4], const int cr[4]) {
    uint32_t d[3];
    ycc_rgb4(yw, cb, cr, d);
    ycc_store(o, d, 12u);
}

// h2v2 fancy upsample of output columns x0 .. x0 + 3 (x0 even) of one row: `near` and `far`
// hold chroma columns cx0 - 1 .. cx0 + 2 of the row's own chroma row and of its neighbour
__device__ __forceinline__ void ycc_up4(uint32_t near, uint32_t far, int c[4]) {
    int s[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = 3 * byte_of(near, k) + byte_of(far, k);
    c[0] = (3 * s[1] + s[0] + 8) >> 4;
    c[1] = (3 * s[1] + s[2] + 7) >> 4;
    c[2] = (3 * s[2] + s[1] + 8) >> 4;
    c[3] = (3 * s[2] + s[3] + 7) >> 4;
}

// h2v1 fancy upsample of output columns x0 .. x0 + 3 (x0 even) of one row: `row` holds chroma
// columns cx0 - 1 .. cx0 + 2 of that row; rep: replicated instead
__device__ __forceinline__ void ycc_up4h(uint32_t row, int rep, int c[4]) {
    const int s0 = byte_of(row, 0), s1 = byte_of(row, 1), s2 = byte_of(row, 2), s3 = byte_of(row, 3);
    c[0] = rep ? s1 : (3 * s1 + s0 + 1) >> 2;
    c[1] = rep ? s1 : (3 * s1 + s2 + 2) >> 2;
    c[2] = rep ? s2 : (3 * s2 + s1 + 1) >> 2;
    c[3] = rep ? s2 : (3 * s2 + s3 + 2) >> 2;
}

// one output pixel by the formulas at the top, every index clamped (edges, cw <= 2, tails)
template <int LAYOUT>
__device__ void ycc_pixel(const YccArgs &a, const u8 *in, u8 *out, uint32_t x, uint32_t y) {
    const uint32_t p = y * a.w + x;
    const u8 *pcb = in + a.npix, *pcr = pcb + a.cpix;
    int cb, cr;
    if (LAYOUT == MIPX_YCC_444) {
        cb = pcb[p], cr = pcr[p];
    } else if (LAYOUT == MIPX_YCC_422) {
        const uint32_t cx = x >> 1;
        uint32_t nx = (x & 1u) ? min(cx + 1u, a.cw - 1u) : (cx ? cx - 1u : 0u);
        if (a.rep) nx = cx;
        const uint32_t cc = y * a.cw + cx, cn = y * a.cw + nx;
        const int bias = (x & 1u) ? 2 : 1;
        cb = (3 * pcb[cc] + pcb[cn] + bias) >> 2;
        cr = (3 * pcr[cc] + pcr[cn] + bias) >> 2;
    } else {
        const uint32_t cy = y >> 1, cx = x >> 1;
        uint32_t ny = (y & 1u) ? min(cy + 1u, a.ch - 1u) : (cy ? cy - 1u : 0u);
        uint32_t nx = (x & 1u) ? min(cx + 1u, a.cw - 1u) : (cx ? cx - 1u : 0u);
        if (a.rep) ny = cy, nx = cx;
        const uint32_t cc = cy * a.cw + cx, cn = cy * a.cw + nx, nc = ny * a.cw + cx, nn = ny * a.cw + nx;
        const int bias = (x & 1u) ? 7 : 8;
        cb = (3 * (3 * pcb[cc] + pcb[nc]) + (3 * pcb[cn] + pcb[nn]) + bias) >> 4;
        cr = (3 * (3 * pcr[cc] + pcr[nc]) + (3 * pcr[cn] + pcr[nn]) + bias) >> 4;
    }
    int r, g, b;
    ycc_rgb(in[p], cb, cr, &r, &g, &b);
    u8 *o = out + 3u * p;
    o[0] = static_cast<u8>(r), o[1] = static_cast<u8>(g), o[2] = static_cast<u8>(b);
}

// chroma columns 2g - 1 .. 2g + 2 of one chroma row as a dword: one load, or for a row's first
// and last lanes the same four columns clamped, byte by byte
__device__ __forceinline__ uint32_t ycc_chroma4(const u8 *row, uint32_t g, uint32_t cw, bool interior) {
    if (interior) return ld32(row + (2u * g - 1u));
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int c = clampi(static_cast<int>(2u * g) - 1 + k, 0, static_cast<int>(cw) - 1);
        v |= static_cast<uint32_t>(row[c]) << (8 * k);
    }
    return v;
}
// Y of pixels x0 .. x0 + px - 1 of one row (px = 4 but in a row's last lane)
__device__ __forceinline__ uint32_t ycc_luma4(const u8 *p, uint32_t px) {
    if (px == 4u) return ld32(p);
    uint32_t v = 0u;
    for (uint32_t k = 0; k < px; ++k) v |= static_cast<uint32_t>(p[k]) << (8 * k);
    return v;
}

// 4:2:0.  Block = 4 waves; wave t walks kYccPairs row pairs j (output rows 2j - 1 and 2j), its
// lanes 64 consecutive groups of 4 columns.  Pair j reads chroma rows j - 1 and j, so each
// step loads one new chroma row per plane and two Y rows, and it loads them for pair j + 1
// before it computes pair j.
constexpr uint32_t kYccPairs = 4;

__global__ void __launch_bounds__(256) k_ycc420(const YccArgs a) {
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t by = blockIdx.x / a.gx, bx = blockIdx.x - by * a.gx;
    // threadIdx.y is the wave: j and the row addresses made from it are scalar
    const uint32_t g = bx * 64u + threadIdx.x;
    const uint32_t j0 = __builtin_amdgcn_readfirstlane((by * 4u + threadIdx.y) * kYccPairs);
    const uint32_t x0 = 4u * g, jend = min(j0 + kYccPairs, a.h / 2u + 1u);
    if (x0 >= a.w || j0 >= jend) return;
    if (a.rep) {  // cw <= 2, so w <= 4: one lane per row pair
        for (uint32_t j = j0; j < jend; ++j)
            for (uint32_t x = x0; x < a.w; ++x) {
                if (j >= 1u) ycc_pixel<MIPX_YCC_420>(a, in, out, x, 2u * j - 1u);
                if (2u * j < a.h) ycc_pixel<MIPX_YCC_420>(a, in, out, x, 2u * j);
            }
        return;
    }
    const u8 *pcb = in + a.npix, *pcr = pcb + a.cpix;
    const bool interior = g >= 1u && 2u * g + 2u <= a.cw - 1u;
    const uint32_t px = min(4u, a.w - x0);  // pixels of this lane
    // row 2j - 1's own chroma row is j - 1, row 2j's is min(j, ch - 1); j - 1 is pair j - 1's second
    const uint32_t r0 = j0 ? j0 - 1u : 0u;
    uint32_t ba = ycc_chroma4(pcb + r0 * a.cw, g, a.cw, interior), ca = ycc_chroma4(pcr + r0 * a.cw, g, a.cw, interior);
    uint32_t bb, cc, yw1 = 0u, yw2 = 0u;
    {
        const uint32_t rb = min(j0, a.ch - 1u);
        bb = ycc_chroma4(pcb + rb * a.cw, g, a.cw, interior), cc = ycc_chroma4(pcr + rb * a.cw, g, a.cw, interior);
        if (j0 >= 1u) yw1 = ycc_luma4(in + (2u * j0 - 1u) * a.w + x0, px);
        if (2u * j0 < a.h) yw2 = ycc_luma4(in + 2u * j0 * a.w + x0, px);
    }
    for (uint32_t j = j0; j < jend; ++j) {
        uint32_t nbb = 0u, ncc = 0u, nyw1 = 0u, nyw2 = 0u;
        if (j + 1u < jend) {  // the next pair's loads first; its row 2j + 1 always exists
            const uint32_t rb = min(j + 1u, a.ch - 1u);
            nbb = ycc_chroma4(pcb + rb * a.cw, g, a.cw, interior), ncc = ycc_chroma4(pcr + rb * a.cw, g, a.cw, interior);
            nyw1 = ycc_luma4(in + (2u * j + 1u) * a.w + x0, px);
            if (2u * j + 2u < a.h) nyw2 = ycc_luma4(in + (2u * j + 2u) * a.w + x0, px);
        }
        int cb[4], cr[4];
        uint32_t d[3];
        if (j >= 1u) {
            ycc_up4(ba, bb, cb), ycc_up4(ca, cc, cr);
            ycc_rgb4(yw1, cb, cr, d);
            ycc_store(out + 3u * ((2u * j - 1u) * a.w + x0), d, 3u * px);
        }
        if (2u * j < a.h) {
            ycc_up4(bb, ba, cb), ycc_up4(cc, ca, cr);
            ycc_rgb4(yw2, cb, cr, d);
            ycc_store(out + 3u * (2u * j * a.w + x0), d, 3u * px);
        }
        ba = bb, ca = cc, bb = nbb, cc = ncc, yw1 = nyw1, yw2 = nyw2;
    }
}

// 4:2:2.  Block = 4 waves; wave t walks kYcc422Rows rows, its lanes 64 consecutive groups of 4
// columns.  A row reads its own chroma row only, so each step loads one chroma dword per plane and
// one Y dword, and it loads them for row y + 1 before it computes row y.
constexpr uint32_t kYcc422Rows = 8;

__global__ void __launch_bounds__(256) k_ycc422(const YccArgs a) {
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t by = blockIdx.x / a.gx, bx = blockIdx.x - by * a.gx;
    // threadIdx.y is the wave: y and the row addresses made from it are scalar
    const uint32_t g = bx * 64u + threadIdx.x;
    const uint32_t y0 = __builtin_amdgcn_readfirstlane((by * 4u + threadIdx.y) * kYcc422Rows);
    const uint32_t x0 = 4u * g, yend = min(y0 + kYcc422Rows, a.h);
    if (x0 >= a.w || y0 >= yend) return;
    if (a.cw <= 2u) {  // so w <= 4: one lane per row
        for (uint32_t y = y0; y < yend; ++y)
            for (uint32_t x = x0; x < a.w; ++x) ycc_pixel<MIPX_YCC_422>(a, in, out, x, y);
        return;
    }
    const u8 *pcb = in + a.npix, *pcr = pcb + a.cpix;
    const bool interior = g >= 1u && 2u * g + 2u <= a.cw - 1u;
    const uint32_t px = min(4u, a.w - x0);  // pixels of this lane
    uint32_t bw = ycc_chroma4(pcb + y0 * a.cw, g, a.cw, interior), rw = ycc_chroma4(pcr + y0 * a.cw, g, a.cw, interior);
    uint32_t yw = ycc_luma4(in + y0 * a.w + x0, px);
    for (uint32_t y = y0; y < yend; ++y) {
        uint32_t nbw = 0u, nrw = 0u, nyw = 0u;
        if (y + 1u < yend) {  // the next row's loads first
            nbw = ycc_chroma4(pcb + (y + 1u) * a.cw, g, a.cw, interior), nrw = ycc_chroma4(pcr + (y + 1u) * a.cw, g, a.cw, interior);
            nyw = ycc_luma4(in + (y + 1u) * a.w + x0, px);
        }
        int cb[4], cr[4];
        uint32_t d[3];
        ycc_up4h(bw, a.rep, cb), ycc_up4h(rw, a.rep, cr);
        ycc_rgb4(yw, cb, cr, d);
        ycc_store(out + 3u * (y * a.w + x0), d, 3u * px);
        bw = nbw, rw = nrw, yw = nyw;
    }
}

// 4:4:4: the three planes have the image's shape, so the walk is flat over w * h pixels, 4
// per lane and kYcc444Unroll groups per lane with their loads issued together
constexpr int kYcc444Unroll = 2;

__global__ void __launch_bounds__(256) k_ycc444(const YccArgs a) {
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t groups = a.npix >> 2;
    constexpr int U = kYcc444Unroll;
    const uint32_t g0 = blockIdx.x * (256u * U) + threadIdx.x;
    uint32_t yw[U], bw[U], rw[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t g = g0 + 256u * u;
        if (g < groups) {
            yw[u] = ld32(in + 4u * g);
            bw[u] = ld32(in + a.npix + 4u * g);
            rw[u] = ld32(in + 2u * a.npix + 4u * g);
        }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const uint32_t g = g0 + 256u * u;
        if (g < groups) {
            int cb[4], cr[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) cb[k] = byte_of(bw[u], k), cr[k] = byte_of(rw[u], k);
            ycc_emit4(out + 12u * g, yw[u], cb, cr);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.npix & 3u)) {  // the last w * h % 4 pixels
        const uint32_t p = 4u * groups + threadIdx.x;
        ycc_pixel<MIPX_YCC_444>(a, in, out, p % a.w, p / a.w);
    }
}

}  // namespace

int ycc_launch(const u8 *d_in, u8 *d_out, int n, int w, int h, int layout, hipStream_t st, bool replicate) {
    const long long npix = static_cast<long long>(w) * h;
    if (npix * 3 > 0xffffffffLL) {  // byte offsets inside an image are 32-bit
        set_error("ycc to rgb: image %dx%d too large (3 * w * h >= 2^32)", w, h);
        return MIPX_EUNSUPPORTED;
    }
    const bool sub = layout == MIPX_YCC_420, h2v1 = layout == MIPX_YCC_422;
    const JpegGeom g(w, h, layout);
    YccArgs a;
    a.in = d_in, a.out = d_out;
    a.w = w, a.h = h;
    a.cw = static_cast<uint32_t>(g.c.w), a.ch = static_cast<uint32_t>(g.c.h);
    a.npix = static_cast<uint32_t>(npix);
    a.cpix = a.cw * a.ch;
    a.in_img = static_cast<long long>(g.plane_bytes), a.out_img = npix * 3;
    a.rep = (sub && a.cw <= 2) || (h2v1 && (a.cw <= 2 || replicate));
    a.gx = 1;
    if (h2v1) {
        const long long groups = (static_cast<long long>(w) + 3) / 4;
        const long long gx = (groups + 63) / 64, gy = (static_cast<long long>(h) + 4 * kYcc422Rows - 1) / (4 * kYcc422Rows);
        if (!grid_ok(gx * gy)) return MIPX_EUNSUPPORTED;
        a.gx = static_cast<uint32_t>(gx);
        hipLaunchKernelGGL(k_ycc422, dim3(static_cast<unsigned>(gx * gy), n), dim3(64, 4), 0, st, a);
        return launch_check("k_ycc422");
    }
    if (sub) {
        const long long groups = (static_cast<long long>(w) + 3) / 4, pairs = h / 2 + 1;
        const long long gx = (groups + 63) / 64, gy = (pairs + 4 * kYccPairs - 1) / (4 * kYccPairs);
        if (!grid_ok(gx * gy)) return MIPX_EUNSUPPORTED;
        a.gx = static_cast<uint32_t>(gx);
        hipLaunchKernelGGL(k_ycc420, dim3(static_cast<unsigned>(gx * gy), n), dim3(64, 4), 0, st, a);
        return launch_check("k_ycc420");
    }
    const long long per_block = 256LL * 4 * kYcc444Unroll;
    const long long blocks = std::max(1LL, (npix + per_block - 1) / per_block);
    if (!grid_ok(blocks)) return MIPX_EUNSUPPORTED;
    hipLaunchKernelGGL(k_ycc444, dim3(static_cast<unsigned>(blocks), n), dim3(256), 0, st, a);
    return launch_check("k_ycc444");
}

}  // namespace mipx
