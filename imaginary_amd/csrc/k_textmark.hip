// k_textmark.hip — bimg vips_watermark (text) after the glyph rendering, on gfx950
// (PARITY_ASSUMPTIONS.md, the text-watermark rows): the host hands over the rendered
// 1-band text mask T (tw x th); the engine does the pixel work at image size:
//   M     = (uchar)(T * opacity)                     vips_linear1 + vips_cast, truncating
//   tile  = vips_embed(M, 100, 100, tw + margin, th + margin), extend black
//   m     = tile(x mod Tw, y mod Th)                 vips_replicate + vips_crop
//   out   = (m * colour + (255 - m) * in + 128) / 255   vips_ifthenelse(blend), 3 bands
// A 1-band image is up-banded against the 3-band colour.  Bit-exact.
//
// Memory-bound (w * h * b bytes in, w * h * 3 out), so the kernel streams: a flat walk
// over each image's output bytes, one 16-byte aligned store per lane.  A 16-byte chunk at
// image byte i0 starts r0 = i0 % 3 bytes into pixel p0 = i0 / 3 and touches six pixels.
// The lane works on the 18 bytes of those six whole pixels (the "window": byte e of it is
// band e % 3 of pixel p0 + e / 3, all static), so the loaded dwords are shifted up by r0
// bytes into the window and the results back down by r0 (one v_perm / v_alignbyte per
// dword).  A chunk inside one image row, on a tile row that carries no text, needs no mask
// look-up at all; the others read their six mask bytes without a branch.  The up-to-15
// bytes in front of and behind an image's aligned core are single bytes on a few lanes of
// its first block.  The mask is small and stays in L2.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "device_common.h"

namespace mipx {
namespace {

using namespace dev;

constexpr int kTmOrigin = 100;  // bimg embeds the mask at (100, 100) of its tile

// Division of a 32-bit n by an invariant d >= 1 (Granlund & Montgomery 1994, fig. 4.1,
// N = 32): l = ceil(log2 d), m = floor(2^32 (2^l - d) / d) + 1, s1 = min(l, 1),
// s2 = max(l - 1, 0); t = mulhi(m, n); n / d = (t + ((n - t) >> s1)) >> s2.
struct TmDiv {
    uint32_t m, s1, s2;
};

TmDiv tm_div_make(uint32_t d) {
    int l = 0;
    while ((1ull << l) < d) ++l;
    TmDiv k;
    k.m = static_cast<uint32_t>((((1ull << l) - d) << 32) / d + 1);
    k.s1 = l < 1 ? l : 1;
    k.s2 = l > 1 ? l - 1 : 0;
    return k;
}

__device__ __forceinline__ uint32_t tm_div(uint32_t n, const TmDiv &k) {
    const uint32_t t = __umulhi(k.m, n);
    return (t + ((n - t) >> k.s1)) >> k.s2;
}

struct TmArgs {
    const u8 *in, *mask;
    u8 *out;
    long long in_img, out_img;  // bytes per image
    uint32_t out_bytes;         // w * h * 3 of one image
    uint32_t npix;              // w * h
    uint32_t w;
    uint32_t tw, th;            // mask
    uint32_t Tw, Th;            // tile: mask + margin
    float opacity;
    uint32_t c[3];
    TmDiv dw, dTw, dTh;
};

// the replicated mask at tile position (tx, ty): k_composite.hip's mask expression.  No
// branch: a position outside the text reads mask byte 0 and drops it, so the six loads of
// a chunk issue back to back instead of each waiting in its own exec region.
__device__ __forceinline__ uint32_t tm_mask(const TmArgs &a, uint32_t tx, uint32_t ty) {
    const uint32_t ux = tx - kTmOrigin, uy = ty - kTmOrigin;
    const bool text = ux < a.tw && uy < a.th;
    const float t = static_cast<float>(a.mask[text ? static_cast<size_t>(uy) * a.tw + ux : 0]);
    const float f = fadd_rn(fmul_rn(t, a.opacity), 0.0f);
    const uint32_t m = f < 0.f ? 0 : (f > 255.f ? 255 : static_cast<int>(f));
    return text ? m : 0u;
}

// v / 255 for v <= 255 * 255 + 128 (v * 65794 < 2^32; exhaustively checked)
__device__ __forceinline__ uint32_t div255(uint32_t v) { return (v * 65794u) >> 24; }

// one output byte the plain way (the bytes around an image's aligned core)
template <int BI>
__device__ u8 tm_byte(const TmArgs &a, const u8 *in, uint32_t i) {
    const uint32_t p = i / 3u, z = i - 3u * p;
    const uint32_t y = p / a.w, x = p - y * a.w;
    const uint32_t m = tm_mask(a, x % a.Tw, y % a.Th);
    const uint32_t s = in[BI == 3 ? i : p];
    return static_cast<u8>(div255(m * a.c[z] + (255u - m) * s + 128u));
}

// Chunks per lane per trip, their loads issued together.  Measured at 3840 x 2160, n = 64:
// 3 bands 0.634 ms with one load per wave in flight, 0.604 ms with four; 1 band (a third of
// the input bytes) 0.460 ms with one, 0.504 ms with four.
template <int BI>
constexpr int kTmUnroll = BI == 3 ? 4 : 1;

// A chunk's input.  BI 3: its 16 bytes; BI 1: its six pixels in bytes 0..5 of L[0], L[1].
template <int BI>
__device__ __forceinline__ void tm_load(const TmArgs &a, const u8 *in, uint32_t i0, uint32_t L[4]) {
    L[0] = L[1] = L[2] = L[3] = 0;
    const uint32_t p0 = i0 / 3u;
    if (BI == 3) {
        uint4 v;
        __builtin_memcpy(&v, in + i0, 16);  // any alignment: one global_load_dwordx4
        L[0] = v.x, L[1] = v.y, L[2] = v.z, L[3] = v.w;
    } else if (p0 + 8u <= a.npix) {
        uint2 v;
        __builtin_memcpy(&v, in + p0, 8);
        L[0] = v.x, L[1] = v.y;
    } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (p0 + k < a.npix) L[k >> 2] |= static_cast<uint32_t>(in[p0 + k]) << (8 * (k & 3));
    }
}

// The 16 output bytes at image byte i0 (out + i0 is 16-byte aligned, i0 + 16 <= out_bytes).
template <int BI>
__device__ __forceinline__ void tm_chunk(const TmArgs &a, u8 *out, uint32_t i0, const uint32_t L[4]) {
    {
        const uint32_t p0 = i0 / 3u, r0 = i0 - 3u * p0;
        uint32_t y = tm_div(p0, a.dw), x = p0 - y * a.w;
        uint32_t tx = x - tm_div(x, a.dTw) * a.Tw, ty = y - tm_div(y, a.dTh) * a.Th;
        // Most chunks lie in one image row on a tile row without text (the margin, the 100
        // rows above the text): nothing to look up, and a wave decides it nearly as one.
        const bool blank = x + 6u <= a.w && ty - kTmOrigin >= a.th;
        uint32_t m[6] = {0, 0, 0, 0, 0, 0};
        if (!blank) {
#pragma unroll
            for (int k = 0; k < 6; ++k) {  // pixel p0 + 5 may lie past the image: its bytes are dropped below
                m[k] = tm_mask(a, tx, ty);
                ++x, ++tx;
                if (x == a.w) {
                    x = 0, tx = 0;
                    if (++ty == a.Th) ty = 0;
                }
                if (tx == a.Tw) tx = 0;
            }
        }
        const bool copy = (m[0] | m[1] | m[2] | m[3] | m[4] | m[5]) == 0;  // m == 0 reproduces the input byte
        uint4 o;
        if (BI == 3 && copy) {
            o = make_uint4(L[0], L[1], L[2], L[3]);
        } else {
            uint32_t R[5] = {0, 0, 0, 0, 0};  // the window's 18 output bytes
            if (BI == 1 && copy) {  // each grey byte three times
                R[0] = __builtin_amdgcn_perm(L[1], L[0], 0x01000000u);
                R[1] = __builtin_amdgcn_perm(L[1], L[0], 0x02020101u);
                R[2] = __builtin_amdgcn_perm(L[1], L[0], 0x03030302u);
                R[3] = __builtin_amdgcn_perm(L[1], L[0], 0x05040404u);
                R[4] = __builtin_amdgcn_perm(L[1], L[0], 0x00000505u);
            } else {
                uint32_t W[5] = {0, 0, 0, 0, 0};
                if (BI == 3) {  // window byte e = chunk byte e - r0
                    const uint32_t up = 0x07060504u - 0x01010101u * r0;
                    W[0] = __builtin_amdgcn_perm(L[0], 0u, up);
                    W[1] = __builtin_amdgcn_perm(L[1], L[0], up);
                    W[2] = __builtin_amdgcn_perm(L[2], L[1], up);
                    W[3] = __builtin_amdgcn_perm(L[3], L[2], up);
                    W[4] = __builtin_amdgcn_perm(0u, L[3], up);
                }
#pragma unroll
                for (int e = 0; e < 18; ++e) {
                    const int p = e / 3, z = e % 3;
                    const uint32_t s = BI == 3 ? (W[e >> 2] >> (8 * (e & 3))) & 255u : (L[p >> 2] >> (8 * (p & 3))) & 255u;
                    R[e >> 2] |= div255(m[p] * a.c[z] + (255u - m[p]) * s + 128u) << (8 * (e & 3));
                }
            }
            o.x = __builtin_amdgcn_alignbyte(R[1], R[0], r0);
            o.y = __builtin_amdgcn_alignbyte(R[2], R[1], r0);
            o.z = __builtin_amdgcn_alignbyte(R[3], R[2], r0);
            o.w = __builtin_amdgcn_alignbyte(R[4], R[3], r0);
        }
        *reinterpret_cast<uint4 *>(out + i0) = o;
    }
}

template <int BI>
__global__ void __launch_bounds__(256) k_textmark(const TmArgs a) {
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t total = a.out_bytes;
    const uint32_t head = min((16u - static_cast<uint32_t>(reinterpret_cast<uintptr_t>(out) & 15u)) & 15u, total);
    const uint32_t chunks = (total - head) >> 4;
    const uint32_t stride = gridDim.x * 256u;
    constexpr int U = kTmUnroll<BI>;
    for (uint32_t c0 = blockIdx.x * 256u + threadIdx.x; c0 < chunks; c0 += U * stride) {
        uint32_t L[U][4];
#pragma unroll
        for (int u = 0; u < U; ++u)  // every load first, then the work
            if (c0 + u * stride < chunks) tm_load<BI>(a, in, head + ((c0 + u * stride) << 4), L[u]);
#pragma unroll
        for (int u = 0; u < U; ++u)
            if (c0 + u * stride < chunks) tm_chunk<BI>(a, out, head + ((c0 + u * stride) << 4), L[u]);
    }
    if (blockIdx.x == 0 && threadIdx.x < 32) {  // the head (lanes 0..15) and the tail (16..31)
        const uint32_t t = threadIdx.x;
        const uint32_t i = t < 16 ? t : head + (chunks << 4) + (t - 16);
        if (t < 16 ? t < head : i < total) out[i] = tm_byte<BI>(a, in, i);
    }
}

}  // namespace

int textmark_launch(const u8 *d_in, const u8 *d_mask, u8 *d_out, int n, int w, int h, int bands, int tw, int th,
                    int margin, float opacity, const int *colour, hipStream_t st) {
    if (bands != 1 && bands != 3) {
        set_error("text watermark on a %d-band image: the 3-band colour needs 1 or 3 bands", bands);
        return MIPX_EUNSUPPORTED;
    }
    const long long npix = static_cast<long long>(w) * h;
    if (npix * 3 > 0xffffffffLL || static_cast<long long>(tw) + margin > 0x7fffffffLL ||
        static_cast<long long>(th) + margin > 0x7fffffffLL) {
        set_error("text watermark: image %dx%d or tile %d+%d x %d+%d too large", w, h, tw, margin, th, margin);
        return MIPX_EINVAL;
    }
    TmArgs a;
    a.in = d_in, a.mask = d_mask, a.out = d_out;
    a.in_img = npix * bands, a.out_img = npix * 3;
    a.out_bytes = static_cast<uint32_t>(npix * 3);
    a.npix = static_cast<uint32_t>(npix);
    a.w = w;
    a.tw = tw, a.th = th;
    a.Tw = tw + margin, a.Th = th + margin;
    a.opacity = opacity;
    for (int z = 0; z < 3; ++z) a.c[z] = colour[z];
    a.dw = tm_div_make(a.w), a.dTw = tm_div_make(a.Tw), a.dTh = tm_div_make(a.Th);
    // enough blocks to fill the device a few times over; the lanes stride over the rest
    const long long need = (static_cast<long long>(a.out_bytes / 16) + 255) / 256;
    const long long cap = std::max(1, device_cu_count() * 16 / n);
    dim3 grid(static_cast<unsigned>(std::max(1LL, std::min(need, cap))), n);
    if (bands == 3) hipLaunchKernelGGL(k_textmark<3>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_textmark<1>, grid, dim3(256), 0, st, a);
    return launch_check("k_textmark");
}

}  // namespace mipx
