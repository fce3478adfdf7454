// k_jpegrt.hip — a JPEG round trip on gfx950 (PARITY_ASSUMPTIONS.md row 20): interleaved RGB in,
// the sample planes a decoder has of the JPEG of that image at quality Q out, at scale 1/s.  It is
// k_jpegc.hip's rule (colour, 4:2:0 downsample, forward DCT, quantisation; row 17) followed by
// k_jpegd.hip's at that scale (dequantisation with the same tables, the N x N inverse DCT, the
// clamp; rows 18 and 19), block by block: blocks are independent, so the coefficients never
// touch memory.  The planes are what k_ycc.hip takes: at full size in 4:2:0 the packed
// MIPX_YCC_420 planes (Y h x w, then Cb, Cr ch x cw: the fancy upsample needs the neighbours'
// chroma, so it stays k_ycc420's), everywhere else three equal planes of ceil(w / s) x
// ceil(h / s), the packed MIPX_YCC_444 layout.  N per component is k_jpegds's: Y and 4:4:4
// chroma 8 / s, 4:2:0 chroma min(8, 16 / s).  Bit-exact against tests/jpegc_ref.py ->
// tests/jpegd_ref.py / tests/jpegds_ref.py.
//
// A workgroup takes k_jpegc's strip of 48 blocks (128 x 16 pixels in 4:2:0, 128 x 8 in 4:4:4) in
// the same LDS image, blocks 144 bytes apart.  Phase A: k_jpegc's (12-byte pixel groups ->
// samples - 128, edge replication included).  Phase B: the rows pass of the forward DCT, one
// lane per block row.  Phase C: one lane per block column runs the columns pass, quantises with
// the reciprocal word (m | q << 21, build_jpegc_recips), dequantises as int16(v q), and runs
// pass 1 of the N-point inverse DCT down the same column in the same registers; it saturates to
// int16 and writes N rows back (N = 1: DS(d00, 3), which is final).  Phase D: one lane per
// block row runs pass 2, + 128, clamps and stores N plane bytes, cropped to the plane's real
// size; lanes go along 16 blocks first, so 16 consecutive lanes store 16 N contiguous bytes of
// one plane row (the strip's whole row of Y).  Every multiply keeps 24-bit operands: the
// bounds in the two kernels' comments carry over, |quantised| <= 2^11 and q <= 255, and the
// product wraps to int16 as the decoder's does.  Global accesses are plain unaligned ones:
// rows, images and both pointers start on any byte.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h"
#include "jpeg_dct.h"

namespace mipx {
namespace {

using namespace dev;

struct JpegrtArgs {
    const u8 *in;
    u8 *out;
    const uint32_t *recips;     // [lum 64 | chr 64]: m | q << 21 (build_jpegc_recips)
    long long in_img, out_img;  // bytes per image
    uint32_t w, h;
    uint32_t ywb, yhb;          // real Y blocks across and down (4:4:4: of every component)
    uint32_t cwb, ch;           // 4:2:0: real chroma blocks (= MCUs) across; chroma rows
    uint32_t pw[2], ph[2];      // plane size in samples; [0]: Y, [1]: Cb and Cr
    uint32_t plane_off[3];      // byte offset of each component's plane in an image's output
    uint32_t gx;                // strips across one image
};

// S: the scale 1, 2, 4 or 8
template <int LAYOUT, int S>
__global__ void __launch_bounds__(256) k_jpegrt(const JpegrtArgs a) {
    constexpr int NY = 8 / S;                                            // the inverse DCT's size for Y ...
    constexpr int NC = LAYOUT == MIPX_YCC_420 && S > 1 ? 16 / S : NY;  // ... and for chroma
    __shared__ __attribute__((aligned(16))) int16_t blocks[kBlocks * kBlockPitch];
    __shared__ uint32_t recips[128];
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t sy = blockIdx.x / a.gx, sx = blockIdx.x - sy * a.gx;
    const uint32_t tid = threadIdx.x;
    if (tid < 128u) recips[tid] = a.recips[tid];

    // ---- A: pixels -> samples - 128 in LDS
    jfdct::strip_samples<LAYOUT>(blocks, in, a.w, a.h, a.ywb, a.cwb, a.ch, sx, sy);
    __syncthreads();

    // the lane's two (block, row / column) tasks of B and C: 384 over 256 threads
    bool real[2];
    uint32_t comp[2], line[2];
    int16_t *blk[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t t = tid + 256u * i;
        uint32_t bx, by;
        real[i] = false, comp[i] = 0u, line[i] = t & 7u;
        blk[i] = blocks + (t >> 3) * kBlockPitch;
        if (t < 8u * kBlocks) real[i] = jfdct::strip_block<LAYOUT>(a.ywb, a.yhb, a.cwb, sx, sy, t >> 3, &comp[i], &bx, &by);
    }

    // ---- B: the rows pass of the forward DCT
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (real[i]) jfdct::fdct8_row(blk[i], line[i]);
    }
    __syncthreads();

    // ---- C: the columns pass, quantise, dequantise, pass 1 of the inverse DCT down the same column
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (!real[i]) continue;
        int16_t *p = blk[i] + line[i];
        const uint32_t *rc = recips + (comp[i] ? 64u : 0u) + line[i];
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[8 * k];
        jfdct::fdct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t e = rc[8 * k];
            d[k] = static_cast<int16_t>(__mul24(jfdct::quantise(d[k], e), static_cast<int>(e >> 21)));
        }
        const auto pass1 = [&](auto n) {
            constexpr int N = decltype(n)::value;
            if constexpr (N == 1) d[0] = (d[0] + 4) >> 3;  // DS(d00, 3): only column 0 is read
            else jidct::idctn<N, 1>(d);
#pragma unroll
            for (int k = 0; k < N; ++k) p[8 * k] = static_cast<int16_t>(clampi(d[k], -32768, 32767));
        };
        if (NC == NY || comp[i] == 0u) pass1(std::integral_constant<int, NY>());
        else pass1(std::integral_constant<int, NC>());
    }
    __syncthreads();

    // ---- D: pass 2 along the rows, + 128, clamp; 16 consecutive lanes store 16 N bytes of a plane row
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t t = tid + 256u * i;
        if (t >= 8u * kBlocks) continue;
        const uint32_t b = (t >> 7) * 16u + (t & 15u), r = (t >> 4) & 7u;
        uint32_t c, bx, by;
        if (!jfdct::strip_block<LAYOUT>(a.ywb, a.yhb, a.cwb, sx, sy, b, &c, &bx, &by)) continue;
        const auto pass2 = [&](auto n) {
            constexpr int N = decltype(n)::value;
            const uint32_t pw = c ? a.pw[1] : a.pw[0], ph = c ? a.ph[1] : a.ph[0];
            const uint32_t x = bx * N, y = by * N + r;
            if (r >= static_cast<uint32_t>(N) || x >= pw || y >= ph) return;
            const uint4 v = *reinterpret_cast<const uint4 *>(blocks + b * kBlockPitch + r * 8u);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
            int d[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[2 * k] = static_cast<int>(u[k] << 16) >> 16;
                d[2 * k + 1] = static_cast<int>(u[k]) >> 16;
            }
            if constexpr (N > 1) jidct::idctn<N, 2>(d);
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (int k = 0; k < N; ++k) o[k >> 2] |= jidct::sample(d[k]) << (8 * (k & 3));
            u8 *dst = out + (c == 0u ? a.plane_off[0] : c == 1u ? a.plane_off[1] : a.plane_off[2]) + y * pw + x;
            if (x + N <= pw) {
                __builtin_memcpy(dst, o, N);  // any alignment: one global_store_dwordx2 / dword / short / byte
            } else {  // the plane's last block column: pw - x of the N samples are real
                for (uint32_t k = 0; x + k < pw; ++k) dst[k] = static_cast<u8>(o[k >> 2] >> (8u * (k & 3u)));
            }
        };
        if (NC == NY || c == 0u) pass2(std::integral_constant<int, NY>());
        else pass2(std::integral_constant<int, NC>());
    }
}

template <int LAYOUT>
void launch(int shrink, dim3 grid, hipStream_t st, const JpegrtArgs &a) {
    switch (shrink) {
        case 1: hipLaunchKernelGGL((k_jpegrt<LAYOUT, 1>), grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL((k_jpegrt<LAYOUT, 2>), grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL((k_jpegrt<LAYOUT, 4>), grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL((k_jpegrt<LAYOUT, 8>), grid, dim3(256), 0, st, a); break;
    }
}

}  // namespace

// The caller has checked that the image's coefficient payload and its RGB are below 2^32 bytes (so
// every byte offset inside an image fits 32 bits), and that shrink is 1, 2, 4 or 8.
int jpegrt_launch(const u8 *d_in, u8 *d_planes, int n, int w, int h, int layout, int quality, int shrink,
                  hipStream_t st) {
    const JpegGeom g(w, h, layout);
    const JpegPlanes p = g.planes(shrink);  // 4:2:0 at full size is the only case whose chroma planes are smaller than Y's
    JpegrtArgs a;
    a.in = d_in, a.out = d_planes;
    a.recips = device_jpegc_recips(quality);
    if (!a.recips) {
        set_error("jpeg round trip: no reciprocal table for quality %d", quality);
        return MIPX_EDEVICE;
    }
    a.in_img = static_cast<long long>(w) * h * 3;
    a.w = w, a.h = h;
    a.ywb = static_cast<uint32_t>(g.y.wb), a.yhb = static_cast<uint32_t>(g.y.hb);
    a.cwb = static_cast<uint32_t>(g.c.wb), a.ch = static_cast<uint32_t>(g.c.h);
    for (int c = 0; c < 2; ++c) a.pw[c] = static_cast<uint32_t>(p.w[c]), a.ph[c] = static_cast<uint32_t>(p.h[c]);
    for (int c = 0; c < 3; ++c) a.plane_off[c] = static_cast<uint32_t>(p.off[c]);
    a.out_img = static_cast<long long>(p.bytes);
    const long long gx = (static_cast<long long>(w) + 127) / 128, gy = static_cast<long long>(g.mh);  // a strip is a row of MCUs
    if (!grid_ok(gx * gy)) return MIPX_EUNSUPPORTED;
    a.gx = static_cast<uint32_t>(gx);
    const dim3 grid(static_cast<unsigned>(gx * gy), n);
    with_output_layout(layout, [&](auto L) {  // the caller has refused grey: no round trip of one component is built
        if constexpr (L.value != MIPX_YCC_GREY) launch<L.value>(shrink, grid, st, a);
    });
    return launch_check("k_jpegrt");
}

}  // namespace mipx
