// k_jpegc.hip — a JPEG encoder's front half on gfx950 (PARITY_ASSUMPTIONS.md row 17): interleaved
// RGB in, quantised DCT coefficients out, as libjpeg computes them with its default settings.
//   colour (jccolor.c), int32, arithmetic shifts:
//     Y  = (19595 R + 38470 G + 7471 B + 32768) >> 16
//     Cb = (-11059 R - 21709 G + 32768 B + 8388608 + 32767) >> 16
//     Cr = (32768 R - 27439 G - 5329 B + 8388608 + 32767) >> 16
//   4:2:0 chroma (jcsample.c h2v2_downsample): (a + b + c + d + bias) >> 2 over 2 x 2 pixels,
//     bias 1 on even output columns and 2 on odd ones
//   edges: columns past w - 1 and rows past h - 1 repeat the last one; 4:2:0 chroma rows past
//     ch - 1 repeat the last DOWNSAMPLED row (rows 2 ch - 2 and min(2 ch - 1, h - 1)), which is
//     not the downsample of the repeated last pixel row
//   forward DCT (jfdctint.c), samples - 128, rows then columns; quantisation (jcdctmgr.c)
//     v = (|c| + (q8 >> 1)) / q8 with q8 = 8 q, the sign restored
// Per image the output is int16 coefficients of the real blocks only: Y, then Cb, then Cr, each
// hb x wb blocks in raster order, a block's 64 coefficients in natural order.  Bit-exact.
//
// A workgroup makes the 48 blocks of one strip of MCUs: 128 x 16 pixels in 4:2:0 (2 x 16 Y
// blocks, 8 Cb, 8 Cr), 128 x 8 in 4:4:4 (16 blocks per component).  Phase A: a lane loads 4
// pixels of one row (4:4:4) or of two rows (4:2:0, one chroma sample pair) as 12-byte loads,
// converts, and writes sample - 128 as int16 into the blocks' LDS image.  Phase B: one lane per
// block row (384 of them over 256 threads) runs the row pass on a 16-byte LDS read and writes
// it back.  Phase C: one lane per block column runs the column pass and quantises.  Phase D:
// a lane stores one coefficient row, 16 bytes: a block is 128 contiguous bytes and the blocks
// of a component's block row follow each other, so a wave stores 1 KiB per instruction.
// Blocks sit 144 bytes apart in LDS, so the 8 blocks of a wave's column reads cover all 32
// banks.  Every multiply has 24-bit operands (v_mad_i32_i24 / v_mul_u32_u24, full rate); the
// division is a multiply by the host-built reciprocal of q (build_jpegc_recips).  Global
// accesses are plain unaligned ones: rows, images and both pointers start on any byte.
#include <hip/hip_runtime.h>

#include "device_common.h"

namespace mipx {
namespace {

using namespace dev;

struct JpegcArgs {
    const u8 *in;
    u8 *out;
    const uint32_t *recips;    // [lum 64 | chr 64]: m | q << 21 (build_jpegc_recips)
    long long in_img, out_img;  // bytes per image
    uint32_t w, h;
    uint32_t ywb, yhb;          // real Y blocks across and down (4:4:4: of every component)
    uint32_t cwb, ch;           // 4:2:0: real chroma blocks (= MCUs) across; chroma rows
    uint32_t cb_off, cr_off;    // byte offsets of the Cb and Cr coefficients in an image's output
    uint32_t gx;                // strips across one image
};

constexpr int kBlocks = 48;      // blocks of one strip
constexpr int kBlockPitch = 72;  // int16s between blocks in LDS: 64 + 8, so 8 blocks' columns cover 32 banks
constexpr uint32_t kNoBlock = 0xffffffffu;

// a * k + c with 24-bit signed a and k: the full-rate v_mad_i32_i24 (k_ycc.hip)
__device__ __forceinline__ int mad24(int a, int k, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(c));
    return r;
}
__device__ __forceinline__ int mul24(int a, int k) {
    int r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "s"(k), "v"(a));
    return r;
}

// 4 pixels of one row from column x0: bytes 3 k + c of d; past w - 1 the last pixel repeats
__device__ __forceinline__ void load_rgb4(const u8 *row, uint32_t x0, uint32_t w, uint32_t d[3]) {
    if (x0 + 4u <= w) {
        __builtin_memcpy(d, row + 3u * x0, 12);  // any alignment: one global_load_dwordx3
        return;
    }
    d[0] = d[1] = d[2] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u8 *p = row + 3u * min(x0 + k, w - 1u);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[(3 * k + c) >> 2] |= static_cast<uint32_t>(p[c]) << (8 * ((3 * k + c) & 3));
    }
}
__device__ __forceinline__ int rgb_byte(const uint32_t d[3], int i) {
    return static_cast<int>((d[i >> 2] >> (8 * (i & 3))) & 255u);
}
// jccolor.c on the 4 pixels of d
__device__ __forceinline__ void rgb_ycc4(const uint32_t d[3], int y[4], int cb[4], int cr[4]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = rgb_byte(d, 3 * k), g = rgb_byte(d, 3 * k + 1), b = rgb_byte(d, 3 * k + 2);
        y[k] = mad24(r, 19595, mad24(g, 38470, mad24(b, 7471, 32768))) >> 16;
        cb[k] = mad24(r, -11059, mad24(g, -21709, mad24(b, 32768, 8388608 + 32767))) >> 16;
        cr[k] = mad24(r, 32768, mad24(g, -27439, mad24(b, -5329, 8388608 + 32767))) >> 16;
    }
}
__device__ __forceinline__ uint32_t pack16(int lo, int hi) {
    return (static_cast<uint32_t>(lo) & 0xffffu) | (static_cast<uint32_t>(hi) << 16);
}
// 4 samples - 128 as int16 at s (8-byte aligned)
__device__ __forceinline__ void put4(int16_t *s, const int v[4]) {
    *reinterpret_cast<uint2 *>(s) = make_uint2(pack16(v[0] - 128, v[1] - 128), pack16(v[2] - 128, v[3] - 128));
}

// One 8-point pass of jfdctint.c in place.  FIRST: the rows pass (outputs scaled up by
// PASS1_BITS = 2); otherwise the columns pass.  |d| <= 128 before the first pass and <= 3784
// before the second, so every product has 24-bit operands and every sum fits int32; the
// rounding constant of the descale rides in the first term of each sum.
template <bool FIRST>
__device__ __forceinline__ void fdct8(int d[8]) {
    constexpr int S = FIRST ? 11 : 15, R = 1 << (S - 1);
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) {
        d[0] = (t10 + t11) << 2, d[4] = (t10 - t11) << 2;
    } else {
        d[0] = (t10 + t11 + 2) >> 2, d[4] = (t10 - t11 + 2) >> 2;
    }
    const int e1 = mad24(t12 + t13, 4433, R);
    d[2] = mad24(t13, 6270, e1) >> S;
    d[6] = mad24(t12, -15137, e1) >> S;
    const int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = mad24(z3 + z4, 9633, R);
    const int z3p = mad24(z3, -16069, z5), z4p = mad24(z4, -3196, z5);
    const int a1 = mul24(z1, -7373), a2 = mul24(z2, -20995);
    d[7] = mad24(t4, 2446, a1 + z3p) >> S;
    d[5] = mad24(t5, 16819, a2 + z4p) >> S;
    d[3] = mad24(t6, 25172, a2 + z3p) >> S;
    d[1] = mad24(t7, 12299, a1 + z4p) >> S;
}

// jcdctmgr.c: (|c| + 4 q) / (8 q) = ((|c| + 4 q) >> 3) / q, the division as a multiply by
// m = ceil(2^20 / q): exact for |c| + 4 q < 2^15 (the test walks every q and numerator)
__device__ __forceinline__ int quantise(int c, uint32_t e) {
    const uint32_t q = e >> 21, m = e & 0x1fffffu;
    const uint32_t n = (static_cast<uint32_t>(c < 0 ? -c : c) + 4u * q) >> 3;
    const int v = static_cast<int>(__umul24(n, m) >> kJpegcRecipShift);
    return c < 0 ? -v : v;
}

// Where block `blk` of strip (sx, sy) goes in the image's output, in bytes; kNoBlock for a block
// outside the real ones (the entropy coder's dummy blocks).  *chroma: which table quantises it.
template <int LAYOUT>
__device__ __forceinline__ uint32_t block_offset(const JpegcArgs &a, uint32_t sx, uint32_t sy, uint32_t blk,
                                                 uint32_t *chroma) {
    if (LAYOUT == MIPX_YCC_444) {
        const uint32_t comp = blk >> 4, bx = sx * 16u + (blk & 15u);
        *chroma = comp ? 64u : 0u;
        if (bx >= a.ywb) return kNoBlock;
        return (comp == 0 ? 0u : comp == 1 ? a.cb_off : a.cr_off) + (sy * a.ywb + bx) * 128u;
    }
    if (blk < 32u) {
        const uint32_t bx = sx * 16u + (blk & 15u), by = sy * 2u + (blk >> 4);
        *chroma = 0u;
        if (bx >= a.ywb || by >= a.yhb) return kNoBlock;
        return (by * a.ywb + bx) * 128u;
    }
    const uint32_t bx = sx * 8u + (blk & 7u);
    *chroma = 64u;
    if (bx >= a.cwb) return kNoBlock;
    return (blk < 40u ? a.cb_off : a.cr_off) + (sy * a.cwb + bx) * 128u;
}

template <int LAYOUT>
__global__ void __launch_bounds__(256) k_jpegc(const JpegcArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t blocks[kBlocks * kBlockPitch];
    __shared__ uint32_t recips[128];
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    const uint32_t sy = blockIdx.x / a.gx, sx = blockIdx.x - sy * a.gx;
    const uint32_t tid = threadIdx.x;
    if (tid < 128u) recips[tid] = a.recips[tid];

    // ---- A: pixels -> samples - 128 in LDS
    {
        const uint32_t g = tid & 31u, r = tid >> 5;  // group of 4 columns; row (4:4:4) or row pair (4:2:0)
        const uint32_t x0 = sx * 128u + 4u * g;
        const uint32_t row_bytes = 3u * a.w;
        uint32_t d[3];
        int y[4], cb[4], cr[4];
        if (LAYOUT == MIPX_YCC_444) {
            if (x0 < 8u * a.ywb) {
                const uint32_t py = min(sy * 8u + r, a.h - 1u);
                load_rgb4(in + py * row_bytes, x0, a.w, d);
                rgb_ycc4(d, y, cb, cr);
                int16_t *s = blocks + (g >> 1) * kBlockPitch + r * 8u + (g & 1u) * 4u;
                put4(s, y);
                put4(s + 16 * kBlockPitch, cb);
                put4(s + 32 * kBlockPitch, cr);
            }
        } else if (x0 < 16u * a.cwb) {
            const uint32_t j = sy * 8u + r;  // the image's row pair
            const uint32_t y0 = min(2u * j, a.h - 1u), y1 = min(2u * j + 1u, a.h - 1u);
            int sb[2], sr[2];
            uint32_t d1[3];
            load_rgb4(in + y0 * row_bytes, x0, a.w, d);
            load_rgb4(in + y1 * row_bytes, x0, a.w, d1);
            int16_t *s = blocks + ((r >> 2) * 16u + (g >> 1)) * kBlockPitch + (2u * r & 7u) * 8u + (g & 1u) * 4u;
            rgb_ycc4(d, y, cb, cr);
            put4(s, y);
            sb[0] = cb[0] + cb[1], sb[1] = cb[2] + cb[3], sr[0] = cr[0] + cr[1], sr[1] = cr[2] + cr[3];
            rgb_ycc4(d1, y, cb, cr);
            put4(s + 8, y);
            sb[0] += cb[0] + cb[1], sb[1] += cb[2] + cb[3], sr[0] += cr[0] + cr[1], sr[1] += cr[2] + cr[3];
            if (j >= a.ch) {  // below the last chroma row: its rows again, not the repeated pixel row
                const uint32_t c0 = 2u * a.ch - 2u, c1 = min(c0 + 1u, a.h - 1u);
                load_rgb4(in + c0 * row_bytes, x0, a.w, d);
                load_rgb4(in + c1 * row_bytes, x0, a.w, d1);
                rgb_ycc4(d, y, cb, cr);
                sb[0] = cb[0] + cb[1], sb[1] = cb[2] + cb[3], sr[0] = cr[0] + cr[1], sr[1] = cr[2] + cr[3];
                rgb_ycc4(d1, y, cb, cr);
                sb[0] += cb[0] + cb[1], sb[1] += cb[2] + cb[3], sr[0] += cr[0] + cr[1], sr[1] += cr[2] + cr[3];
            }
            // the lane's chroma columns are 2 g (even: bias 1) and 2 g + 1 (odd: bias 2)
            int16_t *c = blocks + (32u + (g >> 2)) * kBlockPitch + r * 8u + (g & 3u) * 2u;
            *reinterpret_cast<uint32_t *>(c) = pack16(((sb[0] + 1) >> 2) - 128, ((sb[1] + 2) >> 2) - 128);
            *reinterpret_cast<uint32_t *>(c + 8 * kBlockPitch) =
                pack16(((sr[0] + 1) >> 2) - 128, ((sr[1] + 2) >> 2) - 128);
        }
    }
    __syncthreads();

    // the lane's two (block, row / column) tasks: 384 over 256 threads
    uint32_t off[2], chroma[2];
    int16_t *blk[2];
    uint32_t line[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const uint32_t t = tid + 256u * i;
        off[i] = kNoBlock, chroma[i] = 0u, line[i] = t & 7u;
        blk[i] = blocks + (t >> 3) * kBlockPitch;
        if (t < 8u * kBlocks) off[i] = block_offset<LAYOUT>(a, sx, sy, t >> 3, &chroma[i]);
    }

    // ---- B: the rows pass
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (off[i] == kNoBlock) continue;
        uint4 *p = reinterpret_cast<uint4 *>(blk[i] + line[i] * 8u);
        const uint4 v = *p;
        const uint32_t u[4] = {v.x, v.y, v.z, v.w};
        int d[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[2 * k] = static_cast<int>(u[k] << 16) >> 16;
            d[2 * k + 1] = static_cast<int>(u[k]) >> 16;
        }
        fdct8<true>(d);
        *p = make_uint4(pack16(d[0], d[1]), pack16(d[2], d[3]), pack16(d[4], d[5]), pack16(d[6], d[7]));
    }
    __syncthreads();

    // ---- C: the columns pass, then quantisation
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (off[i] == kNoBlock) continue;
        int16_t *p = blk[i] + line[i];
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[8 * k];
        fdct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k)
            p[8 * k] = static_cast<int16_t>(quantise(d[k], recips[chroma[i] + 8u * k + line[i]]));
    }
    __syncthreads();

    // ---- D: a coefficient row per lane, 16 bytes
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        if (off[i] == kNoBlock) continue;
        const uint4 v = *reinterpret_cast<const uint4 *>(blk[i] + line[i] * 8u);
        __builtin_memcpy(out + off[i] + line[i] * 16u, &v, 16);  // any alignment: one global_store_dwordx4
    }
}

}  // namespace

int jpegc_launch(const u8 *d_in, u8 *d_out, int n, int w, int h, int layout, int quality, hipStream_t st) {
    const long long in_img = static_cast<long long>(w) * h * 3;
    const long long out_img = static_cast<long long>(mipx_jpegc_bytes(w, h, layout));
    if (in_img > 0xffffffffLL || out_img > 0xffffffffLL) {  // byte offsets inside an image are 32-bit
        set_error("rgb to jpeg coefficients: image %dx%d too large (an image's bytes >= 2^32)", w, h);
        return MIPX_EUNSUPPORTED;
    }
    const bool sub = layout == MIPX_YCC_420;
    JpegcArgs a;
    a.in = d_in, a.out = d_out;
    a.recips = device_jpegc_recips(quality);
    if (!a.recips) {
        set_error("rgb to jpeg coefficients: no reciprocal table for quality %d", quality);
        return MIPX_EDEVICE;
    }
    a.in_img = in_img, a.out_img = out_img;
    a.w = w, a.h = h;
    a.ywb = (static_cast<uint32_t>(w) + 7u) / 8u, a.yhb = (static_cast<uint32_t>(h) + 7u) / 8u;
    a.ch = (static_cast<uint32_t>(h) + 1u) / 2u;
    a.cwb = sub ? ((static_cast<uint32_t>(w) + 1u) / 2u + 7u) / 8u : a.ywb;
    const uint32_t chb = sub ? (a.ch + 7u) / 8u : a.yhb;
    a.cb_off = a.ywb * a.yhb * 128u;
    a.cr_off = a.cb_off + a.cwb * chb * 128u;
    const long long gx = (static_cast<long long>(w) + 127) / 128;
    const long long gy = sub ? chb : a.yhb;
    if (!grid_ok(gx * gy)) return MIPX_EUNSUPPORTED;
    a.gx = static_cast<uint32_t>(gx);
    const dim3 grid(static_cast<unsigned>(gx * gy), n);
    if (sub) hipLaunchKernelGGL(k_jpegc<MIPX_YCC_420>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_jpegc<MIPX_YCC_444>, grid, dim3(256), 0, st, a);
    return launch_check("k_jpegc");
}

}  // namespace mipx
