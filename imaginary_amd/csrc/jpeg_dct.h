// jpeg_dct.h — the device functions the JPEG kernels share (k_jpegc.hip, k_jpegd.hip,
// k_jpegrt.hip): libjpeg's colour conversion and downsample into the blocks' LDS image, the
// place of each of a strip's blocks in its component's grid, its
// forward DCT and quantisation (jfdct), its dequantisation and inverse DCTs (jidct).  One copy
// of each pass; the rules themselves are stated at the top of k_jpegc.hip and k_jpegd.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.h"

namespace mipx {

constexpr int kBlocks = 48;      // blocks of one strip of MCUs (k_jpegc.hip)
constexpr int kBlockPitch = 72;  // int16s between blocks in LDS: 64 + 8, so 8 blocks' columns cover 32 banks

// ---- the encoder's side: RGB -> samples - 128, forward DCT, quantisation (k_jpegc.hip) ----
namespace jfdct {

using namespace dev;

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

// 4 samples of one row of a 1-band image from column x0, byte k of the result; past w - 1 the last repeats
__device__ __forceinline__ uint32_t load_grey4(const u8 *row, uint32_t x0, uint32_t w) {
    uint32_t d = 0u;
    if (x0 + 4u <= w) {
        __builtin_memcpy(&d, row + x0, 4);  // any alignment: one global_load_dword
        return d;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) d |= static_cast<uint32_t>(row[min(x0 + k, w - 1u)]) << (8 * k);
    return d;
}

// The pixels of strip (sx, sy) of a w x h image -> samples - 128 in the strip's LDS image, 256
// threads.  The strip is 128 x 8 pixels in 4:4:4 (blocks 0..15 Y, 16..31 Cb, 32..47 Cr) and
// 128 x 16 in 4:2:0 (blocks 0..31 two rows of Y, 32..39 Cb, 40..47 Cr).  ywb: real Y blocks
// across; cwb, ch (4:2:0): real chroma blocks across, chroma rows.  A lane loads 4 pixels of one
// row (4:4:4) or of two rows (4:2:0, one chroma sample pair) as 12-byte loads.  In MIPX_YCC_GREY the
// image has 1 band and the strip is 384 x 8 pixels, the 48 blocks of one block row in order: a lane
// loads 4 samples three times, 96 lanes to a row.
template <int LAYOUT>
__device__ __forceinline__ void strip_samples(int16_t *blocks, const u8 *in, uint32_t w, uint32_t h, uint32_t ywb,
                                              uint32_t cwb, uint32_t ch, uint32_t sx, uint32_t sy) {
    const uint32_t tid = threadIdx.x;
    if (LAYOUT == MIPX_YCC_GREY) {
#pragma unroll
        for (uint32_t i = 0; i < 3u; ++i) {
            const uint32_t t = tid + 256u * i, gr = t / 96u, gg = t - 96u * gr;  // row; group of 4 columns
            const uint32_t gx0 = sx * 384u + 4u * gg;
            if (gx0 < 8u * ywb) {
                const uint32_t v = load_grey4(in + min(sy * 8u + gr, h - 1u) * w, gx0, w);
                const int s4[4] = {static_cast<int>(v & 255u), static_cast<int>((v >> 8) & 255u),
                                   static_cast<int>((v >> 16) & 255u), static_cast<int>(v >> 24)};
                put4(blocks + (gg >> 1) * kBlockPitch + gr * 8u + (gg & 1u) * 4u, s4);
            }
        }
        return;
    }
    const uint32_t g = tid & 31u, r = tid >> 5;  // group of 4 columns; row (4:4:4) or row pair (4:2:0)
    const uint32_t x0 = sx * 128u + 4u * g;
    const uint32_t row_bytes = 3u * w;
    uint32_t d[3];
    int y[4], cb[4], cr[4];
    if (LAYOUT == MIPX_YCC_444) {
        if (x0 < 8u * ywb) {
            const uint32_t py = min(sy * 8u + r, h - 1u);
            load_rgb4(in + py * row_bytes, x0, w, d);
            rgb_ycc4(d, y, cb, cr);
            int16_t *s = blocks + (g >> 1) * kBlockPitch + r * 8u + (g & 1u) * 4u;
            put4(s, y);
            put4(s + 16 * kBlockPitch, cb);
            put4(s + 32 * kBlockPitch, cr);
        }
    } else if (x0 < 16u * cwb) {
        const uint32_t j = sy * 8u + r;  // the image's row pair
        const uint32_t y0 = min(2u * j, h - 1u), y1 = min(2u * j + 1u, h - 1u);
        int sb[2], sr[2];
        uint32_t d1[3];
        load_rgb4(in + y0 * row_bytes, x0, w, d);
        load_rgb4(in + y1 * row_bytes, x0, w, d1);
        int16_t *s = blocks + ((r >> 2) * 16u + (g >> 1)) * kBlockPitch + (2u * r & 7u) * 8u + (g & 1u) * 4u;
        rgb_ycc4(d, y, cb, cr);
        put4(s, y);
        sb[0] = cb[0] + cb[1], sb[1] = cb[2] + cb[3], sr[0] = cr[0] + cr[1], sr[1] = cr[2] + cr[3];
        rgb_ycc4(d1, y, cb, cr);
        put4(s + 8, y);
        sb[0] += cb[0] + cb[1], sb[1] += cb[2] + cb[3], sr[0] += cr[0] + cr[1], sr[1] += cr[2] + cr[3];
        if (j >= ch) {  // below the last chroma row: its rows again, not the repeated pixel row
            const uint32_t c0 = 2u * ch - 2u, c1 = min(c0 + 1u, h - 1u);
            load_rgb4(in + c0 * row_bytes, x0, w, d);
            load_rgb4(in + c1 * row_bytes, x0, w, d1);
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

// Block `blk` of that strip: its component (0: Y, 1: Cb, 2: Cr) and its column and row in that
// component's block grid; false for a block outside the real ones (ywb, yhb: real Y blocks across
// and down; cwb: real chroma blocks across).  k_jpegc.hip's block_offset keeps a copy of this map.
template <int LAYOUT>
__device__ __forceinline__ bool strip_block(uint32_t ywb, uint32_t yhb, uint32_t cwb, uint32_t sx, uint32_t sy,
                                            uint32_t blk, uint32_t *comp, uint32_t *bx, uint32_t *by) {
    if (LAYOUT == MIPX_YCC_444) {
        *comp = blk >> 4, *bx = sx * 16u + (blk & 15u), *by = sy;
        return *bx < ywb;
    }
    if (blk < 32u) {
        *comp = 0u, *bx = sx * 16u + (blk & 15u), *by = sy * 2u + (blk >> 4);
        return *bx < ywb && *by < yhb;
    }
    *comp = blk < 40u ? 1u : 2u, *bx = sx * 8u + (blk & 7u), *by = sy;
    return *bx < cwb;
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

// The rows pass on row `line` of a block's LDS image: a 16-byte read, the pass, a 16-byte write
__device__ __forceinline__ void fdct8_row(int16_t *blk, uint32_t line) {
    uint4 *p = reinterpret_cast<uint4 *>(blk + line * 8u);
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

// jcdctmgr.c: (|c| + 4 q) / (8 q) = ((|c| + 4 q) >> 3) / q, the division as a multiply by
// m = ceil(2^20 / q): exact for |c| + 4 q < 2^15 (the test walks every q and numerator)
__device__ __forceinline__ int quantise(int c, uint32_t e) {
    const uint32_t q = e >> 21, m = e & 0x1fffffu;
    const uint32_t n = (static_cast<uint32_t>(c < 0 ? -c : c) + 4u * q) >> 3;
    const int v = static_cast<int>(__umul24(n, m) >> kJpegcRecipShift);
    return c < 0 ? -v : v;
}

}  // namespace jfdct

// ---- the decoder's side: dequantisation, the inverse DCTs, the final clamp (k_jpegd.hip) ----
namespace jidct {

using namespace dev;

typedef unsigned short ushort2v __attribute__((ext_vector_type(2)));

// a * k + c and a * k modulo 2^32, with 24-bit signed a and k: the full-rate v_mad_i32_i24 /
// v_mul_i32_i24 (k_jpegc.hip)
__device__ __forceinline__ uint32_t mad24(int a, int k, uint32_t c) {
    uint32_t r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(k), "v"(c));
    return r;
}
__device__ __forceinline__ uint32_t mul24(int a, int k) {
    uint32_t r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "s"(k), "v"(a));
    return r;
}

// the low 16 bits of both 16-bit products (v_pk_mul_lo_u16): signed or not, they are the same
__device__ __forceinline__ uint32_t dequant2(uint32_t coefs, uint32_t q) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(ushort2v, coefs) * __builtin_bit_cast(ushort2v, q));
}

__device__ __forceinline__ int descale(uint32_t v, int s) { return static_cast<int>(v) >> s; }

// One 8-point pass of jidctint.c in place, |i| <= 2^15.  Sums are unsigned, so they wrap; the
// rounding constant of the descale rides in t0 and t1, which every output contains once.
template <int S>
__device__ __forceinline__ void idct8(int i[8]) {
    constexpr uint32_t R = 1u << (S - 1);
    const uint32_t e1 = mul24(i[2] + i[6], 4433);
    const uint32_t t2 = mad24(i[6], -15137, e1), t3 = mad24(i[2], 6270, e1);
    const uint32_t t0 = (static_cast<uint32_t>(i[0] + i[4]) << 13) + R;
    const uint32_t t1 = (static_cast<uint32_t>(i[0] - i[4]) << 13) + R;
    const uint32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const int z1 = i[7] + i[1], z2 = i[5] + i[3], z3 = i[7] + i[3], z4 = i[5] + i[1];
    const uint32_t z5 = mul24(z3 + z4, 9633);
    const uint32_t z3p = mad24(z3, -16069, z5), z4p = mad24(z4, -3196, z5);
    const uint32_t m1 = mul24(z1, -7373), m2 = mul24(z2, -20995);
    const uint32_t a0 = mad24(i[7], 2446, m1 + z3p), a1 = mad24(i[5], 16819, m2 + z4p);
    const uint32_t a2 = mad24(i[3], 25172, m2 + z3p), a3 = mad24(i[1], 12299, m1 + z4p);
    i[0] = descale(t10 + a3, S), i[7] = descale(t10 - a3, S);
    i[1] = descale(t11 + a2, S), i[6] = descale(t11 - a2, S);
    i[2] = descale(t12 + a1, S), i[5] = descale(t12 - a1, S);
    i[3] = descale(t13 + a0, S), i[4] = descale(t13 - a0, S);
}

// clamp(v + 128, 0, 255).  The asm barrier keeps the backend from fusing shift + clamp + byte
// packing into v_ashr_pk_u8_i32 with the next byte ORed into its unwritten half (k_sep.hip
// fixed_round_i).
__device__ __forceinline__ uint32_t sample(int v) {
    int s = clampi(v + 128, 0, 255);
    asm("" : "+v"(s));
    return static_cast<uint32_t>(s);
}

// which of a line's 8 inputs the N-point pass reads (the rule at k_jpegds in k_jpegd.hip)
template <int N>
__device__ __forceinline__ constexpr bool idct_reads(uint32_t k) {
    return N == 8 || (N == 4 && k != 4u) || (N == 2 && (k == 0u || (k & 1u)));
}

// One pass of jidctred.c's 4 x 4 inverse DCT: i[0..3] from i[0 1 2 3 5 6 7]; the rounding
// constant rides in t0
template <int S>
__device__ __forceinline__ void idct4(int i[8]) {
    const uint32_t t0 = (static_cast<uint32_t>(i[0]) << 14) + (1u << (S - 1));
    const uint32_t t2 = mad24(i[6], -6270, mul24(i[2], 15137));
    const uint32_t t10 = t0 + t2, t12 = t0 - t2;
    const uint32_t a0 = mad24(i[1], 8697, mad24(i[3], -17799, mad24(i[5], 11893, mul24(i[7], -1730))));
    const uint32_t a2 = mad24(i[1], 20995, mad24(i[3], 7373, mad24(i[5], -4926, mul24(i[7], -4176))));
    i[0] = descale(t10 + a2, S), i[3] = descale(t10 - a2, S);
    i[1] = descale(t12 + a0, S), i[2] = descale(t12 - a0, S);
}

// ... and of its 2 x 2 one: i[0..1] from i[0 1 3 5 7]
template <int S>
__device__ __forceinline__ void idct2(int i[8]) {
    const uint32_t t10 = (static_cast<uint32_t>(i[0]) << 15) + (1u << (S - 1));
    const uint32_t t0 = mad24(i[1], 29692, mad24(i[3], -10426, mad24(i[5], 6967, mul24(i[7], -5906))));
    i[0] = descale(t10 + t0, S), i[1] = descale(t10 - t0, S);
}

template <int N, int PASS>
__device__ __forceinline__ void idctn(int i[8]) {
    if constexpr (N == 8) idct8<PASS == 1 ? 11 : 18>(i);
    if constexpr (N == 4) idct4<PASS == 1 ? 12 : 19>(i);
    if constexpr (N == 2) idct2<PASS == 1 ? 13 : 20>(i);
}

}  // namespace jidct

}  // namespace mipx
