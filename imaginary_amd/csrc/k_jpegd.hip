// k_jpegd.hip — a JPEG decoder's middle on gfx950 (PARITY_ASSUMPTIONS.md row 18): the file's
// quantised DCT coefficients in, sample planes out, as libjpeg computes them with its default
// settings (jddctmgr.c, jidctint.c jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2), made total:
//   dequantise: d = int16(coef * q), the low 16 bits of the product as a signed value
//   one 8-point pass on i0..i7 with descale shift S, int32 sums that wrap modulo 2^32:
//     z1 = (i2 + i6) * 4433;  t2 = z1 - i6 * 15137;  t3 = z1 + i2 * 6270
//     t0 = (i0 + i4) << 13;   t1 = (i0 - i4) << 13
//     t10 = t0 + t3; t13 = t0 - t3; t11 = t1 + t2; t12 = t1 - t2
//     a0 = i7; a1 = i5; a2 = i3; a3 = i1
//     z1 = a0 + a3; z2 = a1 + a2; z3 = a0 + a2; z4 = a1 + a3; z5 = (z3 + z4) * 9633
//     a0 *= 2446; a1 *= 16819; a2 *= 25172; a3 *= 12299
//     z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5
//     a0 += z1 + z3; a1 += z2 + z4; a2 += z2 + z3; a3 += z1 + z4
//     out = (t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3),
//           each (v + (1 << (S - 1))) >> S, the shift arithmetic
//   pass 1 down the columns, S = 11, saturated to int16; pass 2 along the rows, S = 18;
//   sample = clamp(v + 128, 0, 255)
// libjpeg's shortcut for a column without AC terms gives the same number as the full pass.
// Per image the input is 384 bytes of tables (Y, Cb, Cr; 64 uint16 each, natural order), then
// the int16 coefficients of the real blocks only: Y, then Cb, then Cr, each hb x wb blocks in
// raster order, natural order inside a block (what k_jpegc.hip writes).  The output is the
// packed planes k_ycc.hip takes: Y (h x w), then Cb, then Cr (ch x cw each), cropped to the real
// sizes.  Bit-exact against tests/jpegd_ref.py.
//
// A workgroup takes a run of 32 consecutive blocks of one component's block row: 4 KiB of
// contiguous coefficients.  Phase A: a lane loads one coefficient row, 16 bytes (a wave loads
// 1 KiB per instruction), multiplies it by its row of the component's table as packed 16-bit
// products, and writes the 8 int16 into the blocks' LDS image.  Phase B: one lane per block
// column runs pass 1 in place.  Phase C: one lane per block row runs pass 2 on a 16-byte LDS read
// and holds 8 output bytes; lanes go along the run first, so 32 consecutive lanes store the 256
// contiguous bytes of one plane row of the run.  Only the last block column of a plane stores
// fewer than 8 bytes, and rows past the plane's height are not stored.  Blocks sit 144 bytes
// apart in LDS (k_jpegc.hip): the 8 blocks of a wave's column accesses cover all 32 banks, and
// so do 8 consecutive lanes' 16-byte row reads.  The operands of every multiply are below 2^18
// (int16 inputs, sums of at most four), so the full-rate 24-bit multiplies are exact modulo
// 2^32.  Global accesses are plain unaligned ones: images and both pointers start on any byte.
#include <hip/hip_runtime.h>

#include "device_common.h"

namespace mipx {
namespace {

using namespace dev;

struct JpegdArgs {
    const u8 *in;
    u8 *out;
    long long in_img, out_img;  // bytes per image
    // [0]: Y, [1]: Cb and Cr
    uint32_t wb[2], hb[2];      // real blocks across and down
    uint32_t pw[2], ph[2];      // plane size in samples
    uint32_t runs[2];           // runs of kRun blocks in one block row
    uint32_t coef_off[3];       // byte offset of each component's coefficients in an image's input
    uint32_t plane_off[3];      // byte offset of each component's plane in an image's output
    uint32_t groups[2];         // workgroups of one image's Y, and of one chroma component
};

constexpr int kRun = 32;         // blocks of one workgroup; 8 lanes per block
constexpr int kBlockPitch = 72;  // int16s between blocks in LDS: 64 + 8 (k_jpegc.hip)

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

__global__ void __launch_bounds__(256) k_jpegd(const JpegdArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t blocks[kRun * kBlockPitch];
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    // which component, block row and run: uniform over the workgroup
    uint32_t g = blockIdx.x, comp = 0;
    if (g >= a.groups[0]) {
        g -= a.groups[0];
        comp = 1;
        if (g >= a.groups[1]) g -= a.groups[1], comp = 2;
    }
    const uint32_t c = comp ? 1u : 0u;
    const uint32_t by = g / a.runs[c], bx0 = (g - by * a.runs[c]) * kRun;
    const uint32_t wb = a.wb[c], pw = a.pw[c], ph = a.ph[c];
    const uint32_t tid = threadIdx.x;

    // ---- A: a coefficient row per lane, dequantised into LDS
    {
        const uint32_t b = tid >> 3, r = tid & 7u;
        if (bx0 + b < wb) {
            uint4 v, q;
            // any alignment: one global_load_dwordx4 each
            __builtin_memcpy(&v, in + MIPX_JPEGD_HEADER_BYTES + a.coef_off[comp] + (by * wb + bx0) * 128u + tid * 16u, 16);
            __builtin_memcpy(&q, in + comp * 128u + r * 16u, 16);
            *reinterpret_cast<uint4 *>(blocks + b * kBlockPitch + r * 8u) =
                make_uint4(dequant2(v.x, q.x), dequant2(v.y, q.y), dequant2(v.z, q.z), dequant2(v.w, q.w));
        }
    }
    __syncthreads();

    // ---- B: pass 1, a block column per lane, in place
    {
        const uint32_t b = tid >> 3, col = tid & 7u;
        if (bx0 + b < wb) {
            int16_t *p = blocks + b * kBlockPitch + col;
            int d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = p[8 * k];
            idct8<11>(d);
#pragma unroll
            for (int k = 0; k < 8; ++k) p[8 * k] = static_cast<int16_t>(clampi(d[k], -32768, 32767));
        }
    }
    __syncthreads();

    // ---- C: pass 2, a block row per lane; 32 consecutive lanes make 256 bytes of one plane row
    {
        const uint32_t b = tid & 31u, r = tid >> 5;
        const uint32_t x = (bx0 + b) * 8u, y = by * 8u + r;
        if (bx0 + b < wb && y < ph) {
            const uint4 v = *reinterpret_cast<const uint4 *>(blocks + b * kBlockPitch + r * 8u);
            const uint32_t u[4] = {v.x, v.y, v.z, v.w};
            int d[8];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[2 * k] = static_cast<int>(u[k] << 16) >> 16;
                d[2 * k + 1] = static_cast<int>(u[k]) >> 16;
            }
            idct8<18>(d);
            uint32_t o[2];
#pragma unroll
            for (int k = 0; k < 2; ++k)
                o[k] = sample(d[4 * k]) | (sample(d[4 * k + 1]) << 8) | (sample(d[4 * k + 2]) << 16) |
                       (sample(d[4 * k + 3]) << 24);
            u8 *dst = out + a.plane_off[comp] + y * pw + x;
            if (x + 8u <= pw) {
                __builtin_memcpy(dst, o, 8);  // any alignment: one global_store_dwordx2
            } else {  // the plane's last block column: pw - x of the 8 samples are real
                for (uint32_t k = 0; x + k < pw; ++k) dst[k] = static_cast<u8>(o[k >> 2] >> (8u * (k & 3u)));
            }
        }
    }
}

}  // namespace

// The caller has checked that an image's payload and its RGB are below 2^32 bytes, so every
// byte offset inside an image fits 32 bits.
int jpegd_launch(const u8 *d_in, u8 *d_planes, int n, int w, int h, int layout, hipStream_t st) {
    const bool sub = layout == MIPX_YCC_420;
    JpegdArgs a;
    a.in = d_in, a.out = d_planes;
    a.in_img = static_cast<long long>(mipx_jpegd_bytes(w, h, layout));
    a.out_img = static_cast<long long>(mipx_ycc_bytes(w, h, layout));
    a.pw[0] = w, a.ph[0] = h;
    a.pw[1] = sub ? (static_cast<uint32_t>(w) + 1u) / 2u : w;
    a.ph[1] = sub ? (static_cast<uint32_t>(h) + 1u) / 2u : h;
    long long total = 0;
    for (int c = 0; c < 2; ++c) {
        a.wb[c] = (a.pw[c] + 7u) / 8u, a.hb[c] = (a.ph[c] + 7u) / 8u;
        a.runs[c] = (a.wb[c] + kRun - 1u) / kRun;
        a.groups[c] = a.runs[c] * a.hb[c];
        total += static_cast<long long>(a.runs[c]) * a.hb[c] * (c ? 2 : 1);
    }
    if (!grid_ok(total)) return MIPX_EUNSUPPORTED;
    a.coef_off[0] = 0u, a.plane_off[0] = 0u;
    a.coef_off[1] = a.wb[0] * a.hb[0] * 128u, a.plane_off[1] = a.pw[0] * a.ph[0];
    a.coef_off[2] = a.coef_off[1] + a.wb[1] * a.hb[1] * 128u, a.plane_off[2] = a.plane_off[1] + a.pw[1] * a.ph[1];
    hipLaunchKernelGGL(k_jpegd, dim3(static_cast<unsigned>(total), n), dim3(256), 0, st, a);
    return launch_check("k_jpegd");
}

}  // namespace mipx
