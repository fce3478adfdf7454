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
#include "jpeg_dct.h"

namespace mipx {
namespace {

using namespace dev;
using namespace jidct;

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
    const JpegGeom g(w, h, layout);
    JpegdArgs a;
    a.in = d_in, a.out = d_planes;
    a.in_img = static_cast<long long>(MIPX_JPEGD_HEADER_BYTES + g.coef_bytes);
    a.out_img = static_cast<long long>(g.plane_bytes);
    long long total = 0;
    for (int c = 0; c < 2; ++c) {
        a.pw[c] = static_cast<uint32_t>(g.of(c).w), a.ph[c] = static_cast<uint32_t>(g.of(c).h);
        a.wb[c] = static_cast<uint32_t>(g.of(c).wb), a.hb[c] = static_cast<uint32_t>(g.of(c).hb);
        a.runs[c] = (a.wb[c] + kRun - 1u) / kRun;  // grey's chroma class: 0 runs, 0 groups
        a.groups[c] = a.runs[c] * a.hb[c];
        total += static_cast<long long>(a.runs[c]) * a.hb[c] * (c ? 2 : 1);
    }
    if (!grid_ok(total)) return MIPX_EUNSUPPORTED;
    for (int c = 0; c < 3; ++c)
        a.coef_off[c] = static_cast<uint32_t>(g.coef_off[c]), a.plane_off[c] = static_cast<uint32_t>(g.plane_off[c]);
    hipLaunchKernelGGL(k_jpegd, dim3(static_cast<unsigned>(total), n), dim3(256), 0, st, a);
    return launch_check("k_jpegd");
}

// ---- k_jpegds: the same payload decoded at 1/2, 1/4 or 1/8 (PARITY_ASSUMPTIONS.md row 19) ----
// libjpeg's shrink-on-load (jdmaster.c, jddctmgr.c, jidctred.c): at scale 1/s every component
// gets an N x N inverse DCT of its 8 x 8 blocks, which then tile its plane at pitch N.  Y and
// 4:4:4 chroma take N = 8 / s; 4:2:0 chroma takes N = 16 / s, so all three planes come out at
// ceil(W / s) x ceil(H / s) and there is no upsampling: the output is three equal planes, the
// packed MIPX_YCC_444 layout k_ycc.hip takes.  4:2:2 chroma takes N = 8 / s like Y (its vertical
// ratio is 1, and jdmaster.c enlarges a component's N only when both ratios allow it): it comes
// out ceil(H / s) high and ceil(ceil(W / s) / 2) wide, so the output is the packed MIPX_YCC_422
// planes of the decoded size, which k_ycc.hip then upsamples.  Dequantisation, pass order, the int16 saturation
// after pass 1 and the final clamp are k_jpegd's; with DS(v, S) = (v + (1 << (S - 1))) >> S:
//   N = 8: the pass above, S = 11 then 18
//   N = 4: on i0 i1 i2 i3 i5 i6 i7 (i4 is never read), S = 12 then 19:
//     t0 = i0 << 14;  t2 = i2 * 15137 - i6 * 6270;  t10 = t0 + t2;  t12 = t0 - t2
//     a0 = -i7 * 1730 + i5 * 11893 - i3 * 17799 + i1 * 8697
//     a2 = -i7 * 4176 - i5 * 4926 + i3 * 7373 + i1 * 20995
//     out = DS(t10 + a2), DS(t12 + a0), DS(t12 - a0), DS(t10 - a2)
//   N = 2: on i0 i1 i3 i5 i7, S = 13 then 20:
//     t10 = i0 << 15;  t0 = -i7 * 5906 + i5 * 6967 - i3 * 10426 + i1 * 29692
//     out = DS(t10 + t0), DS(t10 - t0)
//   N = 1: DS(d00, 3)
// Bit-exact against tests/jpegds_ref.py.  Every multiplier is below 2^15 and every operand an
// int16, so the 24-bit multiplies stay exact modulo 2^32.
//
// One launch; a workgroup is uniform in its component and so in its N.  For N = 8, 4, 2 it takes
// a run of 256 / N consecutive blocks of one block row (32, 64, 128: 4, 8, 16 KiB of contiguous
// coefficients) and runs k_jpegd's three phases on them.  The run grows as N shrinks because a
// block gives only N bytes of a plane row: with 256 / N blocks a plane row of the run is 256
// contiguous bytes at every N.  In phase C a lane holds 8 or 4 bytes of one output row (one block
// at N = 8 and 4, two neighbouring blocks at N = 2, where half the lanes then rest: the pass is
// 4 multiplies and a 2-byte store per lane would halve what a store instruction moves), lanes
// along the run first, so 32 or 64 consecutive lanes store those 256 bytes with dwordx2 or dword
// stores: at N = 4 and 2 one wave stores one whole row of the run.  Phase A keeps one 16-byte coefficient row per lane and
// instruction (a wave loads 1 KiB), 8 / N rows per lane, and leaves out the rows no pass reads
// (row 4 at N = 4; rows 2, 4, 6 at N = 2): their lanes load and write nothing.  Phase B leaves
// out the same columns.  The LDS image keeps k_jpegd's 144-byte block pitch, so the bank
// arithmetic is unchanged.  N = 1 occurs only where the plane is the block grid itself
// (pw = wb, ph = hb), so it is linear: a lane reads the DC terms of 4 consecutive blocks (2 bytes
// each, 128 apart; nothing else of the block is touched) and stores 4 bytes, a wave 256.
// Only the last block column of a plane stores fewer than N bytes, and rows past the plane's
// height are not stored.  MIPX_YCC_GREY: Y's workgroups alone, as in k_jpegd; the output is the
// 1-band image of ceil(W / s) x ceil(H / s), at N = 1 the block grid's DC terms.
namespace {

struct JpegdsArgs {
    const u8 *in;
    u8 *out;
    long long in_img, out_img;  // bytes per image
    // [0]: Y, [1]: Cb and Cr
    uint32_t pw[2], ph;         // plane size: ceil(W / s) x ceil(H / s); 4:2:2 chroma half as wide
    uint32_t plane_off[3];      // byte offset of each component's plane in an image's output
    uint32_t nidct[2];          // 8, 4, 2 or 1
    uint32_t wb[2], hb[2];      // real blocks across and down (the file's)
    uint32_t runs[2];           // runs of 256 / N blocks in one block row (N > 1)
    uint32_t groups[2];         // workgroups of one image's Y, and of one chroma component
    uint32_t coef_off[3];       // byte offset of each component's coefficients in an image's input
};

constexpr int kMaxRun = 128;     // N = 2
constexpr int kDcPerLane = 4;    // N = 1: blocks of one lane

// A run of 256 / N blocks of block row `by`, from block bx0, of a component whose coefficients
// start at `coefs` and whose table is `qt`; `plane` is its output plane
template <int N>
__device__ __forceinline__ void jpegds_run(int16_t *blocks, const u8 *coefs, const u8 *qt, u8 *plane, uint32_t by,
                                           uint32_t bx0, uint32_t wb, uint32_t pw, uint32_t ph) {
    constexpr uint32_t kR = 256 / N;  // blocks of the run
    const uint32_t tid = threadIdx.x;
    const uint32_t sub = tid & 7u;    // the coefficient row (A) or the block column (B) of this lane

    // ---- A: 8 / N coefficient rows per lane, dequantised into LDS; unread rows are left out
    if (idct_reads<N>(sub)) {
        uint4 q;
        __builtin_memcpy(&q, qt + sub * 16u, 16);
        const u8 *src = coefs + (by * wb + bx0) * 128u;
#pragma unroll
        for (uint32_t k = 0; k < 8u / N; ++k) {
            const uint32_t slot = tid + 256u * k, b = slot >> 3;
            if (bx0 + b < wb) {
                uint4 v;
                __builtin_memcpy(&v, src + slot * 16u, 16);  // any alignment: one global_load_dwordx4
                *reinterpret_cast<uint4 *>(blocks + b * kBlockPitch + sub * 8u) =
                    make_uint4(dequant2(v.x, q.x), dequant2(v.y, q.y), dequant2(v.z, q.z), dequant2(v.w, q.w));
            }
        }
    }
    __syncthreads();

    // ---- B: pass 1, 8 / N block columns per lane, in place: N results from the rows that are read
    if (idct_reads<N>(sub)) {
#pragma unroll
        for (uint32_t k = 0; k < 8u / N; ++k) {
            const uint32_t b = (tid + 256u * k) >> 3;
            if (bx0 + b < wb) {
                int16_t *p = blocks + b * kBlockPitch + sub;
                int d[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) d[r] = idct_reads<N>(r) ? p[8 * r] : 0;
                idctn<N, 1>(d);
#pragma unroll
                for (int r = 0; r < N; ++r) p[8 * r] = static_cast<int16_t>(clampi(d[r], -32768, 32767));
            }
        }
    }
    __syncthreads();

    // ---- C: pass 2, 4 or 8 bytes of one output row per lane: one block, two at N = 2 (then half the
    // lanes rest); kR / kPer consecutive lanes make the 256 bytes of a plane row of the run
    {
        constexpr uint32_t kPer = N == 2 ? 2u : 1u;   // blocks of a lane
        constexpr uint32_t kBytes = kPer * N;         // ... and their bytes of the row
        const uint32_t b = (tid % (kR / kPer)) * kPer, r = tid / (kR / kPer);
        const uint32_t x = (bx0 + b) * N, y = by * N + r;
        if (r < static_cast<uint32_t>(N) && bx0 + b < wb && x < pw && y < ph) {
            uint32_t o[2] = {0u, 0u};
#pragma unroll
            for (uint32_t j = 0; j < kPer; ++j) {
                if (bx0 + b + j < wb) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(blocks + (b + j) * kBlockPitch + r * 8u);
                    const uint32_t u[4] = {v.x, v.y, v.z, v.w};
                    int d[8];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        d[2 * k] = static_cast<int>(u[k] << 16) >> 16;
                        d[2 * k + 1] = static_cast<int>(u[k]) >> 16;
                    }
                    idctn<N, 2>(d);
#pragma unroll
                    for (int k = 0; k < N; ++k) o[(j * N + k) >> 2] |= sample(d[k]) << (8u * ((j * N + k) & 3u));
                }
            }
            u8 *dst = plane + y * pw + x;
            if (x + kBytes <= pw) {  // wb * N >= pw: the blocks of these samples are all there
                __builtin_memcpy(dst, o, kBytes);  // any alignment: one global_store_dwordx2 / dword
            } else {  // the end of the plane row: pw - x of the samples are real
                for (uint32_t k = 0; x + k < pw; ++k) dst[k] = static_cast<u8>(o[k >> 2] >> (8u * (k & 3u)));
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_jpegds(const JpegdsArgs a) {
    __shared__ __attribute__((aligned(16))) int16_t blocks[kMaxRun * kBlockPitch];
    const u8 *in = a.in + blockIdx.y * a.in_img;
    u8 *out = a.out + blockIdx.y * a.out_img;
    // which component and group: uniform over the workgroup
    uint32_t g = blockIdx.x, comp = 0;
    if (g >= a.groups[0]) {
        g -= a.groups[0];
        comp = 1;
        if (g >= a.groups[1]) g -= a.groups[1], comp = 2;
    }
    const uint32_t c = comp ? 1u : 0u;
    const uint32_t n = a.nidct[c], wb = a.wb[c], pw = a.pw[c], ph = a.ph;
    const u8 *coefs = in + MIPX_JPEGD_HEADER_BYTES + a.coef_off[comp];
    const u8 *qt = in + comp * 128u;
    u8 *plane = out + a.plane_off[comp];
    if (n == 1u) {  // the plane is the block grid: sample i is the DC term of block i
        const uint32_t total = wb * a.hb[c];
        const uint32_t i0 = (g * 256u + threadIdx.x) * kDcPerLane;
        if (i0 >= total) return;
        unsigned short q0;
        __builtin_memcpy(&q0, qt, 2);
        uint32_t o = 0u;
#pragma unroll
        for (uint32_t k = 0; k < static_cast<uint32_t>(kDcPerLane); ++k) {
            if (i0 + k < total) {
                unsigned short v;
                __builtin_memcpy(&v, coefs + (i0 + k) * 128u, 2);  // any alignment: one global_load_ushort
                const int d = static_cast<int16_t>(static_cast<unsigned short>(static_cast<uint32_t>(v) * q0));
                o |= sample((d + 4) >> 3) << (8u * k);
            }
        }
        if (i0 + kDcPerLane <= total) {
            __builtin_memcpy(plane + i0, &o, 4);  // any alignment: one global_store_dword
        } else {
            for (uint32_t k = 0; i0 + k < total; ++k) plane[i0 + k] = static_cast<u8>(o >> (8u * k));
        }
        return;
    }
    const uint32_t by = g / a.runs[c], bx0 = (g - by * a.runs[c]) * (256u / n);
    if (n == 8u) jpegds_run<8>(blocks, coefs, qt, plane, by, bx0, wb, pw, ph);
    else if (n == 4u) jpegds_run<4>(blocks, coefs, qt, plane, by, bx0, wb, pw, ph);
    else jpegds_run<2>(blocks, coefs, qt, plane, by, bx0, wb, pw, ph);
}

}  // namespace

// w x h is the file's size.  The caller has checked that the payload and the RGB at the output
// size are below 2^32 bytes, and that shrink is 2, 4 or 8.
int jpegds_launch(const u8 *d_in, u8 *d_planes, int n, int w, int h, int layout, int shrink, hipStream_t st) {
    const JpegGeom g(w, h, layout);
    const JpegPlanes p = g.planes(shrink);  // below full size both planes are ceil(h / shrink) high
    JpegdsArgs a;
    a.in = d_in, a.out = d_planes;
    a.in_img = static_cast<long long>(MIPX_JPEGD_HEADER_BYTES + g.coef_bytes);
    a.out_img = static_cast<long long>(p.bytes);
    a.ph = static_cast<uint32_t>(p.h[0]);
    for (int c = 0; c < 3; ++c) a.plane_off[c] = static_cast<uint32_t>(p.off[c]);
    long long total = 0;
    for (int c = 0; c < 2; ++c) {
        a.pw[c] = static_cast<uint32_t>(p.w[c]), a.nidct[c] = p.n[c];
        a.wb[c] = static_cast<uint32_t>(g.of(c).wb), a.hb[c] = static_cast<uint32_t>(g.of(c).hb);
        if (a.wb[c] == 0u) {  // grey has no chroma: no workgroup is of this class, none reads runs[1]
            a.runs[c] = a.groups[c] = 0u;
            continue;
        }
        if (a.nidct[c] == 1u) {  // linear over the block grid, which is the plane
            if (a.wb[c] != a.pw[c] || a.hb[c] != a.ph) return MIPX_EINVAL;
            const uint32_t per = 256u * kDcPerLane;
            a.runs[c] = 1u;
            a.groups[c] = static_cast<uint32_t>((static_cast<unsigned long long>(a.wb[c]) * a.hb[c] + per - 1u) / per);
        } else {
            const uint32_t run = 256u / a.nidct[c];
            a.runs[c] = (a.wb[c] + run - 1u) / run;
            a.groups[c] = a.runs[c] * a.hb[c];
        }
        total += static_cast<long long>(a.groups[c]) * (c ? 2 : 1);
    }
    if (!grid_ok(total)) return MIPX_EUNSUPPORTED;
    for (int c = 0; c < 3; ++c) a.coef_off[c] = static_cast<uint32_t>(g.coef_off[c]);
    hipLaunchKernelGGL(k_jpegds, dim3(static_cast<unsigned>(total), n), dim3(256), 0, st, a);
    return launch_check("k_jpegds");
}

}  // namespace mipx
