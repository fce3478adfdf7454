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
//
// MIPX_YCC_GREY (PARITY_ASSUMPTIONS.md row 26): 1-band pixels in, Y's coefficients alone out: sample
// - 128, the same edge rule, the luminance reciprocals.  Its strip is 384 x 8 pixels, the 48 blocks
// of ONE block row, not three block rows of 128: a strip's pixel rows are then 384 contiguous bytes
// (a wave and a half of 4-byte loads each) where three rows of 128 would be 24 pieces of 128, and
// its 48 blocks are 6 KiB of contiguous output, so phases B to D run unchanged with all 384 tasks
// busy wherever the image is 48 blocks across; only the last strip of a block row idles lanes.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "jpeg_dct.h"

namespace mipx {
namespace {

using namespace dev;
using namespace jfdct;

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

constexpr uint32_t kNoBlock = 0xffffffffu;

// Where block `blk` of strip (sx, sy) goes in the image's output, in bytes; kNoBlock for a block
// outside the real ones (the entropy coder's dummy blocks).  *chroma: which table quantises it.
// Its own copy of the strip's block map, which jpeg_dct.h's strip_block states for k_jpegrt.hip: built
// on that one the 4:2:0 kernel measured 0.6 % slower in four rounds of five (profiles/r16).
template <int LAYOUT>
__device__ __forceinline__ uint32_t block_offset(const JpegcArgs &a, uint32_t sx, uint32_t sy, uint32_t blk,
                                                 uint32_t *chroma) {
    if (LAYOUT == MIPX_YCC_GREY) {  // 48 blocks of block row sy
        const uint32_t bx = sx * 48u + blk;
        *chroma = 0u;
        if (bx >= a.ywb) return kNoBlock;
        return (sy * a.ywb + bx) * 128u;
    }
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
    strip_samples<LAYOUT>(blocks, in, a.w, a.h, a.ywb, a.cwb, a.ch, sx, sy);
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
        fdct8_row(blk[i], line[i]);
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
    const JpegGeom g(w, h, layout);
    const bool grey = layout == MIPX_YCC_GREY;
    const long long in_img = static_cast<long long>(w) * h * jpeg_layout_bands(layout);
    const long long out_img = static_cast<long long>(g.coef_bytes);
    if (in_img > 0xffffffffLL || out_img > 0xffffffffLL) {  // byte offsets inside an image are 32-bit
        set_error("rgb to jpeg coefficients: image %dx%d too large (an image's bytes >= 2^32)", w, h);
        return MIPX_EUNSUPPORTED;
    }
    JpegcArgs a;
    a.in = d_in, a.out = d_out;
    a.recips = device_jpegc_recips(quality);
    if (!a.recips) {
        set_error("rgb to jpeg coefficients: no reciprocal table for quality %d", quality);
        return MIPX_EDEVICE;
    }
    a.in_img = in_img, a.out_img = out_img;
    a.w = w, a.h = h;
    a.ywb = static_cast<uint32_t>(g.y.wb), a.yhb = static_cast<uint32_t>(g.y.hb);
    a.cwb = static_cast<uint32_t>(g.c.wb), a.ch = static_cast<uint32_t>(g.c.h);
    a.cb_off = static_cast<uint32_t>(g.coef_off[1]), a.cr_off = static_cast<uint32_t>(g.coef_off[2]);
    // a strip is a row of MCUs, 128 pixels of it; grey's is 384 pixels of a block row
    const long long gx = (static_cast<long long>(w) + (grey ? 383 : 127)) / (grey ? 384 : 128), gy = static_cast<long long>(g.mh);
    if (!grid_ok(gx * gy)) return MIPX_EUNSUPPORTED;
    a.gx = static_cast<uint32_t>(gx);
    const dim3 grid(static_cast<unsigned>(gx * gy), n);
    with_output_layout(layout,
                       [&](auto L) { hipLaunchKernelGGL(k_jpegc<L.value>, grid, dim3(256), 0, st, a); });
    return launch_check("k_jpegc");
}

}  // namespace mipx
