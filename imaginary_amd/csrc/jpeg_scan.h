// jpeg_scan.h — the device functions the entropy coder and decoder share (k_jpege.hip,
// k_jpegh.hip): the zigzag order of a block's coefficients, the workgroup prefix sum both are
// built on, and the order of an interleaved scan's blocks (scan_block: the decoder's; the coder
// keeps its own copy in block_src, see there).  One copy of each.
#pragma once

#include <hip/hip_runtime.h>

#include "device_common.h"

namespace mipx {
namespace jscan {

// zigzag index -> natural index of a coefficient
static __constant__ uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                                           12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                                           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                                           58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// Exclusive prefix of v over a workgroup of 256 lanes; *total = the sum.  wsum: 4 words of LDS.
template <class T>
__device__ __forceinline__ T block_scan(T v, T *wsum, T *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    T inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T t = __shfl_up(inc, d);
        if (lane >= static_cast<uint32_t>(d)) inc += t;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    T base = 0, tot = 0;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const T s = wsum[i];
        base += i < wave ? s : T(0);
        tot += s;
    }
    __syncthreads();  // wsum is free again
    *total = tot;
    return base + inc - v;
}

// blocks of an MCU: Y Cb Cr; Y00 Y01 Y10 Y11 Cb Cr; 4:2:2's Y0 Y1 Cb Cr; grey's one block (the scan of
// one component is not interleaved)
template <int LAYOUT>
constexpr uint32_t per_mcu() {
    return LAYOUT == MIPX_YCC_GREY ? 1u : LAYOUT == MIPX_YCC_444 ? 3u : LAYOUT == MIPX_YCC_422 ? 4u : 6u;
}

// Block s of the scan.  A component whose block grid is the MCU grid (chroma, and 4:4:4's Y) has
// block m of that grid, in raster order, in MCU m.  The Y of a subsampled layout is `placed`: at
// column bx and row by of the Y grid, and a dummy block where that is outside the real blocks.
struct ScanBlock {
    uint32_t comp;    // 0: Y, 1: Cb, 2: Cr
    uint32_t m, j;    // its MCU (mw of them across), and which of the MCU's blocks it is
    bool placed;
    uint32_t bx, by;  // only when placed
};
template <int LAYOUT>
__device__ __forceinline__ ScanBlock scan_block(uint32_t s, uint32_t mw) {
    if (LAYOUT == MIPX_YCC_GREY) {  // block s of Y's grid: its own MCU, never placed, never a dummy
        ScanBlock g;
        g.comp = 0u, g.m = s, g.j = 0u, g.placed = false, g.bx = g.by = 0u;
        return g;
    }
    constexpr uint32_t kPer = per_mcu<LAYOUT>(), kY = kPer - 2u;  // Y blocks of an MCU: 1, 2 across, 2 x 2
    ScanBlock b;
    b.m = s / kPer, b.j = s - kPer * b.m;
    b.comp = b.j < kY ? 0u : b.j - (kY - 1u);
    b.placed = LAYOUT != MIPX_YCC_444 && b.j < kY;
    b.bx = b.by = 0u;
    if (b.placed) {
        const uint32_t my = b.m / mw, mx = b.m - my * mw;
        b.bx = 2u * mx + (b.j & 1u);
        b.by = LAYOUT == MIPX_YCC_420 ? 2u * my + (b.j >> 1) : my;
    }
    return b;
}

}  // namespace jscan
}  // namespace mipx
