// reduce2_geom.h — which tiles of k_reduce2x2's one-pass body (k_reduce.hip) touch no edge.
// A tile is a strip of `tw` output pixels from x0 and a band of `band_rows` output rows from
// y0 (a multiple of 12) of the computed region [.., x_end) x [.., y_end) of an ow-wide
// output; it reads input rows 2 y0 - 5 .. 2 (y0 + rows - 1) + 5 (clamped to the image) and
// intermediate pixels 2 x0 - 5 .. 2 (x0 + tw - 1) + 5 (replicated past the image), and
// stores items of 4 (RGB) / 2 (RGBA) output pixels.  No HIP: a host test compiles it, a kernel
// may.  The kernel does not branch on it today: a straight-line body for these tiles measured
// no faster than the general one (profiles/r18); the predicate and its tests pin the geometry
// that body, and the counts in the kernel's records (C2: 10 x 43 of 12 x 45 tiles), rely on.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MIPX_R2_HD __host__ __device__
#else
#define MIPX_R2_HD
#endif

namespace mipx {

constexpr int kReduce2TileRows = 24;  // the one-pass tile: two chunks of 12 output rows

// the stores of a walk are whole items at their natural alignment: 12 bytes on a dword (RGB),
// 8 bytes on 8 (RGBA)
MIPX_R2_HD inline uint32_t reduce2_store_align(int b) { return b == 3 ? 4u : 8u; }

// True when the tile clamps no row, replicates no pixel, clips no item and stores only
// aligned whole items, so that straight-line code without any edge handling computes it:
//  * the band has all 24 rows inside the computed region: band_rows == 24, y0 + 24 <= y_end;
//  * every input row 2 y0 - 5 .. 2 (y0 + 23) + 5 lies in [0, h - 1];
//  * every intermediate pixel 2 x0 - 5 .. 2 (x0 + tw - 1) + 5 lies in [0, w - 1];
//  * the strip ends inside the computed region and that inside the row: x0 + tw <= x_end <= ow;
//  * the output row pitch ow * b and out_misalign, the low bits of the address of the
//    image's first output byte, are multiples of the store alignment (x0 * b and an item's
//    bytes always are: strips are 160 / 120 pixels, items 12 / 8 bytes).
MIPX_R2_HD inline bool reduce2_tile_interior(int w, int h, int ow, int b, int x0, int y0, int tw, int band_rows,
                                             int x_end, int y_end, uint32_t out_misalign) {
    const bool rows = band_rows == kReduce2TileRows && y0 + kReduce2TileRows <= y_end && 2 * y0 - 5 >= 0 &&
                      2 * (y0 + kReduce2TileRows - 1) + 5 <= h - 1;
    const bool cols = 2 * x0 - 5 >= 0 && 2 * (x0 + tw - 1) + 5 <= w - 1 && x0 + tw <= x_end && x_end <= ow;
    const uint32_t al = reduce2_store_align(b);
    const bool stores = static_cast<uint32_t>(ow * b) % al == 0 && out_misalign % al == 0;
    return rows && cols && stores;
}

}  // namespace mipx
