// reduce2_geom.h — the tile geometry of k_reduce2x2 (k_reduce.hip), in one place: the constants
// of a tile, the launch of an output window, and which tiles touch no edge.
// A tile is a strip of TW output pixels from x0 and a band of `band_rows` output rows from
// y0 (a multiple of 12) of the computed region [.., x_end) x [.., y_end) of an ow-wide
// output; it reads input rows 2 y0 - 5 .. 2 (y0 + rows - 1) + 5 (clamped to the image) and
// intermediate pixels 2 x0 - 5 .. 2 (x0 + TW - 1) + 5 (replicated past the image), and
// stores items of 4 (RGB) / 2 (RGBA) output pixels.  No HIP: a host test compiles it, the kernel
// takes its constants and the launcher its arguments from it.  The kernel does not branch on the
// predicate: a straight-line body for interior tiles measured no faster than the general one
// (profiles/r18); the predicate and its tests pin the geometry that body, and the counts in the
// kernel's records (C2: 10 x 43 of 12 x 45 tiles), rely on.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define MIPX_R2_HD __host__ __device__
#else
#define MIPX_R2_HD
#endif

namespace mipx {

constexpr int kReduce2Threads = 256;    // lanes of a workgroup
constexpr int kReduce2Pitch = 288;      // LDS dwords per intermediate row
constexpr int kReduce2ChunkRows = 12;   // output rows per load round: 2 periods of the odd-row ring
constexpr int kReduce2TileRows = 24;    // the one-pass tile: two chunks of 12 output rows

template <int B>
struct Reduce2Geom {
    static_assert(B == 3 || B == 4, "RGB or RGBA");
    static constexpr int TW = B == 3 ? 160 : 120;        // output pixels per strip
    static constexpr int K = B == 3 ? 4 : 2;             // output pixels per horizontal item
    static constexpr int NPX = 2 * TW + 9;               // intermediate px 2x0-5 .. 2x0+2TW+3
    static constexpr int OFF0 = B == 3 ? 1 : 0;          // B*(2x0-5) - floor4(B*(2x0-5))
    static constexpr int ND = (B * NPX + OFF0 + 3) / 4;  // dwords per row
    static constexpr int IPR = TW / K;                   // items per row: 40 / 60
    static constexpr int RPI = kReduce2Threads / IPR;    // rows a walk step advances: 6 / 4
    static constexpr int W0 = (B * 2 * K) / 4;           // dwords between the windows of two items
    static_assert(ND <= kReduce2Threads && ND <= kReduce2Pitch, "strip too wide");
    static_assert(IPR * K == TW, "items must tile the strip");
    static_assert((B * 2 * K) % 8 == 0, "window start must be 8-byte aligned");
    static_assert(W0 * (IPR - 1) + 14 <= kReduce2Pitch, "the walk's last read stays inside the row");
    static_assert(B == 3 || (RPI * B) % 8 == 0, "RGBA: a walk step keeps the store alignment");
};

constexpr int reduce2_strip_width(int b) { return b == 3 ? Reduce2Geom<3>::TW : Reduce2Geom<4>::TW; }

// The launch of the output window [x0, x1) x [y0, y1): strips from s_base, bands of band_rows
// rows from row y_base, clipped at x_end / y_end; n_strips * n_bands tiles per image.
struct Reduce2Launch {
    int ow, oh;
    int s_base, y_base, x_end, y_end;
    int n_strips, n_bands, band_rows;
    long long tiles_per_image() const { return static_cast<long long>(n_strips) * n_bands; }
};

// The window is rounded out to whole strips on the left and to a multiple of 12 rows at the top;
// a tile is two chunks of 12 rows, one when the window has no more.  False for a window that is
// empty or leaves the (w + 1) / 2 x (h + 1) / 2 output.
inline bool reduce2_launch_geom(int w, int h, int b, int x0, int y0, int x1, int y1, Reduce2Launch *l) {
    constexpr int R = kReduce2ChunkRows;
    l->ow = (w + 1) / 2;  // VIPS_ROUND(in / 2)
    l->oh = (h + 1) / 2;
    if (x0 < 0 || y0 < 0 || x1 > l->ow || y1 > l->oh || x0 >= x1 || y0 >= y1) return false;
    const int tw = reduce2_strip_width(b);
    l->s_base = x0 / tw;
    l->x_end = x1;
    l->y_base = y0 / R * R;
    l->y_end = y1;
    l->n_strips = (x1 + tw - 1) / tw - l->s_base;
    const int chunks = (y1 - l->y_base + R - 1) / R;
    l->band_rows = (chunks < 2 ? chunks : 2) * R;
    l->n_bands = (y1 - l->y_base + l->band_rows - 1) / l->band_rows;
    return true;
}

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
