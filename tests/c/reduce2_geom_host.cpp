// reduce2_geom_host.cpp — reduce2_tile_interior (csrc/reduce2_geom.h) against a brute-force walk
// of the tile, on the host: no HIP, no GPU; includes the header only.
//
// The launch geometry is restated from reduce2_window_launch (k_reduce.hip): strips of 160 (RGB) /
// 120 (RGBA) output pixels from the strip that holds the window's x0, bands of 24 rows (12 when the
// window has at most 12) from its y0 rounded down to 12.  The walk is restated from the one-pass
// body: 256 lanes, lane t loads dword t of the strip's bytes from floor4(B (2 x0 - 5)) in rows
// 2 y0 - 5 .. 2 (y0 + 23) + 5 (t < ND), then 240 lanes take an item column (4 / 2 pixels) and walk
// 24 rows, 6 / 4 apart, reading intermediate pixels 2 x - 5 .. 2 (x + K - 1) + 5 and storing
// K * B bytes at (y * ow + x) * B of the image's output.
//
//   (no argument)  enumerate shapes and windows; for every tile the predicate must equal "the walk
//                  leaves the image, the window or the store alignment nowhere".  Prints the number
//                  of tiles of each kind and "ok"; exits 1 at the first difference.
//   count W H B    the interior tiles per image of the full W x H x B launch
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <set>
#include <string_view>

#include "reduce2_geom.h"

using namespace mipx;

namespace {

struct Launch {
    int w, h, b, ow, oh, tw, s_base, y_base, x_end, y_end, n_strips, n_bands, band_rows;
};

bool make_launch(int w, int h, int b, int x0, int y0, int x1, int y1, Launch *l) {
    l->w = w, l->h = h, l->b = b;
    l->ow = (w + 1) / 2, l->oh = (h + 1) / 2;  // VIPS_ROUND(in / 2)
    if (x0 < 0 || y0 < 0 || x1 > l->ow || y1 > l->oh || x0 >= x1 || y0 >= y1) return false;
    l->tw = b == 3 ? 160 : 120;
    l->s_base = x0 / l->tw;
    l->x_end = x1;
    l->y_base = y0 / 12 * 12;
    l->y_end = y1;
    l->n_strips = (x1 + l->tw - 1) / l->tw - l->s_base;
    const int chunks = (y1 - l->y_base + 11) / 12;
    l->band_rows = (chunks < 2 ? chunks : 2) * 12;
    l->n_bands = (y1 - l->y_base + l->band_rows - 1) / l->band_rows;
    return true;
}

// would straight-line code with no edge handling stay inside the image, the window and the store alignment on
// this tile?  misalign: low bits of the address of image 0's output; 3 images are walked
bool walk_is_plain(const Launch &l, int x0, int y0, uint32_t misalign) {
    if (l.band_rows != 24) return false;  // it walks 24 rows
    const int B = l.b, K = B == 3 ? 4 : 2, ipr = l.tw / K, rpi = 256 / ipr;
    const int npx = 2 * l.tw + 9, off0 = B == 3 ? 1 : 0, nd = (B * npx + off0 + 3) / 4;
    const uint32_t al = B == 3 ? 4 : 8;
    const long long row_bytes = static_cast<long long>(l.w) * B;
    // loads: rows of the burst and of the 24-row pass, lanes t < nd
    for (int k = 0; k < 5; ++k) {
        const int r = 2 * (y0 - 3 + k) + 1;
        if (r < 0 || r > l.h - 1) return false;
    }
    for (int u = 0; u < 24; ++u)
        for (int r : {2 * (y0 + u + 2) + 1, 2 * (y0 + u)})
            if (r < 0 || r > l.h - 1) return false;
    const int px0 = 2 * x0 - 5;
    const int base = (B * px0) & ~3;
    for (int t = 0; t < nd; ++t) {
        const long long byte0 = static_cast<long long>(base) + 4 * t;
        if (byte0 < 0 || byte0 + 4 > row_bytes) return false;
    }
    // the walk
    const long long out_img = static_cast<long long>(l.ow) * l.oh * B;
    for (int t = 0; t < ipr * rpi; ++t) {
        const int u0 = t / ipr, j = t % ipr;
        const int x = x0 + K * j;
        for (int p = 2 * x - 5; p <= 2 * (x + K - 1) + 5; ++p)
            if (p < 0 || p > l.w - 1) return false;
        if (x + K > l.x_end || x + K > l.ow) return false;  // no item past x_end
        for (int u = u0; u < 24; u += rpi) {
            const int y = y0 + u;
            if (y >= l.y_end || y >= l.oh) return false;
            for (int img = 0; img < 3; ++img) {
                const long long at = misalign + img * out_img + (static_cast<long long>(y) * l.ow + x) * B;
                if (at % al != 0) return false;
            }
        }
    }
    return true;
}

long long n_interior, n_other;

bool check_launch(const Launch &l) {
    const long long out_img = static_cast<long long>(l.ow) * l.oh * l.b;
    for (uint32_t base_mis : {0u, 4u, 2u}) {
        // what the launcher passes: the low bits of out | out_img
        const uint32_t mis = static_cast<uint32_t>((base_mis | static_cast<uint64_t>(out_img)) & 7u);
        for (int band = 0; band < l.n_bands; ++band)
            for (int strip = 0; strip < l.n_strips; ++strip) {
                const int x0 = (l.s_base + strip) * l.tw, y0 = l.y_base + band * l.band_rows;
                const bool said = reduce2_tile_interior(l.w, l.h, l.ow, l.b, x0, y0, l.tw, l.band_rows, l.x_end,
                                                        l.y_end, mis);
                const bool plain = walk_is_plain(l, x0, y0, base_mis);
                if (said != plain) {
                    std::printf("w %d h %d b %d window .. %d .. %d from strip %d row %d, tile x0 %d y0 %d, "
                                "misalign %u: predicate %d, walk %d\n",
                                l.w, l.h, l.b, l.x_end, l.y_end, l.s_base, l.y_base, x0, y0, base_mis, said, plain);
                    return false;
                }
                (said ? n_interior : n_other) += 1;
            }
    }
    return true;
}

int count_full(int w, int h, int b) {
    Launch l;
    if (!make_launch(w, h, b, 0, 0, (w + 1) / 2, (h + 1) / 2, &l)) return -1;
    int n = 0;
    for (int band = 0; band < l.n_bands; ++band)
        for (int strip = 0; strip < l.n_strips; ++strip)
            n += reduce2_tile_interior(w, h, l.ow, b, (l.s_base + strip) * l.tw, l.y_base + band * l.band_rows, l.tw,
                                       l.band_rows, l.x_end, l.y_end, 0u);
    return n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && std::string_view(argv[1]) == "count") {
        std::printf("%d\n", count_full(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4])));
        return 0;
    }
    // w 8 .. 1400 by 11 and h 8 .. 220 by 7 (every residue mod 8), and every size around those at
    // which a tile turns interior: the right edge of strips 1, 2, ... and the last row of bands 1, 2, ...
    std::set<int> ws, hs;
    for (int w = 8; w <= 1400; w += 11) ws.insert(w);
    for (int c : {484, 644, 724, 964, 1204, 1284})
        for (int d = -6; d <= 6; ++d) ws.insert(c + d);
    for (int h = 8; h <= 220; h += 7) hs.insert(h);
    for (int c : {100, 148, 196})
        for (int d = -4; d <= 4; ++d) hs.insert(c + d);
    long long launches = 0;
    for (int b : {3, 4})
        for (int w : ws) {
            if ((w * b) % 4 != 0) continue;  // reduce2_eligible: dword-aligned rows only
            for (int h : hs) {
                const int ow = (w + 1) / 2, oh = (h + 1) / 2, tw = b == 3 ? 160 : 120;
                const int windows[][4] = {{0, 0, ow, oh},                  // the full image
                                          {0, 12, ow, oh},                 // bands off the 24-row grid
                                          {0, 0, ow - 37, oh},             // ends inside a strip
                                          {tw + 3, 24, ow - 1, oh - 5},    // starts and ends inside strips
                                          {tw, 24, ow, 47},                // one row short of a band
                                          {5, 36, ow - tw / 2, oh - 13}};
                for (const auto &win : windows) {
                    Launch l;
                    if (!make_launch(w, h, b, win[0], win[1], win[2], win[3], &l)) continue;
                    if (!check_launch(l)) return 1;
                    ++launches;
                }
            }
        }
    std::printf("launches %lld interior %lld other %lld\n", launches, n_interior, n_other);
    std::printf("ok\n");
    return 0;
}
