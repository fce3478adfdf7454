// reduce2_geom_host.cpp — k_reduce2x2's geometry (csrc/reduce2_geom.h) on the host: no HIP, no
// GPU; includes the header only.
//
// The launch of a window (reduce2_launch_geom, what the launcher in k_reduce.hip fills the
// kernel's arguments from) is checked against a table of launches worked out by hand from the
// rules: strips of 160 (RGB) / 120 (RGBA) output pixels from the strip that holds the window's x0,
// bands of 24 rows (12 when the window has at most 12) from its y0 rounded down to 12.
// reduce2_tile_interior is checked against a brute-force walk of the tile, restated from the
// kernel's body with the header's constants: 256 lanes, lane t loads dword t of the strip's
// bytes from floor4(B (2 x0 - 5)) in rows 2 y0 - 5 .. 2 (y0 + 23) + 5 (t < ND), then 240 lanes take
// an item column (4 / 2 pixels) and walk 24 rows, 6 / 4 apart, reading intermediate pixels
// 2 x - 5 .. 2 (x + K - 1) + 5 and storing K * B bytes at (y * ow + x) * B of the image's output.
//
//   (no argument)  the launch table, then enumerate shapes and windows; for every tile the
//                  predicate must equal "the walk leaves the image, the window or the store
//                  alignment nowhere".  Prints the number of tiles of each kind and "ok"; exits 1
//                  at the first difference.
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

// the header's launch of a window, with the image it belongs to
struct Launch : Reduce2Launch {
    int w, h, b, tw;
};

bool launch_of(int w, int h, int b, int x0, int y0, int x1, int y1, Launch *l) {
    l->w = w, l->h = h, l->b = b, l->tw = reduce2_strip_width(b);
    return reduce2_launch_geom(w, h, b, x0, y0, x1, y1, l);
}

// Launches worked out by hand from the rules at the top; the output is (w + 1) / 2 x (h + 1) / 2.
// Window {-1, ..}: the full image.
struct Expect {
    int w, h, b, x0, y0, x1, y1;
    int s_base, y_base, n_strips, n_bands, band_rows;
};
constexpr Expect kLaunches[] = {
    {3840, 2160, 3, -1, 0, 0, 0, /**/ 0, 0, 12, 45, 24},  // C2: 1920 / 160 strips, 1080 / 24 bands
    {3840, 2160, 4, -1, 0, 0, 0, /**/ 0, 0, 16, 45, 24},  // 1920 / 120
    {644, 98, 3, 0, 12, 322, 30, /**/ 0, 12, 3, 1, 24},   // 18 rows from a multiple of 12: one band of 2 chunks
    {644, 98, 3, 150, 0, 170, 49, /**/ 0, 0, 2, 3, 24},   // columns 150 .. 169 lie in strips 0 and 1 of 160
    {644, 98, 4, 150, 0, 170, 49, /**/ 1, 0, 1, 3, 24},   // and in strip 1 of 120 alone
    {40, 24, 3, -1, 0, 0, 0, /**/ 0, 0, 1, 1, 12},        // 12 output rows: one chunk
    {40, 26, 3, -1, 0, 0, 0, /**/ 0, 0, 1, 1, 24},        // 13 rows: two chunks
    {8, 8, 4, -1, 0, 0, 0, /**/ 0, 0, 1, 1, 12},
};

bool check_table() {
    for (const Expect &e : kLaunches) {
        const int ow = (e.w + 1) / 2, oh = (e.h + 1) / 2;
        const bool full = e.x0 < 0;
        const int x0 = full ? 0 : e.x0, y0 = full ? 0 : e.y0, x1 = full ? ow : e.x1, y1 = full ? oh : e.y1;
        Reduce2Launch l;
        const bool ok = reduce2_launch_geom(e.w, e.h, e.b, x0, y0, x1, y1, &l);
        if (!ok || l.ow != ow || l.oh != oh || l.s_base != e.s_base || l.y_base != e.y_base || l.x_end != x1 ||
            l.y_end != y1 || l.n_strips != e.n_strips || l.n_bands != e.n_bands || l.band_rows != e.band_rows ||
            l.tiles_per_image() != static_cast<long long>(e.n_strips) * e.n_bands) {
            std::printf("launch %d x %d x %d window %d %d %d %d: ok %d, out %d x %d, s_base %d y_base %d x_end %d "
                        "y_end %d, %d strips x %d bands of %d rows\n",
                        e.w, e.h, e.b, x0, y0, x1, y1, ok, l.ow, l.oh, l.s_base, l.y_base, l.x_end, l.y_end,
                        l.n_strips, l.n_bands, l.band_rows);
            return false;
        }
    }
    // 644 x 98 gives 322 x 49: empty windows, windows past the output, negative origins
    const int bad[][4] = {{10, 0, 10, 49}, {11, 0, 10, 49}, {0, 20, 322, 20}, {0, 21, 322, 20}, {0, 0, 323, 49},
                          {0, 0, 322, 50}, {-1, 0, 322, 49}, {0, -1, 322, 49}, {-160, -12, 322, 49}};
    for (const auto &win : bad) {
        Reduce2Launch l;
        if (reduce2_launch_geom(644, 98, 3, win[0], win[1], win[2], win[3], &l)) {
            std::printf("window %d %d %d %d of 322 x 49 was not rejected\n", win[0], win[1], win[2], win[3]);
            return false;
        }
    }
    return true;
}

// would straight-line code with no edge handling stay inside the image, the window and the store alignment on
// this tile?  misalign: low bits of the address of image 0's output; 3 images are walked
template <int B>
bool walk_is_plain_b(const Launch &l, int x0, int y0, uint32_t misalign) {
    using G = Reduce2Geom<B>;
    if (l.band_rows != kReduce2TileRows) return false;  // it walks 24 rows
    constexpr int K = G::K, ipr = G::IPR, rpi = G::RPI, nd = G::ND;
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

bool walk_is_plain(const Launch &l, int x0, int y0, uint32_t misalign) {
    return l.b == 3 ? walk_is_plain_b<3>(l, x0, y0, misalign) : walk_is_plain_b<4>(l, x0, y0, misalign);
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
    if (!launch_of(w, h, b, 0, 0, (w + 1) / 2, (h + 1) / 2, &l)) return -1;
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
    if (!check_table()) return 1;
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
                    if (!launch_of(w, h, b, win[0], win[1], win[2], win[3], &l)) continue;
                    if (!check_launch(l)) return 1;
                    ++launches;
                }
            }
        }
    std::printf("launches %lld interior %lld other %lld\n", launches, n_interior, n_other);
    std::printf("ok\n");
    return 0;
}
