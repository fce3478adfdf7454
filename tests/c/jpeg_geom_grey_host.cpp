// jpeg_geom_grey_host.cpp — prints the JPEG geometry of the one-component layout (MIPX_YCC_GREY) on
// the host: no HIP call, no GPU; csrc/jpeg_geom.h alone.  One line per (w, h): hs, vs and the fields
// of JpegGeom in the order tests/c/jpeg_geom_host.cpp prints them, then planes(s) for s = 1, 2, 4, 8;
// the predicates; and jpeg_max beside the grey layout's own capacity and block count.
// tests/test_jpeggrey_cpu.py compares them with the one-component sampling rule.
#include <cstdint>
#include <cstdio>
#include <initializer_list>
#include <utility>

#include "jpeg_geom.h"

using namespace mipx;

namespace {

void geom_line(int w, int h) {
    const JpegGeom g(w, h, MIPX_YCC_GREY);
    std::printf("geom %d %d :", w, h);
    for (uint64_t v : {g.hs, g.vs, g.y.w, g.y.h, g.y.wb, g.y.hb, g.c.w, g.c.h, g.c.wb, g.c.hb, g.coef_off[0], g.coef_off[1],
                       g.coef_off[2], g.plane_off[0], g.plane_off[1], g.plane_off[2], g.coef_bytes, g.plane_bytes,
                       g.mw, g.mh, g.per_mcu, g.blocks})
        std::printf(" %llu", static_cast<unsigned long long>(v));
    for (int s : {1, 2, 4, 8}) {
        const JpegPlanes p = g.planes(s);
        std::printf(" |");
        for (uint64_t v : {static_cast<uint64_t>(p.n[0]), static_cast<uint64_t>(p.n[1]), p.w[0], p.h[0], p.w[1], p.h[1],
                           p.off[0], p.off[1], p.off[2], p.bytes})
            std::printf(" %llu", static_cast<unsigned long long>(v));
    }
    std::printf("\n");
}

}  // namespace

int main() {
    for (int w = 1; w <= 40; ++w)
        for (int h = 1; h <= 40; ++h) geom_line(w, h);
    for (const auto &s : {std::pair<int, int>{197, 117}, {1027, 13}, {3840, 2160}, {65535, 65535}})
        geom_line(s.first, s.second);
    // sizes that are not positive leave every field 0
    for (const auto &s : {std::pair<int, int>{0, 8}, {8, -1}}) geom_line(s.first, s.second);
    for (int layout : {-1, 0, 1, 2, 3, 4, 5, 6, 7, 1 << 20})
        std::printf("layout %d : %d %d %d %d %d\n", layout, ycc_input_layout(layout) ? 1 : 0,
                    ycc_output_layout(layout) ? 1 : 0, jpeg_input_layout(layout) ? 1 : 0,
                    jpeg_output_layout(layout) ? 1 : 0, jpeg_layout_bands(layout));
    // grey never passes what the workspaces are sized by
    for (int w = 1; w <= 40; ++w)
        for (int h = 1; h <= 40; ++h) {
            const JpegGeom g(w, h, MIPX_YCC_GREY);
            const JpegMax o = jpeg_max(w, h, false), i = jpeg_max(w, h, true);
            std::printf("max %d %d : %llu %llu | %llu %llu | %llu %llu\n", w, h, static_cast<unsigned long long>(g.coef_bytes),
                        static_cast<unsigned long long>(g.blocks), static_cast<unsigned long long>(o.cap),
                        static_cast<unsigned long long>(o.blocks), static_cast<unsigned long long>(i.cap),
                        static_cast<unsigned long long>(i.blocks));
        }
    return 0;
}
