// jpeg_geom_host.cpp — pins the JPEG geometry of libmipx on the host: no HIP call, no GPU; links
// mipx_planner.cpp only.  Two parts:
//   pin   every size the engine reports for (w, h, layout): the six mipx_*_bytes functions,
//         jpeg_opt_in_range and every field of JpegeWork and JpeghWork, as FNV-1a-64 hashes, one line
//         per (layout, w) over h = 1..40 and one line per large size.  Written against the names the
//         engine had before csrc/jpeg_geom.h existed; tests/golden/jpeg_geom_host.txt is this part as
//         the commit before that header printed it.
//   geom  the fields of the JpegGeom struct itself, in plain numbers, for tests/test_jpeg_geom_host.py
//         to compare with libjpeg's sampling-factor rule.  Only where the header exists.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <utility>

#include "mipx_internal.h"
#if __has_include("jpeg_geom.h")
#include "jpeg_geom.h"
#define HAVE_GEOM 1
#endif

namespace mipx {
// what mipx_planner.cpp needs from the rest of the engine
void set_error(const char *, ...) {}
int reduce_sampling_now() { return 0; }
bool jpeg_qtables(int, uint8_t *, uint8_t *) { return false; }
}  // namespace mipx

using namespace mipx;

namespace {

struct Fnv {
    uint64_t h = 0xcbf29ce484222325ULL;
    void add(uint64_t v) {
        for (int i = 0; i < 8; ++i) h = (h ^ ((v >> (8 * i)) & 255u)) * 0x100000001b3ULL;
    }
};

const int kLayouts[] = {MIPX_YCC_444, MIPX_YCC_420, MIPX_YCC_422};

void add_bytes(Fnv &f, int w, int h, int layout) {
    f.add(mipx_ycc_bytes(w, h, layout));
    f.add(mipx_jpegc_bytes(w, h, layout));
    f.add(mipx_jpegd_bytes(w, h, layout));
    f.add(mipx_jpegh_bytes(w, h, layout));
    f.add(mipx_jpeg_scan_bytes(w, h, layout));
    f.add(mipx_jpeg_scan_opt_bytes(w, h, layout));
}

void add_work(Fnv &f, int n, int w, int h) {
    for (int optimise = 0; optimise < 2; ++optimise) {
        const JpegeWork e(n, w, h, optimise != 0);
        for (size_t v : {e.cap, e.blocks, e.tiles, e.chunks, e.coefs, e.info, e.stream, e.counts, e.tile_sums,
                         e.tile_offs, e.chunk_sums, e.chunk_offs, e.hist, e.opt_codes, e.total})
            f.add(v);
    }
    const JpeghWork d(n, w, h);
    for (size_t v : {d.cap, d.blocks, d.tiles, d.chunks, d.seqs, d.sstride, d.status, d.info, d.stream, d.chunk_sums,
                     d.chunk_offs, d.entries, d.counts, d.seq_exit, d.seq_sums, d.seq_offs, d.dcdiff, d.dc_sums,
                     d.dc_offs, d.payload, d.planes, d.total})
        f.add(v);
}

// everything the engine reports of a valid (w, h, layout)
void add_all(Fnv &f, int w, int h, int layout) {
    add_bytes(f, w, h, layout);
    f.add(jpeg_opt_in_range(w, h, layout));
    for (int n : {1, 3}) add_work(f, n, w, h);
}

void pin() {
    for (int layout : kLayouts)
        for (int w = 1; w <= 40; ++w) {
            Fnv f;
            for (int h = 1; h <= 40; ++h) add_all(f, w, h, layout);
            std::printf("pin layout %d w %d : %016llx\n", layout, w, static_cast<unsigned long long>(f.h));
        }
    // bad arguments: the layouts that are none, and sizes that are not positive
    for (int layout : {-1, 2, 4, 5, 1 << 20}) {
        Fnv f;
        for (int w = 1; w <= 40; ++w)
            for (int h = 1; h <= 40; ++h) add_bytes(f, w, h, layout);
        std::printf("pin layout %d : %016llx\n", layout, static_cast<unsigned long long>(f.h));
    }
    for (int layout : kLayouts) {
        Fnv f;
        const int bad[] = {0, -1, -8, INT32_MIN};
        for (int b : bad)
            for (int g : {1, 8, 40, 0, -1}) add_bytes(f, b, g, layout), add_bytes(f, g, b, layout);
        std::printf("pin layout %d sizes <= 0 : %016llx\n", layout, static_cast<unsigned long long>(f.h));
    }
    // the large sizes, then for one width per limit the last height below it and the first at it, in the
    // order 4:4:4, 4:2:2, 4:2:0: the coefficients reach 2^29 bytes (w = 9464), the payload passes 2^32 - 1
    // bytes (w = 26760), 64 x the scan's blocks reach 10^9 (w = 18264 and 25824: 4:4:4, which 4:2:2 counts as,
    // then 4:2:0), and 3 w h passes 2^32 - 1 (w = 37838)
    const int big[][2] = {{197, 117},     {1027, 13},     {3840, 2160},   {4000, 3000},   {23171, 23171}, {65535, 65535},
                          {9464, 9448},   {9464, 9449},   {9464, 14168},  {9464, 14169},  {9464, 18896},  {9464, 18897},
                          {26760, 26744}, {26760, 26745}, {26760, 40112}, {26760, 40113}, {26760, 53488}, {26760, 53489},
                          {18264, 18248}, {18264, 18249}, {18264, 36480}, {18264, 36481}, {25824, 12904}, {25824, 12905},
                          {25824, 25808}, {25824, 25809}, {37838, 37836}, {37838, 37837}, {1, 65535},     {65535, 1}};
    for (const auto &s : big)
        for (int layout : kLayouts) {
            Fnv f;
            add_all(f, s[0], s[1], layout);
            std::printf("pin layout %d %dx%d : %016llx jpegc %zu opt %d\n", layout, s[0], s[1],
                        static_cast<unsigned long long>(f.h), mipx_jpegc_bytes(s[0], s[1], layout),
                        jpeg_opt_in_range(s[0], s[1], layout) ? 1 : 0);
        }
}

#ifdef HAVE_GEOM
void geom_line(int w, int h, int layout) {
    const JpegGeom g(w, h, layout);
    std::printf("geom %d %d %d :", layout, w, h);
    for (uint64_t v : {g.y.w, g.y.h, g.y.wb, g.y.hb, g.c.w, g.c.h, g.c.wb, g.c.hb, g.coef_off[0], g.coef_off[1],
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

void geom() {
    for (int layout : kLayouts)
        for (int w = 1; w <= 40; ++w)
            for (int h = 1; h <= 40; ++h) geom_line(w, h, layout);
    for (int layout : kLayouts)
        for (const auto &s : {std::pair<int, int>{197, 117}, {1027, 13}, {3840, 2160}, {65535, 65535}})
            geom_line(s.first, s.second, layout);
    // the workspaces' maxima against the structs' own
    for (int w = 1; w <= 40; ++w)
        for (int h = 1; h <= 40; ++h) {
            const JpegMax o = jpeg_max(w, h, false), i = jpeg_max(w, h, true);
            const JpegeWork e(1, w, h);
            const JpeghWork d(1, w, h);
            std::printf("max %d %d : %llu %llu %zu %zu | %llu %llu %zu %zu\n", w, h,
                        static_cast<unsigned long long>(o.cap), static_cast<unsigned long long>(o.blocks), e.cap, e.blocks,
                        static_cast<unsigned long long>(i.cap), static_cast<unsigned long long>(i.blocks), d.cap, d.blocks);
        }
}
#endif

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "geom")) {
#ifdef HAVE_GEOM
        geom();
        return 0;
#else
        return 2;
#endif
    }
    pin();
    return 0;
}
