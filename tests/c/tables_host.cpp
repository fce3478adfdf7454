// tables_host.cpp — runs every host table builder of libmipx (csrc/mipx_tables.cpp) over a
// fixed list of parameter sets and prints one line per table:
//     name params : FNV-1a-64 of the bytes, length, metadata, rows   (or "none": no such table)
// No HIP call, no GPU: links mipx_tables.cpp and mipx_planner.cpp (the libvips maths) only;
// tests/test_tables_host.py compares the output with tests/golden/tables_host.txt.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mipx_tables.h"

namespace mipx {
// what mipx_planner.cpp needs from the rest of the engine
void set_error(const char *, ...) {}
int reduce_sampling_now() { return 0; }
}  // namespace mipx

using namespace mipx;

static void emit(const HostTable &t, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    if (t.bytes.empty()) {
        std::printf(" : none\n");
        return;
    }
    uint64_t h = 0xcbf29ce484222325ULL;
    for (uint8_t b : t.bytes) h = (h ^ b) * 0x100000001b3ULL;
    std::printf(" : %016llx %zu meta %d %d rows %d\n", static_cast<unsigned long long>(h), t.bytes.size(), t.meta[0],
                t.meta[1], t.rows);
}

int main() {
    const double shrinks[] = {1.02, 1.3333333333333333, 1.6, 2.0, 2.75};  // 7, 9, 11, 13, 17 taps
    for (double s : shrinks) {
        emit(build_reduce_table(s), "reduce_table %.17g", s);
        emit(build_reduce_pairs(s), "reduce_pairs %.17g", s);
        emit(build_reduce_i8(s), "reduce_i8 %.17g", s);
        for (int b = 1; b <= 4; ++b) {
            emit(build_reduce_i8s(s, b), "reduce_i8s %.17g b%d", s, b);
            emit(build_reduce_i8s_fold(s, b), "reduce_i8s_fold %.17g b%d", s, b);
        }
        for (int centre = 0; centre < 2; ++centre)
            for (int rows : {16, 1025}) emit(build_rcol_vplan(s, centre, rows), "rcol_vplan %.17g c%d rows%d", s, centre, rows);
    }
    emit(build_reduce_i8s(2.0, 0), "reduce_i8s 2 b0");
    emit(build_reduce_i8s_fold(2.0, 5), "reduce_i8s_fold 2 b5");
    emit(build_rcol_vplan(2.0, false, 0), "rcol_vplan 2 c0 rows0");

    // k_rcol's horizontal operands: {ox0, ow, w}
    for (double s : shrinks) {
        const int full = out_size_reduce(1000, s), narrow = out_size_reduce(4, s);
        const int geo[][3] = {
            {100, 64, 1000},          // one strip inside the image
            {0, 65, 1000},            // left edge, two strips
            {full - 63, 63, 1000},    // right edge, a window with ox0 > 0
            {0, out_size_reduce(200, s), 200},  // both edges, several strips
            {0, narrow, 4},           // narrower than the mask (both folds at once)
            {0, 1, 200}, {0, 63, 200}, {0, 64, 200}, {3, 65, 200},
        };
        for (const auto &g : geo)
            for (int b = 3; b <= 4; ++b)
                for (int centre = 0; centre < 2; ++centre)
                    for (int k4 = 0; k4 < 2; ++k4)
                        for (int nks = 1; nks <= 2; ++nks)
                            emit(build_rcol_hops(s, b, centre, g[0], g[1], g[2], k4, nks),
                                 "rcol_hops %.17g b%d c%d ox%d ow%d w%d k4%d nks%d", s, b, centre, g[0], g[1], g[2], k4, nks);
    }
    emit(build_rcol_hops(2.0, 2, false, 0, 64, 200, 0, 1), "rcol_hops 2 b2");
    emit(build_rcol_hops(2.0, 3, false, 0, 64, 200, 0, 3), "rcol_hops 2 nks3");
    emit(build_rcol_hops(2.0, 3, false, 0, 0, 200, 0, 1), "rcol_hops 2 ow0");

    for (double sigma : {0.5, 1.5, 5.0}) {
        emit(build_gauss_table(sigma, 0.2), "gauss_table %.17g 0.2", sigma);
        std::vector<int> mask;
        int scale = 0;
        const int taps = gaussmat(sigma, 0.2, mask, scale);
        for (int b : {1, 3, 4})
            for (int delta : {0, 3})
                for (int vperm = 0; vperm < 2; ++vperm) {
                    const int nks = (16 + delta + b * (taps - 1) + 63) / 64;  // k_bcol's K steps
                    emit(build_blur_ops(mask, b, delta, nks, vperm), "blur_ops %.17g b%d d%d nks%d v%d", sigma, b, delta,
                         nks, vperm);
                }
    }
    emit(build_gauss_table(0.0, 0.2), "gauss_table 0 0.2");
    emit(build_colour_tables(), "colour_tables");
    emit(build_bicubic_table(), "bicubic_table");
    return 0;
}
