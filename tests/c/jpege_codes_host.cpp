// jpege_codes_host.cpp — prints the Huffman code table k_jpege reads (build_jpege_codes,
// csrc/mipx_tables.cpp), one line per code: table (0 DC luminance, 1 AC luminance, 2 DC
// chrominance, 3 AC chrominance), symbol, code, length.  tests/test_jpege_cpu.py compares the lines
// with the canonical codes codec.py derives from the Annex K.3 counts and symbols.
// No HIP call, no GPU: links mipx_tables.cpp and mipx_planner.cpp only.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "mipx_tables.h"

namespace mipx {
// what mipx_planner.cpp needs from the rest of the engine
void set_error(const char *, ...) {}
int reduce_sampling_now() { return 0; }
}  // namespace mipx

using namespace mipx;

int main() {
    const HostTable t = build_jpege_codes();
    if (t.bytes.size() != 4 * kJpegeCodesPerTable * sizeof(uint32_t)) return std::printf("table size %zu\n", t.bytes.size()), 1;
    for (int i = 0; i < 4 * kJpegeCodesPerTable; ++i) {
        uint32_t e;
        std::memcpy(&e, t.bytes.data() + 4 * i, 4);
        if (e) std::printf("%d %d %u %u\n", i / kJpegeCodesPerTable, i % kJpegeCodesPerTable, e & 0xffffu, e >> 16);
    }
    return 0;
}
