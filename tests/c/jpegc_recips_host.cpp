// jpegc_recips_host.cpp — k_jpegc divides by multiplying with the host-built reciprocals of
// build_jpegc_recips (csrc/mipx_tables.cpp).  For every q in 1..255, with m = ceil(2^20 / q),
// the kernel's expression ((n >> 3) * m) >> 20 must equal n / (8 q) for every numerator
// n = |c| + 4 q below 2^15 (the forward DCT's largest |c| is under 7600, so the rule's largest
// n is under 9000), with the product inside 32 bits and both factors inside 24.  Then the
// builder's table of every quality must unpack to that quality's q and to exactly that m.
// No HIP call, no GPU: links mipx_tables.cpp and mipx_planner.cpp only (tests/test_jpegc_cpu.py).
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
    uint32_t recip[256] = {};
    for (uint32_t q = 1; q <= 255; ++q) {
        uint32_t m = (1u << kJpegcRecipShift) / q;
        if (m * q != (1u << kJpegcRecipShift)) ++m;   // ceil
        recip[q] = m;
        for (uint32_t n = 0; n < (1u << 15); ++n) {
            const uint64_t wide = static_cast<uint64_t>(n >> 3) * m;
            if (m >= (1u << 24) || wide >= (1ull << 32))
                return std::printf("q %u n %u: the product leaves the 24 x 24 -> 32 bit multiply\n", q, n), 1;
            if (static_cast<uint32_t>(wide >> kJpegcRecipShift) != n / (8 * q))
                return std::printf("q %u n %u: %u != %u\n", q, n, static_cast<uint32_t>(wide >> kJpegcRecipShift), n / (8 * q)), 1;
        }
    }
    for (int quality = 1; quality <= 100; ++quality) {
        uint8_t q[128];
        if (!jpeg_qtables(quality, q, q + 64)) return std::printf("no tables at quality %d\n", quality), 1;
        const HostTable t = build_jpegc_recips(quality);
        if (t.bytes.size() != 128 * sizeof(uint32_t)) return std::printf("table size at quality %d\n", quality), 1;
        uint32_t e[128];
        std::memcpy(e, t.bytes.data(), sizeof(e));
        for (int k = 0; k < 128; ++k) {
            const uint32_t qq = e[k] >> 21, m = e[k] & 0x1fffffu;
            if (qq != q[k] || qq < 1 || qq > 255) return std::printf("quality %d entry %d: q %u\n", quality, k, qq), 1;
            if (m != recip[qq]) return std::printf("quality %d entry %d: m %u, not %u\n", quality, k, m, recip[qq]), 1;
        }
    }
    if (!build_jpegc_recips(0).bytes.empty() || !build_jpegc_recips(101).bytes.empty())
        return std::printf("a quality outside 1..100 gave a table\n"), 1;
    std::printf("ok\n");
    return 0;
}
