// jpego_tables_host.cpp — runs the host builder of one optimised Huffman table
// (jpeg_optimal_table, csrc/mipx_tables.cpp: the serial form k_jpege_tables is held to) on the
// histograms of a text file, 256 counts per line, and prints per histogram three lines: the longest
// code length before the limiting, then the DHT's 16 counts, then its symbols; then "codes" and one
// `symbol code length` triple per coded symbol.  tests/test_jpegeo_cpu.py compares them with
// codec.jpeg_optimal_table.  The DHT's zero padding and the codes of absent symbols are checked here.
// No HIP call, no GPU: links mipx_tables.cpp and mipx_planner.cpp only.
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

int main(int argc, char **argv) {
    if (argc != 2) return std::printf("usage: %s histograms.txt\n", argv[0]), 2;
    std::FILE *in = std::fopen(argv[1], "r");
    if (!in) return std::printf("cannot read %s\n", argv[1]), 2;
    std::vector<uint32_t> freq(256);
    for (;;) {
        int got = 0;
        for (; got < 256; ++got) {
            unsigned long long v;
            if (std::fscanf(in, "%llu", &v) != 1) break;
            freq[got] = static_cast<uint32_t>(v);
        }
        if (got == 0) break;
        if (got != 256) return std::printf("a histogram of %d counts\n", got), 1;
        std::vector<uint8_t> dht(kJpegDhtBytes, 0xAB);
        std::vector<uint32_t> codes(kJpegeCodesPerTable, 0xABABABABu);
        const int raw = jpeg_optimal_table(freq.data(), dht.data(), codes.data());
        int n = 0;
        std::printf("%d\n", raw);
        for (int i = 0; i < 16; ++i) std::printf("%d%c", dht[i], i == 15 ? '\n' : ' '), n += dht[i];
        for (int i = 0; i < n; ++i) std::printf("%d ", dht[16 + i]);
        std::printf("\ncodes");
        for (int i = 16 + n; i < kJpegDhtBytes; ++i)
            if (dht[i]) return std::printf("\nbyte %d behind the symbols is %d\n", i, dht[i]), 1;
        for (int s = 0; s < kJpegeCodesPerTable; ++s) {
            if (freq[s] == 0 && codes[s]) return std::printf("\nsymbol %d has no count and the code %x\n", s, codes[s]), 1;
            if (codes[s]) std::printf(" %d %u %u", s, codes[s] & 0xffffu, codes[s] >> 16);
        }
        std::printf("\n");
    }
    std::fclose(in);
    return 0;
}
