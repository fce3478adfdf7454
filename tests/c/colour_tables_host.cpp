// colour_tables_host.cpp — writes the smartcrop scorer's two colour look-ups as the engine
// builds them (csrc/mipx_planner.cpp: 256 floats sRGB -> linear, then kQuantElements floats
// of Lab's f(t)) to stdout, raw.  No HIP call, no GPU; tests/test_smartcrop_cpu.py compares
// them with the same tables computed from the formulas.
#include <cstdio>

#include "mipx_tables.h"

namespace mipx {
// what mipx_planner.cpp needs from the rest of the engine
void set_error(const char *, ...) {}
int reduce_sampling_now() { return 0; }
}  // namespace mipx

int main() {
    if (std::fwrite(mipx::v2y8_table(), sizeof(float), 256, stdout) != 256) return 1;
    const size_t n = mipx::kQuantElements;
    return std::fwrite(mipx::cbrt_table(), sizeof(float), n, stdout) == n ? 0 : 1;
}
