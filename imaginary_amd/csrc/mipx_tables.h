// mipx_tables.h — the libvips table maths and the host builders of every device-resident
// table (mipx_tables.cpp, mipx_planner.cpp).  No HIP here: a plain host program can build and
// check every table (tests/c/tables_host.cpp).  mipx_device_tables.cpp uploads and caches what
// the builders return.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace mipx {

// ---- libvips resample constants (resample/templates.h, [U]) ----------------
constexpr int kTransformScale = 128;  // VIPS_TRANSFORM_SCALE: 129 sub-pixel phases
constexpr int kInterpShift = 12;      // VIPS_INTERPOLATE_SHIFT
constexpr int kInterpScale = 1 << kInterpShift;

// Lanczos3 reduce geometry (libvips reduceh.cpp / reducev.cpp).
int reduce_points(double shrink);                      // 2 * rint(3 * shrink) + 1
void reduce_table(double shrink, std::vector<int> &t); // 129 x n truncated 12-bit taps
int out_size_reduce(int in, double shrink);            // VIPS_ROUND(in / shrink)
int out_size_shrink(int in, int shrink);               // VIPS_ROUND(in / shrink)
// where output o of a reduce samples its input, under the corner or the centre convention
inline double reduce_x_host(int o, double s, bool centre) { return centre ? (o + 0.5) * s - 0.5 : o * s; }

// Integer gaussmat (libvips create/gaussmat.c): returns width, fills mask/scale.
int gaussmat(double sigma, double min_ampl, std::vector<int> &mask, int &scale);

// Colour LUTs for the smartcrop scorer (libvips colour/*.c, [U]).
constexpr int kQuantElements = 100000;
const float *v2y8_table();    // 256 entries: sRGB 8-bit -> linear
const float *cbrt_table();    // kQuantElements entries: Lab f(t)
const float *y2v8_table();    // 257 entries: linear Y x 255 -> sRGB 8-bit (B_W)
void bicubic_table(int *t);   // 129 x 4 bicubic taps (vips_affine)

// ---- table layouts the kernels share with the builders -----------------------
constexpr int kHmTabW = 64;     // k_hmfma i8 tap rows: bytes per (phase, hi / lo) row (16.5 KB: L1-resident)
constexpr int kHmTabPad = 16;   // zero bytes in front of tap 0 (taps <= 16; windows clamped to [-16, 16])
constexpr int kRsTabPad = 128;  // k_rmf4 stride-B tap rows: zero bytes in front of tap 0
constexpr int kRsTabW = 272;    // bytes per (phase, hi / lo) row: pad + 2 K steps + a fragment (70 KB per table)
constexpr int kRcolPlanRow = 144;                              // k_rcol's vertical plan: bytes per output row
constexpr int kRcolHopRec(int nks) { return 32 * nks + 16; }   // k_rcol's horizontal operands: bytes per lane record
constexpr int kJpegcRecipShift = 20;                            // k_jpegc's reciprocals: m = ceil(2^20 / q)

// ---- JPEG quantisation tables (libjpeg jpeg_set_quality(quality, TRUE) over Annex K) ------
// natural (row-major) order; false for a quality outside 1..100
bool jpeg_qtables(int quality, uint8_t lum[64], uint8_t chr[64]);

// ---- host builders (mipx_tables.cpp) --------------------------------------------
// What a builder returns: the table as it goes to the device, and what its fetcher reports
// besides the pointer.  No bytes = no such table (parameters outside what the kernel takes).
struct HostTable {
    std::vector<uint8_t> bytes;
    int meta[2] = {0, 0};
    int rows = 0;  // growable tables: the rows this build holds
};
HostTable build_reduce_table(double shrink);                       // meta: taps
HostTable build_reduce_pairs(double shrink);                       // meta: taps, tpa
HostTable build_reduce_i8(double shrink);                          // meta: taps, byte offset of the sums
HostTable build_reduce_i8s(double shrink, int bands);              // meta: taps
HostTable build_reduce_i8s_fold(double shrink, int bands);         // meta: taps
HostTable build_rcol_vplan(double shrink, bool centre, int rows);  // rows: 1024 << k >= rows asked for
size_t rcol_hops_bytes(int bands, int ow, int nks);                // size of the next one's table
HostTable build_rcol_hops(double hs, int bands, bool centre, int ox0, int ow, int w, int k4, int nks);  // meta: strips
HostTable build_blur_ops(const std::vector<int> &mask, int bands, int delta, int nks, int vperm);
HostTable build_gauss_table(double sigma, double min_ampl);        // meta: taps, scale
HostTable build_colour_tables();
HostTable build_bicubic_table();
// k_jpegc's quantisation divisors at one quality: [lum 64 | chr 64] uint32 in natural order, each
// m | q << 21 with m = ceil(2^kJpegcRecipShift / q): (n * m) >> kJpegcRecipShift == n / q for
// every n < 2^12, so ((c + 4 q) >> 3) through it is (c + 4 q) / (8 q) for c + 4 q < 2^15
HostTable build_jpegc_recips(int quality);
// k_jpege's Huffman codes, canonical (Annex C) from the code counts and symbols of Annex K.3:
// [DC lum | AC lum | DC chr | AC chr], kJpegeCodesPerTable uint32 each, indexed by the symbol (a DC
// category 0..11, or an AC run << 4 | size), each length << 16 | code; 0 where the table has no code
constexpr int kJpegeCodesPerTable = 256;
HostTable build_jpege_codes();
// One optimised Huffman table (libjpeg jchuff.c jpeg_gen_optimal_table, PARITY_ASSUMPTIONS.md row 24)
// of the counts of its 256 symbols: the DHT as the engine's slots hold it (16 code counts per length,
// then the symbols by code, zero-padded) and the codes in build_jpege_codes' format.  The serial
// form k_jpege_tables is held to.  Returns the longest code length before the limiting to 16 bits
// (0 for a table of no symbol).  Counts that sum to 2^30 or more are outside the rule.
constexpr int kJpegDhtBytes = 272;
int jpeg_optimal_table(const uint32_t freq[256], uint8_t dht[kJpegDhtBytes], uint32_t codes[kJpegeCodesPerTable]);

// The directory of packed scan slots (mipx_op_*_scan_packed) as mipx_jpeg_scan_unpack and the request
// path's completer take it: off[0] = 0, non-decreasing, every step a multiple of 16 and at least
// `head`, off[n] <= packed_bytes.
bool scan_dir_ok(const uint64_t *dir, int32_t n, size_t head, size_t packed_bytes);

}  // namespace mipx
