// mipx_tables.cpp — host builders of the device-resident tables: the libvips taps laid out
// as each kernel reads them (per-lane MFMA operands, K-index permutations, folded edges,
// seeds).  No HIP call in this file; mipx_device_tables.cpp uploads and caches the results.
// Built without FP contraction, as the oracle (positions are separately rounded doubles).
#include <algorithm>
#include <cstring>

#include "mipx.h"
#include "mipx_tables.h"

namespace mipx {
namespace {

template <class T>
std::vector<uint8_t> as_bytes(const std::vector<T> &v) {
    std::vector<uint8_t> b(v.size() * sizeof(T));
    if (!b.empty()) std::memcpy(b.data(), v.data(), b.size());
    return b;
}

// a 12-bit tap as two i8 MFMA operands: c = 64 hi + lo, hi = c >> 6 (signed), lo = c & 63
inline void split_tap(int c, uint8_t *hi, uint8_t *lo) {
    *hi = static_cast<uint8_t>(static_cast<signed char>(c >> 6));
    *lo = static_cast<uint8_t>(c & 63);
}

// the first input pixel of output o's taps (pad = taps / 2 - 1) and its phase
inline int reduce_pos(int o, double shrink, bool centre, int pad, int *phase) {
    const double X = reduce_x_host(o, shrink, centre);
    if (phase) *phase = ((static_cast<int>(X * 256.0) & 255) + 1) >> 1;
    return static_cast<int>(X) - pad;
}

// libvips' COPY edge folded into a tap row c[0 .. n).  Left, amount a: the first tap pixel is
// -a, so taps 0..a land on pixel 0 (their sum at tap a, zeros before).  Right, amount a: the
// last tap pixel is w - 1 + a, so taps n-1-a .. n-1 land on pixel w - 1 (their sum at tap
// n-1-a, zeros after).
void fold_left(const int *c, int n, int a, int *f) {
    int sum = 0;
    for (int k = 0; k < n; ++k) {
        if (k <= a) sum += c[k];
        f[k] = k < a ? 0 : k == a ? sum : c[k];
    }
}
void fold_right(const int *c, int n, int a, int *f) {
    const int e = n - 1 - a;
    int sum = 0;
    for (int k = e; k < n; ++k) sum += c[k];
    for (int k = 0; k < n; ++k) f[k] = k > e ? 0 : k == e ? sum : c[k];
}

}  // namespace

// float copy of reduce_table(shrink): [129 phases][taps]
HostTable build_reduce_table(double shrink) {
    std::vector<int> t;
    reduce_table(shrink, t);
    HostTable r;
    r.bytes = as_bytes(std::vector<float>(t.begin(), t.end()));
    r.meta[0] = reduce_points(shrink);
    return r;
}

// The same taps as int16 pairs for v_dot2: [129 phases][2 alignments][tpa]
// words, tpa = taps / 2 + 1; alignment 0 = (c[2m], c[2m+1]), alignment 1 =
// (c[2m-1], c[2m]) (taps outside [0, taps) are 0).  k_rstrip reads them directly.
HostTable build_reduce_pairs(double shrink) {
    const int n = reduce_points(shrink), w = n / 2 + 1;
    std::vector<int> t;
    reduce_table(shrink, t);
    std::vector<uint32_t> h(static_cast<size_t>(kTransformScale + 1) * 2 * w);
    auto tap = [&](int ph, int i) -> uint32_t {
        return (i < 0 || i >= n) ? 0u : static_cast<uint32_t>(t[static_cast<size_t>(ph) * n + i]) & 0xffffu;
    };
    for (int ph = 0; ph <= kTransformScale; ++ph)
        for (int al = 0; al < 2; ++al)
            for (int m = 0; m < w; ++m)
                h[(static_cast<size_t>(ph) * 2 + al) * w + m] = tap(ph, 2 * m - al) | (tap(ph, 2 * m + 1 - al) << 16);
    HostTable r;
    r.bytes = as_bytes(h);
    r.meta[0] = n;
    r.meta[1] = w;
    return r;
}

// The same taps split for the i8 MFMA horizontal reduce (k_hmfma): per phase two
// rows of kHmTabW bytes, hi = c >> 6 and lo = c & 63 (c = 64 hi + lo, both fit
// i8), tap i at byte kHmTabPad + i, zeros around; after the 129 x 2 rows, 129
// ints holding each phase's tap sum (the bias of the pixel - 128 offset).
HostTable build_reduce_i8(double shrink) {
    const int n = reduce_points(shrink);
    if (n > 16) return {};  // k_hmfma: a 16-byte fragment window holds every tap
    const size_t rows_bytes = static_cast<size_t>(kTransformScale + 1) * 2 * kHmTabW;
    std::vector<int> t;
    reduce_table(shrink, t);
    HostTable r;
    r.bytes.assign(rows_bytes + (kTransformScale + 1) * sizeof(int), 0);
    for (int ph = 0; ph <= kTransformScale; ++ph) {
        uint8_t *row = r.bytes.data() + static_cast<size_t>(ph) * 2 * kHmTabW + kHmTabPad;
        int sum = 0;
        for (int i = 0; i < n; ++i) {
            const int c = t[static_cast<size_t>(ph) * n + i];
            sum += c;
            split_tap(c, row + i, row + kHmTabW + i);
        }
        std::memcpy(r.bytes.data() + rows_bytes + ph * sizeof(int), &sum, sizeof(int));
    }
    r.meta[0] = n;
    r.meta[1] = static_cast<int>(rows_bytes);
    return r;
}

// The same split taps at a byte stride of `bands` (k_rmf4's horizontal products on
// interleaved pixel bytes): row (phase, hi / lo) holds tap i at byte kRsTabPad + bands * i,
// zeros elsewhere, so a 16-byte window at any offset in [-kRsTabPad, 64) is an MFMA
// fragment of one output byte's taps.
HostTable build_reduce_i8s(double shrink, int bands) {
    const int n = reduce_points(shrink);
    if (n > 16 || bands < 1 || bands > 4) return {};
    std::vector<int> t;
    reduce_table(shrink, t);
    HostTable r;
    r.bytes.assign(static_cast<size_t>(kTransformScale + 1) * 2 * kRsTabW, 0);
    for (int ph = 0; ph <= kTransformScale; ++ph) {
        uint8_t *row = r.bytes.data() + static_cast<size_t>(ph) * 2 * kRsTabW + kRsTabPad;
        for (int i = 0; i < n; ++i) split_tap(t[static_cast<size_t>(ph) * n + i], row + bands * i, row + kRsTabW + bands * i);
    }
    r.meta[0] = n;
    return r;
}

// The stride-B split taps with libvips' COPY edge folded in (k_rcol's edge operands):
// rows [2 sides][taps - 1 amounts][129 phases][hi, lo][kRsTabW]; side 0 is fold_left by the
// amount, side 1 fold_right.
HostTable build_reduce_i8s_fold(double shrink, int bands) {
    const int n = reduce_points(shrink);
    if (n > 16 || n < 2 || bands < 1 || bands > 4) return {};
    std::vector<int> t;
    reduce_table(shrink, t);
    const size_t per_side = static_cast<size_t>(n - 1) * (kTransformScale + 1) * 2 * kRsTabW;
    HostTable r;
    r.bytes.assign(2 * per_side, 0);
    std::vector<int> f(n);
    for (int side = 0; side < 2; ++side)
        for (int a = 1; a < n; ++a)
            for (int ph = 0; ph <= kTransformScale; ++ph) {
                const int *c = t.data() + static_cast<size_t>(ph) * n;
                if (side == 0) fold_left(c, n, a, f.data());
                else fold_right(c, n, a, f.data());
                uint8_t *row = r.bytes.data() + side * per_side +
                               ((static_cast<size_t>(a - 1) * (kTransformScale + 1) + ph) * 2) * kRsTabW + kRsTabPad;
                for (int k = 0; k < n; ++k) split_tap(f[k], row + bands * k, row + kRsTabW + bands * k);
            }
    r.meta[0] = n;
    return r;
}

// k_rcol's vertical plan for one shrink and sampling convention over output rows
// 0 .. cap - 1: per output row o, kRcolPlanRow bytes = [64 hi][64 lo] i8 taps placed
// at the K index of their input row relative to the first input row of o's 16-row
// group (K index 16 g + e holds relative row 8 g + e for e < 8, 32 + 8 g + e - 8
// otherwise: the transposed LDS reads' row order), the accumulator seed
// 128 * sum + 2048 - (128 << 12) (pixels enter as p - 128, the result leaves as u8 - 128),
// 12 pad bytes; then per 16-row group k two ints: its first input row start(16 k) and
// its end start(16 k + 15) + taps.  cap = 1024 << k, the first that holds the rows asked for.
HostTable build_rcol_vplan(double shrink, bool centre, int rows) {
    const int n = reduce_points(shrink);
    if (rows <= 0 || n > 16) return {};
    int cap = 1024;
    while (cap < rows) cap *= 2;
    std::vector<int> t;
    reduce_table(shrink, t);
    const int pad = n / 2 - 1;
    auto start = [&](int o, int *phase) { return reduce_pos(o, shrink, centre, pad, phase); };
    const size_t rows_bytes = static_cast<size_t>(cap) * kRcolPlanRow;
    HostTable r;
    std::vector<uint8_t> &h = r.bytes;
    h.assign(rows_bytes + static_cast<size_t>(cap / 16) * 2 * sizeof(int), 0);
    for (int o = 0; o < cap; ++o) {
        int ph = 0;
        const int d = start(o, &ph) - start(o & ~15, nullptr);
        const int *c = t.data() + static_cast<size_t>(ph) * n;
        uint8_t *row = h.data() + static_cast<size_t>(o) * kRcolPlanRow;
        int sum = 0;
        for (int i = 0; i < n; ++i) sum += c[i];
        for (int k = 0; k < 64; ++k) {
            const int e = k & 15, g = k >> 4;
            const int rel = e < 8 ? 8 * g + e : 32 + 8 * g + e - 8;
            const int ti = rel - d;
            split_tap(ti >= 0 && ti < n ? c[ti] : 0, row + k, row + 64 + k);
        }
        const int seed = 128 * sum + 2048 - (128 << 12);
        std::memcpy(row + 128, &seed, sizeof(int));
    }
    for (int k = 0; k < cap / 16; ++k) {
        const int se[2] = {start(16 * k, nullptr), start(16 * k + 15, nullptr) + n};
        std::memcpy(h.data() + rows_bytes + static_cast<size_t>(k) * 2 * sizeof(int), se, sizeof(se));
    }
    r.rows = cap;
    return r;
}

// k_rcol's host-built horizontal operands of one window geometry (r06).  The same
// arithmetic as k_rcol's set-up (positions as separately rounded doubles: this file is
// built without FP contraction, as the oracle).  Per 64-pixel strip, per 16-byte output unit
// u < 4 bands, per lane: per K step the hi / lo tap fragments (COPY edge folded, odd K
// blocks' halves swapped), then the four per-byte seeds, kRcolHopRec(nks) bytes; then per
// (strip, unit) the K origin (int).
size_t rcol_hops_bytes(int bands, int ow, int nks) {
    const size_t units = static_cast<size_t>((ow + 63) / 64) * 4 * bands;
    return units * 64 * kRcolHopRec(nks) + units * sizeof(int);
}

HostTable build_rcol_hops(double hs, int bands, bool centre, int ox0, int ow, int w, int k4, int nks) {
    if (ow <= 0 || w <= 0 || bands < 3 || bands > 4 || nks < 1 || nks > 2) return {};
    const size_t rsz = kRcolHopRec(nks);
    const int n = reduce_points(hs), B = bands, pad = n / 2 - 1;
    if (n > 16 || n < 2) return {};
    const int ns = (ow + 63) / 64, units = 4 * B;
    const size_t recs = static_cast<size_t>(ns) * units * 64;
    std::vector<int> t;
    reduce_table(hs, t);
    std::vector<int> sums(kTransformScale + 1, 0);
    for (int ph = 0; ph <= kTransformScale; ++ph)
        for (int i = 0; i < n; ++i) sums[ph] += t[static_cast<size_t>(ph) * n + i];
    auto pos = [&](int o, int *ph) { return reduce_pos(o, hs, centre, pad, ph); };
    HostTable r;
    std::vector<uint8_t> &h = r.bytes;
    h.assign(rcol_hops_bytes(B, ow, nks), 0);
    int *kbs = reinterpret_cast<int *>(h.data() + recs * rsz);
    std::vector<int> f(n);
    for (int s = 0; s < ns; ++s) {
        const int x0 = 64 * s, x_last = std::min(x0 + 63, ow - 1);
        int ph = 0;
        const int lo = pos(ox0 + x0, &ph);
        const int org = lo & (lo < 0 && B == 3 ? ~15 : ~3);
        for (int u = 0; u < units; ++u) {
            const int sf = pos(ox0 + std::min(x0 + (16 * u) / B, x_last), &ph);
            const int kb = (B * (sf - org) + (16 * u) % B) & (k4 ? ~3 : ~7);
            kbs[s * units + u] = kb;
            for (int lane = 0; lane < 64; ++lane) {
                const int nn = lane & 15, kg = lane >> 4;
                uint8_t *rec = h.data() + ((static_cast<size_t>(s) * units + u) * 64 + lane) * rsz;
                const int o = 16 * u + nn, xl = o / B, c = o - B * xl;
                int pp = 0;
                const int sp = pos(ox0 + std::min(x0 + xl, x_last), &pp);
                const int *cr = t.data() + static_cast<size_t>(pp) * n;
                const int lfold = -sp, rfold = sp + n - 1 - (w - 1);
                const bool both = lfold > 0 && rfold > 0;
                // the tap row k_rcol reads: plain, or the COPY edge folded onto pixel 0 / w - 1
                if (!both && lfold > 0) fold_left(cr, n, lfold, f.data());
                else if (!both && rfold > 0) fold_right(cr, n, rfold, f.data());
                else std::copy(cr, cr + n, f.begin());
                for (int ks = 0; ks < nks; ++ks) {
                    const int j0 = kb + 64 * ks + 16 * kg;
                    uint8_t fh[16], fl[16];
                    for (int e = 0; e < 16; ++e) {
                        int v = 0;
                        const int d = j0 + e - c;
                        if (both) {  // images narrower than the mask (rc_edge_frag)
                            if (d >= 0 && d % B == 0) {
                                const int p = org + d / B;
                                if (p >= 0 && p <= w - 1)
                                    for (int k = 0; k < n; ++k)
                                        if (std::min(std::max(sp + k, 0), w - 1) == p) v += cr[k];
                            }
                        } else {
                            const int rr = d - B * (sp - org);  // tap k sits at rr = B k
                            if (rr >= 0 && rr % B == 0 && rr / B < n) v = f[rr / B];
                        }
                        split_tap(v, fh + e, fl + e);
                    }
                    // odd K blocks read their second 8 bytes first (k_rcol's swz)
                    const int sw = (kg & 1) ? 8 : 0;
                    for (int e = 0; e < 16; ++e) {
                        rec[32 * ks + e] = fh[(e + sw) & 15];
                        rec[32 * ks + 16 + e] = fl[(e + sw) & 15];
                    }
                }
                const int eb = 16 * u + 4 * kg;
                for (int j = 0; j < 4; ++j) {
                    int p2 = 0;
                    pos(ox0 + std::min(x0 + (eb + j) / B, x_last), &p2);
                    const int seed = 128 * sums[p2] + 2048;
                    std::memcpy(rec + 32 * nks + 4 * j, &seed, sizeof(int));
                }
            }
        }
    }
    r.meta[0] = ns;
    return r;
}

// k_bmf operands (i8, 16 bytes per lane in the v_mfma_i32_16x16x64_i8 layouts):
// [nks][64 lanes] horizontal A: lane l row m = l & 15 (output byte), K bytes
// 64 ks + 16 (l >> 4) + j hold tap k where K = m + delta + bands * k; then
// [64 lanes] vertical B: K index 16 (l >> 4) + j holds relative row R = K (vperm 0) or
// R = 8 (l >> 4) + j (j < 8) / 32 + 8 (l >> 4) + j - 8 (vperm 1, k_bcol's transposed reads
// of consecutive rows); output row l & 15 holds tap R - row.
HostTable build_blur_ops(const std::vector<int> &mask, int bands, int delta, int nks, int vperm) {
    const int n = static_cast<int>(mask.size());
    HostTable r;
    std::vector<uint8_t> &h = r.bytes;
    h.assign(static_cast<size_t>(nks + 1) * 64 * 16, 0);
    const auto i8 = [](int v) { return static_cast<uint8_t>(static_cast<signed char>(v)); };
    for (int ks = 0; ks < nks; ++ks)
        for (int l = 0; l < 64; ++l)
            for (int j = 0; j < 16; ++j) {
                const int m = l & 15, kk = 64 * ks + 16 * (l >> 4) + j - m - delta;
                if (kk >= 0 && kk % bands == 0 && kk / bands < n) h[(static_cast<size_t>(ks) * 64 + l) * 16 + j] = i8(mask[kk / bands]);
            }
    for (int l = 0; l < 64; ++l)
        for (int j = 0; j < 16; ++j) {
            const int rel = vperm ? (j < 8 ? 8 * (l >> 4) + j : 32 + 8 * (l >> 4) + j - 8) : 16 * (l >> 4) + j;
            const int k = rel - (l & 15);
            if (k >= 0 && k < n) h[(static_cast<size_t>(nks) * 64 + l) * 16 + j] = i8(mask[k]);
        }
    return r;
}

// float copy of the integer gaussmat mask; scale = mask sum
HostTable build_gauss_table(double sigma, double min_ampl) {
    std::vector<int> mask;
    int sc = 0;
    const int n = gaussmat(sigma, min_ampl, mask, sc);
    if (n <= 0) return {};
    HostTable r;
    r.bytes = as_bytes(std::vector<float>(mask.begin(), mask.end()));
    r.meta[0] = n;
    r.meta[1] = sc;
    return r;
}

// [256 v2y | kQuantElements cbrt | 257 y2v] floats
HostTable build_colour_tables() {
    std::vector<float> h(256 + kQuantElements + 257);
    std::memcpy(h.data(), v2y8_table(), 256 * sizeof(float));
    std::memcpy(h.data() + 256, cbrt_table(), kQuantElements * sizeof(float));
    std::memcpy(h.data() + 256 + kQuantElements, y2v8_table(), 257 * sizeof(float));
    HostTable r;
    r.bytes = as_bytes(h);
    return r;
}

HostTable build_bicubic_table() {
    std::vector<int> t((kTransformScale + 1) * 4);
    bicubic_table(t.data());
    HostTable r;
    r.bytes = as_bytes(t);
    return r;
}

// jcparam.c: the Annex K.1 / K.2 tables (natural order) scaled by jpeg_quality_scaling and
// clamped to 1..255 (force_baseline)
bool jpeg_qtables(int quality, uint8_t lum[64], uint8_t chr[64]) {
    static const uint8_t std_lum[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,
                                        14, 13, 16, 24, 40,  57,  69,  56,  14, 17, 22, 29, 51,  87,  80,  62,
                                        18, 22, 37, 56, 68,  109, 103, 77,  24, 35, 55, 64, 81,  104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
    static const uint8_t std_chr[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                                        24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                        99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
    if (quality < 1 || quality > 100 || !lum || !chr) return false;
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        lum[k] = static_cast<uint8_t>(std::min(std::max((std_lum[k] * s + 50) / 100, 1), 255));
        chr[k] = static_cast<uint8_t>(std::min(std::max((std_chr[k] * s + 50) / 100, 1), 255));
    }
    return true;
}

HostTable build_jpegc_recips(int quality) {
    uint8_t q[128];
    if (!jpeg_qtables(quality, q, q + 64)) return {};
    std::vector<uint32_t> t(128);
    for (int k = 0; k < 128; ++k) {
        const uint32_t m = ((1u << kJpegcRecipShift) + q[k] - 1u) / q[k];
        t[k] = m | static_cast<uint32_t>(q[k]) << 21;
    }
    HostTable r;
    r.bytes = as_bytes(t);
    return r;
}

// Annex K.3.3: code counts per length 1..16, then the symbols in code order
namespace {

struct HuffSpec {
    uint8_t counts[16];
    const uint8_t *symbols;
};
const uint8_t kDcSymbols[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const uint8_t kAcLumSymbols[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
    0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
    0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
    0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
    0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
    0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const uint8_t kAcChrSymbols[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
    0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
    0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
    0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
    0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
    0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
    0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
    0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
const HuffSpec kHuffSpecs[4] = {
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, kDcSymbols},       // DC luminance
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, kAcLumSymbols},  // AC luminance
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, kDcSymbols},       // DC chrominance
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}, kAcChrSymbols},  // AC chrominance
};

}  // namespace

HostTable build_jpege_codes() {
    std::vector<uint32_t> t(4 * kJpegeCodesPerTable, 0u);
    for (int i = 0; i < 4; ++i) {
        uint32_t code = 0;
        int k = 0;
        for (uint32_t length = 1; length <= 16; ++length) {
            for (int c = 0; c < kHuffSpecs[i].counts[length - 1]; ++c)
                t[i * kJpegeCodesPerTable + kHuffSpecs[i].symbols[k++]] = length << 16 | code++;
            code <<= 1;
        }
    }
    HostTable r;
    r.bytes = as_bytes(t);
    return r;
}

int jpeg_optimal_table(const uint32_t freq[256], uint8_t dht[kJpegDhtBytes], uint32_t codes[kJpegeCodesPerTable]) {
    constexpr int kMaxLen = 63;  // lengths past it would need counts that sum past 2^30
    uint64_t f[257];
    int codesize[257], others[257], bits[kMaxLen + 1];
    for (int i = 0; i < 256; ++i) f[i] = freq[i];
    f[256] = 1;  // the reserved point: no code is all ones
    for (int i = 0; i <= 256; ++i) codesize[i] = 0, others[i] = -1;
    for (int i = 0; i <= kMaxLen; ++i) bits[i] = 0;
    std::memset(dht, 0, kJpegDhtBytes);
    for (int i = 0; i < kJpegeCodesPerTable; ++i) codes[i] = 0;
    for (;;) {
        int c1 = -1, c2 = -1;  // the least frequency, the largest index among equals; then again without c1
        for (int i = 0; i <= 256; ++i)
            if (f[i] && (c1 < 0 || f[i] <= f[c1])) c1 = i;
        for (int i = 0; i <= 256; ++i)
            if (f[i] && i != c1 && (c2 < 0 || f[i] <= f[c2])) c2 = i;
        if (c2 < 0) break;
        f[c1] += f[c2], f[c2] = 0;
        for (++codesize[c1]; others[c1] >= 0; ++codesize[c1]) c1 = others[c1];
        others[c1] = c2;
        for (++codesize[c2]; others[c2] >= 0; ++codesize[c2]) c2 = others[c2];
    }
    int raw = 0;
    for (int i = 0; i <= 256; ++i) {
        if (!codesize[i]) continue;
        if (codesize[i] > kMaxLen) codesize[i] = kMaxLen;
        ++bits[codesize[i]];
        if (codesize[i] > raw) raw = codesize[i];
    }
    for (int i = kMaxLen; i > 16; --i)
        while (bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && bits[j] == 0) --j;
            if (j == 0 || bits[i] < 2) {  // not reached for counts in range
                bits[i] = 0;
                break;
            }
            bits[i] -= 2, bits[i - 1] += 1, bits[j + 1] += 2, bits[j] -= 1;
        }
    int longest = 16;
    while (longest > 0 && bits[longest] == 0) --longest;
    if (longest) --bits[longest];  // the reserved point's code
    for (int len = 1; len <= 16; ++len) dht[len - 1] = static_cast<uint8_t>(bits[len]);
    int p = 0;
    for (int len = 1; len <= kMaxLen; ++len)  // by raw length, then by value
        for (int i = 0; i < 256; ++i)
            if (codesize[i] == len && p < 256) dht[16 + p++] = static_cast<uint8_t>(i);
    uint32_t code = 0;
    int k = 0;
    for (uint32_t len = 1; len <= 16; ++len) {  // Annex C
        for (int c = 0; c < bits[len] && k < p; ++c) codes[dht[16 + k++]] = len << 16 | code++;
        code <<= 1;
    }
    return raw;
}

}  // namespace mipx

// ---- packed scan slots (k_jpege.hip's packed mode): the host side, HIP-free --------------------
namespace mipx {

bool scan_dir_ok(const uint64_t *dir, int32_t n, size_t head, size_t packed_bytes) {
    if (!dir || n <= 0 || head < MIPX_JPEG_SCAN_HEADER_BYTES || dir[0] != 0) return false;
    for (int32_t i = 0; i < n; ++i) {
        if (dir[i + 1] < dir[i]) return false;
        const uint64_t step = dir[i + 1] - dir[i];
        if ((step & 15u) || step < head) return false;
    }
    return dir[n] <= packed_bytes;
}

}  // namespace mipx

extern "C" size_t mipx_jpeg_scan_packed_dir_bytes(int32_t n) {
    return n > 0 ? 8 * (static_cast<size_t>(n) + 1) : 0;
}

extern "C" int mipx_jpeg_scan_unpack(const uint64_t *dir, int32_t n, const uint8_t *packed, size_t packed_bytes, int32_t i,
                                     size_t head, uint8_t *slot, size_t slot_bytes) {
    if (!dir || !packed || !slot || n <= 0 || i < 0 || i >= n) return MIPX_EINVAL;
    if (head != MIPX_JPEG_SCAN_HEADER_BYTES && head != MIPX_JPEG_SCAN_OPT_HEADER_BYTES) return MIPX_EINVAL;
    if (!mipx::scan_dir_ok(dir, n, head, packed_bytes)) return MIPX_EDATA;
    const uint8_t *from = packed + dir[i];
    uint32_t length, status;
    std::memcpy(&length, from, 4);
    std::memcpy(&status, from + 4, 4);
    // an OVERFLOW header's length is a need, above the capacity: it has no bytes behind it
    const uint64_t bytes = head + (status == MIPX_JPEG_SCAN_OK ? static_cast<uint64_t>(length) : 0u);
    if (bytes > dir[i + 1] - dir[i] || bytes > slot_bytes) return MIPX_EDATA;
    std::memcpy(slot, from, static_cast<size_t>(bytes));
    return MIPX_OK;
}
