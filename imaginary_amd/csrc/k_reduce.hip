// k_reduce.hip — libvips vips_reduce (Lanczos3) on gfx950.
//
// reduce.c runs reducev then reduceh with a uchar intermediate; every tap is a
// 12-bit integer (matrixi, truncated) and each uchar result is
// (sum + 2048) >> 12 clipped (reduceh.cpp / reducev.cpp / templates.h,
// restated in oracle/vips_ref.c).  Sums stay exact in fp32 (< 2^24), so the
// kernels are bit-identical to the integer C path.
//
//  * k_reduce2x2     fused reducev -> reduceh for shrink 2 x 2 (north star C2)
//  * any other shrink: the generic separable passes of k_sep.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "device_common.h"
#include "lds_ops.h"
#include "reduce2_geom.h"

namespace mipx {
namespace {

using namespace dev;

// ===========================================================================
// Lanczos3 reduce by exactly 2 x 2, fused reducev -> reduceh (the north-star
// kernel: 4K -> 1080p).
//
// At shrink 2 with the corner convention every output samples phase 0, whose
// 13-tap mask has zeros at the odd integer positions of the Lanczos lobe and is
// symmetric, so output o = c0 * p[2o] + c1 * (p[2o-1] + p[2o+1])
//                      + c3 * (p[2o-3] + p[2o+3]) + c5 * (p[2o-5] + p[2o+5]).
// The host verifies that shape on the actual integer table before choosing
// this kernel, so the arithmetic is exactly libvips' 13-tap sum.
//
// One workgroup (256 lanes) = one tile: a strip of TW = 160 (RGB) / 120 (RGBA) output
// pixels x a band of 24 output rows; the constants and the launch of a window are
// reduce2_geom.h's.
//  * Vertical pass (reduce2_vpass): lane t owns dword t of the strip's input bytes
//    (channel agnostic) and walks down the band with the six odd rows of the current
//    window in a static register ring (slot = odd-row index mod 6); each input byte is
//    loaded and converted once.  The rounded uchar intermediate (libvips materialises it
//    between reducev and reduceh) is packed back to a dword and written to LDS in input
//    byte order: one conflict-free ds_write_b32 per lane and row.
//  * Horizontal pass (reduce2_hwalk): an item is K = 4 / 2 output pixels of one row; it
//    reads the 13-dword byte window it needs, converts each byte once and stores 12 / 8
//    contiguous output bytes.  240 lanes each own an item column and walk down it 6 / 4
//    rows at a time, with an LDS address and an output pointer that advance by constants;
//    the window comes as ds_read_b64 (RGB: lane stride 6 dwords) / ds_read_b128 (RGBA: 4
//    dwords) with an explicit wait.
// The intermediate never touches HBM; the 24-row LDS image is 27 KB per workgroup, and
// both it and the registers (84 VGPRs) allow 5 workgroups per CU.
// Schedule of a tile (reduce2_onepass): the tile's (img, band, strip) decoded on the scalar
// unit by multiply-shift division, one burst of 29 raw loads (s_setprio 2 from kernel entry
// to the burst's 17th load: profiles/r18), one straight-line vertical pass over the band's
// 24 rows (each consumed register pair refetches the row 12 ahead, every wait is a counted
// vmcnt), one barrier (two on strips that touch the image edge), one horizontal pass; the
// kernel ends after its stores, so no wait covers a store.  What else was built and
// measured (other strip widths and LDS pitches, packed taps, cache hints, a loop over
// 12-row chunks) is DESIGN 4.1's to tell.
// ===========================================================================
constexpr int kR = kReduce2ChunkRows;  // output rows per load round (2 ring periods)

struct Reduce2Args {
    const u8 *in;
    u8 *out;
    int w, h, ow, oh;
    int n_strips, n_bands, band_rows;  // band_rows multiple of kR
    // computed output region (demand-driven execution, mipx_runtime.cpp plan_demand):
    // strips from s_base, bands from row y_base (a multiple of kR), clipped at x_end /
    // y_end; the full image is s_base = y_base = 0, x_end = ow, y_end = oh
    int s_base, y_base, x_end, y_end;
    long long in_img, out_img;
    // taps pre-scaled by 1/4096 (exact: powers of two); the bias 2^-13 turns the
    // exact chain into RNE(sum/4096 + 2^-13) == floor(sum/4096 + 0.5) at the cvt
    float c0, c1, c3, c5, bias;
    int remap;       // XCD-aware tile order (MIPX_R2_REMAP=0 disables, for A/B)
    int band_major;  // tile order inside an XCD range (MIPX_R2_ORDER=1: bands fastest)
    // t / n_strips and t / n_bands as (t * mul) >> sh, exact for every t < 2^31
    // (udiv_magic below): the tile decode is a few scalar multiplies
    uint32_t strips_mul, strips_sh, bands_mul, bands_sh;
};

// floor(t / d) == (t * mul) >> sh for every t < 2^31, with l = ceil(log2 d), sh = 31 + l and
// mul = ceil(2^sh / d) < 2^32 (d > 2^(l-1)).  Proof: mul * d = 2^sh + e with 0 <= e < d, so
// t * mul / 2^sh = t / d + t * e / (d * 2^sh); t < 2^31 and e < d <= 2^l give
// t * e < 2^sh, an excess below 1 / d, which cannot carry t / d over the next integer.
inline void udiv_magic(uint32_t d, uint32_t *mul, uint32_t *sh) {
    uint32_t l = 0;
    while (l < 31 && (1u << l) < d) ++l;
    *sh = 31 + l;
    *mul = static_cast<uint32_t>(((1ull << (31 + l)) + d - 1) / d);
}
// on uniform operands: s_mul_i32, s_mul_hi_u32, s_lshr_b64
__device__ __forceinline__ uint32_t udiv_by(uint32_t t, uint32_t mul, uint32_t sh) {
    return static_cast<uint32_t>((static_cast<unsigned long long>(t) * mul) >> sh);
}

typedef float f4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f4v cvt4_once(uint32_t v) {
    return f4v{ubyte_once<0>(v), ubyte_once<1>(v), ubyte_once<2>(v), ubyte_once<3>(v)};
}

// c0 e + c1 (m1 + p1) + c3 (m3 + p3) + c5 (m5 + p5) with pre-scaled taps and the
// bias: every partial is exact on a 1/8192 grid below 2^9, so the result is
// exactly sum/4096 + 2^-13
__device__ __forceinline__ float tap7(float c0, float c1, float c3, float c5, float bias, float e, float m1,
                                      float p1, float m3, float p3, float m5, float p5) {
    float acc = __builtin_fmaf(c0, e, bias);
    acc = __builtin_fmaf(c1, m1 + p1, acc);
    acc = __builtin_fmaf(c3, m3 + p3, acc);
    return __builtin_fmaf(c5, m5 + p5, acc);
}
// v_cvt_pk_u8_f32 rounds to nearest-even and saturates to 0..255; on the
// 1/4096 grid RNE(sum/4096 + 2^-13) == floor(sum/4096 + 0.5) (no ties occur)
__device__ __forceinline__ uint32_t pack4b(float a, float b, float c, float d) {
    uint32_t v = __builtin_amdgcn_cvt_pk_u8_f32(a, 0, 0u);
    v = __builtin_amdgcn_cvt_pk_u8_f32(b, 1, v);
    v = __builtin_amdgcn_cvt_pk_u8_f32(c, 2, v);
    return __builtin_amdgcn_cvt_pk_u8_f32(d, 3, v);
}

// Horizontal pass of the tile, walked by column.  An item is K output pixels of one row: a
// 13-dword window of packed intermediate bytes, each converted once, and one contiguous 12- /
// 8-byte store per lane (bytewise where the row's end clips the item or the address is
// unaligned).  Lane tid < IPR * RPI takes item column j = tid % IPR (IPR = 40 RGB, 60 RGBA)
// and rows u = tid / IPR, + RPI, ... < rows (RPI = 6 / 4: 240 lanes walk 4 / 6 rows); the
// LDS address and the output pointer are computed once and advance by constants, so no
// division or multiply stays in the walk.  The window comes through lds_ops.h as seven
// ds_read_b64 (RGB, 8-byte aligned start) or three ds_read_b128 and a ds_read_b64 (RGBA),
// which the compiler cannot fuse into ds_read2_b64; the last read fetches one dword past
// the window, still inside the row.
template <int B>
__device__ __forceinline__ void reduce2_hwalk(const Reduce2Args &a, int img, const uint32_t *lds, int x0, int y0,
                                              int rows, float c0, float c1, float c3, float c5, float bias) {
    using G = Reduce2Geom<B>;
    constexpr int K = G::K, IPR = G::IPR, RPI = G::RPI, W0 = G::W0, kPitch = kReduce2Pitch;
    const int tid = threadIdx.x;
    const int u0 = tid / IPR;
    const int j = tid - u0 * IPR;
    const int x = x0 + K * j;
    if (u0 >= RPI || x >= a.x_end) return;
    u8 *q = a.out + img * a.out_img + (static_cast<size_t>(y0 + u0) * a.ow + x) * B;
    const size_t qstep = static_cast<size_t>(RPI) * a.ow * B;
    uint32_t la = rc_lds(lds) + static_cast<uint32_t>(u0 * kPitch + W0 * j) * 4u;
    const bool full = x + K <= a.ow;
    for (int u = u0; u < rows; u += RPI, la += RPI * kPitch * 4, q += qstep) {
        uint32_t win[14];
        if constexpr (B == 3) {
            rc_u2 w0 = lds_rd64_at<0>(la), w1 = lds_rd64_at<8>(la), w2 = lds_rd64_at<16>(la),
                  w3 = lds_rd64_at<24>(la), w4 = lds_rd64_at<32>(la), w5 = lds_rd64_at<40>(la),
                  w6 = lds_rd64_at<48>(la);
            lgkm_wait_for<0>(w0, w1, w2, w3, w4, w5, w6);
            win[0] = w0.x, win[1] = w0.y, win[2] = w1.x, win[3] = w1.y, win[4] = w2.x, win[5] = w2.y;
            win[6] = w3.x, win[7] = w3.y, win[8] = w4.x, win[9] = w4.y, win[10] = w5.x, win[11] = w5.y;
            win[12] = w6.x, win[13] = w6.y;
        } else {
            rc_u4 w0 = lds_rd128_at<0>(la), w1 = lds_rd128_at<16>(la), w2 = lds_rd128_at<32>(la);
            rc_u2 w3 = lds_rd64_at<48>(la);
            lgkm_wait_for<0>(w0, w1, w2, w3);
            win[0] = w0.x, win[1] = w0.y, win[2] = w0.z, win[3] = w0.w, win[4] = w1.x, win[5] = w1.y;
            win[6] = w1.z, win[7] = w1.w, win[8] = w2.x, win[9] = w2.y, win[10] = w2.z, win[11] = w2.w;
            win[12] = w3.x, win[13] = w3.y;
        }
        float o[K][B];
#pragma unroll
        for (int c = 0; c < B; ++c) {
            // px[t]: intermediate pixel 2x - 5 + t of channel c
            float px[2 * K + 9];
#pragma unroll
            for (int t = 0; t < 2 * K + 9; ++t) {
                const int lb = B * t + c + G::OFF0;
                const uint32_t dd = win[lb >> 2];
                switch (lb & 3) {
                    case 0: px[t] = ubyte_once<0>(dd); break;
                    case 1: px[t] = ubyte_once<1>(dd); break;
                    case 2: px[t] = ubyte_once<2>(dd); break;
                    default: px[t] = ubyte_once<3>(dd); break;
                }
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int m = 2 * k + 5;
                o[k][c] = tap7(c0, c1, c3, c5, bias, px[m], px[m - 1], px[m + 1], px[m - 3], px[m + 3], px[m - 5],
                               px[m + 5]);
            }
        }
        if (B == 3) {
            const uint32_t d0 = pack4b(o[0][0], o[0][1], o[0][2], o[1][0]);
            const uint32_t d1 = pack4b(o[1][1], o[1][2], o[2][0], o[2][1]);
            const uint32_t d2 = pack4b(o[2][2], o[3][0], o[3][1], o[3][2]);
            if (full && (reinterpret_cast<uintptr_t>(q) & 3u) == 0) {
                *reinterpret_cast<uint3 *>(q) = uint3{d0, d1, d2};
            } else {
                const uint32_t dd[3] = {d0, d1, d2};
                const int nb = (full ? K : a.ow - x) * B;
                for (int i = 0; i < nb; ++i) q[i] = static_cast<u8>(dd[i >> 2] >> (8 * (i & 3)));
            }
        } else {
            const uint32_t d0 = pack4b(o[0][0], o[0][1], o[0][2], o[0][3]);
            const uint32_t d1 = pack4b(o[1][0], o[1][1], o[1][2], o[1][3]);
            uint32_t *q32 = reinterpret_cast<uint32_t *>(q);
            if (full && (reinterpret_cast<uintptr_t>(q) & 7u) == 0) {
                *reinterpret_cast<uint2 *>(q) = uint2{d0, d1};
            } else {
                q32[0] = d0;
                if (full) q32[1] = d1;
            }
        }
    }
}

// Vertical pass of the tile over NR (12 or 24) output rows from y0: one burst of raw
// loads (the five ring rows and the first 12 odd / even pairs, nothing converted before
// all are issued), then NR rows of straight-line code.  A consumed register pair is
// refilled with the row 12 ahead while rows remain, so the 24-row pass keeps 24 loads
// in flight and every wait is a counted one.
template <int B, int NR, class LoadRow>
__device__ __forceinline__ void reduce2_vpass(const LoadRow &load_row, int y0, int tid, float c0, float c1,
                                              float c3, float c5, float bias, uint32_t *L) {
    constexpr int R = kR, ND = Reduce2Geom<B>::ND, kPitch = kReduce2Pitch;
    static_assert(NR == R || NR == kReduce2TileRows, "one or two chunks");
    uint32_t r5[5], odd[R], even[R];
#pragma unroll
    for (int k = 0; k < 5; ++k) r5[k] = load_row(2 * (y0 - 3 + k) + 1);
#pragma unroll
    for (int u = 0; u < R; ++u) {
        odd[u] = load_row(2 * (y0 + u + 2) + 1);
        even[u] = load_row(2 * (y0 + u));
        // the kernel raised this wave's priority at entry; 17 of the burst's 29 loads are out, the
        // rest go at the priority of the waves that compute (measured best, profiles/r18)
        if (u == R / 2 - 1) __builtin_amdgcn_s_setprio(0);
    }
    // odd-row ring: slot s holds odd row 2m+1 with m = s (mod 6); y0 % 6 == 0
    f4v ring[6];
    ring[3] = cvt4_once(r5[0]);
    ring[4] = cvt4_once(r5[1]);
    ring[5] = cvt4_once(r5[2]);
    ring[0] = cvt4_once(r5[3]);
    ring[1] = cvt4_once(r5[4]);
    ring[2] = f4v{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NR; ++u) {
        const int s = u % R;
        ring[(u + 2) % 6] = cvt4_once(odd[s]);
        const f4v e = cvt4_once(even[s]);
        if (u + R < NR) {  // rotate: this register pair now fetches the row 12 ahead
            odd[s] = load_row(2 * (y0 + R + u + 2) + 1);
            even[s] = load_row(2 * (y0 + R + u));
        }
        const f4v m5 = ring[(u + 3) % 6], m3 = ring[(u + 4) % 6], m1 = ring[(u + 5) % 6];
        const f4v p1 = ring[u % 6], p3 = ring[(u + 1) % 6], p5 = ring[(u + 2) % 6];
        const uint32_t d = pack4b(tap7(c0, c1, c3, c5, bias, e.x, m1.x, p1.x, m3.x, p3.x, m5.x, p5.x),
                                  tap7(c0, c1, c3, c5, bias, e.y, m1.y, p1.y, m3.y, p3.y, m5.y, p5.y),
                                  tap7(c0, c1, c3, c5, bias, e.z, m1.z, p1.z, m3.z, p3.z, m5.z, p5.z),
                                  tap7(c0, c1, c3, c5, bias, e.w, m1.w, p1.w, m3.w, p3.w, m5.w, p5.w));
        if (tid < ND) L[u * kPitch + tid] = d;  // ND <= 256 lanes hold a row's dwords
    }
}

// One tile: its 24 rows go through one load burst, one vertical pass, one barrier and one
// horizontal pass.  The LDS is one 24-row image of packed intermediate bytes; the kernel
// ends after its output stores, so no wait covers a store.  A band of at most 12 rows (the
// last tile of a window, a short image) takes the 12-row vertical pass.
template <int B>
__device__ __forceinline__ void reduce2_onepass(const Reduce2Args &a, int img, int strip, int band,
                                                uint32_t *lds) {
    using G = Reduce2Geom<B>;
    constexpr int kThreads = kReduce2Threads, kPitch = kReduce2Pitch;
    constexpr int TW = G::TW;
    const int tid = threadIdx.x;
    const int x0 = (a.s_base + strip) * TW;
    const int row_bytes = a.w * B;
    const int px0 = 2 * x0 - 5;          // first intermediate pixel of the strip
    const int base = (B * px0) & ~3;     // floor to a dword (two's complement)
    const int byte0 = base + 4 * tid;
    const bool vlane = tid < G::ND && byte0 >= 0 && byte0 + 4 <= row_bytes;
    // raw buffer loads: per-lane byte offset in voffset, row offset in soffset;
    // lanes outside the row get an out-of-range voffset and read 0
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<u8 *>(a.in + img * a.in_img), 0, static_cast<int>(a.in_img), 0x00020000);
    const uint32_t voff = vlane ? static_cast<uint32_t>(byte0) : 0x80000000u;
    const int y0 = a.y_base + band * a.band_rows;
    const int y1 = min(y0 + a.band_rows, a.y_end);
    const int rows = y1 - y0;            // 1 .. 24
    const float c0 = a.c0, c1 = a.c1, c3 = a.c3, c5 = a.c5, bias = a.bias;
    // strip pixels outside the image (COPY edge): LDS pixels [0, nl) copy pixel 0,
    // [fr, fr_end] copy pixel w-1; filled after the vertical pass
    const int nl = px0 < 0 ? -px0 : 0;
    const int x_last = min(x0 + TW, a.x_end) - 1;
    const int fr = a.w - px0;                                   // LDS index of pixel w
    const int fr_end = min(2 * x_last + 5 - px0, G::NPX - 1);   // last LDS pixel read
    const int nr = fr_end >= fr ? fr_end - fr + 1 : 0;

    auto load_row = [&](int r) -> uint32_t {
        r = clampi(r, 0, a.h - 1);
        return static_cast<uint32_t>(__builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, r * row_bytes, 0));
    };
    // ---- vertical pass: all intermediate rows of the tile -> LDS (packed uchar) ----
    if (rows > kR) reduce2_vpass<B, kReduce2TileRows>(load_row, y0, tid, c0, c1, c3, c5, bias, lds);
    else reduce2_vpass<B, kR>(load_row, y0, tid, c0, c1, c3, c5, bias, lds);
    if (nl > 0 || nr > 0) {  // replicate the edge pixels (EXTEND_COPY) inside the LDS image
        __syncthreads();
        u8 *Lb = reinterpret_cast<u8 *>(lds);
        const int nfill = nl + nr;
        for (int i = tid; i < rows * nfill * B; i += kThreads) {
            const int u = i / (nfill * B);
            const int rem = i - u * nfill * B;
            const int f = rem / B, c = rem - f * B;
            const int dst = f < nl ? f : fr + (f - nl);
            const int srcp = f < nl ? nl : fr - 1;
            Lb[u * kPitch * 4 + B * dst + G::OFF0 + c] = Lb[u * kPitch * 4 + B * srcp + G::OFF0 + c];
        }
    }
    __syncthreads();
    // ---- horizontal pass: 2 K output pixels per item, lanes walk down item columns ----
    reduce2_hwalk<B>(a, img, lds, x0, y0, rows, c0, c1, c3, c5, bias);
}

// The centre sampling convention's 2 x 2 reduce is k_reduce2m (k_reduce2m.hip); its
// all-VALU predecessor k_reduce2c (r04, 1.84-1.88 ms per C2 step) was removed once the
// matrix-core kernel beat it, its measurements are under profiles/r04/reduce2c/.

// ID is the build's recorded identity in profiles/ and in the benchmark, not a selector.
template <int B, int ID>
__global__ void __launch_bounds__(kReduce2Threads) k_reduce2x2(Reduce2Args a) {
    static_assert(ID == 66, "k_reduce2x2<B, 66> is the one build");
    __shared__ __attribute__((aligned(16))) uint32_t lds[kReduce2TileRows * kReduce2Pitch];
    // A new tile is the youngest wave on its SIMD and would queue for issue behind the older
    // waves' arithmetic; it runs above them through the tile decode and the first 17 loads of
    // its burst (reduce2_vpass lowers it again), so its rows are on their way early
    __builtin_amdgcn_s_setprio(2);
    const uint32_t t = a.remap ? xcd_remap(blockIdx.x, gridDim.x) : blockIdx.x;
    // t -> (img, band, strip) by exact multiply-shift division: all uniform, so it stays on
    // the scalar unit (a plain / would go through the vector float reciprocal, and every
    // load address waits on it)
    int strip, band, img;
    if (a.band_major) {  // tiles ordered (img, strip, band): vertical neighbours adjacent
        const uint32_t rest = udiv_by(t, a.bands_mul, a.bands_sh);
        band = static_cast<int>(t - rest * static_cast<uint32_t>(a.n_bands));
        img = static_cast<int>(udiv_by(rest, a.strips_mul, a.strips_sh));
        strip = static_cast<int>(rest - static_cast<uint32_t>(img) * static_cast<uint32_t>(a.n_strips));
    } else {             // (img, band, strip): horizontal neighbours adjacent
        const uint32_t rest = udiv_by(t, a.strips_mul, a.strips_sh);
        strip = static_cast<int>(t - rest * static_cast<uint32_t>(a.n_strips));
        img = static_cast<int>(udiv_by(rest, a.bands_mul, a.bands_sh));
        band = static_cast<int>(rest - static_cast<uint32_t>(img) * static_cast<uint32_t>(a.n_bands));
    }
    reduce2_onepass<B>(a, img, strip, band, lds);
}

}  // namespace

// ===========================================================================
// launchers
// ===========================================================================
int reducev_launch(const u8 *in, u8 *out, int n, int w, int h, int b, double vshrink, hipStream_t st) {
    SepSpec spec;
    if (!sep_spec_reduce(vshrink, &spec)) return MIPX_EDEVICE;
    SepWindow win{};
    win.bands = b;
    win.in_pitch = w * b;
    win.in_base = 0;
    win.in_img = img_bytes(w, h, b);
    win.in_len = h;
    win.o0 = 0;
    win.out_w = w;
    win.out_h = out_size_reduce(h, vshrink);
    return vpass_launch(in, out, n, spec, win, st);
}

int reduceh_launch(const u8 *in, u8 *out, int n, int w, int h, int b, double hshrink, hipStream_t st) {
    SepSpec spec;
    if (!sep_spec_reduce(hshrink, &spec)) return MIPX_EDEVICE;
    SepWindow win{};
    win.bands = b;
    win.in_pitch = w * b;
    win.in_base = 0;
    win.in_img = img_bytes(w, h, b);
    win.in_len = w;
    win.o0 = 0;
    win.out_w = out_size_reduce(w, hshrink);
    win.out_h = h;
    return hpass_launch(in, out, n, spec, win, st);
}

// Both shrinks > 1 in one launch, output window [ox0, ox0 + ow) x [oy0, oy0 + oh):
// the column walker k_rcol (matrix cores, LDS row ring; dword-aligned input rows,
// <= 16 taps) first, then k_rmf2 (matrix cores, rows of any alignment), then the
// small-image strip walker and fused kernel (> 16 taps); MIPX_EUNSUPPORTED leaves it
// to the two separable passes.  MIPX_RCOL=0 / MIPX_RMFMA=0 turn the first two off
// (A/B); MIPX_RSTRIP=1 puts the strip walker first.
int reduce_one_launch(const u8 *in, u8 *out, int n, int w, int h, int b, double hs, double vs, int ox0, int oy0,
                      int ow, int oh, hipStream_t st) {
    const char *ef = tune_env("MIPX_RSTRIP");
    const bool strip_first = ef && *ef == '1';
    if (strip_first) {
        const int se = reduce_strip_launch(in, out, n, w, h, b, hs, vs, ox0, oy0, ow, oh, st);
        if (se != MIPX_EUNSUPPORTED) return se;
    }
    const char *ec = tune_env("MIPX_RCOL");
    if (!(ec && *ec == '0')) {
        const int ce = reduce_col_launch(in, out, n, w, h, b, hs, vs, ox0, oy0, ow, oh, st);
        if (ce != MIPX_EUNSUPPORTED) return ce;
    }
    const int me = reduce_mfma_launch(in, out, n, w, h, b, hs, vs, ox0, oy0, ow, oh, st);
    if (me != MIPX_EUNSUPPORTED) return me;
    if (!strip_first) {
        const int se = reduce_strip_launch(in, out, n, w, h, b, hs, vs, ox0, oy0, ow, oh, st);
        if (se != MIPX_EUNSUPPORTED) return se;
    }
    return reduce_fused_launch(in, out, n, w, h, b, hs, vs, ox0, oy0, ow, oh, st);
}

// vips_reduce followed by vips_extract_area(left, top, ow, oh): only the
// window's output rows (vertical pass) and columns (horizontal pass) are
// computed.  Every output is the same sum over the same input pixels, so the
// result is identical to reduce-then-extract, minus the discarded work and the
// extract pass.  ws: n * w * oh * b bytes when both shrinks are > 1.
int reduce_window_launch(const u8 *in, u8 *out, int n, int w, int h, int b, double hs, double vs, int left,
                         int top, int ow, int oh, void *ws, size_t ws_bytes, hipStream_t st) {
    const int rw = hs > 1.0 ? out_size_reduce(w, hs) : w;
    const int rh = vs > 1.0 ? out_size_reduce(h, vs) : h;
    if (left < 0 || top < 0 || ow <= 0 || oh <= 0 || left + ow > rw || top + oh > rh) return MIPX_EINVAL;
    const long long in_img = img_bytes(w, h, b);
    SepSpec sv, sh;
    if (vs > 1.0 && !sep_spec_reduce(vs, &sv)) return MIPX_EDEVICE;
    if (hs > 1.0 && !sep_spec_reduce(hs, &sh)) return MIPX_EDEVICE;
    if (vs > 1.0 && hs > 1.0) {
        const int fe = reduce_one_launch(in, out, n, w, h, b, hs, vs, left, top, ow, oh, st);
        if (fe != MIPX_EUNSUPPORTED) return fe;
        const size_t need = align_up(static_cast<size_t>(n) * w * oh * b);
        if (!ws || ws_bytes < need) return MIPX_EINVAL;
        u8 *tmp = static_cast<u8 *>(ws);
        const SepWindow v{b, w * b, 0, in_img, h, top, w, oh};
        int e = vpass_launch(in, tmp, n, sv, v, st);
        if (e) return e;
        const SepWindow hw{b, w * b, 0, img_bytes(w, oh, b), w, left, ow, oh};
        return hpass_launch(tmp, out, n, sh, hw, st);
    }
    if (vs > 1.0) {
        const SepWindow v{b, w * b, static_cast<long long>(left) * b, in_img, h, top, ow, oh};
        return vpass_launch(in, out, n, sv, v, st);
    }
    if (hs > 1.0) {
        const SepWindow hw{b, w * b, static_cast<long long>(top) * w * b, in_img, w, left, ow, oh};
        return hpass_launch(in, out, n, sh, hw, st);
    }
    return extract_launch(in, out, n, w, h, b, left, top, ow, oh, st);
}

// Is the phase-0 mask of shrink 2 the 7-nonzero symmetric shape the fused
// kernel hard-wires?  Returns the four distinct taps.
bool reduce2_taps(float c[4]) {
    std::vector<int> t;
    reduce_table(2.0, t);
    const int n = reduce_points(2.0);
    if (n != 13) return false;
    const int *r = t.data();  // phase 0
    static const int zero[] = {1, 3, 7, 9, 11, 12};
    for (int z : zero)
        if (r[z] != 0) return false;
    if (r[4] != r[6] || r[2] != r[8] || r[0] != r[10]) return false;
    c[0] = static_cast<float>(r[5]);
    c[1] = static_cast<float>(r[4]);
    c[2] = static_cast<float>(r[2]);
    c[3] = static_cast<float>(r[0]);
    return true;
}

// The centre convention's phase-64 mask: 12 non-zero taps symmetric about 5.5 and a
// zero tap 12 (k_reduce2m).  Returns t_0..t_5.
bool reduce2c_taps(float t[6]) {
    std::vector<int> tab;
    reduce_table(2.0, tab);
    const int n = reduce_points(2.0);
    if (n != 13) return false;
    const int *r = tab.data() + 64 * n;
    if (r[12] != 0) return false;
    for (int i = 0; i < 6; ++i) {
        if (r[i] != r[11 - i]) return false;
        t[i] = static_cast<float>(r[i]);
    }
    return true;
}


// Fused path applies to shrink exactly 2 x 2 on 3- or 4-band images whose rows
// are dword aligned: k_reduce2x2 at the corner convention, k_reduce2m at the centre one.
bool reduce2_eligible(const u8 *in, int w, int h, int b, double hs, double vs) {
    if (hs != 2.0 || vs != 2.0) return false;
    const char *e2 = tune_env("MIPX_REDUCE2");  // 0: leave 2 x 2 to the generic reduce (A/B)
    if (e2 && *e2 == '0') return false;
    if (b != 3 && b != 4) return false;
    if ((w * b) % 4 != 0 || (reinterpret_cast<uintptr_t>(in) % 4) != 0) return false;
    if (w < 8 || h < 8) return false;
    if (reduce_centre()) {
        static const bool centre_ok = [] { float t[6]; return reduce2c_taps(t); }();
        return centre_ok;
    }
    static const bool shape_ok = [] { float c[4]; return reduce2_taps(c); }();
    return shape_ok;
}

int reduce2_launch(const u8 *in, u8 *out, int n, int w, int h, int b, hipStream_t st) {
    return reduce2_window_launch(in, out, n, w, h, b, 0, 0, out_size_reduce(w, 2.0), out_size_reduce(h, 2.0), st);
}

// Only the output region [x0, x1) x [y0, y1) is computed (rounded out to whole
// strips and 12-row chunks); the rest of the full-size output is left as it was.
// Every computed pixel is the same sum as in the full launch.  One workgroup per tile of
// reduce2_launch_geom's strips x bands (reduce2_geom.h) and image; MIPX_R2_REMAP and
// MIPX_R2_ORDER set the order the tile index walks them in.
int reduce2_window_launch(const u8 *in, u8 *out, int n, int w, int h, int b, int x0, int y0, int x1, int y1,
                          hipStream_t st) {
    if (reduce_centre()) {  // k_reduce2m: both passes on the matrix cores
        float tf[6];
        if (!reduce2c_taps(tf)) return MIPX_EINVAL;
        int taps[12];
        for (int i = 0; i < 6; ++i) taps[i] = taps[11 - i] = static_cast<int>(tf[i]);
        return reduce2m_window_launch(in, out, n, w, h, b, x0, y0, x1, y1, taps, st);
    }
    float c[4];
    if (!reduce2_taps(c)) return MIPX_EINVAL;
    Reduce2Launch g;
    if (!reduce2_launch_geom(w, h, b, x0, y0, x1, y1, &g)) return MIPX_EINVAL;
    Reduce2Args a{};
    a.in = in;
    a.out = out;
    a.w = w;
    a.h = h;
    a.ow = g.ow;
    a.oh = g.oh;
    a.s_base = g.s_base;
    a.x_end = g.x_end;
    a.y_base = g.y_base;
    a.y_end = g.y_end;
    a.n_strips = g.n_strips;
    a.band_rows = g.band_rows;
    a.n_bands = g.n_bands;
    a.in_img = img_bytes(w, h, b);
    a.out_img = img_bytes(a.ow, a.oh, b);
    a.c0 = c[0] / 4096.0f;
    a.c1 = c[1] / 4096.0f;
    a.c3 = c[2] / 4096.0f;
    a.c5 = c[3] / 4096.0f;
    a.bias = 1.0f / 8192.0f;
    const char *er = tune_env("MIPX_R2_REMAP");
    a.remap = (er && *er) ? std::atoi(er) : 1;
    const char *eo = tune_env("MIPX_R2_ORDER");
    a.band_major = (eo && *eo) ? std::atoi(eo) : 0;
    const long long tiles = g.tiles_per_image() * n;
    if (tiles > 0x7fffffffLL) return MIPX_EINVAL;  // also what the decode's divisions rely on
    udiv_magic(static_cast<uint32_t>(a.n_strips), &a.strips_mul, &a.strips_sh);
    udiv_magic(static_cast<uint32_t>(a.n_bands), &a.bands_mul, &a.bands_sh);
    const dim3 grid(static_cast<unsigned>(tiles)), blk(kReduce2Threads);
    if (b == 3) hipLaunchKernelGGL((k_reduce2x2<3, 66>), grid, blk, 0, st, a);
    else hipLaunchKernelGGL((k_reduce2x2<4, 66>), grid, blk, 0, st, a);
    return launch_check("k_reduce2x2");
}

}  // namespace mipx
