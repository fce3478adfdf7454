// k_jpege.hip — a JPEG encoder's back half on gfx950 (PARITY_ASSUMPTIONS.md row 21): the quantised
// coefficients k_jpegc.hip writes in, the finished entropy-coded scan out, one slot per image
// (include/mipx.h, MIPX_OP_JPEGE): baseline Huffman coding with the Annex K.3 tables, one
// interleaved scan, libjpeg's dummy blocks, 1-padding, 0xFF stuffing.  Integer only; the output
// does not depend on the order workgroups run in.
//
// A block's bits depend on the block and on the DC of the block before it in scan order, and
// both are in memory, so nothing is serial but two prefix sums: of the blocks' bit counts (where a
// block starts) and of the 0xFF bytes (where a byte lands after stuffing).  Every dependency
// between workgroups is a launch boundary on the stream; no kernel waits for another workgroup.
//   memset           the per-image records and the unstuffed streams (the pack kernel ORs into them)
//   k_jpege_count    one lane per block of the scan, dummy blocks included, kJpegeTile blocks per
//                    workgroup: its bit count, the tile's sum, a flag for a value without a code
//   k_jpege_scan<0>  one workgroup per image over the tile sums (a few hundred): where each tile
//                    starts, the scan's bits, and the verdict: uncodable, or too long for the slot
//   k_jpege_pack     the same lanes code their blocks again, now at their bit offset, into the
//                    unstuffed stream: whole words by plain stores, a block's first and last
//                    word by a 32-bit atomic OR (order-independent); the last block pads with 1s
//   k_jpege_ffcount  0xFF bytes per kJpegeChunk bytes of stream
//   k_jpege_scan<1>  one workgroup per image over those counts: the final length, overflow again
//   k_jpege_stuff    bytes to the slot with the 0x00s inserted, every store checked against the
//                    capacity; the header
// Images whose verdict is not "ok" are skipped by every later kernel but for the header.
//
// Packed output (mipx_op_*_scan_packed, the request path's download): the slots stand back to back,
// each rounded up to 16 bytes, instead of a capacity apart.  Every image's final length is known
// after k_jpege_scan<1>, before a byte of output is stored, so one launch goes in between and no
// byte moves twice:
//   k_jpege_place    one workgroup over the n images: the directory, n + 1 byte offsets, off[i + 1] =
//                    off[i] + align16(head + length), a slot that is not "ok" being its header alone
// and k_jpege_stuff<true> takes a slot's base from the directory and stores nothing but the header
// and `length` bytes.  With optimised tables k_jpege_tables<true> parks the four DHTs in the image's
// histogram, which it has read by then, and k_jpege_stuff<true> copies them behind the header: no
// launch more than that one.
//
// With optimised tables (PARITY_ASSUMPTIONS.md row 24) two launches go in front, and the count and
// pack kernels read the image's own codes from the workspace instead of the Annex K ones:
//   k_jpege_hist     the same lanes walk their blocks once and count the symbols: a histogram of
//                    4 tables x 256 per workgroup in LDS, then its non-zero bins into the image's by
//                    integer atomic adds (sums do not depend on the order)
//   k_jpege_tables   one workgroup per image, one wave per table: libjpeg's jpeg_gen_optimal_table,
//                    the code tables into the workspace and the four DHTs into the slot's header
//
// The count and pack kernels stage their tile's blocks through LDS with coalesced 16-byte loads
// (8 lanes per block), blocks 33 dwords apart, so that the lanes of a wave, each walking its own
// block in zigzag order, read 32 different banks.  Scan order is not memory order (4:2:0
// interleaves two Y block rows and both chroma planes), but every block is one whole 128-byte line.
// Coefficients and slots start on any byte: global accesses to them are plain unaligned ones.
//
// MIPX_YCC_GREY (PARITY_ASSUMPTIONS.md row 26): the scan of one component is not interleaved.  Block
// s of the scan is block s of Y's grid in raster order, every block is real, the predictor is the
// block before, and tables 0 code everything.  With optimised tables the histograms of DC 1 and AC 1
// stay zero; see k_jpege_tables for what its two waves then do.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "jpeg_scan.h"

namespace mipx {
namespace {

using namespace dev;
using namespace jscan;

constexpr uint32_t kTile = kJpegeTile;    // threads of every kernel here, and blocks per tile
constexpr uint32_t kChunk = kJpegeChunk;  // stream bytes per workgroup: a dword per lane
constexpr uint32_t kPitch = 33;           // dwords between two blocks in LDS
constexpr uint32_t kNone = 0xffffffffu;
static_assert(kChunk == 4 * kTile, "a dword of stream per lane");
static_assert(kTile == 256, "block_scan sums four waves");

struct JpegeInfo {  // per image, zeroed every call
    unsigned long long bits;  // the scan before padding and stuffing
    uint32_t ff;              // its 0xFF bytes
    uint32_t status;          // MIPX_JPEG_SCAN_*
    uint32_t flags;           // 1: a coefficient without a code
    uint32_t pad[3];
};
static_assert(sizeof(JpegeInfo) == 32, "JpegeWork sizes the records");

struct JpegeArgs {
    const u8 *coefs;  // cap bytes per image
    u8 *out;          // 16 + cap bytes per image
    const uint32_t *codes;  // build_jpege_codes, or k_jpege_tables' in the workspace
    uint32_t codes_stride;  // words between two images' codes: 0 (Annex K for all), or 4 tables' worth
    uint32_t head;          // bytes of a slot in front of its scan
    uint32_t *hist;         // optimised tables only: 4 x 256 symbol counts per image, in the codes' order
    uint32_t *opt_codes;    // ... and the codes made of them
    JpegeInfo *info;
    uint32_t *stream;  // cap bytes per image
    uint32_t *counts;
    uint32_t *tile_sums;
    unsigned long long *tile_offs;
    uint32_t *chunk_sums;
    unsigned long long *chunk_offs;
    uint32_t cap;             // bytes of one image's coefficients = the capacity of its scan
    uint32_t ywb, yhb;        // real Y blocks across and down
    uint32_t mw;              // MCUs across
    uint32_t cb_off, cr_off;  // byte offsets of the Cb and Cr coefficients
    uint32_t blocks, tiles, chunks;  // per image: blocks of the scan, tiles of them, chunks of the stream
    unsigned long long *dir;  // packed output only: n + 1 byte offsets of the slots in `out`
    uint32_t n;               // images
};

__device__ __forceinline__ int load_i16(const u8 *p) {
    int16_t v;
    __builtin_memcpy(&v, p, 2);
    return v;
}

// Block s of the scan: the byte offset of the block its DC comes from (itself, or for a dummy block
// the real block libjpeg copies it from), whether it is real, which tables code it, and the block
// before it of the same component (kNone: the component's first, predicted from 0).
// Its own copy of the scan's block order, which jpeg_scan.h's scan_block states for k_jpegh.hip's
// block_dst: built on that one the optimised-table coder measured 0.1 to 0.25 % slower (profiles/r16).
template <int LAYOUT>
__device__ __forceinline__ uint32_t block_src(const JpegeArgs &a, uint32_t s, bool *real, uint32_t *chroma,
                                              uint32_t *prev) {
    if (LAYOUT == MIPX_YCC_GREY) {  // an MCU is a block; no dummy blocks
        *real = true, *chroma = 0u;
        *prev = s ? s - 1u : kNone;
        return s * 128u;
    }
    if (LAYOUT == MIPX_YCC_444) {  // Y Cb Cr per MCU; MCUs are the blocks in raster order
        const uint32_t m = s / 3u, c = s - 3u * m;
        *real = true, *chroma = c ? 1u : 0u;
        *prev = m ? s - 3u : kNone;
        return (c == 0u ? 0u : c == 1u ? a.cb_off : a.cr_off) + m * 128u;
    }
    const uint32_t m = s / 6u, j = s - 6u * m;  // Y00 Y01 Y10 Y11 Cb Cr
    if (j >= 4u) {
        *real = true, *chroma = 1u;
        *prev = m ? s - 6u : kNone;
        return (j == 4u ? a.cb_off : a.cr_off) + m * 128u;
    }
    *chroma = 0u;
    *prev = j ? s - 1u : (m ? s - 3u : kNone);
    const uint32_t my = m / a.mw, mx = m - my * a.mw;
    uint32_t by = 2u * my + (j >> 1), bx = 2u * mx + (j & 1u);
    *real = by < a.yhb && bx < a.ywb;
    if (by >= a.yhb) by -= 1u, bx = 2u * mx + 1u;  // a dummy row: the last block of the MCU's row above
    if (bx >= a.ywb) bx = a.ywb - 1u;               // a dummy column: the block to the left
    return (by * a.ywb + bx) * 128u;
}

// What a lane knows of its block once the tile is staged.
struct Lane {
    bool real;  // its coefficients are staged; a dummy block has only the DC
    int dc, pred;
    uint32_t chroma;
    bool valid;  // a block of the scan (the last tile has lanes past it)
};

// Stages the tile's real blocks into `blk` and describes the lane's own one.  Ends with a barrier.
template <int LAYOUT>
__device__ __forceinline__ Lane stage_tile(const JpegeArgs &a, const u8 *coefs, uint32_t tile, uint32_t *blk,
                                           uint32_t *src) {
    const uint32_t tid = threadIdx.x, s = tile * kTile + tid;
    Lane me;
    me.valid = s < a.blocks;
    me.real = false, me.dc = 0, me.pred = 0, me.chroma = 0;
    uint32_t mine = kNone;
    if (me.valid) {
        bool preal;
        uint32_t prev, pchroma, pprev;
        const uint32_t off = block_src<LAYOUT>(a, s, &me.real, &me.chroma, &prev);
        me.dc = load_i16(coefs + off);
        if (prev != kNone) me.pred = load_i16(coefs + block_src<LAYOUT>(a, prev, &preal, &pchroma, &pprev));
        if (me.real) mine = off;
    }
    src[tid] = mine;
    __syncthreads();
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {  // 8 lanes load a block's 128 bytes
        const uint32_t t = tid + kTile * i, b = t >> 3, part = t & 7u;
        const uint32_t off = src[b];
        if (off == kNone) continue;
        uint4 v;
        __builtin_memcpy(&v, coefs + off + part * 16u, 16);  // any alignment: one global_load_dwordx4
        uint32_t *d = blk + b * kPitch + part * 4u;
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    __syncthreads();
    return me;
}

__device__ __forceinline__ uint32_t bit_length(uint32_t v) { return v ? 32u - __builtin_clz(v) : 0u; }

// Walks one block (coef: its staged coefficients, natural order) and hands `sink` its symbols:
// sink.dc(size, low) for the DC category, sink.ac(run << 4 | size, size, low) per coded coefficient
// and for EOB (0, 0, 0), sink.zrl() per 0xF0; `low` are the `size` bits behind the code.  True when a
// value had no code.  Such a value is coded as the largest category, so that counting and packing
// still agree.
// The walker has a coefficient's size in a register when it makes the symbol, so it hands it over:
// a sink does not take it out of the symbol again per coefficient.
template <class Sink>
__device__ __forceinline__ bool walk_block(const Lane &me, const int16_t *coef, Sink &sink) {
    bool bad = false;
    {
        const int d = me.dc - me.pred;
        uint32_t size = bit_length(static_cast<uint32_t>(d < 0 ? -d : d));
        if (size > 11u) bad = true, size = 11u;
        sink.dc(size, static_cast<uint32_t>(d < 0 ? d - 1 : d) & ((1u << size) - 1u));
    }
    uint32_t run = 0;
    if (me.real) {
        for (uint32_t k0 = 1; k0 < 64u; k0 += 7u) {  // 9 groups of 7: the group's LDS reads go out together
            int group[7];
#pragma unroll
            for (uint32_t j = 0; j < 7u; ++j) group[j] = coef[kZigzag[k0 + j]];
#pragma unroll
            for (uint32_t j = 0; j < 7u; ++j) {
                const int v = group[j];
                if (v == 0) {
                    ++run;
                    continue;
                }
                for (; run > 15u; run -= 16u) sink.zrl();
                uint32_t size = bit_length(static_cast<uint32_t>(v < 0 ? -v : v));
                if (size > 10u) bad = true, size = 10u;
                sink.ac(run << 4 | size, size, static_cast<uint32_t>(v < 0 ? v - 1 : v) & ((1u << size) - 1u));
                run = 0;
            }
        }
    } else {
        run = 63;
    }
    if (run) sink.ac(0u, 0u, 0u);  // EOB, unless coefficient 63 is coded
    return bad;
}

// The three sinks.  The two that need codes take the block's pair of tables (DC, then AC) in LDS.
struct HistSink {  // counts into the workgroup's histogram: the block's DC table, then its AC table
    uint32_t *hist;
    __device__ __forceinline__ void dc(uint32_t sym, uint32_t) { atomicAdd(hist + sym, 1u); }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t, uint32_t) { atomicAdd(hist + kJpegeCodesPerTable + sym, 1u); }
    __device__ __forceinline__ void zrl() { atomicAdd(hist + kJpegeCodesPerTable + 0xf0u, 1u); }
};

struct CountSink {
    const uint32_t *dc_codes, *ac_codes;
    uint32_t zrl_bits;
    uint32_t bits = 0;
    __device__ __forceinline__ CountSink(const uint32_t *codes)
        : dc_codes(codes), ac_codes(codes + kJpegeCodesPerTable), zrl_bits(ac_codes[0xf0] >> 16) {}
    __device__ __forceinline__ void dc(uint32_t sym, uint32_t) { bits += (dc_codes[sym] >> 16) + sym; }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t size, uint32_t) { bits += (ac_codes[sym] >> 16) + size; }
    __device__ __forceinline__ void zrl() { bits += zrl_bits; }
};

// Bits into the image's unstuffed stream from bit `at` on, most significant first.  The stream is
// bytes; a word holds 4 of them little-endian, so a word of 32 stream bits is stored byte-swapped.
struct PackSink {
    const uint32_t *dc_codes, *ac_codes;
    uint32_t zrl_code;
    uint32_t *words;
    uint32_t limit;  // words of the stream
    uint32_t wi, fill;
    unsigned long long acc;
    bool first = true;
    __device__ __forceinline__ PackSink(const uint32_t *codes, uint32_t *w, uint32_t lim, unsigned long long at)
        : dc_codes(codes), ac_codes(codes + kJpegeCodesPerTable), zrl_code(ac_codes[0xf0]), words(w), limit(lim),
          wi(static_cast<uint32_t>(at >> 5)), fill(static_cast<uint32_t>(at) & 31u), acc(0) {}
    __device__ __forceinline__ void dc(uint32_t sym, uint32_t low) {
        const uint32_t e = dc_codes[sym];
        put((e & 0xffffu) << sym | low, (e >> 16) + sym);
    }
    __device__ __forceinline__ void ac(uint32_t sym, uint32_t size, uint32_t low) {
        const uint32_t e = ac_codes[sym];
        put((e & 0xffffu) << size | low, (e >> 16) + size);
    }
    __device__ __forceinline__ void zrl() { put(zrl_code & 0xffffu, zrl_code >> 16); }
    __device__ __forceinline__ void put(uint32_t v, uint32_t count) {  // count <= 27
        acc = acc << count | v;
        fill += count;
        if (fill >= 32u) {
            fill -= 32u;
            const uint32_t w = __builtin_bswap32(static_cast<uint32_t>(acc >> fill));
            acc &= (1ull << fill) - 1ull;
            if (wi < limit) {
                if (first) atomicOr(words + wi, w);  // shared with the block before
                else words[wi] = w;                  // all 32 bits are this block's
            }
            first = false;
            ++wi;
        }
    }
    __device__ __forceinline__ void finish() {  // the last, partial word: shared with the block after
        if (fill && wi < limit) atomicOr(words + wi, __builtin_bswap32(static_cast<uint32_t>(acc << (32u - fill))));
    }
};

__device__ __forceinline__ void load_codes(const JpegeArgs &a, uint32_t img, uint32_t *codes) {
    const uint32_t *from = a.codes + static_cast<size_t>(img) * a.codes_stride;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) codes[threadIdx.x + kTile * i] = from[threadIdx.x + kTile * i];
}

// ---- optimised tables: the symbols' histogram, then libjpeg's jpeg_gen_optimal_table ----------
template <int LAYOUT>
__global__ void __launch_bounds__(kTile) k_jpege_hist(const JpegeArgs a) {
    __shared__ uint32_t blk[kTile * kPitch];
    __shared__ uint32_t hist[4 * kJpegeCodesPerTable];
    __shared__ uint32_t src[kTile];
    const uint32_t img = blockIdx.y, tile = blockIdx.x;
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) hist[threadIdx.x + kTile * i] = 0u;
    const Lane me = stage_tile<LAYOUT>(a, a.coefs + static_cast<size_t>(img) * a.cap, tile, blk, src);  // barriers
    bool bad = false;
    if (me.valid) {
        HistSink sink{hist + me.chroma * 2u * kJpegeCodesPerTable};
        bad = walk_block(me, reinterpret_cast<const int16_t *>(blk + threadIdx.x * kPitch), sink);
    }
    __syncthreads();
    uint32_t *mine = a.hist + static_cast<size_t>(img) * (4u * kJpegeCodesPerTable);
#pragma unroll
    for (uint32_t i = 0; i < 4u; ++i) {
        const uint32_t v = hist[threadIdx.x + kTile * i];
        if (v) atomicAdd(mine + threadIdx.x + kTile * i, v);
    }
    if (bad) atomicOr(&a.info[img].flags, 1u);
}

constexpr uint32_t kMaxLen = 63;  // code lengths before the limiting: below 44 for counts that sum below 2^30
constexpr unsigned long long kNoKey = ~0ull;

// The two least of four keys, a1 < a2 and b1 < b2 (or kNoKey), into a1 < a2.
__device__ __forceinline__ void least_two(unsigned long long &a1, unsigned long long &a2, unsigned long long b1,
                                          unsigned long long b2) {
    const unsigned long long lo = a1 < b1 ? a1 : b1, hi = a1 < b1 ? b1 : a1, rest = a2 < b2 ? a2 : b2;
    a1 = lo, a2 = hi < rest ? hi : rest;
}

__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int mask) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), mask), hi = __shfl_xor(static_cast<uint32_t>(v >> 32), mask);
    return static_cast<unsigned long long>(hi) << 32 | lo;
}

// One workgroup per image, wave t on table t of the histogram (DC 0, AC 0, DC 1, AC 1).  A lane keeps
// five of the 257 frequencies (index lane + 64 j; 256 is the reserved point) in registers with, per
// entry, its code size and the root of the tree it is in.  A merge is one butterfly over the key
// frequency << 9 | 256 - index, whose two least values are the library's c1 and c2 (least frequency,
// then largest index); every entry of either tree then grows by one bit and joins c1's, which is
// what the library's walk along its `others` chains does.  The waves run different numbers of merges
// and meet again at the barriers behind them.
// A table no symbol was counted into (MIPX_YCC_GREY's DC 1 and AC 1) has one live key, the reserved
// point: its wave leaves the merge loop at the first test, no entry gets a size, lane 0 finds no
// longest length and takes no code away, and the wave writes 272 zero bytes as the DHT and 256 zero
// codes, which no block reads.  Zeros are "a table the file does not define" in a MIPX_OP_JPEGH slot.
// So jpeg_gen_optimal_table's merges never run on an all-zero histogram, and the two idle waves only
// keep the barriers' company.
// PACKED: the slot's place is not known yet, so the DHTs go to the head of the image's histogram
// (every wave has its counts in registers before the first barrier) for k_jpege_stuff to copy.
template <bool PACKED>
__global__ void __launch_bounds__(kTile) k_jpege_tables(const JpegeArgs a) {
    __shared__ uint32_t size_of[4][256];          // raw code size per symbol, 0: not in the table
    __shared__ uint32_t bits[4][kMaxLen + 1];     // codes per length, raw and then limited
    __shared__ uint32_t first_code[4][17], before[4][18];  // per length: its first code, and the codes shorter than it
    __shared__ uint8_t dht[4][kJpegDhtBytes];
    const uint32_t img = blockIdx.x, lane = threadIdx.x & 63u, t = threadIdx.x >> 6;
    const uint32_t *freq = a.hist + static_cast<size_t>(img) * (4u * kJpegeCodesPerTable) + t * kJpegeCodesPerTable;
    uint32_t f[5], size[5], root[5];
#pragma unroll
    for (uint32_t j = 0; j < 5u; ++j) {
        const uint32_t i = lane + 64u * j;
        f[j] = i < 256u ? freq[i] : i == 256u ? 1u : 0u;
        size[j] = 0u, root[j] = i;
    }
    for (uint32_t i = lane; i <= kMaxLen; i += 64u) bits[t][i] = 0u;
    for (uint32_t i = lane; i < kJpegDhtBytes; i += 64u) dht[t][i] = 0;
    __syncthreads();  // the zeros are in place before any lane adds to bits[] or writes dht[]
    for (;;) {
        unsigned long long k1 = kNoKey, k2 = kNoKey;
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) {
            const uint32_t i = lane + 64u * j;
            const unsigned long long k = f[j] ? static_cast<unsigned long long>(f[j]) << 9 | (256u - i) : kNoKey;
            least_two(k1, k2, k, kNoKey);
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) least_two(k1, k2, shfl_xor64(k1, m), shfl_xor64(k2, m));
        if (k2 == kNoKey) break;  // the same in every lane of the wave
        const uint32_t c1 = 256u - (static_cast<uint32_t>(k1) & 511u), c2 = 256u - (static_cast<uint32_t>(k2) & 511u);
        const uint32_t f2 = static_cast<uint32_t>(k2 >> 9);
#pragma unroll
        for (uint32_t j = 0; j < 5u; ++j) {
            const uint32_t i = lane + 64u * j;
            if (i == c1) f[j] += f2;
            if (i == c2) f[j] = 0u;
            if (root[j] == c1 || root[j] == c2) ++size[j], root[j] = c1;
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 5u; ++j) {
        const uint32_t i = lane + 64u * j, s = size[j] < kMaxLen ? size[j] : kMaxLen;
        if (i < 256u) size_of[t][i] = s;
        if (i <= 256u && s) atomicAdd(&bits[t][s], 1u);
    }
    __syncthreads();
    if (lane == 0u) {  // the library's limiting to 16 bits, and the reserved point's code dropped
        uint32_t *b = bits[t];
        for (uint32_t i = kMaxLen; i > 16u; --i)
            while (b[i] > 0u) {
                uint32_t j = i - 2u;
                while (j > 0u && b[j] == 0u) --j;  // a shorter code exists: the lengths came from a full tree
                if (j == 0u || b[i] < 2u) {         // not reached for counts in range; ends the loop in any case
                    b[i] = 0u;
                    break;
                }
                b[i] -= 2u, b[i - 1u] += 1u, b[j + 1u] += 2u, b[j] -= 1u;
            }
        uint32_t longest = 16u;
        while (longest > 0u && b[longest] == 0u) --longest;
        if (longest) --b[longest];
        uint32_t code = 0u, seen = 0u;
        for (uint32_t len = 1; len <= 16u; ++len) {  // Annex C
            first_code[t][len] = code, before[t][len] = seen;
            code = (code + b[len]) << 1, seen += b[len];
            dht[t][len - 1u] = static_cast<uint8_t>(b[len]);
        }
        before[t][17] = seen;
    }
    __syncthreads();
    // A symbol's place among the coded ones, by raw size and then by value, gives its length and code.
    uint32_t *codes = a.opt_codes + static_cast<size_t>(img) * (4u * kJpegeCodesPerTable) + t * kJpegeCodesPerTable;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = lane + 64u * j, s = size_of[t][i];
        uint32_t rank = 0u;
        for (uint32_t k = 0; k < 256u; ++k) {
            const uint32_t o = size_of[t][k];
            rank += (o != 0u && (o < s || (o == s && k < i))) ? 1u : 0u;
        }
        uint32_t entry = 0u;
        if (s && rank < before[t][17]) {
            uint32_t len = 1u;
            while (before[t][len + 1u] <= rank) ++len;  // ends: rank < before[17]
            entry = len << 16 | (first_code[t][len] + rank - before[t][len]);
            dht[t][16u + rank] = static_cast<uint8_t>(i);
        }
        codes[i] = entry;
    }
    __syncthreads();
    // the slot's tables are DC 0, DC 1, AC 0, AC 1
    u8 *to = (PACKED ? reinterpret_cast<u8 *>(a.hist + static_cast<size_t>(img) * (4u * kJpegeCodesPerTable))
                     : a.out + static_cast<size_t>(img) * (static_cast<size_t>(a.head) + a.cap) +
                           MIPX_JPEG_SCAN_HEADER_BYTES) +
             ((t & 1u) * 2u + (t >> 1)) * kJpegDhtBytes;
    for (uint32_t i = lane; i < kJpegDhtBytes; i += 64u) to[i] = dht[t][i];
}

template <int LAYOUT>
__global__ void __launch_bounds__(kTile) k_jpege_count(const JpegeArgs a) {
    __shared__ uint32_t blk[kTile * kPitch];
    __shared__ uint32_t codes[4 * kJpegeCodesPerTable];
    __shared__ uint32_t src[kTile];
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t img = blockIdx.y, tile = blockIdx.x;
    load_codes(a, img, codes);
    const Lane me = stage_tile<LAYOUT>(a, a.coefs + static_cast<size_t>(img) * a.cap, tile, blk, src);
    CountSink sink(codes + me.chroma * 2u * kJpegeCodesPerTable);
    bool bad = false;
    if (me.valid) {
        bad = walk_block(me, reinterpret_cast<const int16_t *>(blk + threadIdx.x * kPitch), sink);
        a.counts[static_cast<size_t>(img) * a.blocks + tile * kTile + threadIdx.x] = sink.bits;
    }
    uint32_t total;
    block_scan(sink.bits, wsum, &total);
    if (threadIdx.x == 0) a.tile_sums[static_cast<size_t>(img) * a.tiles + tile] = total;
    if (bad) atomicOr(&a.info[img].flags, 1u);
}

// One workgroup per image: the exclusive scan of its per-tile (STAGE 0) or per-chunk (STAGE 1)
// sums, and what follows from the total.
template <int STAGE>
__global__ void __launch_bounds__(kTile) k_jpege_scan(const JpegeArgs a) {
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    JpegeInfo *info = a.info + img;
    uint32_t count = a.tiles;
    const uint32_t *sums = a.tile_sums + static_cast<size_t>(img) * a.tiles;
    unsigned long long *offs = a.tile_offs + static_cast<size_t>(img) * a.tiles;
    unsigned long long bytes = 0;
    if (STAGE == 1) {
        if (info->status != MIPX_JPEG_SCAN_OK) return;
        bytes = (info->bits + 7ull) >> 3;  // <= cap
        count = static_cast<uint32_t>((bytes + kChunk - 1ull) / kChunk);  // the chunks k_jpege_ffcount wrote
        sums = a.chunk_sums + static_cast<size_t>(img) * a.chunks;
        offs = a.chunk_offs + static_cast<size_t>(img) * a.chunks;
    }
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < count; base += kTile) {
        const uint32_t i = base + tid;
        uint32_t total;
        const uint32_t before = block_scan(i < count ? sums[i] : 0u, wsum, &total);
        if (i < count) offs[i] = carry + before;
        carry += total;
    }
    if (tid != 0) return;
    if (STAGE == 0) {
        info->bits = carry;
        info->status = info->flags ? MIPX_JPEG_SCAN_UNCODABLE
                                   : ((carry + 7ull) >> 3) > a.cap ? MIPX_JPEG_SCAN_OVERFLOW : MIPX_JPEG_SCAN_OK;
    } else {
        info->ff = static_cast<uint32_t>(carry);
        if (bytes + carry > a.cap) info->status = MIPX_JPEG_SCAN_OVERFLOW;
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(kTile) k_jpege_pack(const JpegeArgs a) {
    __shared__ uint32_t blk[kTile * kPitch];
    __shared__ uint32_t codes[4 * kJpegeCodesPerTable];
    __shared__ uint32_t src[kTile];
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t img = blockIdx.y, tile = blockIdx.x, s = tile * kTile + threadIdx.x;
    if (a.info[img].status != MIPX_JPEG_SCAN_OK) return;  // the whole workgroup
    load_codes(a, img, codes);
    const Lane me = stage_tile<LAYOUT>(a, a.coefs + static_cast<size_t>(img) * a.cap, tile, blk, src);
    uint32_t total;
    const uint32_t before = block_scan(me.valid ? a.counts[static_cast<size_t>(img) * a.blocks + s] : 0u, wsum, &total);
    if (!me.valid) return;
    const unsigned long long at = a.tile_offs[static_cast<size_t>(img) * a.tiles + tile] + before;
    PackSink sink(codes + me.chroma * 2u * kJpegeCodesPerTable, a.stream + static_cast<size_t>(img) * (a.cap / 4u),
                  a.cap / 4u, at);
    walk_block(me, reinterpret_cast<const int16_t *>(blk + threadIdx.x * kPitch), sink);
    if (s + 1u == a.blocks) {  // the scan's last block: 1-bits up to the byte
        const uint32_t pad = (8u - (static_cast<uint32_t>(a.info[img].bits) & 7u)) & 7u;
        if (pad) sink.put((1u << pad) - 1u, pad);
    }
    sink.finish();
}

__device__ __forceinline__ uint32_t ff_bytes(uint32_t word, unsigned long long first, unsigned long long bytes) {
    uint32_t c = 0;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) c += (first + j < bytes && ((word >> (8u * j)) & 0xffu) == 0xffu) ? 1u : 0u;
    return c;
}

__global__ void __launch_bounds__(kTile) k_jpege_ffcount(const JpegeArgs a) {
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t img = blockIdx.y, chunk = blockIdx.x;
    const JpegeInfo *info = a.info + img;
    if (info->status != MIPX_JPEG_SCAN_OK) return;
    const unsigned long long bytes = (info->bits + 7ull) >> 3;
    const unsigned long long first = static_cast<unsigned long long>(chunk) * kChunk + threadIdx.x * 4u;
    if (static_cast<unsigned long long>(chunk) * kChunk >= bytes) return;
    const uint32_t word = first < a.cap ? a.stream[static_cast<size_t>(img) * (a.cap / 4u) + first / 4u] : 0u;
    uint32_t total;
    block_scan(ff_bytes(word, first, bytes), wsum, &total);
    if (threadIdx.x == 0) a.chunk_sums[static_cast<size_t>(img) * a.chunks + chunk] = total;
}

// What the slot's header says of its scan: the bytes behind the header when the status is "ok", a
// lower bound of the need when it is "overflow".
__device__ __forceinline__ unsigned long long slot_length(const JpegeInfo *info) {
    const unsigned long long bytes = (info->bits + 7ull) >> 3;
    return info->status == MIPX_JPEG_SCAN_OK ? bytes + info->ff : info->status == MIPX_JPEG_SCAN_OVERFLOW ? bytes : 0ull;
}

// One workgroup: the packed slots' directory.  A slot takes its header and, when "ok", its scan
// (which fits the capacity, so off[n] <= n slots' bytes), rounded up to 16 bytes.  The sums run in
// units of 16 bytes, split in two 16-bit halves: 256 slots of nearly 2^32 bytes pass 32 bits.
__global__ void __launch_bounds__(kTile) k_jpege_place(const JpegeArgs a) {
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t tid = threadIdx.x;
    unsigned long long carry = 0;
    for (uint32_t base = 0; base < a.n; base += kTile) {
        const uint32_t i = base + tid;
        unsigned long long units = 0;
        if (i < a.n) {
            const JpegeInfo *info = a.info + i;
            units = (a.head + (info->status == MIPX_JPEG_SCAN_OK ? slot_length(info) : 0ull) + 15ull) >> 4;
        }
        uint32_t lo_total, hi_total;
        const uint32_t lo = block_scan(static_cast<uint32_t>(units & 0xffffu), wsum, &lo_total);
        const uint32_t hi = block_scan(static_cast<uint32_t>(units >> 16), wsum, &hi_total);
        if (i < a.n) a.dir[i + 1] = (carry + (static_cast<unsigned long long>(hi) << 16) + lo + units) << 4;
        carry += (static_cast<unsigned long long>(hi_total) << 16) + lo_total;
    }
    if (tid == 0) a.dir[0] = 0ull;
}

// PACKED: the slot starts where the directory says, and nothing is stored but its header (with the
// tables k_jpege_tables<true> parked) and its `length` bytes: not the pad up to the next slot.
template <bool PACKED>
__global__ void __launch_bounds__(kTile) k_jpege_stuff(const JpegeArgs a) {
    __shared__ uint32_t wsum[kTile / 64];
    const uint32_t img = blockIdx.y, chunk = blockIdx.x;
    const JpegeInfo *info = a.info + img;
    u8 *slot = a.out + (PACKED ? static_cast<size_t>(a.dir[img])
                               : static_cast<size_t>(img) * (static_cast<size_t>(a.head) + a.cap));
    const uint32_t status = info->status;
    const unsigned long long bits = info->bits, bytes = (bits + 7ull) >> 3;
    if (PACKED && chunk == 0 && a.head != MIPX_JPEG_SCAN_HEADER_BYTES) {  // the four tables, a dword per lane
        const u8 *dht = reinterpret_cast<const u8 *>(a.hist + static_cast<size_t>(img) * (4u * kJpegeCodesPerTable));
        for (uint32_t i = threadIdx.x * 4u; i < 4u * kJpegDhtBytes; i += kTile * 4u)
            __builtin_memcpy(slot + MIPX_JPEG_SCAN_HEADER_BYTES + i, dht + i, 4);  // any alignment
    }
    if (chunk == 0 && threadIdx.x == 0) {
        const unsigned long long length = slot_length(info);
        uint4 hdr;
        hdr.x = length > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(length);
        hdr.y = status;
        hdr.z = bits > 0xffffffffull ? 0xffffffffu : static_cast<uint32_t>(bits);
        hdr.w = a.head == MIPX_JPEG_SCAN_HEADER_BYTES ? 0u : 1u;  // 1: the four tables follow
        __builtin_memcpy(slot, &hdr, 16);  // any alignment: one global_store_dwordx4
    }
    if (status != MIPX_JPEG_SCAN_OK || static_cast<unsigned long long>(chunk) * kChunk >= bytes) return;
    const unsigned long long first = static_cast<unsigned long long>(chunk) * kChunk + threadIdx.x * 4u;
    const uint32_t word = first < a.cap ? a.stream[static_cast<size_t>(img) * (a.cap / 4u) + first / 4u] : 0u;
    uint32_t total;
    const uint32_t before = block_scan(ff_bytes(word, first, bytes), wsum, &total);
    unsigned long long pos = first + a.chunk_offs[static_cast<size_t>(img) * a.chunks + chunk] + before;
    u8 *data = slot + a.head;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        if (first + j >= bytes) break;
        const uint32_t b = (word >> (8u * j)) & 0xffu;
        if (pos < a.cap) data[pos] = static_cast<u8>(b);
        ++pos;
        if (b == 0xffu) {
            if (pos < a.cap) data[pos] = 0;
            ++pos;
        }
    }
}

}  // namespace

int jpege_launch(const u8 *d_coefs, u8 *d_out, int n, int w, int h, int layout, bool optimise, u8 *work,
                 hipStream_t st, unsigned long long *d_dir) {
    const JpegeWork W(n, w, h, optimise);
    const JpegGeom g(w, h, layout);
    JpegeArgs a;
    a.coefs = d_coefs, a.out = d_out;
    a.dir = d_dir, a.n = static_cast<uint32_t>(n);
    a.hist = reinterpret_cast<uint32_t *>(work + W.hist);
    a.opt_codes = reinterpret_cast<uint32_t *>(work + W.opt_codes);
    a.codes = optimise ? a.opt_codes : device_jpege_codes();
    a.codes_stride = optimise ? 4u * kJpegeCodesPerTable : 0u;
    a.head = optimise ? MIPX_JPEG_SCAN_OPT_HEADER_BYTES : MIPX_JPEG_SCAN_HEADER_BYTES;
    if (!a.codes) {
        set_error("jpeg coefficients to scan: no Huffman code table on the device");
        return MIPX_EDEVICE;
    }
    a.info = reinterpret_cast<JpegeInfo *>(work + W.info);
    a.stream = reinterpret_cast<uint32_t *>(work + W.stream);
    a.counts = reinterpret_cast<uint32_t *>(work + W.counts);
    a.tile_sums = reinterpret_cast<uint32_t *>(work + W.tile_sums);
    a.tile_offs = reinterpret_cast<unsigned long long *>(work + W.tile_offs);
    a.chunk_sums = reinterpret_cast<uint32_t *>(work + W.chunk_sums);
    a.chunk_offs = reinterpret_cast<unsigned long long *>(work + W.chunk_offs);
    const uint64_t tiles = (g.blocks + kTile - 1) / kTile, chunks = (g.coef_bytes + kChunk - 1) / kChunk;
    if (g.coef_bytes > W.cap || g.blocks > W.blocks || !grid_ok(tiles) || !grid_ok(chunks)) return MIPX_EUNSUPPORTED;
    a.cap = static_cast<uint32_t>(g.coef_bytes);  // below 2^32: the caller's check
    a.ywb = static_cast<uint32_t>(g.y.wb), a.yhb = static_cast<uint32_t>(g.y.hb);
    a.mw = static_cast<uint32_t>(g.mw);
    a.cb_off = static_cast<uint32_t>(g.coef_off[1]), a.cr_off = static_cast<uint32_t>(g.coef_off[2]);
    a.blocks = static_cast<uint32_t>(g.blocks);
    a.tiles = static_cast<uint32_t>(tiles), a.chunks = static_cast<uint32_t>(chunks);
    MIPX_HIP(hipMemsetAsync(work + W.info, 0, (W.stream - W.info) + static_cast<size_t>(n) * a.cap, st));
    const dim3 threads(kTile), by_tile(a.tiles, n), by_chunk(a.chunks, n), by_image(n);
    int e;
    if (optimise) {
        MIPX_HIP(hipMemsetAsync(a.hist, 0, static_cast<size_t>(n) * 4u * kJpegeCodesPerTable * sizeof(uint32_t), st));
        with_output_layout(layout,
                           [&](auto L) { hipLaunchKernelGGL(k_jpege_hist<L.value>, by_tile, threads, 0, st, a); });
        if ((e = launch_check("k_jpege_hist"))) return e;
        if (d_dir) hipLaunchKernelGGL(k_jpege_tables<true>, by_image, threads, 0, st, a);
        else hipLaunchKernelGGL(k_jpege_tables<false>, by_image, threads, 0, st, a);
        if ((e = launch_check("k_jpege_tables"))) return e;
    }
    with_output_layout(layout,
                       [&](auto L) { hipLaunchKernelGGL(k_jpege_count<L.value>, by_tile, threads, 0, st, a); });
    if ((e = launch_check("k_jpege_count"))) return e;
    hipLaunchKernelGGL(k_jpege_scan<0>, by_image, threads, 0, st, a);
    if ((e = launch_check("k_jpege_scan<0>"))) return e;
    with_output_layout(layout,
                       [&](auto L) { hipLaunchKernelGGL(k_jpege_pack<L.value>, by_tile, threads, 0, st, a); });
    if ((e = launch_check("k_jpege_pack"))) return e;
    hipLaunchKernelGGL(k_jpege_ffcount, by_chunk, threads, 0, st, a);
    if ((e = launch_check("k_jpege_ffcount"))) return e;
    hipLaunchKernelGGL(k_jpege_scan<1>, by_image, threads, 0, st, a);
    if ((e = launch_check("k_jpege_scan<1>"))) return e;
    if (!d_dir) {
        hipLaunchKernelGGL(k_jpege_stuff<false>, by_chunk, threads, 0, st, a);
        return launch_check("k_jpege_stuff");
    }
    hipLaunchKernelGGL(k_jpege_place, dim3(1), threads, 0, st, a);
    if ((e = launch_check("k_jpege_place"))) return e;
    hipLaunchKernelGGL(k_jpege_stuff<true>, by_chunk, threads, 0, st, a);
    return launch_check("k_jpege_stuff<packed>");
}

}  // namespace mipx
