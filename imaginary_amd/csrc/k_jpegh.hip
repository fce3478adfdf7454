// k_jpegh.hip — a baseline JPEG decoder's front half on gfx950 (PARITY_ASSUMPTIONS.md row 22): the
// file's entropy-coded scan in, one slot per image (include/mipx.h, MIPX_OP_JPEGH), the payload of
// MIPX_OP_JPEGD out (quantisation tables, int16 coefficients), so k_jpegd / k_jpegds run unchanged
// behind it.  Integer only; the output does not depend on the order workgroups run in.
//
// A Huffman stream has no known codeword boundaries, so the decoders are started speculatively and
// synchronise: the unstuffed stream is cut into subsequences of kJpeghSub bytes, one lane each, and
// sequences of kJpeghSeq subsequences, one workgroup each.  The state a decoder needs at a bit is
// (block index inside the MCU, zigzag index); an MCU is 3 blocks in 4:4:4, 6 in 4:2:0 and 4 in
// 4:2:2 (Y left, Y right, Cb, Cr; the chroma grid is then the MCU grid), and the one block in
// MIPX_YCC_GREY, whose scan is not interleaved (row 26): block s is block s of Y's grid, there are no
// dummy blocks, a restart interval counts blocks, and one DC chain runs where the others have three
// (JpeghArgs::comps; dc_sums and dc_offs keep their stride of 3).  Every dependency
// between workgroups is a launch boundary on the stream; no kernel waits for another workgroup;
// every loop has a bound.
//   memset             the statuses, the per-image records, the payloads (zero coefficients)
//   k_jpegh_ffcount    FF 00 pairs per kChunk bytes of the stuffed scan; FF + anything else: BAD
//   k_jpegh_prep       one workgroup per image: the scan of those counts, the unstuffed length,
//                      the Huffman tables' validity
//   k_jpegr_index, k_jpegr_decode
//                      the images with restart intervals, whose codeword boundaries are their
//                      markers: see "restart intervals" below.  For them the two kernels above
//                      count and check the markers instead, every kernel below returns at once
//                      (k_jpegh_dcwrite after their quantisation tables and final status), and
//                      these two return at once for every other image
//   k_jpegh_unstuff    the scan without the stuffed zeros into the workspace
//   k_jpegh_sync x (1 + kJpeghRounds)
//                      lane i decodes subsequence i from its entry state (values skipped, blocks
//                      counted) and hands its exit state to lane i + 1, until nothing changes; the
//                      first lane of sequence 0 starts with the truth, every other first lane with a
//                      guess in the first launch and with its predecessor's exit of the launch
//                      before in the later ones
//   k_jpegh_place      one workgroup per image: every sequence's exit equal in the last two
//                      launches (then all states are the true ones, by induction from sequence 0),
//                      else UNSYNCED; the scan of the sequences' block counts
//   k_jpegh_write      the same lanes decode again, with values: non-zero AC coefficients to their
//                      place in the payload, every block's DC difference to the workspace
//   k_jpegh_dcsum, k_jpegh_dcscan, k_jpegh_dcwrite
//                      per-component prefix sums of the differences in scan order: per tile, over
//                      the tiles, and the DCs into the payload; the quantisation tables
// Images whose status is not OK are skipped by every later kernel.
//
// Decoding is total: on a path that is not yet known to be the true one an unknown code skips one
// bit, a run past coefficient 63 ends the block, a DC symbol counts as symbol & 15 bits.  The write
// pass follows the very same rules (so it walks the states the sync passes verified) and reports
// each of them, inside the scan's blocks, as BAD.  tests/jpegh_ref.py restates the rules.
//
// The decoding kernels stage their sequence's 32 KiB through LDS with coalesced loads, kStagePitch
// dwords per lane (the subsequence, the 8 bytes a look-ahead reads behind it, and one to make the
// pitch odd): lanes that each walk their own subsequence then read 64 different banks, where the
// same reads from global memory touched 64 cache lines per instruction.  The Huffman look-ups sit
// in LDS beside it: a 512-entry first level per table and the canonical maxcode walk for codes of
// 10 to 16 bits.  Slots and payloads start on any byte: accesses to them are plain unaligned ones.
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "jpeg_scan.h"

namespace mipx {
namespace {

using namespace dev;
using namespace jscan;

constexpr uint32_t kLanes = kJpeghSeq;       // threads of every kernel here
constexpr uint32_t kSubBits = 8u * kJpeghSub;
constexpr uint32_t kChunk = 4u * kLanes;     // stuffed bytes per workgroup: 4 per lane
constexpr uint32_t kLut = 9;                 // bits of the first-level Huffman look-up
constexpr uint32_t kNone = 0xffffffffu;
// The status of a restart image between k_jpegh_prep and k_jpegh_dcwrite, never seen by a caller: the
// kernels of the synchronising path skip it as they skip every status but OK
constexpr uint32_t kPending = 3u;
static_assert(kPending != MIPX_JPEGH_OK && kPending != MIPX_JPEGH_UNSYNCED && kPending != MIPX_JPEGH_BAD, "internal");
// dwords of LDS per lane of a decoding kernel: the subsequence's 32, the 2 a look-ahead reads past
// them, and one more so that the lanes of a wave, each at its own bit, read 64 different banks
constexpr uint32_t kStagePitch = kJpeghSub / 4u + 3u;
static_assert(kJpeghSub % 4 == 0 && (kStagePitch & 1u) == 1u, "an odd pitch spreads the lanes over the banks");
constexpr uint32_t kTablesOff = 416, kTableBytes = 272, kSelOff = 400, kQuantOff = 16;
static_assert(kLanes == 256, "block_scan sums four waves");

struct JpeghInfo {  // per image, zeroed every call
    uint32_t ulen;   // bytes of the unstuffed stream
    uint32_t flags;  // 1: the slot cannot be decoded (k_jpegh_ffcount); 2: the same, found on the restart path
    uint32_t rst;    // the restart interval in MCUs of an image on the restart path (k_jpegh_prep), else 0
    uint32_t pad[5];
};
static_assert(sizeof(JpeghInfo) == 32, "JpeghWork sizes the records");

typedef unsigned long long u64;

struct JpeghArgs {
    const u8 *slots;   // kJpeghHeader + cap bytes per image
    u8 *payloads;      // MIPX_JPEGD_HEADER_BYTES + cap bytes per image
    uint32_t *status;  // per image MIPX_JPEGH_*
    JpeghInfo *info;
    uint32_t *stream;  // sstride bytes per image
    uint32_t *chunk_sums, *chunk_offs;
    u64 *entries;      // per subsequence: its lane's entry state
    uint32_t *counts;  // per subsequence: blocks its lane completed
    u64 *seq_exit;     // [2][n][seqs]: the sequences' exit states of the even and odd launches
    uint32_t *seq_sums, *seq_offs;
    int *dcdiff;       // per block of the scan
    int *dc_sums;      // [n][tiles][3]
    long long *dc_offs;
    uint32_t n, cap, sstride;
    uint32_t chunks, seqs, tiles;  // per image, by the capacity (W's, the strides of the arrays above)
    uint32_t blocks;               // of this image's scan, dummy ones included
    uint32_t mcus;                 // of this image's scan
    uint32_t wblocks;              // the stride of dcdiff
    uint32_t ywb, yhb, mw;
    uint32_t cb_off, cr_off;       // byte offsets of Cb and Cr in the payload's coefficients
    uint32_t comps;                // components of the scan: 3, or 1 (grey)
};

__device__ __forceinline__ uint32_t load_u32(const u8 *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}

// ---- unstuffing ---------------------------------------------------------------------------

// The lane's 4 stuffed bytes from `first` on: which of them are dropped (a 00 behind an FF), and
// whether one of them is an FF that no 00 follows inside `length`.  Reads no byte at or past length.
__device__ __forceinline__ uint32_t stuffed4(const u8 *scan, uint32_t first, uint32_t length, uint32_t *bytes,
                                             bool *marker) {
    uint32_t drop = 0;
    uint32_t prev = first > 0u && first - 1u < length ? scan[first - 1u] : 0u;
    *marker = false;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = first + j;
        const uint32_t b = i < length ? scan[i] : 0u;
        bytes[j] = b;
        if (i < length) {
            if (b == 0u && prev == 0xffu) drop |= 1u << j;
            if (b == 0xffu && (i + 1u >= length || scan[i + 1u] != 0u)) *marker = true;
        }
        prev = b;
    }
    return drop;
}

__device__ __forceinline__ uint32_t slot_length(const JpeghArgs &a, const u8 *slot) {
    const uint32_t length = load_u32(slot);
    return length > a.cap ? 0u : length;  // k_jpegh_prep reports it; nothing reads past the slot
}

// The slot's restart interval in MCUs when the image takes the restart path: 1..65535 and two
// intervals or more (K = ceil(mcus / Ri) >= 2).  Else 0: the image is an ordinary scan.
__device__ __forceinline__ uint32_t slot_restart(const JpeghArgs &a, const u8 *slot) {
    const uint32_t ri = load_u32(slot + 4u);
    return ri >= 1u && ri <= 65535u && ri < a.mcus ? ri : 0u;
}

// The restart path's view of the lane's 4 stuffed bytes from `first` on: bit j set where an FF that
// D0..D7 follows starts (an FF is always the first byte of a pair: no pair ends in one), and whether
// one of them is an FF that neither 00 nor D0..D7 follows inside `length`.  Reads no byte at or past
// length.
__device__ __forceinline__ uint32_t marks4(const u8 *scan, uint32_t first, uint32_t length, bool *other) {
    uint32_t marks = 0;
    *other = false;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t i = first + j;
        if (i < length && scan[i] == 0xffu) {
            const uint32_t next = i + 1u < length ? scan[i + 1u] : 0xffu;
            if ((next & 0xf8u) == 0xd0u) marks |= 1u << j;
            else if (next != 0u) *other = true;
        }
    }
    return marks;
}

__global__ void __launch_bounds__(kLanes) k_jpegh_ffcount(const JpeghArgs a) {
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, chunk = blockIdx.x;
    const u8 *slot = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap));
    const uint32_t length = slot_length(a, slot);
    if (static_cast<u64>(chunk) * kChunk >= length) return;
    uint32_t bytes[4];
    bool marker;
    // an ordinary scan: the stuffed zeros; a restart image: the restart markers
    const uint32_t first = chunk * kChunk + threadIdx.x * 4u;
    const uint32_t drop = slot_restart(a, slot) ? marks4(slot + kJpeghHeader, first, length, &marker)
                                                : stuffed4(slot + kJpeghHeader, first, length, bytes, &marker);
    uint32_t total;
    block_scan<uint32_t>(__builtin_popcount(drop), wsum, &total);
    if (threadIdx.x == 0) a.chunk_sums[static_cast<size_t>(img) * a.chunks + chunk] = total;
    if (marker) atomicOr(&a.info[img].flags, 1u);
}

// Whether table t of the slot is a Huffman table: at most 256 codes, none past its length's range.
// The canonical (Annex C) first code - 1 + count per length into maxcode (-1: no code of that
// length), and symbol index - code into valoff.
__device__ __forceinline__ bool canonical(const u8 *table, int *maxcode, int *valoff) {
    uint32_t code = 0, k = 0;
    bool ok = true;
    for (uint32_t l = 1; l <= 16u; ++l) {
        const uint32_t c = table[l - 1u];
        maxcode[l] = -1, valoff[l] = 0;
        if (ok && c) {
            if (k + c > 256u || code + c > (1u << l)) {
                ok = false;
            } else {
                valoff[l] = static_cast<int>(k) - static_cast<int>(code);
                maxcode[l] = static_cast<int>(code + c) - 1;
                code += c, k += c;
            }
        }
        code <<= 1;
    }
    if (!ok)
        for (uint32_t l = 1; l <= 16u; ++l) maxcode[l] = -1;
    return ok;
}

__global__ void __launch_bounds__(kLanes) k_jpegh_prep(const JpeghArgs a) {
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    const u8 *slot = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap));
    const uint32_t raw = load_u32(slot), length = slot_length(a, slot);
    bool bad = raw > a.cap;
    if (tid < 4u) {
        int maxcode[17], valoff[17];
        if (!canonical(slot + kTablesOff + kTableBytes * tid, maxcode, valoff)) bad = true;
    } else if (tid < 10u) {  // the table indices of the components the scan has: DC of 0 1 2, then AC
        if ((tid - 4u) % 3u < a.comps && slot[kSelOff + tid - 4u] > 1u) bad = true;
    }
    const uint32_t count = (length + kChunk - 1u) / kChunk;
    const uint32_t *sums = a.chunk_sums + static_cast<size_t>(img) * a.chunks;
    uint32_t *offs = a.chunk_offs + static_cast<size_t>(img) * a.chunks;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < count; base += kLanes) {
        const uint32_t i = base + tid;
        uint32_t total;
        const uint32_t before = block_scan<uint32_t>(i < count ? sums[i] : 0u, wsum, &total);
        if (i < count) offs[i] = carry + before;
        carry += total;
    }
    const bool any_bad = __syncthreads_or(bad);
    if (tid != 0) return;
    a.info[img].ulen = length - carry;
    // a restart image: `carry` is its markers, one less than its intervals
    const uint32_t ri = load_u32(slot + 4u), rst = slot_restart(a, slot);
    a.info[img].rst = rst;
    const bool count_bad = rst != 0u && carry != (a.mcus + rst - 1u) / rst - 1u;
    if (any_bad || a.info[img].flags || ri > 65535u || count_bad) a.status[img] = MIPX_JPEGH_BAD;
    else if (rst != 0u) a.status[img] = kPending;  // k_jpegr_index, k_jpegr_decode take it; k_jpegh_dcwrite ends it
}

__global__ void __launch_bounds__(kLanes) k_jpegh_unstuff(const JpeghArgs a) {
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, chunk = blockIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const u8 *slot = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap));
    const uint32_t length = slot_length(a, slot);
    if (static_cast<u64>(chunk) * kChunk >= length) return;
    const uint32_t first = chunk * kChunk + threadIdx.x * 4u;
    uint32_t bytes[4];
    bool marker;
    const uint32_t drop = stuffed4(slot + kJpeghHeader, first, length, bytes, &marker);
    uint32_t total;
    const uint32_t before = block_scan<uint32_t>(__builtin_popcount(drop), wsum, &total);
    // at most `first` bytes were dropped before `first`, so pos <= first + j < length <= cap
    uint32_t pos = first - (a.chunk_offs[static_cast<size_t>(img) * a.chunks + chunk] + before);
    u8 *out = reinterpret_cast<u8 *>(a.stream) + static_cast<size_t>(img) * a.sstride;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        if (first + j >= length) break;
        if (drop >> j & 1u) continue;
        if (pos < a.cap) out[pos] = static_cast<u8>(bytes[j]);
        ++pos;
    }
}

// ---- decoding -----------------------------------------------------------------------------

struct Huff {  // an image's four tables: DC 0, DC 1, AC 0, AC 1
    uint16_t first[4][1u << kLut];  // by the next kLut bits: length << 8 | symbol; 0: a longer code, or none
    int maxcode[4][17];
    int valoff[4][17];
    u8 syms[4][256];
    uint32_t dcsel, acsel;  // bit b: block b of the MCU takes table 1
};

// Ends with a barrier.
template <int LAYOUT>
__device__ __forceinline__ void load_tables(const u8 *slot, Huff &H) {
    const uint32_t tid = threadIdx.x;
    if (tid < 4u) canonical(slot + kTablesOff + kTableBytes * tid, H.maxcode[tid], H.valoff[tid]);
#pragma unroll
    for (uint32_t t = 0; t < 4u; ++t) H.syms[t][tid] = slot[kTablesOff + kTableBytes * t + 16u + tid];
    if (tid == 4u) {
        const uint32_t d[3] = {slot[kSelOff] & 1u, slot[kSelOff + 1u] & 1u, slot[kSelOff + 2u] & 1u};
        const uint32_t c[3] = {slot[kSelOff + 3u] & 1u, slot[kSelOff + 4u] & 1u, slot[kSelOff + 5u] & 1u};
        if (LAYOUT == MIPX_YCC_GREY) {  // Y's alone: bytes 400 and 403
            H.dcsel = d[0];
            H.acsel = c[0];
        } else if (LAYOUT == MIPX_YCC_444) {
            H.dcsel = d[0] | d[1] << 1 | d[2] << 2;
            H.acsel = c[0] | c[1] << 1 | c[2] << 2;
        } else if (LAYOUT == MIPX_YCC_422) {
            H.dcsel = d[0] * 3u | d[1] << 2 | d[2] << 3;
            H.acsel = c[0] * 3u | c[1] << 2 | c[2] << 3;
        } else {
            H.dcsel = d[0] * 15u | d[1] << 4 | d[2] << 5;
            H.acsel = c[0] * 15u | c[1] << 4 | c[2] << 5;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 4u << kLut; i += kLanes) {
        const uint32_t t = i >> kLut, e = i & ((1u << kLut) - 1u);
        uint32_t entry = 0;
        for (uint32_t l = 1; l <= kLut; ++l) {
            const int code = static_cast<int>(e >> (kLut - l));
            if (code <= H.maxcode[t][l]) {
                entry = l << 8 | H.syms[t][(H.valoff[t][l] + code) & 255];
                break;
            }
        }
        H.first[t][e] = static_cast<uint16_t>(entry);
    }
    __syncthreads();
}

// The workgroup's sequence of the stream into LDS, kStagePitch dwords per lane: the lane's own
// subsequence and the 8 bytes behind it (coalesced loads; words past the stream's room read 0).  A
// lane's decoder starts at or behind its subsequence's first bit and takes its last step before the
// subsequence's end, so these are all the bytes it looks at.  Ends with a barrier.
__device__ __forceinline__ void stage_sequence(const uint32_t *stream, uint32_t seq, uint32_t room, uint32_t *stage) {
    constexpr uint32_t kPer = kJpeghSub / 4u + 2u;
    for (uint32_t i = threadIdx.x; i < kLanes * kPer; i += kLanes) {
        const uint32_t lane = i / kPer, j = i - lane * kPer;
        const uint32_t wi = (seq * kLanes + lane) * (kJpeghSub / 4u) + j;
        stage[lane * kStagePitch + j] = wi < room ? stream[wi] : 0u;
    }
    __syncthreads();
}

// The 32 bits of the stream from bit `rel` of the lane's staged words on, most significant first;
// avail: bits of the stream from there to its end (> 0), the bits behind them read 0.  The stream is
// bytes, a word holds 4 of them little-endian.  rel < kSubBits: the word of rel and the next one.
__device__ __forceinline__ uint32_t peek32(const uint32_t *words, uint32_t rel, uint32_t avail) {
    const uint32_t wi = rel >> 5, sh = rel & 31u;
    const uint32_t hi = __builtin_bswap32(words[wi]), lo = __builtin_bswap32(words[wi + 1u]);
    uint32_t v = sh ? hi << sh | lo >> (32u - sh) : hi;
    if (avail < 32u) v &= ~(0xffffffffu >> avail);
    return v;
}

struct State {
    uint32_t pos;  // bit of the stream
    uint32_t b;    // block inside the MCU
    uint32_t k;    // zigzag index of the next coefficient; 0: a DC code comes next
};
__device__ __forceinline__ u64 pack(const State &s) { return static_cast<u64>(s.pos) | static_cast<u64>(s.b) << 32 | static_cast<u64>(s.k) << 40; }
__device__ __forceinline__ State unpack(u64 v) {
    State s;
    s.pos = static_cast<uint32_t>(v), s.b = static_cast<uint32_t>(v >> 32) & 255u, s.k = static_cast<uint32_t>(v >> 40) & 255u;
    return s;
}

// What one step of the decoder did, for the pass that writes.
struct Step {
    bool error;      // an unknown code, a run past 63, a DC symbol above 15
    bool value;      // `coef` is coefficient `k` of the block (k = 0: the DC difference)
    bool block_end;
    uint32_t k;
    int coef;
};

// One code and its value bits, of v, the stream's next 32 bits.  Total: every input moves pos by
// 1..31 bits and leaves a state.
template <int LAYOUT>
__device__ __forceinline__ Step step_bits(State &s, const Huff &H, const uint32_t v) {
    constexpr uint32_t kPerMcu = per_mcu<LAYOUT>();
    Step r;
    r.error = false, r.value = false, r.block_end = false, r.k = 0, r.coef = 0;
    const uint32_t t = s.k == 0u ? (H.dcsel >> s.b & 1u) : 2u + (H.acsel >> s.b & 1u);
    uint32_t e = H.first[t][v >> (32u - kLut)];
    if (e == 0u) {
        for (uint32_t l = kLut + 1u; l <= 16u; ++l) {
            const int code = static_cast<int>(v >> (32u - l));
            if (code <= H.maxcode[t][l]) {
                e = l << 8 | H.syms[t][(H.valoff[t][l] + code) & 255];
                break;
            }
        }
    }
    if (e == 0u) {  // no such code: skip a bit
        r.error = true;
        s.pos += 1u;
        return r;
    }
    const uint32_t len = e >> 8, sym = e & 255u, size = sym & 15u;
    bool end = false;
    if (s.k == 0u) {
        if (sym > 15u) r.error = true;
        r.value = true, r.k = 0u;
        s.k = 1u;
    } else {
        const uint32_t run = sym >> 4;
        if (size == 0u) {
            if (run == 15u) s.k += 16u;  // sixteen zeros
            end = run != 15u || s.k > 63u;
        } else {
            s.k += run;
            if (s.k > 63u) {
                r.error = true, end = true;
            } else {
                r.value = true, r.k = s.k;
                s.k += 1u;
                end = s.k > 63u;
            }
        }
    }
    s.pos += len;
    if (r.value) {
        if (size) {
            const int bits = static_cast<int>((v << len) >> (32u - size));
            r.coef = bits < (1 << (size - 1u)) ? bits - (1 << size) + 1 : bits;
        }
        s.pos += size;
    }
    if (end) {
        s.k = 0u;
        s.b = s.b + 1u == kPerMcu ? 0u : s.b + 1u;
        r.block_end = true;
    }
    return r;
}

template <int LAYOUT>
__device__ __forceinline__ Step step(State &s, const Huff &H, const uint32_t *words, uint32_t origin, uint32_t total) {
    return step_bits<LAYOUT>(s, H, peek32(words, s.pos - origin, total - s.pos));
}

struct Span {  // an image's stream, as every decoding workgroup sees it
    uint32_t total;  // bits
    uint32_t nsub;   // subsequences that hold a bit of it
    uint32_t nseq;
};
__device__ __forceinline__ Span span_of(const JpeghInfo &info) {
    Span sp;
    sp.total = info.ulen * 8u;  // cap < 2^29
    sp.nsub = (sp.total + kSubBits - 1u) / kSubBits;
    sp.nseq = (sp.nsub + kLanes - 1u) / kLanes;
    return sp;
}

template <int LAYOUT>
__global__ void __launch_bounds__(kLanes) k_jpegh_sync(const JpeghArgs a, const uint32_t round) {
    __shared__ Huff H;
    __shared__ u64 ent[kLanes + 1];
    __shared__ uint32_t stage[kLanes * kStagePitch];
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, seq = blockIdx.x, tid = threadIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const Span sp = span_of(a.info[img]);
    if (seq >= sp.nseq) return;
    const u64 *ex_old = a.seq_exit + (static_cast<size_t>((round & 1u) ^ 1u) * a.n + img) * a.seqs;
    u64 *ex_new = a.seq_exit + (static_cast<size_t>(round & 1u) * a.n + img) * a.seqs;
    const uint32_t sub = seq * kLanes + tid;
    const size_t at = static_cast<size_t>(img) * a.seqs * kLanes + sub;
    const bool active = sub < sp.nsub;
    const uint32_t last = min(kLanes - 1u, sp.nsub - 1u - seq * kLanes);  // the sequence's last active lane
    State guess;
    guess.pos = sub * kSubBits, guess.b = 0u, guess.k = 0u;
    u64 my = pack(guess);
    uint32_t cnt = 0;
    bool changed = active;
    if (round != 0u) {
        my = a.entries[at], cnt = a.counts[at];
        changed = false;
        if (tid == 0u && seq != 0u) {
            const u64 e = ex_old[seq - 1u];
            changed = e != my;
            my = e;
        }
        if (!__syncthreads_or(changed)) {  // the same entry: the same exit
            if (tid == 0u) ex_new[seq] = ex_old[seq];
            return;
        }
    }
    load_tables<LAYOUT>(a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap)), H);
    ent[tid] = my;
    if (tid == 0u) ent[kLanes] = round != 0u ? ex_old[seq] : 0ull;
    stage_sequence(a.stream + static_cast<size_t>(img) * (a.sstride / 4u), seq, a.sstride / 4u, stage);
    const uint32_t *words = stage + tid * kStagePitch;
    const uint32_t origin = sub * kSubBits, limit = min(origin + kSubBits, sp.total);
    // Lane 0's entry is fixed, and a lane whose entry is final publishes a final exit, so the
    // final states advance at least one lane per iteration.
    for (uint32_t it = 0; it < kLanes; ++it) {
        if (changed) {
            State s = unpack(my);
            cnt = 0;
            // a step takes at least one bit, and starts before the subsequence's end
            for (uint32_t i = 0; i < kSubBits && s.pos >= origin && s.pos < limit; ++i)
                cnt += step<LAYOUT>(s, H, words, origin, sp.total).block_end ? 1u : 0u;
            ent[tid + 1u] = pack(s);
        }
        __syncthreads();
        changed = false;
        if (tid != 0u) {
            const u64 e = ent[tid];
            changed = active && e != my;
            my = e;
        }
        if (!__syncthreads_or(changed)) break;
    }
    a.entries[at] = my, a.counts[at] = cnt;
    uint32_t total;
    block_scan<uint32_t>(active ? cnt : 0u, wsum, &total);
    if (tid == 0u) {
        ex_new[seq] = ent[last + 1u];
        a.seq_sums[static_cast<size_t>(img) * a.seqs + seq] = total;
    }
}

__global__ void __launch_bounds__(kLanes) k_jpegh_place(const JpeghArgs a) {
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const Span sp = span_of(a.info[img]);
    const u64 *ex_a = a.seq_exit + (static_cast<size_t>(kJpeghRounds & 1) * a.n + img) * a.seqs;
    const u64 *ex_b = a.seq_exit + (static_cast<size_t>((kJpeghRounds & 1) ^ 1) * a.n + img) * a.seqs;
    bool differ = false;
    for (uint32_t j = tid; j < sp.nseq; j += kLanes) differ = differ || ex_a[j] != ex_b[j];
    if (__syncthreads_or(differ)) {
        if (tid == 0u) a.status[img] = MIPX_JPEGH_UNSYNCED;
        return;
    }
    const uint32_t *sums = a.seq_sums + static_cast<size_t>(img) * a.seqs;
    uint32_t *offs = a.seq_offs + static_cast<size_t>(img) * a.seqs;
    u64 carry = 0;  // a block is 2 bits or more, so a sequence's count is below 2^18
    for (uint32_t base = 0; base < sp.nseq; base += kLanes) {
        const uint32_t j = base + tid;
        uint32_t total;
        const uint32_t before = block_scan<uint32_t>(j < sp.nseq ? sums[j] : 0u, wsum, &total);
        if (j < sp.nseq) offs[j] = static_cast<uint32_t>(min(carry + before, static_cast<u64>(kNone)));
        carry += total;
    }
    if (tid == 0u && carry < a.blocks) a.status[img] = MIPX_JPEGH_BAD;  // the stream ends inside the scan
}

// Byte offset in the payload's coefficients of block `cur` of the scan; kNone for a dummy block.
template <int LAYOUT>
__device__ __forceinline__ uint32_t block_dst(const JpeghArgs &a, uint32_t cur, uint32_t *comp) {
    const ScanBlock b = scan_block<LAYOUT>(cur, a.mw);
    *comp = b.comp;
    if (!b.placed) return (b.comp == 0u ? 0u : b.comp == 1u ? a.cb_off : a.cr_off) + b.m * 128u;
    return b.by < a.yhb && b.bx < a.ywb ? (b.by * a.ywb + b.bx) * 128u : kNone;
}

template <int LAYOUT>
__global__ void __launch_bounds__(kLanes) k_jpegh_write(const JpeghArgs a) {
    __shared__ Huff H;
    __shared__ uint32_t stage[kLanes * kStagePitch];
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, seq = blockIdx.x, tid = threadIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const Span sp = span_of(a.info[img]);
    if (seq >= sp.nseq) return;
    const uint32_t sub = seq * kLanes + tid;
    const size_t at = static_cast<size_t>(img) * a.seqs * kLanes + sub;
    const bool active = sub < sp.nsub;
    load_tables<LAYOUT>(a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap)), H);
    stage_sequence(a.stream + static_cast<size_t>(img) * (a.sstride / 4u), seq, a.sstride / 4u, stage);
    uint32_t total;
    const uint32_t before = block_scan<uint32_t>(active ? a.counts[at] : 0u, wsum, &total);
    if (!active) return;
    const u64 base = static_cast<u64>(a.seq_offs[static_cast<size_t>(img) * a.seqs + seq]) + before;
    if (base >= a.blocks) return;  // padding bits
    uint32_t cur = static_cast<uint32_t>(base);  // the block the lane is in
    const uint32_t *words = stage + tid * kStagePitch;
    u8 *coefs = a.payloads + static_cast<size_t>(img) * (MIPX_JPEGD_HEADER_BYTES + static_cast<size_t>(a.cap)) +
                MIPX_JPEGD_HEADER_BYTES;
    int *dcdiff = a.dcdiff + static_cast<size_t>(img) * a.wblocks;
    const uint32_t origin = sub * kSubBits, limit = min(origin + kSubBits, sp.total);
    State s = unpack(a.entries[at]);
    uint32_t comp;
    uint32_t dst = block_dst<LAYOUT>(a, cur, &comp);
    bool bad = false;
    for (uint32_t i = 0; i < kSubBits && s.pos >= origin && s.pos < limit && cur < a.blocks; ++i) {
        const Step r = step<LAYOUT>(s, H, words, origin, sp.total);
        if (r.error || s.pos > sp.total) bad = true;
        if (r.value) {
            if (r.k == 0u) {
                dcdiff[cur] = r.coef;
            } else if (dst != kNone && r.coef != 0) {
                const int16_t c = static_cast<int16_t>(r.coef);  // 15 bits and a sign at most
                __builtin_memcpy(coefs + dst + 2u * kZigzag[r.k], &c, 2);  // dst + 128 <= cap
            }
        }
        if (r.block_end) {
            ++cur;
            if (cur < a.blocks) dst = block_dst<LAYOUT>(a, cur, &comp);
        }
    }
    if (bad) atomicMax(&a.status[img], static_cast<uint32_t>(MIPX_JPEGH_BAD));
}

// ---- the DC prediction chain ----------------------------------------------------------------

template <int LAYOUT>
__global__ void __launch_bounds__(kLanes) k_jpegh_dcsum(const JpeghArgs a) {
    __shared__ int wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, tile = blockIdx.x, cur = tile * kLanes + threadIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const int d = cur < a.blocks ? a.dcdiff[static_cast<size_t>(img) * a.wblocks + cur] : 0;
    const uint32_t comp = scan_block<LAYOUT>(cur, 1u).comp;
    constexpr uint32_t kComps = LAYOUT == MIPX_YCC_GREY ? 1u : 3u;
#pragma unroll
    for (uint32_t c = 0; c < kComps; ++c) {
        int total;  // 256 differences of 15 bits and a sign
        block_scan<int>(comp == c ? d : 0, wsum, &total);
        if (threadIdx.x == 0) a.dc_sums[(static_cast<size_t>(img) * a.tiles + tile) * 3u + c] = total;
    }
}

__global__ void __launch_bounds__(kLanes) k_jpegh_dcscan(const JpeghArgs a) {
    __shared__ long long wsum[kLanes / 64];
    const uint32_t img = blockIdx.x, tid = threadIdx.x;
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const uint32_t count = (a.blocks + kLanes - 1u) / kLanes;
    const int *sums = a.dc_sums + static_cast<size_t>(img) * a.tiles * 3u;
    long long *offs = a.dc_offs + static_cast<size_t>(img) * a.tiles * 3u;
    for (uint32_t c = 0; c < a.comps; ++c) {  // grey's k_jpegh_dcsum writes component 0 alone
        long long carry = 0;
        for (uint32_t base = 0; base < count; base += kLanes) {
            const uint32_t i = base + tid;
            long long total;
            const long long before = block_scan<long long>(i < count ? sums[i * 3u + c] : 0, wsum, &total);
            if (i < count) offs[i * 3u + c] = carry + before;
            carry += total;
        }
    }
}

template <int LAYOUT>
__global__ void __launch_bounds__(kLanes) k_jpegh_dcwrite(const JpeghArgs a) {
    __shared__ int wsum[kLanes / 64];
    const uint32_t img = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x, cur = tile * kLanes + tid;
    u8 *payload = a.payloads + static_cast<size_t>(img) * (MIPX_JPEGD_HEADER_BYTES + static_cast<size_t>(a.cap));
    if (tile == 0u && tid < MIPX_JPEGD_HEADER_BYTES / 2u) {  // the quantisation tables
        const u8 *q = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap)) + kQuantOff;
        payload[2u * tid] = q[2u * tid], payload[2u * tid + 1u] = q[2u * tid + 1u];
    }
    if (a.info[img].rst) {  // a restart image: k_jpegr_decode wrote its DCs; this last launch ends kPending
        if (tile == 0u && tid == 0u && a.status[img] == kPending)
            a.status[img] = a.info[img].flags & 2u ? MIPX_JPEGH_BAD : MIPX_JPEGH_OK;
        return;
    }
    if (a.status[img] != MIPX_JPEGH_OK) return;
    const bool valid = cur < a.blocks;
    const int d = valid ? a.dcdiff[static_cast<size_t>(img) * a.wblocks + cur] : 0;
    uint32_t comp = 0;
    const uint32_t dst = valid ? block_dst<LAYOUT>(a, cur, &comp) : kNone;
    long long dc = 0;
    constexpr uint32_t kComps = LAYOUT == MIPX_YCC_GREY ? 1u : 3u;
#pragma unroll
    for (uint32_t c = 0; c < kComps; ++c) {
        int total;
        const int before = block_scan<int>(valid && comp == c ? d : 0, wsum, &total);
        if (comp == c) dc = a.dc_offs[(static_cast<size_t>(img) * a.tiles + tile) * 3u + c] + before + d;
    }
    if (dst == kNone) return;
    if (dc < -32768 || dc > 32767) {
        atomicMax(&a.status[img], static_cast<uint32_t>(MIPX_JPEGH_BAD));
        return;
    }
    const int16_t v = static_cast<int16_t>(dc);
    __builtin_memcpy(payload + MIPX_JPEGD_HEADER_BYTES + dst, &v, 2);
}

// ---- restart intervals ----------------------------------------------------------------------
// An image whose slot names a restart interval (JpeghInfo::rst != 0) has its codeword boundaries in
// the byte stream: interval k starts behind marker k - 1, at block 0 of MCU k * rst, with the three
// DC predictors 0.  k_jpegh_prep leaves it the status kPending, which keeps it out of the kernels
// of the synchronising path; these two kernels report what they find in JpeghInfo::flags, and
// k_jpegh_dcwrite, the last launch, turns that into OK or BAD.  Its interval table (the first byte
// of every interval) lies in the image's part of `counts`, which only the synchronising path
// uses: K <= mcus <= 3 ywb yhb <= seqs * kLanes.

// Every marker's place into the table, and its number checked: marker k is FF D0 + (k & 7).
__global__ void __launch_bounds__(kLanes) k_jpegr_index(const JpeghArgs a) {
    __shared__ uint32_t wsum[kLanes / 64];
    const uint32_t img = blockIdx.y;
    if (a.status[img] != kPending) return;  // nothing changes it during this launch
    const uint32_t rst = a.info[img].rst;
    const u8 *slot = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap));
    const uint32_t length = slot_length(a, slot);
    const u8 *scan = slot + kJpeghHeader;
    uint32_t *table = a.counts + static_cast<size_t>(img) * a.seqs * kLanes;
    const uint32_t intervals = (a.mcus + rst - 1u) / rst;
    if (blockIdx.x == 0u && threadIdx.x == 0u) table[0] = 0u;
    bool bad = false;
    // the grid is a fixed number of workgroups per image, not one per chunk of the capacity: an
    // ordinary image pays a handful of workgroups that return at once
    const uint32_t count = (length + kChunk - 1u) / kChunk;  // <= a.chunks: length <= cap
    for (uint32_t chunk = blockIdx.x; chunk < count; chunk += gridDim.x) {
        const uint32_t first = chunk * kChunk + threadIdx.x * 4u;
        bool other;
        const uint32_t marks = marks4(scan, first, length, &other);
        uint32_t total;
        uint32_t k = a.chunk_offs[static_cast<size_t>(img) * a.chunks + chunk] +
                     block_scan<uint32_t>(__builtin_popcount(marks), wsum, &total);
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            if (!(marks >> j & 1u)) continue;
            // k_jpegh_prep counted intervals - 1 markers, so k + 1 < intervals; first + j + 1 < length
            if (k + 1u < intervals) table[k + 1u] = first + j + 2u;
            if (scan[first + j + 1u] != 0xd0u + (k & 7u)) bad = true;
            ++k;
        }
    }
    if (bad) atomicOr(&a.info[img].flags, 2u);
}

// One lane per interval.  The lane reads its interval's stuffed bytes from the slot, dropping the 00
// behind an FF as it refills its bit buffer, walks exactly its MCUs by the rules of step_bits, keeps
// the three DCs and stores every real block's DC and non-zero ACs into the payload (its quantisation
// tables are k_jpegh_dcwrite's, as for every image).  Any broken rule, a DC outside int16 and an
// interval that ends before its last block are BAD; bits behind the last block are ignored.  A step
// takes a bit or more, so the loop ends within the interval's bits.
template <int LAYOUT>
__global__ void __launch_bounds__(kLanes) k_jpegr_decode(const JpeghArgs a) {
    constexpr uint32_t kPerMcu = per_mcu<LAYOUT>();
    __shared__ Huff H;
    const uint32_t img = blockIdx.y, tid = threadIdx.x;
    if (a.status[img] != kPending) return;  // nothing changes it during this launch
    const uint32_t rst = a.info[img].rst;
    const u8 *slot = a.slots + static_cast<size_t>(img) * (kJpeghHeader + static_cast<size_t>(a.cap));
    u8 *payload = a.payloads + static_cast<size_t>(img) * (MIPX_JPEGD_HEADER_BYTES + static_cast<size_t>(a.cap));
    const uint32_t intervals = (a.mcus + rst - 1u) / rst;
    if (blockIdx.x * kLanes >= intervals) return;
    load_tables<LAYOUT>(slot, H);
    const uint32_t k = blockIdx.x * kLanes + tid;
    if (k >= intervals) return;
    const uint32_t length = slot_length(a, slot);
    const uint32_t *table = a.counts + static_cast<size_t>(img) * a.seqs * kLanes;
    const uint32_t start = table[k];
    const uint32_t end = k + 1u < intervals ? table[k + 1u] - 2u : length;  // the marker's FF, or the scan's end
    if (start > end || end > length) {  // not with the table k_jpegr_index makes of K - 1 markers
        atomicOr(&a.info[img].flags, 2u);
        return;
    }
    const u8 *scan = slot + kJpeghHeader;
    u8 *coefs = payload + MIPX_JPEGD_HEADER_BYTES;
    uint32_t cur = k * rst * kPerMcu;  // the block the lane is in; k * rst < mcus
    const uint32_t stop = cur + min(rst, a.mcus - k * rst) * kPerMcu;  // <= a.blocks
    u64 buf = 0;         // the stream's next bits, the first in bit 63
    uint32_t nbits = 0;  // bits of buf in use; behind the interval's last byte they are zeros
    uint32_t real = 0;   // bits of the interval taken into buf so far
    uint32_t pos = start;
    int dc0 = 0, dc1 = 0, dc2 = 0;
    State s;
    s.pos = 0u, s.b = 0u, s.k = 0u;  // pos: bits consumed
    uint32_t comp;
    uint32_t dst = block_dst<LAYOUT>(a, cur, &comp);
    bool bad = false;
    const uint32_t bits = 8u * (end - start);  // cap < 2^29
    for (uint32_t i = 0; i <= bits && cur < stop; ++i) {
        while (nbits <= 56u) {
            uint32_t b = 0;
            if (pos < end) {
                b = scan[pos++];
                real += 8u;
                if (b == 0xffu) ++pos;  // its stuffed 00: every other FF made the slot BAD before
            }
            buf |= static_cast<u64>(b) << (56u - nbits);
            nbits += 8u;
        }
        const uint32_t before = s.pos;
        const Step r = step_bits<LAYOUT>(s, H, static_cast<uint32_t>(buf >> 32));
        const uint32_t used = s.pos - before;  // 1..31 <= nbits
        buf <<= used, nbits -= used;
        if (r.error || s.pos > real) {
            bad = true;
            break;
        }
        if (r.value) {
            if (r.k == 0u) {
                // a real block follows within the MCU, and its check keeps the sums inside an int
                const int dc = comp == 0u ? (dc0 += r.coef) : comp == 1u ? (dc1 += r.coef) : (dc2 += r.coef);
                if (dst != kNone) {
                    if (dc < -32768 || dc > 32767) {
                        bad = true;
                        break;
                    }
                    const int16_t c = static_cast<int16_t>(dc);
                    __builtin_memcpy(coefs + dst, &c, 2);
                }
            } else if (dst != kNone && r.coef != 0) {
                const int16_t c = static_cast<int16_t>(r.coef);
                __builtin_memcpy(coefs + dst + 2u * kZigzag[r.k], &c, 2);  // dst + 128 <= cap
            }
        }
        if (r.block_end) {
            ++cur;
            if (cur < stop) dst = block_dst<LAYOUT>(a, cur, &comp);
        }
    }
    if (bad || cur < stop) atomicOr(&a.info[img].flags, 2u);
}

}  // namespace

int jpegh_launch(const u8 *d_slots, u8 *d_payloads, uint32_t *d_status, int n, int w, int h, int layout, u8 *work,
                 hipStream_t st) {
    const JpeghWork W(n, w, h);
    const JpegGeom g(w, h, layout);
    JpeghArgs a;
    a.slots = d_slots, a.payloads = d_payloads, a.status = d_status;
    a.info = reinterpret_cast<JpeghInfo *>(work + W.info);
    a.stream = reinterpret_cast<uint32_t *>(work + W.stream);
    a.chunk_sums = reinterpret_cast<uint32_t *>(work + W.chunk_sums);
    a.chunk_offs = reinterpret_cast<uint32_t *>(work + W.chunk_offs);
    a.entries = reinterpret_cast<u64 *>(work + W.entries);
    a.counts = reinterpret_cast<uint32_t *>(work + W.counts);
    a.seq_exit = reinterpret_cast<u64 *>(work + W.seq_exit);
    a.seq_sums = reinterpret_cast<uint32_t *>(work + W.seq_sums);
    a.seq_offs = reinterpret_cast<uint32_t *>(work + W.seq_offs);
    a.dcdiff = reinterpret_cast<int *>(work + W.dcdiff);
    a.dc_sums = reinterpret_cast<int *>(work + W.dc_sums);
    a.dc_offs = reinterpret_cast<long long *>(work + W.dc_offs);
    a.n = static_cast<uint32_t>(n);
    // the grids of this image: by its own capacity, inside the workspace's strides
    const uint64_t chunks = (g.coef_bytes + kChunk - 1) / kChunk;
    const uint64_t seqs = (g.coef_bytes + kJpeghSub * kLanes - 1) / (kJpeghSub * kLanes);
    const uint64_t tiles = (g.blocks + kLanes - 1) / kLanes, mcus = g.mw * g.mh;
    if (g.coef_bytes > W.cap || !jpeg_scan_fits_decoder(g) || g.blocks > W.blocks || chunks > W.chunks ||
        seqs > W.seqs || tiles > W.tiles || !grid_ok(chunks) || !grid_ok(tiles) ||
        mcus > W.seqs * kLanes)  // the interval table's room in `counts`
        return MIPX_EUNSUPPORTED;
    a.cap = static_cast<uint32_t>(g.coef_bytes);
    a.sstride = static_cast<uint32_t>(W.sstride);
    a.chunks = static_cast<uint32_t>(W.chunks), a.seqs = static_cast<uint32_t>(W.seqs), a.tiles = static_cast<uint32_t>(W.tiles);
    a.wblocks = static_cast<uint32_t>(W.blocks);
    a.ywb = static_cast<uint32_t>(g.y.wb), a.yhb = static_cast<uint32_t>(g.y.hb), a.mw = static_cast<uint32_t>(g.mw);
    a.cb_off = static_cast<uint32_t>(g.coef_off[1]), a.cr_off = static_cast<uint32_t>(g.coef_off[2]);
    a.blocks = static_cast<uint32_t>(g.blocks), a.mcus = static_cast<uint32_t>(mcus);
    a.comps = static_cast<uint32_t>(jpeg_layout_bands(layout));
    MIPX_HIP(hipMemsetAsync(d_status, 0, static_cast<size_t>(n) * 4, st));
    MIPX_HIP(hipMemsetAsync(work + W.info, 0, static_cast<size_t>(n) * sizeof(JpeghInfo), st));
    MIPX_HIP(hipMemsetAsync(d_payloads, 0, static_cast<size_t>(n) * (MIPX_JPEGD_HEADER_BYTES + static_cast<size_t>(a.cap)), st));
    const dim3 threads(kLanes), by_chunk(chunks, n), by_seq(seqs, n), by_tile(tiles, n), by_image(n);
    const dim3 by_interval((a.mcus + kLanes - 1u) / kLanes, n);  // at most one interval per MCU; below tiles
    const dim3 by_index(chunks < 128u ? chunks : 128u, n);       // k_jpegr_index strides over the chunks
    int e;
    hipLaunchKernelGGL(k_jpegh_ffcount, by_chunk, threads, 0, st, a);
    if ((e = launch_check("k_jpegh_ffcount"))) return e;
    hipLaunchKernelGGL(k_jpegh_prep, by_image, threads, 0, st, a);
    if ((e = launch_check("k_jpegh_prep"))) return e;
    // the restart path: images with a restart interval finish here, every other leaves at once
    hipLaunchKernelGGL(k_jpegr_index, by_index, threads, 0, st, a);
    if ((e = launch_check("k_jpegr_index"))) return e;
    with_input_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_jpegr_decode<L.value>, by_interval, threads, 0, st, a); });
    if ((e = launch_check("k_jpegr_decode"))) return e;
    hipLaunchKernelGGL(k_jpegh_unstuff, by_chunk, threads, 0, st, a);
    if ((e = launch_check("k_jpegh_unstuff"))) return e;
    for (uint32_t round = 0; round <= kJpeghRounds; ++round) {
        with_input_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_jpegh_sync<L.value>, by_seq, threads, 0, st, a, round); });
        if ((e = launch_check("k_jpegh_sync"))) return e;
    }
    hipLaunchKernelGGL(k_jpegh_place, by_image, threads, 0, st, a);
    if ((e = launch_check("k_jpegh_place"))) return e;
    with_input_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_jpegh_write<L.value>, by_seq, threads, 0, st, a); });
    if ((e = launch_check("k_jpegh_write"))) return e;
    with_input_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_jpegh_dcsum<L.value>, by_tile, threads, 0, st, a); });
    if ((e = launch_check("k_jpegh_dcsum"))) return e;
    hipLaunchKernelGGL(k_jpegh_dcscan, by_image, threads, 0, st, a);
    if ((e = launch_check("k_jpegh_dcscan"))) return e;
    with_input_layout(layout, [&](auto L) { hipLaunchKernelGGL(k_jpegh_dcwrite<L.value>, by_tile, threads, 0, st, a); });
    return launch_check("k_jpegh_dcwrite");
}

}  // namespace mipx
