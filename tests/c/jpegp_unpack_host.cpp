// jpegp_unpack_host.cpp — mipx_jpeg_scan_unpack (csrc/mipx_tables.cpp) on hand-made packed slots in heap
// buffers of exactly the sizes it is told, so that under AddressSanitizer a read past the packed bytes or
// a write past the destination is an error of this program: for both header sizes a batch of an OK slot,
// an OVERFLOW header of length 0xffffffff, an UNCODABLE one and a second OK slot, every slot taken out
// into a destination of exactly the bytes it needs; then each inconsistent directory or header, which must
// be MIPX_EDATA with the destination untouched.  Prints "ok" and exits 0, or says what differed.
// No HIP call, no GPU: links mipx_tables.cpp and mipx_planner.cpp only (tests/test_jpegp_cpu.py).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mipx.h"

namespace mipx {
// what mipx_planner.cpp needs from the rest of the engine
void set_error(const char *, ...) {}
int reduce_sampling_now() { return 0; }
}  // namespace mipx

static int failures = 0;
#define EXPECT(cond)                                                      \
    do {                                                                  \
        if (!(cond)) std::printf("line %d: %s\n", __LINE__, #cond), ++failures; \
    } while (0)

static size_t align16(size_t v) { return (v + 15) / 16 * 16; }

struct Batch {
    std::vector<uint64_t> dir;
    std::vector<uint8_t> bytes;  // exactly off[n]
    std::vector<size_t> span;    // bytes of each slot that count
};

static Batch make(size_t head, const std::vector<uint32_t> &lengths, const std::vector<uint32_t> &statuses) {
    Batch b;
    b.dir.push_back(0);
    for (size_t i = 0; i < lengths.size(); ++i) {
        b.span.push_back(head + (statuses[i] == MIPX_JPEG_SCAN_OK ? lengths[i] : 0));
        b.dir.push_back(b.dir.back() + align16(b.span[i]));
    }
    b.bytes.assign(b.dir.back(), 0);
    for (size_t i = 0; i < lengths.size(); ++i) {
        uint8_t *s = b.bytes.data() + b.dir[i];
        for (size_t k = 0; k < b.span[i]; ++k) s[k] = static_cast<uint8_t>(31 * i + 7 * k + 1);
        const uint32_t hdr[4] = {lengths[i], statuses[i], 8 * lengths[i], head == MIPX_JPEG_SCAN_HEADER_BYTES ? 0u : 1u};
        std::memcpy(s, hdr, 16);
    }
    return b;
}

// The call on heap copies of exactly the stated sizes; the destination comes back.
static int unpack(const std::vector<uint64_t> &dir, const std::vector<uint8_t> &bytes, size_t packed_bytes, int i,
                  size_t head, size_t slot_bytes, std::vector<uint8_t> *slot) {
    std::vector<uint8_t> packed(bytes.begin(), bytes.begin() + (packed_bytes < bytes.size() ? packed_bytes : bytes.size()));
    slot->assign(slot_bytes, 0xA5);
    return mipx_jpeg_scan_unpack(dir.data(), static_cast<int32_t>(dir.size() - 1), packed.data(), packed_bytes, i, head,
                                 slot->data(), slot_bytes);
}

static bool untouched(const std::vector<uint8_t> &slot) {
    for (uint8_t v : slot)
        if (v != 0xA5) return false;
    return true;
}

int main() {
    for (size_t head : {size_t(MIPX_JPEG_SCAN_HEADER_BYTES), size_t(MIPX_JPEG_SCAN_OPT_HEADER_BYTES)}) {
        const Batch b = make(head, {333, 0xffffffffu, 0, 48}, {MIPX_JPEG_SCAN_OK, MIPX_JPEG_SCAN_OVERFLOW,
                                                                 MIPX_JPEG_SCAN_UNCODABLE, MIPX_JPEG_SCAN_OK});
        std::vector<uint8_t> slot;
        for (int i = 0; i < 4; ++i) {
            EXPECT(unpack(b.dir, b.bytes, b.bytes.size(), i, head, b.span[i], &slot) == MIPX_OK);
            EXPECT(std::memcmp(slot.data(), b.bytes.data() + b.dir[i], b.span[i]) == 0);
            EXPECT(unpack(b.dir, b.bytes, b.bytes.size(), i, head, b.span[i] + 100, &slot) == MIPX_OK);
            EXPECT(untouched(std::vector<uint8_t>(slot.begin() + b.span[i], slot.end())));
        }
        EXPECT(b.span[1] == head && b.span[2] == head);
        const auto refused = [&](const std::vector<uint64_t> &dir, const std::vector<uint8_t> &bytes, size_t packed_bytes,
                                 int i, size_t slot_bytes) {
            std::vector<uint8_t> dst;
            return unpack(dir, bytes, packed_bytes, i, head, slot_bytes, &dst) == MIPX_EDATA && untouched(dst);
        };
        const size_t room = head + 400;
        std::vector<uint64_t> d = b.dir;
        d[0] = 16;
        EXPECT(refused(d, b.bytes, b.bytes.size(), 0, room));  // off[0] is not 0
        d = b.dir, d[2] = d[1] - 16;
        EXPECT(refused(d, b.bytes, b.bytes.size(), 0, room));  // a decreasing step
        EXPECT(refused(d, b.bytes, b.bytes.size(), 3, room));
        d = b.dir;
        for (size_t k = 1; k < d.size(); ++k) d[k] += 8;
        EXPECT(refused(d, b.bytes, b.bytes.size() + 8, 0, room));  // a step that is no multiple of 16
        d = b.dir;
        for (size_t k = 2; k < d.size(); ++k) d[k] -= 16;
        EXPECT(refused(d, b.bytes, b.bytes.size(), 0, room));  // a step below head
        EXPECT(refused(b.dir, b.bytes, b.bytes.size() - 1, 0, room));  // off[n] past packed_bytes
        std::vector<uint8_t> longer = b.bytes;
        const uint32_t past = static_cast<uint32_t>(b.dir[1] - head + 1);
        std::memcpy(longer.data(), &past, 4);
        EXPECT(refused(b.dir, longer, longer.size(), 0, room + 4096));  // an OK length past its step
        EXPECT(refused(b.dir, b.bytes, b.bytes.size(), 0, b.span[0] - 1));  // an OK length past slot_bytes
        EXPECT(refused(b.dir, b.bytes, b.bytes.size(), 3, b.span[3] - 1));
        EXPECT(unpack(b.dir, b.bytes, b.bytes.size(), 4, head, room, &slot) == MIPX_EINVAL && untouched(slot));
        EXPECT(unpack(b.dir, b.bytes, b.bytes.size(), 0, 32, room, &slot) == MIPX_EINVAL && untouched(slot));
    }
    EXPECT(mipx_jpeg_scan_packed_dir_bytes(3) == 32 && mipx_jpeg_scan_packed_dir_bytes(0) == 0);
    if (!failures) std::printf("ok\n");
    return failures ? 1 : 0;
}
