// mipx_device_tables.cpp — the device-resident tables: one cache of what the host builders
// (mipx_tables.cpp) return, uploaded once per (device, kind, parameters) and freed by
// mipx_shutdown.  Every device_* fetcher of mipx_internal.h is a key, a builder and the
// unpacking of the entry's metadata around fetch().
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "mipx_internal.h"

namespace mipx {
namespace {

enum Kind {
    kReduce, kPairs, kI8, kI8s, kI8sFold, kVPlan, kHops, kBlurOps, kGauss, kColour, kBicubic, kBlob, kEnlmAxis, kJpegc, kJpegeCodes, kKinds
};

// The parameters a table was built from.  Fixed-size kinds leave `contents` empty (no heap
// allocation on a hit); k_bmf's operands and the blobs are keyed by what they hold.
struct Key {
    int kind;
    double d0 = 0, d1 = 0;
    int i[6] = {0, 0, 0, 0, 0, 0};
    std::string contents;
    int dev = 0;  // filled in by fetch()
    auto tie() const { return std::tie(kind, dev, d0, d1, i[0], i[1], i[2], i[3], i[4], i[5], contents); }
    bool operator<(const Key &o) const { return tie() < o.tie(); }
};

struct Entry {
    void *d = nullptr;
    int meta[2] = {0, 0};
    int rows = 0;
};

// A kind with a budget stops building once its tables (all devices together) would pass it:
// a server sees many geometries, and tables in use cannot be freed before shutdown.
struct Budget {
    const char *env_mb;  // another cap (tests)
    size_t bytes;
};
const Budget *budget_of(int kind) {
    // k_rcol's horizontal operands: past the cap the launcher keeps the builds that compute them
    static const Budget hops{"MIPX_RCOL_HOPCAP_MB", size_t(256) << 20};
    return kind == kHops ? &hops : nullptr;
}

struct Cache {
    std::mutex mu;
    std::map<Key, Entry> map;
    std::vector<std::pair<int, void *>> retired;  // (device, table): replaced by a grown one
    size_t used[kKinds] = {};                      // bytes of the kinds with a budget
};
Cache &cache() {
    static Cache *c = new Cache();  // leaked on purpose: outlives static dtors
    return *c;
}
std::atomic<unsigned> g_table_gen{1};

void *upload(const std::vector<uint8_t> &h) {
    void *d = nullptr;
    if (hipMalloc(&d, h.size()) == hipSuccess) {
        if (hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice) == hipSuccess) return d;
        (void)hipFree(d);
    }
    (void)hipGetLastError();  // a launch after this one must not report this failure as its own
    return nullptr;
}

// The table of `key` on the current device, built by build() (under the lock) and uploaded
// on first use; d == nullptr when there is no such table or the device refused it.
// min_rows: a growable table is rebuilt when it holds fewer rows; the replaced one stays
// allocated (kernels in flight may read it) until shutdown.  need_bytes: what a build of a
// kind with a budget will take.
template <class Build>
Entry fetch(Key key, Build &&build, int min_rows = 0, size_t need_bytes = 0) {
    if (hipGetDevice(&key.dev) != hipSuccess) return {};
    Cache &c = cache();
    std::lock_guard<std::mutex> lk(c.mu);
    auto it = c.map.find(key);
    if (it != c.map.end() && it->second.rows >= min_rows) return it->second;
    if (const Budget *b = budget_of(key.kind)) {
        const char *e = tune_env(b->env_mb);
        const size_t cap = e && *e ? static_cast<size_t>(std::max(0LL, std::atoll(e))) << 20 : b->bytes;
        if (c.used[key.kind] + need_bytes > cap) return {};
    }
    const HostTable h = build();
    if (h.bytes.empty()) return {};
    Entry e;
    e.d = upload(h.bytes);
    if (!e.d) return {};
    e.meta[0] = h.meta[0], e.meta[1] = h.meta[1], e.rows = h.rows;
    if (budget_of(key.kind)) c.used[key.kind] += h.bytes.size();
    if (it != c.map.end()) {
        c.retired.emplace_back(key.dev, it->second.d);
        it->second = e;
    } else {
        c.map.emplace(std::move(key), e);
    }
    return e;
}

Key key_of(int kind, double d0 = 0, int i0 = 0, int i1 = 0, int i2 = 0, int i3 = 0, int i4 = 0, int i5 = 0) {
    Key k{kind};
    k.d0 = d0;
    const int i[6] = {i0, i1, i2, i3, i4, i5};
    std::copy(i, i + 6, k.i);
    return k;
}

template <class T>
const T *as(const Entry &e) {
    return static_cast<const T *>(e.d);
}

}  // namespace

const float *device_reduce_table(double shrink, int *n_taps) {
    const Entry e = fetch(key_of(kReduce, shrink), [&] { return build_reduce_table(shrink); });
    if (e.d) *n_taps = e.meta[0];
    return as<float>(e);
}

const uint32_t *device_reduce_pairs(double shrink, int *n_taps, int *tpa) {
    *n_taps = reduce_points(shrink);
    *tpa = *n_taps / 2 + 1;
    return as<uint32_t>(fetch(key_of(kPairs, shrink), [&] { return build_reduce_pairs(shrink); }));
}

const signed char *device_reduce_i8(double shrink, int *n_taps, const int **sums) {
    *n_taps = reduce_points(shrink);
    const Entry e = fetch(key_of(kI8, shrink), [&] { return build_reduce_i8(shrink); });
    if (e.d) *sums = reinterpret_cast<const int *>(as<signed char>(e) + e.meta[1]);
    return as<signed char>(e);
}

const signed char *device_reduce_i8s(double shrink, int bands, int *n_taps) {
    *n_taps = reduce_points(shrink);
    return as<signed char>(fetch(key_of(kI8s, shrink, bands), [&] { return build_reduce_i8s(shrink, bands); }));
}

const signed char *device_reduce_i8s_fold(double shrink, int bands, int *n_taps) {
    *n_taps = reduce_points(shrink);
    return as<signed char>(fetch(key_of(kI8sFold, shrink, bands), [&] { return build_reduce_i8s_fold(shrink, bands); }));
}

// Grown (never shrunk) to the rows asked for.
const uint8_t *device_rcol_vplan(double shrink, bool centre, int rows, int *cap_rows) {
    if (rows <= 0) return nullptr;
    const Entry e = fetch(key_of(kVPlan, shrink, centre), [&] { return build_rcol_vplan(shrink, centre, rows); }, rows);
    if (e.d) *cap_rows = e.rows;
    return as<uint8_t>(e);
}

const uint8_t *device_rcol_hops(double hs, int bands, bool centre, int ox0, int ow, int w, int k4, int nks, int *strips) {
    *strips = (ow + 63) / 64;
    return as<uint8_t>(fetch(key_of(kHops, hs, bands, centre, ox0, ow, w, k4 + 2 * nks),
                             [&] { return build_rcol_hops(hs, bands, centre, ox0, ow, w, k4, nks); }, 0,
                             rcol_hops_bytes(bands, ow, nks)));
}

const signed char *device_blur_ops(const std::vector<int> &mask, int bands, int delta, int nks, int vperm) {
    Key k = key_of(kBlurOps, 0, bands, delta, nks, vperm);
    k.contents.assign(reinterpret_cast<const char *>(mask.data()), mask.size() * sizeof(int));
    return as<signed char>(fetch(std::move(k), [&] { return build_blur_ops(mask, bands, delta, nks, vperm); }));
}

const float *device_gauss_table(double sigma, double min_ampl, int *n_taps, int *scale) {
    Key k = key_of(kGauss, sigma);
    k.d1 = min_ampl;
    const Entry e = fetch(std::move(k), [&] { return build_gauss_table(sigma, min_ampl); });
    if (e.d) *n_taps = e.meta[0], *scale = e.meta[1];
    return as<float>(e);
}

bool sep_spec_gauss(double sigma, double min_ampl, SepSpec *s) {
    int taps = 0, scale = 0;
    s->tab = device_gauss_table(sigma, min_ampl, &taps, &scale);
    if (!s->tab) return false;
    s->taps = taps;
    s->mode = kSepConv;
    s->shrink = 1.0;
    s->scale = scale;
    return true;
}

const float *device_colour_tables() { return as<float>(fetch(key_of(kColour), build_colour_tables)); }

const int *device_bicubic_table() { return as<int>(fetch(key_of(kBicubic), build_bicubic_table)); }

const uint32_t *device_jpegc_recips(int quality) {
    return as<uint32_t>(fetch(key_of(kJpegc, 0, quality), [&] { return build_jpegc_recips(quality); }));
}

const uint32_t *device_jpege_codes() { return as<uint32_t>(fetch(key_of(kJpegeCodes), build_jpege_codes)); }

// Small host-built constant tables (per-lane MFMA operands and the like) copied to the
// current device once, keyed by their contents.
const void *device_blob(const void *data, size_t bytes) {
    Key k = key_of(kBlob);
    k.contents.assign(static_cast<const char *>(data), bytes);
    return fetch(std::move(k), [&] {
        HostTable h;
        h.bytes.assign(static_cast<const uint8_t *>(data), static_cast<const uint8_t *>(data) + bytes);
        return h;
    }).d;
}

// k_enlm's per-axis records at one scale: k_affine.hip builds them and keeps the host copy
// (its planning reads it); the device copy grows with it like the vertical plan.
const void *device_enlm_axis(double scale, const std::vector<int> &host, int rec_ints, int min_rows) {
    return fetch(key_of(kEnlmAxis, scale), [&] {
        HostTable h;
        h.bytes.assign(reinterpret_cast<const uint8_t *>(host.data()), reinterpret_cast<const uint8_t *>(host.data() + host.size()));
        h.rows = static_cast<int>(host.size()) / rec_ints;
        return h;
    }, min_rows).d;
}

unsigned device_tables_generation() { return g_table_gen.load(std::memory_order_acquire); }

void free_device_tables() {
    Cache &c = cache();
    std::lock_guard<std::mutex> lk(c.mu);
    g_table_gen.fetch_add(1, std::memory_order_acq_rel);  // pointers cached outside the map are stale now
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const auto &kv : c.map) c.retired.emplace_back(kv.first.dev, kv.second.d);
    for (const auto &r : c.retired) {
        (void)hipSetDevice(r.first);
        (void)hipFree(r.second);
    }
    c.map.clear();
    c.retired.clear();
    std::fill(c.used, c.used + kKinds, size_t(0));
    (void)hipSetDevice(cur);
}

}  // namespace mipx
