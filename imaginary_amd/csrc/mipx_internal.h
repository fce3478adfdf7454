// mipx_internal.h — shared declarations between the planner, the runtime and
// the gfx950 kernels of libmipx.so.  Not part of the ABI (see include/mipx.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "jpeg_geom.h"    // the JPEG layouts: sizes, offsets, predicates, limits (no HIP)
#include "mipx.h"
#include "mipx_tables.h"  // the libvips table maths, table layouts and host builders (no HIP)

namespace mipx {

// ---- errors -------------------------------------------------------------
void set_error(const char *fmt, ...);
int hip_fail(hipError_t e, const char *what);  // records detail, returns MIPX_EDEVICE
#define MIPX_HIP(call)                                                    \
    do {                                                                  \
        hipError_t e_ = (call);                                           \
        if (e_ != hipSuccess) return ::mipx::hip_fail(e_, #call);         \
    } while (0)

// ---- kernel-selection knobs (mipx_tuning.cpp) -------------------------------
// The MIPX_* environment variables as snapshotted on first use (or by
// mipx_tuning_reload): nullptr when unset.  Launchers call this, never getenv.
const char *tune_env(const char *name);
void tune_reload();
// The Lanczos reduce sampling convention (PARITY_ASSUMPTIONS.md row 1): under
// MIPX_SAMPLE_CENTRE output o samples (o + 0.5) * shrink - 0.5 (libvips' centre
// convention) instead of o * shrink.  reduce_centre() is what every reduce launcher and
// the demand-region walk read: the innermost SamplingScope of this thread, else the
// process setting (mipx_set_reduce_sampling).  execute_plan opens a scope with the
// convention each reduce / smartcrop step recorded at mipx_plan_make time (step a[7]), and
// the per-op entry points snapshot the process setting once per call, so one launch never
// mixes conventions.
bool reduce_centre();
int reduce_sampling_now();  // the process setting (what mipx_plan_make records)
class SamplingScope {
   public:
    explicit SamplingScope(int convention);  // this convention until the scope ends
    SamplingScope();                          // snapshot: the enclosing scope's, else the process setting
    ~SamplingScope();
    SamplingScope(const SamplingScope &) = delete;
    SamplingScope &operator=(const SamplingScope &) = delete;

   private:
    int prev_;
};
// requests submitted through mipx_submit and not yet retired (mipx_runtime.cpp)
long long requests_in_flight();

// ---- device properties, cached per device (mipx_tuning.cpp) --------------------
// compute units of the current device (256 on an MI355X in SPX mode; fewer per
// partition in CPX / DPX modes)
int device_cu_count();
// resident workgroups per CU for kernel fn at `threads` threads and `lds` dynamic LDS
// bytes on the current device (hipOccupancyMaxActiveBlocksPerMultiprocessor, queried
// once per (device, fn, threads, lds)); `fallback` when the query fails
int occupancy_per_cu(const void *fn, int threads, size_t lds, int fallback);

// ---- device capability probes (k_probe.hip), run once per device -------------
// Do direct-to-LDS dword buffer loads honour byte offsets that are not multiples of 4?
bool lds_dma_unaligned_ok();

// vips_resize() downsize schedule used by the smartcrop scorer.
struct ResizeSchedule {
    int shrink_h = 1, shrink_v = 1;    // integer box shrink
    double reduce_h = 1.0, reduce_v = 1.0;  // residual Lanczos3 (1.0 = none)
    int w1 = 0, h1 = 0;                // after shrink
    int w2 = 0, h2 = 0;                // after reduce
};
int resize_schedule(int w, int h, double hscale, double vscale, ResizeSchedule &s);

// ---- device-side cached tables (mipx_device_tables.cpp) -----------------------
// Each fetcher returns the table on the current device, built (mipx_tables.h) and uploaded on
// first use; nullptr when there is no such table or the device refused it.
// float copy of reduce_table(shrink) resident on the current device.
const float *device_reduce_table(double shrink, int *n_taps);
// the same taps packed as int16 pairs: [129][2 alignments][*tpa] (k_rstrip)
const uint32_t *device_reduce_pairs(double shrink, int *n_taps, int *tpa);
const signed char *device_reduce_i8(double shrink, int *n_taps, const int **sums);
const signed char *device_reduce_i8s(double shrink, int bands, int *n_taps);  // taps at a byte stride of bands
// the same with the COPY edge folded in: [2 sides][taps - 1][129][hi, lo][kRsTabW] (k_rcol)
const signed char *device_reduce_i8s_fold(double shrink, int bands, int *n_taps);
// k_rcol's vertical plan (per output row: K-placed split taps + seed; per 16-row group:
// first / end input rows) over at least `rows` op-output rows; *cap_rows = rows it holds
const uint8_t *device_rcol_vplan(double shrink, bool centre, int rows, int *cap_rows);
// k_rcol's horizontal operands of one window geometry, built on the host (r06): per 64-pixel
// strip, per 16-byte output unit u < 4 bands, per lane: per K step the hi / lo tap fragments
// (COPY edge folded, odd K blocks' halves swapped), then the four per-byte seeds,
// kRcolHopRec(nks) bytes; then per (strip, unit) the K origin (int).  The specialised k_rcol
// builds load these instead of computing the positions in the block's set-up.
const uint8_t *device_rcol_hops(double hs, int bands, bool centre, int ox0, int ow, int w, int k4, int nks, int *strips);
// k_bmf's i8 MFMA operands for a blur mask (cached per device): [nks][64][16]
// horizontal taps at byte stride `bands` shifted by delta, then [64][16] vertical taps
const signed char *device_blur_ops(const std::vector<int> &mask, int bands, int delta, int nks, int vperm);
const float *device_colour_tables();  // [256 v2y | kQuantElements cbrt | 257 y2v]
const int *device_bicubic_table();     // 129 x 4
const uint32_t *device_jpegc_recips(int quality);  // k_jpegc: [lum 64 | chr 64] reciprocals of the quality's tables
const uint32_t *device_jpege_codes();               // k_jpege: the four Annex K Huffman tables (build_jpege_codes)
// float copy of the integer gaussmat mask; *scale = mask sum
const float *device_gauss_table(double sigma, double min_ampl, int *n_taps, int *scale);
// `bytes` of host data on the current device, cached by contents (small constant tables)
const void *device_blob(const void *data, size_t bytes);
// k_enlm's per-axis records (host: [rows][rec_ints] ints, built and kept by k_affine.hip) on the
// current device, holding at least min_rows rows; grown like the vertical plan
const void *device_enlm_axis(double scale, const std::vector<int> &host, int rec_ints, int min_rows);
// frees every table above on every device (mipx_shutdown, after every queue drained)
void free_device_tables();
// bumped by free_device_tables: a launcher that caches a table pointer of its own
// keeps the generation it was made in and refetches when it changed
unsigned device_tables_generation();

// ---- generic separable passes (k_sep.hip) -----------------------------------
enum { kSepReduce = 0, kSepConv = 1 };
struct SepSpec {            // one 1-D integer mask family
    const float *tab;       // device table: reduce 129 x taps phases, conv 1 x taps
    int taps;
    int mode;               // kSepReduce / kSepConv
    double shrink;          // reduce
    int scale;              // conv: divisor (mask sum)
};
struct SepWindow {          // geometry of one pass over a batch of n images
    int bands;
    int in_pitch;           // bytes between input rows
    long long in_base;      // byte offset of the local input origin inside an image
    long long in_img;       // bytes per input image
    int in_len;             // local input length along the pass axis (COPY clamp)
    int o0;                 // first output position along the pass axis (op-output coords)
    int out_w, out_h;       // packed output image of the pass
};
bool sep_spec_reduce(double shrink, SepSpec *s);
bool sep_spec_gauss(double sigma, double min_ampl, SepSpec *s);
int vpass_launch(const uint8_t *in, uint8_t *out, int n, const SepSpec &spec, const SepWindow &w, hipStream_t st);
int hpass_launch(const uint8_t *in, uint8_t *out, int n, const SepSpec &spec, const SepWindow &w, hipStream_t st);
int reduce_fused_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int ox0,
                        int oy0, int ow, int oh, hipStream_t st);
// k_rstrip.hip: streaming fused reduce (LDS row ring + LDS intermediate), any shrink pair
// both shrinks > 1 in one launch (k_rcol, else k_rmf2, else the strip walker, else the
// small-image fused kernel); MIPX_EUNSUPPORTED = run the two separable passes
int reduce_one_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int ox0,
                      int oy0, int ow, int oh, hipStream_t st);
// k_bcol.hip: the column-walking gaussblur (both convsep passes on the matrix cores)
int blur_col_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int left, int top, int ow, int oh,
                    const std::vector<int> &mask, int scale, hipStream_t st);
// k_rcol.hip: the column walker (LDS row ring, both passes on the matrix cores)
int reduce_col_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int ox0,
                      int oy0, int ow, int oh, hipStream_t st);
int reduce_mfma_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int ox0,
                       int oy0, int ow, int oh, hipStream_t st);
int reduce_strip_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int ox0,
                        int oy0, int ow, int oh, hipStream_t st);

// ---- kernel launchers (k_*.hip); batches of n images packed back to back -----
// k_reduce.hip
int reducev_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double vshrink, hipStream_t st);
int reduceh_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hshrink, hipStream_t st);
int reduce_window_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double hs, double vs, int left,
                         int top, int ow, int oh, void *ws, size_t ws_bytes, hipStream_t st);
bool reduce2_eligible(const uint8_t *in, int w, int h, int b, double hs, double vs);
int reduce2_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, hipStream_t st);
int reduce2_window_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int x0, int y0, int x1,
                          int y1, hipStream_t st);
// k_reduce2m.hip: the centre-convention 2 x 2 reduce with its vertical pass on the matrix
// cores; taps12 = matrixi[64][0..11]
int reduce2m_window_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int x0, int y0, int x1,
                           int y1, const int *taps12, hipStream_t st);
// the corner convention's 2 x 2 mask as k_reduce2x2 uses it: c0, c1, c3, c5 (k_reduce.hip)
bool reduce2_taps(float c[4]);
// k_shrink.hip
int shrink_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int hs, int vs, hipStream_t st);
int shrink_window_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int hs, int vs, int x0, int y0,
                         int x1, int y1, hipStream_t st);
// k_geometry.hip
int embed_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int x, int y, int ow, int oh,
                 int extend, const int *bg, const int *d_origins, hipStream_t st);
int flip_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int vertical, hipStream_t st);
int rot_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int angle, hipStream_t st);
int device_copy(void *dst, const void *src, size_t bytes, hipStream_t st);  // a batch, device to device
int extract_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int left, int top, int ow, int oh,
                   hipStream_t st);
// k_blur.hip (ws: n * w * h * b bytes for the uchar intermediate)
int blur_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double sigma, double min_ampl,
                void *ws, size_t ws_bytes, hipStream_t st);
int blur_window_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int left, int top, int ow,
                       int oh, double sigma, double min_ampl, void *ws, size_t ws_bytes, hipStream_t st);
// k_affine.hip
int affine_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, double xs, double ys, int extend,
                  hipStream_t st);
int zoom_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, int xf, int yf, hipStream_t st);
// k_colour.hip
int flatten_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, const int *bg, hipStream_t st);
int bw_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int b, hipStream_t st);
// k_composite.hip
int watermark_launch(const uint8_t *base, const uint8_t *wm, uint8_t *out, int n, int w, int h, int bands, int ww,
                     int wh, int wb, int left, int top, float opacity, hipStream_t st);
// k_textmark.hip: the rendered text mask (tw x th x 1) tiled and blended in; 1 or 3 bands -> 3
int textmark_launch(const uint8_t *in, const uint8_t *mask, uint8_t *out, int n, int w, int h, int bands, int tw,
                    int th, int margin, float opacity, const int *colour, hipStream_t st);
// k_ycc.hip: packed JPEG planes (MIPX_YCC_*) -> RGB.  replicate: 4:2:2 chroma is replicated at every
// width, as libjpeg does behind its 1 / 8 decode; the other layouts ignore it
int ycc_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int layout, hipStream_t st,
               bool replicate = false);
// k_jpegc.hip: RGB -> the quantised DCT coefficients of a JPEG (MIPX_YCC_* layout, quality 1..100)
int jpegc_launch(const uint8_t *in, uint8_t *out, int n, int w, int h, int layout, int quality, hipStream_t st);
// k_jpegd.hip: quantisation tables + quantised coefficients (MIPX_OP_JPEGD) -> the packed planes ycc_launch takes
int jpegd_launch(const uint8_t *in, uint8_t *planes, int n, int w, int h, int layout, hipStream_t st);
// the same payload of a w x h file at 1/shrink (2, 4, 8) -> three planes of ceil(w / shrink) x ceil(h / shrink),
// packed as MIPX_YCC_444; of a 4:2:2 file the planes of that size packed as MIPX_YCC_422
int jpegds_launch(const uint8_t *in, uint8_t *planes, int n, int w, int h, int layout, int shrink, hipStream_t st);
// k_jpegrt.hip: RGB -> the planes ycc_launch takes of the JPEG of each image at `quality`, decoded at 1/shrink
// (1, 2, 4, 8): packed as `layout` at full size, as three ceil(w / shrink) x ceil(h / shrink) planes otherwise
int jpegrt_launch(const uint8_t *in, uint8_t *planes, int n, int w, int h, int layout, int quality, int shrink,
                  hipStream_t st);
// k_jpege.hip: the coefficients k_jpegc writes -> one output slot per image (mipx_jpeg_scan_bytes): the
// Huffman-coded, padded and stuffed scan behind a 16-byte header; with `optimise` coded with the image's own
// tables (row 24), which stand behind the header (mipx_jpeg_scan_opt_bytes).  work: a JpegeWork of
// (n, w, h, optimise), 16-byte aligned.  With d_dir (device memory, 8-byte aligned, n + 1 offsets) the slots
// are packed back to back instead, each rounded up to 16 bytes: d_dir[i] is slot i's byte offset in `out`,
// d_dir[n] the end; only a slot's header and its `length` bytes are written
int jpege_launch(const uint8_t *coefs, uint8_t *out, int n, int w, int h, int layout, bool optimise, uint8_t *work,
                 hipStream_t st, unsigned long long *d_dir = nullptr);
// The coder's workspace, sized without the layout (both fit): byte offsets of its parts, each a multiple
// of 256, and the total.  Per image (jpeg_max of the output layouts): cap = the 4:4:4 coefficients'
// bytes; blocks = the scan's blocks, dummy ones included, of whichever output layout has more.
constexpr int kJpegeTile = 256;     // scan blocks per workgroup of the count and pack kernels
constexpr int kJpegeChunk = 1024;   // stream bytes per workgroup of the stuffing kernels
struct JpegeWork {
    size_t cap, blocks, tiles, chunks;
    size_t coefs;      // n * cap: k_jpegc's output, when the call starts from RGB
    size_t info;       // n * 32: per image bits (u64), 0xFF bytes (u32), status (u32), flags (u32)
    size_t stream;     // n * cap: the scan before stuffing; follows info, one memset clears both
    size_t counts;     // n * blocks u32: bits per block
    size_t tile_sums;  // n * tiles u32, then their exclusive scan as u64
    size_t tile_offs;
    size_t chunk_sums;  // n * chunks u32, then their exclusive scan as u64
    size_t chunk_offs;
    size_t hist;       // optimised tables only: n * 4 * 256 u32 symbol counts, then as many codes
    size_t opt_codes;
    size_t total;
    JpegeWork(int n, int w, int h, bool optimise = false) {
        auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
        const JpegMax most = jpeg_max(w, h, false);
        const size_t N = static_cast<size_t>(n);
        cap = most.cap, blocks = most.blocks;
        tiles = (blocks + kJpegeTile - 1) / kJpegeTile;
        chunks = (cap + kJpegeChunk - 1) / kJpegeChunk;
        coefs = 0;
        info = coefs + up(N * cap);
        stream = info + up(N * 32);
        counts = stream + up(N * cap);
        tile_sums = counts + up(N * blocks * 4);
        tile_offs = tile_sums + up(N * tiles * 4);
        chunk_sums = tile_offs + up(N * tiles * 8);
        chunk_offs = chunk_sums + up(N * chunks * 4);
        hist = chunk_offs + up(N * chunks * 8);
        opt_codes = hist + (optimise ? N * 4096 : 0);
        total = opt_codes + (optimise ? N * 4096 : 0);
    }
};
// k_jpegh.hip: n input slots (mipx_jpegh_bytes: header, Huffman tables, the file's entropy-coded scan) ->
// n payloads of MIPX_OP_JPEGD (mipx_jpegd_bytes) and n statuses (MIPX_JPEGH_*, 4-byte aligned).
// work: a JpeghWork of (n, w, h), 16-byte aligned; its parts before `payload` are the decoder's own
int jpegh_launch(const uint8_t *slots, uint8_t *payloads, uint32_t *status, int n, int w, int h, int layout,
                 uint8_t *work, hipStream_t st);
constexpr int kJpeghHeader = MIPX_JPEGH_HEADER_BYTES;
constexpr int kJpeghSub = 128;   // bytes of unstuffed stream per lane of the decoding kernels
constexpr int kJpeghSeq = 256;   // lanes, so subsequences, per workgroup: a sequence is 32 KiB
constexpr int kJpeghRounds = 2;  // launches that carry states across sequences, after the first
// The decoder's workspace, sized without the layout like JpegeWork: byte offsets of its parts, each a
// multiple of 256, and the total.  The statuses lead, so a plan's caller finds them at the head.
// blocks is the most of the three input layouts (jpeg_max).
struct JpeghWork {
    size_t cap, blocks, tiles, chunks, seqs, sstride;
    size_t status;      // n u32: MIPX_JPEGH_* per image
    size_t info;        // n * 32: per image the unstuffed length and flags
    size_t stream;      // n * sstride: the scan without its stuffed zeros, 8 spare bytes behind
    size_t chunk_sums;  // n * chunks u32: stuffed zeros per 1024 bytes of scan, then their exclusive scan
    size_t chunk_offs;
    size_t entries;     // n * seqs * kJpeghSeq u64: entry state per subsequence
    size_t counts;      // n * seqs * kJpeghSeq u32: blocks completed per subsequence
    size_t seq_exit;    // 2 * n * seqs u64: exit state per sequence, of the even and of the odd launches
    size_t seq_sums;    // n * seqs u32: blocks per sequence, then their exclusive scan
    size_t seq_offs;
    size_t dcdiff;      // n * blocks i32: DC difference per block of the scan
    size_t dc_sums;     // n * tiles * 3 i32: per tile and component, then their exclusive scan as i64
    size_t dc_offs;
    size_t payload;     // n * (384 + cap): MIPX_OP_JPEGD's payloads, when the call goes on to pixels
    size_t planes;      // n * w * h * 3: MIPX_OP_JPEGD's own workspace
    size_t total;
    JpeghWork(int n, int w, int h) {
        auto up = [](size_t v) { return (v + 255) & ~static_cast<size_t>(255); };
        const JpegMax most = jpeg_max(w, h, true);
        const size_t N = static_cast<size_t>(n);
        cap = most.cap, blocks = most.blocks;
        tiles = (blocks + kJpeghSeq - 1) / kJpeghSeq;
        chunks = (cap + 4 * kJpeghSeq - 1) / (4 * kJpeghSeq);
        seqs = (cap + kJpeghSub * kJpeghSeq - 1) / (kJpeghSub * kJpeghSeq);
        sstride = up(cap + 8);
        status = 0;
        info = status + up(N * 4);
        stream = info + up(N * 32);
        chunk_sums = stream + N * sstride;
        chunk_offs = chunk_sums + up(N * chunks * 4);
        entries = chunk_offs + up(N * chunks * 4);
        counts = entries + up(N * seqs * kJpeghSeq * 8);
        seq_exit = counts + up(N * seqs * kJpeghSeq * 4);
        seq_sums = seq_exit + up(2 * N * seqs * 8);
        seq_offs = seq_sums + up(N * seqs * 4);
        dcdiff = seq_offs + up(N * seqs * 4);
        dc_sums = dcdiff + up(N * blocks * 4);
        dc_offs = dc_sums + up(N * tiles * 12);
        payload = dc_offs + up(N * tiles * 24);
        planes = payload + up(N * (384 + cap));
        total = planes + up(N * static_cast<size_t>(w) * h * 3);
    }
};
// k_smartcrop.hip
size_t smartcrop_workspace_bytes(int n, int w, int h, int bands);
int smartcrop_origins(const uint8_t *in, int *origins, int n, int w, int h, int b, int cw, int ch, void *ws,
                      size_t ws_bytes, hipStream_t st);
int smartcrop_extract(const uint8_t *in, uint8_t *out, int n, int w, int h, int bands, int cw, int ch, void *ws,
                      size_t ws_bytes, hipStream_t st);
// mipx_ops.cpp
size_t op_workspace_bytes(int op, int n, int w, int h, int bands, double p0, double p1);

// mipx_planner.cpp: bytes per image of the plan's input buffer: w * h * bands, or the packed
// planes when step 0 is MIPX_OP_YCC, the coefficient payload when it is MIPX_OP_JPEGD, the scan's
// slot when it is MIPX_OP_JPEGH (header fields already validated): of the file's size, which a
// scaled step carries in a[2], a[3]
size_t plan_input_bytes(const mipx_plan *p);
// bytes per image of the plan's output buffer: out_w * out_h * out_bands, or the coefficients
// when the last step is MIPX_OP_JPEGC, or the scan's slot when it is MIPX_OP_JPEGE (plan already validated)
size_t plan_output_bytes(const mipx_plan *p);
// whether a w x h scan is inside the optimised tables' rule: 64 x its blocks < 10^9
bool jpeg_opt_in_range(int w, int h, int layout);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

}  // namespace mipx
