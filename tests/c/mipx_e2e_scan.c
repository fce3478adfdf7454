/*
 * mipx_e2e_scan.c — mipx_e2e_ycc.c's request-path measurement with the answer handed back as a
 * JPEG's entropy-coded scan (MIPX_OP_JPEGE, mipx_plan_set_jpeg_scan_output at 4:2:0, Q 75) or, for
 * the comparison on the same build and in the same session, as coefficients or as RGB: T threads
 * each keep `inflight` 4K -> 1920x1080 Lanczos3 requests outstanding (mipx_submit from host memory,
 * mipx_wait on the oldest), over pre-faulted caller buffers.  Prints one JSON line: requests/s, the
 * bytes per request that crossed the host link in each direction (mipx_transfer_stats), the mean
 * `length` of the scans.  MIPX_SCAN_TRIM=0 in the environment makes the engine download whole slots.
 *
 *   mipx_e2e_scan [answer] [threads] [requests_per_thread] [queues_per_device] [inflight] [max_batch] [input.rgb]
 *   answer: scan (default), coefs or rgb
 *   input.rgb: 3840 x 2160 x 3 raw bytes for every request; without it a byte pattern (the coder's worst case)
 *
 * Every answer's status is checked.  Exit 0 = ok; 1 = engine error or a slot that is not OK (nothing
 * further is started then); 77 = no device.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mipx.h"

enum { ANSWER_SCAN, ANSWER_COEFS, ANSWER_RGB };
#define LAYOUT MIPX_YCC_420
#define QUALITY 75

static mipx_plan g_plan;
static int g_answer = ANSWER_SCAN, g_requests = 64, g_inflight = 2;
static volatile int g_failures = 0;
static size_t g_in_bytes, g_out_bytes;
static const uint8_t *g_image;          /* the raw input file, or NULL */
static unsigned long long g_length_sum; /* of the scans' `length` */
static pthread_mutex_t g_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_barrier_t g_start;

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

static void fail(const char *what, int code) {
    pthread_mutex_lock(&g_mu);
    fprintf(stderr, "%s: %d %s (%s)\n", what, code, mipx_strerror(code), mipx_last_error());
    ++g_failures;
    pthread_mutex_unlock(&g_mu);
}

/* One finished request: the engine's code, and for a scan answer the slot's status. */
static void finished(int code, const uint8_t *out, unsigned long long *lengths) {
    if (code) {
        fail("mipx_wait", code);
        return;
    }
    if (g_answer != ANSWER_SCAN) return;
    uint32_t length, status;
    memcpy(&length, out, 4);
    memcpy(&status, out + 4, 4);
    if (status != MIPX_JPEG_SCAN_OK || length > g_out_bytes - MIPX_JPEG_SCAN_HEADER_BYTES) {
        pthread_mutex_lock(&g_mu);
        fprintf(stderr, "slot: status %u, length %u\n", status, length);
        ++g_failures;
        pthread_mutex_unlock(&g_mu);
        return;
    }
    *lengths += length;
}

static void *caller(void *arg) {
    (void)arg;
    const size_t ib = g_in_bytes, ob = g_out_bytes;
    uint8_t **in = calloc(g_inflight, sizeof(uint8_t *)), **out = calloc(g_inflight, sizeof(uint8_t *));
    uint64_t *tk = calloc(g_inflight, sizeof(uint64_t));
    char *queued = calloc(g_inflight, 1);
    unsigned long long lengths = 0;
    for (int s = 0; s < g_inflight; ++s) {  /* pre-faulted, like a server's reused request buffers */
        in[s] = malloc(ib);
        out[s] = malloc(ob);
        if (g_image) memcpy(in[s], g_image, ib);
        else
            for (size_t i = 0; i < ib; ++i) in[s][i] = (uint8_t)(i * 131u + s);
        memset(out[s], 0, ob);
    }
    pthread_barrier_wait(&g_start);
    for (int k = 0; k < g_requests && !g_failures; ++k) {  /* after a failure nothing further is started */
        const int s = k % g_inflight;
        if (queued[s]) {
            queued[s] = 0;
            finished(mipx_wait(tk[s], -1), out[s], &lengths);
            if (g_failures) break;
        }
        mipx_img mi = {in[s], g_plan.in_w, g_plan.in_h, g_plan.in_bands, 0};
        mipx_img mo = {out[s], g_plan.out_w, g_plan.out_h, g_plan.out_bands, 0};
        const int e = mipx_submit(-1, &g_plan, &mi, NULL, &mo, &tk[s]);
        if (e) fail("mipx_submit", e);
        else queued[s] = 1;
    }
    for (int s = 0; s < g_inflight; ++s)  /* what is queued writes these buffers: wait for it in any case */
        if (queued[s]) finished(mipx_wait(tk[s], -1), out[s], &lengths);
    pthread_barrier_wait(&g_start);
    pthread_mutex_lock(&g_mu);
    g_length_sum += lengths;
    pthread_mutex_unlock(&g_mu);
    for (int s = 0; s < g_inflight; ++s) {
        free(in[s]);
        free(out[s]);
    }
    free(in);
    free(out);
    free(tk);
    free(queued);
    return NULL;
}

static void round_of(int nt, pthread_t *th, double *wall) {
    pthread_barrier_init(&g_start, NULL, nt + 1);
    for (int t = 0; t < nt; ++t) pthread_create(&th[t], NULL, caller, NULL);
    pthread_barrier_wait(&g_start);
    const double t0 = now_s();
    pthread_barrier_wait(&g_start);
    *wall = now_s() - t0;
    for (int t = 0; t < nt; ++t) pthread_join(th[t], NULL);
    pthread_barrier_destroy(&g_start);
}

static void totals(uint64_t *batches, uint64_t *requests, uint64_t *h2d, uint64_t *d2h) {
    *batches = *requests = *h2d = *d2h = 0;
    for (int q = 0; q < mipx_queue_count(); ++q) {
        int32_t d;
        uint64_t b = 0, r = 0, up = 0, down = 0;
        int64_t p;
        mipx_queue_stats(q, &d, &b, &r, &p);
        mipx_transfer_stats(q, &up, &down);
        *batches += b, *requests += r, *h2d += up, *d2h += down;
    }
}

int main(int argc, char **argv) {
    const char *answer = argc > 1 ? argv[1] : "scan";
    g_answer = !strcmp(answer, "coefs") ? ANSWER_COEFS : (!strcmp(answer, "rgb") ? ANSWER_RGB : ANSWER_SCAN);
    const int threads = argc > 2 ? atoi(argv[2]) : 16;
    g_requests = argc > 3 ? atoi(argv[3]) : 64;
    const int qpd = argc > 4 ? atoi(argv[4]) : 1;
    g_inflight = argc > 5 ? atoi(argv[5]) : 2;
    const int max_batch = argc > 6 ? atoi(argv[6]) : 8;
    const char *path = argc > 7 ? argv[7] : NULL;
    if (mipx_abi_version() != MIPX_ABI_VERSION || g_inflight < 1 || g_requests < 1) return 1;
    if (mipx_device_count() <= 0) {
        fprintf(stderr, "no device\n");
        return 77;
    }
    mipx_opts o;
    memset(&o, 0, sizeof o);
    o.width = 1920, o.height = 1080, o.extend = MIPX_EXTEND_COPY;
    mipx_input mi;
    memset(&mi, 0, sizeof mi);
    mi.w = 3840, mi.h = 2160, mi.bands = 3, mi.type = MIPX_TYPE_PNG;
    int e = mipx_plan_make(&o, &mi, &g_plan);
    if (e) {
        fprintf(stderr, "plan: %d %s\n", e, mipx_last_error());
        return 1;
    }
    g_in_bytes = (size_t)g_plan.in_w * g_plan.in_h * g_plan.in_bands;
    g_out_bytes = (size_t)g_plan.out_w * g_plan.out_h * g_plan.out_bands;
    if (g_answer == ANSWER_SCAN) {
        e = mipx_plan_set_jpeg_scan_output(&g_plan, LAYOUT, QUALITY);
        g_out_bytes = mipx_jpeg_scan_bytes(g_plan.out_w, g_plan.out_h, LAYOUT);
    } else if (g_answer == ANSWER_COEFS) {
        e = mipx_plan_set_jpegc_output(&g_plan, LAYOUT, QUALITY);
        g_out_bytes = mipx_jpegc_bytes(g_plan.out_w, g_plan.out_h, LAYOUT);
    }
    if (e) {
        fprintf(stderr, "%s output: %d %s\n", answer, e, mipx_last_error());
        return 1;
    }
    uint8_t *image = NULL;
    if (path) {
        FILE *f = fopen(path, "rb");
        image = malloc(g_in_bytes);
        if (!f || !image || fread(image, 1, g_in_bytes, f) != g_in_bytes) {
            fprintf(stderr, "%s: not %zu bytes of raw RGB\n", path, g_in_bytes);
            return 1;
        }
        fclose(f);
        g_image = image;
    }
    mipx_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.max_batch = max_batch;
    cfg.queues_per_device = qpd;
    if ((e = mipx_init(&cfg)) != 0) {
        fprintf(stderr, "init: %d %s\n", e, mipx_last_error());
        return 1;
    }
    const int nt = threads < 256 ? (threads > 0 ? threads : 1) : 256;
    pthread_t th[256];
    double wall = 0;
    {  /* warm-up round (pinned pool growth, first launches) */
        const int saved = g_requests;
        g_requests = g_inflight;
        round_of(nt, th, &wall);
        g_requests = saved;
        g_length_sum = 0;
    }
    uint64_t b0, r0, up0, down0, b1, r1, up1, down1;
    totals(&b0, &r0, &up0, &down0);
    if (!g_failures) round_of(nt, th, &wall);
    totals(&b1, &r1, &up1, &down1);
    mipx_shutdown();
    free(image);
    const double n = (double)(r1 - r0);
    const char *trim = getenv("MIPX_SCAN_TRIM");
    printf("{\"config\": \"E2E-C-SCAN\", \"answer\": \"%s\", \"scan_trim\": \"%s\", \"input\": \"%s\", \"workload\": "
           "\"request path from C: 4K RGB -> %dx%d from host memory, %d caller threads x %d in flight, %d queue(s), "
           "max_batch %d\", \"images_per_sec\": %.1f, \"requests\": %.0f, \"wall_s\": %.4f, \"h2d_bytes_per_request\": %.0f, "
           "\"d2h_bytes_per_request\": %.0f, \"out_buffer_bytes\": %zu, \"mean_length\": %.0f, \"h2d_gbs\": %.2f, "
           "\"d2h_gbs\": %.2f, \"batches\": %llu, \"mean_batch\": %.2f, \"failures\": %d}\n",
           g_answer == ANSWER_SCAN ? "scan" : (g_answer == ANSWER_COEFS ? "coefs" : "rgb"), trim ? trim : "default",
           path ? "file" : "pattern", g_plan.out_w, g_plan.out_h, nt, g_inflight, qpd, max_batch, n > 0 ? n / wall : 0.0, n,
           wall, n > 0 ? (double)(up1 - up0) / n : 0.0, n > 0 ? (double)(down1 - down0) / n : 0.0, g_out_bytes,
           g_answer == ANSWER_SCAN && n > 0 ? (double)g_length_sum / n : 0.0, (double)(up1 - up0) / wall / 1e9,
           (double)(down1 - down0) / wall / 1e9, (unsigned long long)(b1 - b0),
           b1 > b0 ? (double)(r1 - r0) / (double)(b1 - b0) : 0.0, g_failures);
    return g_failures ? 1 : 0;
}
