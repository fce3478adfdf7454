/*
 * mipx_e2e_ycc.c — mipx_e2e.c's request-path measurement with the input handed over as a
 * JPEG decoder's planes (MIPX_OP_YCC, mipx_plan_set_ycc_input) or, for the comparison on the
 * same build and in the same session, as RGB: T threads each keep `inflight` 4K -> 1920x1080
 * requests outstanding (mipx_submit from host memory, mipx_wait on the oldest), over
 * pre-faulted caller buffers.  Prints one JSON line: requests/s, host-link GB/s (bytes in +
 * out as they cross the link), batches.
 *
 *   mipx_e2e_ycc [input] [threads] [requests_per_thread] [queues_per_device] [inflight] [max_batch]
 *   input: rgb (default), 420 or 444
 *
 * Exit 0 = ok; 1 = engine error; 77 = no device.
 */
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "mipx.h"

static mipx_plan g_plan;
static int g_requests = 64, g_inflight = 2, g_failures = 0;
static size_t g_in_bytes;  /* one request's input: RGB pixels or packed planes */
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

static void *caller(void *arg) {
    (void)arg;
    const size_t ib = g_in_bytes;
    const size_t ob = (size_t)g_plan.out_w * g_plan.out_h * g_plan.out_bands;
    uint8_t **in = calloc(g_inflight, sizeof(uint8_t *)), **out = calloc(g_inflight, sizeof(uint8_t *));
    uint64_t *tk = calloc(g_inflight, sizeof(uint64_t));
    for (int s = 0; s < g_inflight; ++s) {  /* pre-faulted, like a server's reused request buffers */
        in[s] = malloc(ib);
        out[s] = malloc(ob);
        for (size_t i = 0; i < ib; ++i) in[s][i] = (uint8_t)(i * 131u + s);
        memset(out[s], 0, ob);
    }
    pthread_barrier_wait(&g_start);
    for (int k = 0; k < g_requests; ++k) {
        const int s = k % g_inflight;
        if (k >= g_inflight) {
            const int e = mipx_wait(tk[s], -1);
            if (e) fail("mipx_wait", e);
        }
        mipx_img mi = {in[s], g_plan.in_w, g_plan.in_h, g_plan.in_bands, 0};
        mipx_img mo = {out[s], g_plan.out_w, g_plan.out_h, g_plan.out_bands, 0};
        const int e = mipx_submit(-1, &g_plan, &mi, NULL, &mo, &tk[s]);
        if (e) fail("mipx_submit", e);
    }
    for (int k = g_requests > g_inflight ? g_requests - g_inflight : 0; k < g_requests; ++k) {
        const int e = mipx_wait(tk[k % g_inflight], -1);
        if (e) fail("mipx_wait", e);
    }
    pthread_barrier_wait(&g_start);
    for (int s = 0; s < g_inflight; ++s) {
        free(in[s]);
        free(out[s]);
    }
    free(in);
    free(out);
    free(tk);
    return NULL;
}

int main(int argc, char **argv) {
    const char *input = argc > 1 ? argv[1] : "rgb";
    const int layout = !strcmp(input, "420") ? MIPX_YCC_420 : (!strcmp(input, "444") ? MIPX_YCC_444 : -1);
    const int threads = argc > 2 ? atoi(argv[2]) : 16;
    g_requests = argc > 3 ? atoi(argv[3]) : 64;
    const int qpd = argc > 4 ? atoi(argv[4]) : 1;
    g_inflight = argc > 5 ? atoi(argv[5]) : 2;
    const int max_batch = argc > 6 ? atoi(argv[6]) : 8;
    if (mipx_abi_version() != MIPX_ABI_VERSION) return 1;
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
    if (layout >= 0) {
        if ((e = mipx_plan_set_ycc_input(&g_plan, layout)) != 0) {
            fprintf(stderr, "planar input: %d %s\n", e, mipx_last_error());
            return 1;
        }
        g_in_bytes = mipx_ycc_bytes(g_plan.in_w, g_plan.in_h, layout);
    }
    mipx_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.max_batch = max_batch;
    cfg.queues_per_device = qpd;
    if ((e = mipx_init(&cfg)) != 0) {
        fprintf(stderr, "init: %d %s\n", e, mipx_last_error());
        return 1;
    }
    const int nt = threads < 256 ? threads : 256;
    pthread_t th[256];
    /* warm-up round (pinned pool growth, first launches) */
    {
        const int saved = g_requests;
        g_requests = g_inflight;
        pthread_barrier_init(&g_start, NULL, nt + 1);
        for (int t = 0; t < nt; ++t) pthread_create(&th[t], NULL, caller, NULL);
        pthread_barrier_wait(&g_start);
        pthread_barrier_wait(&g_start);
        for (int t = 0; t < nt; ++t) pthread_join(th[t], NULL);
        pthread_barrier_destroy(&g_start);
        g_requests = saved;
    }
    uint64_t b0 = 0, r0 = 0;
    for (int q = 0; q < mipx_queue_count(); ++q) {
        int32_t d;
        uint64_t b, r;
        int64_t p;
        mipx_queue_stats(q, &d, &b, &r, &p);
        b0 += b, r0 += r;
    }
    pthread_barrier_init(&g_start, NULL, nt + 1);
    for (int t = 0; t < nt; ++t) pthread_create(&th[t], NULL, caller, NULL);
    pthread_barrier_wait(&g_start);
    const double t0 = now_s();
    pthread_barrier_wait(&g_start);
    const double t1 = now_s();
    for (int t = 0; t < nt; ++t) pthread_join(th[t], NULL);
    pthread_barrier_destroy(&g_start);
    uint64_t b1 = 0, r1 = 0;
    for (int q = 0; q < mipx_queue_count(); ++q) {
        int32_t d;
        uint64_t b, r;
        int64_t p;
        mipx_queue_stats(q, &d, &b, &r, &p);
        b1 += b, r1 += r;
    }
    mipx_shutdown();
    const double n = (double)nt * g_requests, wall = t1 - t0;
    const double up = n * (double)g_in_bytes, down = n * (double)g_plan.out_w * g_plan.out_h * g_plan.out_bands;
    printf("{\"config\": \"E2E-C-YCC\", \"input\": \"%s\", \"workload\": \"request path from C: 4K %s -> %dx%d from host "
           "memory, %d caller threads x %d in flight, %d queue(s), max_batch %d\", \"images_per_sec\": %.1f, "
           "\"requests\": %.0f, \"wall_s\": %.4f, \"in_bytes\": %zu, \"h2d_gbs\": %.2f, \"d2h_gbs\": %.2f, "
           "\"host_link_gbs\": %.2f, \"batches\": %llu, \"mean_batch\": %.2f, \"failures\": %d}\n",
           layout >= 0 ? input : "rgb", layout >= 0 ? "planes" : "RGB", g_plan.out_w, g_plan.out_h, nt, g_inflight, qpd,
           max_batch, n / wall, n, wall, g_in_bytes, up / wall / 1e9, down / wall / 1e9, (up + down) / wall / 1e9,
           (unsigned long long)(b1 - b0), b1 > b0 ? (double)(r1 - r0) / (double)(b1 - b0) : 0.0, g_failures);
    return g_failures ? 1 : 0;
}
