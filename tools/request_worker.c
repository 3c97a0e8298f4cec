/*
 * request_worker.c -- ONE IMP worker process talking to the broker, like tests/c/worker_harness.c, but for any request:
 * the query string goes through impgpu_parse_request (bridge.c:304-372) and the location's watermark, if any, is
 * registered once through the client the way glue/imp_gpu_bridge.c does (PrepareWatermark, bridge.c:199-237).
 *     JPEG file in  ->  the query's operators  ->  JPEG file out (the query's quality=, else 86)
 *
 *   request_worker <pool.bin> <seconds> <id> <dir> broker[:name] <query> <overlay.bin|-> <gx,gy,ox,oy,opacity> [answers.bin]
 * pool.bin / answers.bin / ready / go / the JSON line: as worker_harness.  overlay.bin: u32 width, height, channels, then
 * the rows, tightly packed (B,G,R,A).  tools/worker_scaling.py --query / --watermark starts N of these.
 */
#define _POSIX_C_SOURCE 200809L
#include <impgpu.h>
#include <impgpu_broker.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

typedef struct { unsigned count; unsigned char** blobs; size_t* sizes; } pool_t;

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int load(const char* path, pool_t* p) {
    FILE* f = fopen(path, "rb");
    unsigned i;
    if (!f || fread(&p->count, 4, 1, f) != 1 || p->count == 0) return -1;
    p->blobs = (unsigned char**)malloc(sizeof(unsigned char*) * p->count);
    p->sizes = (size_t*)malloc(sizeof(size_t) * p->count);
    for (i = 0; i < p->count; i++) {
        unsigned sz = 0;
        if (fread(&sz, 4, 1, f) != 1) return -1;
        p->sizes[i] = sz;
        p->blobs[i] = (unsigned char*)malloc(sz ? sz : 1);
        if (fread(p->blobs[i], 1, sz, f) != sz) return -1;
    }
    fclose(f);
    return 0;
}

static int cmp_float(const void* a, const void* b) {
    const float x = *(const float*)a, y = *(const float*)b;
    return x < y ? -1 : x > y;
}

static impgpu_client* g_client;
static impgpu_config g_cfg;
static const impgpu_job* g_job;
static int g_quality = 86, g_watermark_id;
static long g_batch_sum;

static int request(const unsigned char* blob, size_t size, const unsigned char** data, size_t* len) {
    impgpu_client_request r;
    impgpu_client_answer a;
    int rc;
    memset(&r, 0, sizeof r);
    r.in_kind = IMPB_IN_FILE; r.input = blob; r.input_bytes = size;
    r.job = g_job; r.config = &g_cfg; r.watermark_id = g_watermark_id;
    r.out_kind = IMPB_OUT_JPEG; r.quality = g_quality;
    rc = impgpu_client_run(g_client, &r, &a);
    if (rc != IMP_OK) { fprintf(stderr, "client: %s\n", impgpu_client_last_error()); return rc; }
    if (a.code != IMP_OK) { fprintf(stderr, "broker answered %d at step %d: %s\n", a.code, a.step, a.error); return a.code > 0 ? a.code : IMP_ERROR_DECODE_FAILED; }
    *data = a.data; *len = a.bytes;
    g_batch_sum += a.batch_size;
    return IMP_OK;
}

int main(int argc, char** argv) {
    pool_t pool, want;
    double seconds, t0, t1;
    int id, have_want = 0;
    char path[512], *uri;
    float* lat;
    long cap_lat = 4000000, n = 0, bad = 0, i;
    unsigned k;
    struct stat st;
    unsigned char* overlay = NULL;
    unsigned ov_dim[3] = {0, 0, 0};
    impgpu_request* req = NULL;
    if (argc < 9 || strncmp(argv[5], "broker", 6)) {
        fprintf(stderr, "usage: %s pool.bin seconds id dir broker[:name] query overlay.bin|- gx,gy,ox,oy,opacity [answers.bin]\n", argv[0]);
        return 2;
    }
    memset(&pool, 0, sizeof pool); memset(&want, 0, sizeof want);
    if (load(argv[1], &pool)) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    seconds = atof(argv[2]);
    id = atoi(argv[3]);
    if (argc > 9) { if (load(argv[9], &want) || want.count != pool.count) { fprintf(stderr, "cannot read %s\n", argv[9]); return 2; } have_want = 1; }
    memset(&g_cfg, 0, sizeof g_cfg);
    g_cfg.max_target_w = 2000; g_cfg.max_target_h = 2000; g_cfg.max_filters_count = 5;   /* module.c:172-181 defaults */
    g_cfg.watermark_opacity = 100; g_cfg.watermark_gravity_x = 'r'; g_cfg.watermark_gravity_y = 'b';
    if (strcmp(argv[7], "-")) {
        FILE* f = fopen(argv[7], "rb");
        char gx = 0, gy = 0;
        size_t bytes;
        if (!f || fread(ov_dim, 4, 3, f) != 3 || !ov_dim[0] || !ov_dim[1] || ov_dim[2] < 3 || ov_dim[2] > 4) { fprintf(stderr, "cannot read %s\n", argv[7]); return 2; }
        bytes = (size_t)ov_dim[0] * ov_dim[1] * ov_dim[2];
        overlay = (unsigned char*)malloc(bytes);
        if (fread(overlay, 1, bytes, f) != bytes) { fprintf(stderr, "cannot read %s\n", argv[7]); return 2; }
        fclose(f);
        if (sscanf(argv[8], "%c,%c,%d,%d,%d", &gx, &gy, &g_cfg.watermark_offset_x, &g_cfg.watermark_offset_y, &g_cfg.watermark_opacity) != 5) {
            fprintf(stderr, "bad placement %s\n", argv[8]);
            return 2;
        }
        g_cfg.watermark_gravity_x = gx; g_cfg.watermark_gravity_y = gy;
    }
    uri = (char*)malloc(strlen(argv[6]) + 16);
    sprintf(uri, "/pool.jpg?%s", argv[6]);
    if (impgpu_parse_request(uri, "jpg", &g_cfg, &req) != IMP_OK) { fprintf(stderr, "bad query %s\n", argv[6]); return 2; }
    g_job = impgpu_request_job(req);
    if (impgpu_request_quality(req)) g_quality = atoi(impgpu_request_quality(req));
    {
        const char* name = argv[5][6] == ':' ? argv[5] + 7 : NULL;
        if (impgpu_client_attach(name, &g_client) != IMP_OK) { fprintf(stderr, "attach: %s\n", impgpu_client_last_error()); return 3; }
    }
    if (overlay && impgpu_client_prepare_watermark(g_client, overlay, (int)ov_dim[0], (int)ov_dim[1], (int)ov_dim[2],
                                                   (int)(ov_dim[0] * ov_dim[2]), &g_watermark_id) != IMP_OK) {
        fprintf(stderr, "prepare_watermark: %s\n", impgpu_client_last_error());
        return 3;
    }
    lat = (float*)malloc(sizeof(float) * (size_t)cap_lat);
    for (k = 0; k < pool.count; k++) {                             /* every size once before the clock, checked */
        const unsigned char* data = NULL; size_t len = 0;
        if (request(pool.blobs[k], pool.sizes[k], &data, &len) != IMP_OK) return 4;
        if (have_want && (len != want.sizes[k] || memcmp(data, want.blobs[k], len))) bad++;
    }
    g_batch_sum = 0;
    snprintf(path, sizeof path, "%s/ready.%d", argv[4], id);
    { FILE* f = fopen(path, "w"); if (f) fclose(f); }
    snprintf(path, sizeof path, "%s/go", argv[4]);
    while (stat(path, &st) != 0) { struct timespec nap = {0, 500000}; nanosleep(&nap, NULL); }
    t0 = now_s();
    t1 = t0;
    while (t1 - t0 < seconds) {
        const unsigned f = (unsigned)((unsigned long)(id * 13 + n * 7) % pool.count);
        const unsigned char* data = NULL; size_t len = 0;
        const double a = t1;
        if (request(pool.blobs[f], pool.sizes[f], &data, &len) != IMP_OK) return 4;
        if (have_want && (len != want.sizes[f] || memcmp(data, want.blobs[f], len))) bad++;
        t1 = now_s();
        if (n < cap_lat) lat[n] = (float)(1e6 * (t1 - a));
        n++;
    }
    {
        const long m = n < cap_lat ? n : cap_lat;
        double mean = 0;
        qsort(lat, (size_t)m, sizeof(float), cmp_float);
        for (i = 0; i < m; i++) mean += lat[i];
        printf("{\"worker\": %d, \"mode\": \"broker\", \"requests\": %ld, \"seconds\": %.6f, \"mismatches\": %ld, \"checked\": %s, "
               "\"p50_us\": %.1f, \"p95_us\": %.1f, \"p99_us\": %.1f, \"mean_us\": %.1f, \"mean_batch\": %.2f, \"chain_timeouts\": 0, \"refused\": 0}\n",
               id, n, t1 - t0, bad, have_want ? "true" : "false",
               m ? lat[m / 2] : 0.0, m ? lat[(long)(0.95 * (double)(m - 1))] : 0.0, m ? lat[(long)(0.99 * (double)(m - 1))] : 0.0, m ? mean / (double)m : 0.0,
               n ? (double)g_batch_sum / (double)n : 0.0);
    }
    impgpu_client_detach(&g_client);
    impgpu_request_free(&req);
    return bad ? 5 : 0;
}
