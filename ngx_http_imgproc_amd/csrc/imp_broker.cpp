// imp_broker.cpp -- `impgpu_broker`: the one process per GPU that owns the HIP context when IMP runs as N worker
// processes (docs/02 - Configuration.md:18 worker_processes; module.c:100-107 OnEnvStart per worker; module.c:298 /
// bridge.c:302 RunJob synchronous, one request at a time).  Protocol and rationale: include/impgpu_broker.h.
//
// Every broker thread is a lane of libimpgpu.so (its own stream, pools, pinned staging).  A thread takes ALL requests that
// are queued when it looks (up to --batch), so the number of files per launch follows the load by itself: one idle worker
// gets a batch of one (the latency of the in-process path plus two futex hops), 32 busy workers ride 16-32 to a launch.
// A batch is one straight pass: take, prepare, decode, operators, answers, finish --
//     files          impgpu_batch_decode_jpeg_prepared   cvDecodeImage, bridge.c:545-552
//                    impgpu_batch_decode_png (_ex with --png-accept all; --png-inflate device ORs
//                                                        IMPGPU_PNG_DEVICE_INFLATE into its mask: k_png_inflate)
//     GIF pages      impgpu_batch_gif_compose            LoadGIF's compositing, advancedio.c:204-247: all GIFs of the batch
//                                                        in one upload and one launch; each becomes an album
//     FreeImage bits impgpu_image_upload_fi32            LoadSingle, advancedio.c:295-318 (one by one, like frames)
//     operators      impgpu_batch_run_ops                bridge.c:574-656: crop -> resize -> rotate -> watermark -> flatten
//                                                        chains share one launch per channel count; anything else runs
//                                                        request by request (impgpu_run_ops) inside the same call
//     JPEG answers   impgpu_batch_encode_jpeg            cvEncodeImage(".jpg"), bridge.c:704
//     PNG answers    impgpu_batch_encode_png             cvEncodeImage(".png"), bridge.c:704
//     pixel answers  impgpu_batch_download               for the host encoders (PNG, WebP, FreeImage formats)
//     album answers  impgpu_batch_album_download         every frame of every many-frame answer of the batch, one wait
//     FreeImage ans. impgpu_batch_download_fi            IplToFI32 / IplToFI24, advancedio.c:65-101, every frame of every
//                                                        such answer of the batch: a launch per (channels, bpp), one wait
//     json answers   impgpu_batch_calc_perceived_brightness   Info(), bridge.c:283-300 (two or more; one: the lone call)
//     text answers   impgpu_batch_ascii                  ASCII(), bridge.c:668-676 (likewise)
// Nothing a worker writes into its slot is trusted further than a request is: the request record is copied out of shared
// memory once and validated (sizes against the slot, offsets against the text area, frame geometry and GIF page records against the bytes), and
// the answer's placement is the broker's own: it is written to the slot for the worker and never read back from there.
//
//   impgpu_broker [--name /impgpu-broker-0] [--device 0] [--slots 64] [--slot-mb 32] [--register-mb 8] [--threads 2] [--batch 64]
//                 [--gather-us 0] [--png-accept none|all] [--png-inflate host|device] [--jpeg-accept none|progressive]
//                 [--webp-accept none|lossless|all|alpha] [--supervise]
//                 [--ready-file PATH]
// --supervise: this process only forks and watches; the child is the broker.  A child that dies (a lost device, a bug) is
// replaced by a FRESH child -- fork() from a parent that never touched the GPU, no exec of a process that did.
#include <impgpu_broker.h>
#include "imp_broker_check.h"

#include <errno.h>
#include <fcntl.h>
#include <linux/futex.h>
#include <signal.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/syscall.h>
#include <sys/wait.h>
#include <time.h>
#include <unistd.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace {

struct Options {
    std::string name = IMPB_DEFAULT_NAME;
    int device = 0;
    int slots = 64;
    long slot_mb = 32;
    long register_mb = 8;               // page-locked at the front of every slot (0: none)
    // (Measured and removed: a lane that unpacks the next batch while the device writes the answers of the one before -- one
    // box, four lanes, requests/s at 8 / 16 / 32 workers: 11.5 / 15.6 / 21.1 k against 11.7 / 16.7 / 23.0 k one batch at a time.
    // The device idles less, and it does not matter: with N synchronous workers the rate is N / latency, and a request whose
    // lane also unpacks its successor and hands out its predecessor waits longer for its own answer.  Launches of one size
    // class only: DESIGN.md section 6.)
    // (Also measured and not kept: the frames taken ahead of their verdicts -- impgpu_batch_decode_jpeg_pending -- so that a batch's
    // operators and answers are enqueued behind its decode and the lane waits once.  From C, in process, a lone request gains 8-11 us
    // (tests/c/latency_harness.c); through the broker a lone worker's request is level (p50 0.36 ms both ways) and under load the
    // lanes lose: 7.5 / 10.7 / 14.9 / 17.8 k requests/s at 4 / 8 / 16 / 32 workers against 8.6 / 11.9 / 16.8 / 23.5 k.)
    int threads = 2;
    int batch = 64;
    int gather_us = 0;
    // --png-accept all: the batch's PNG uploads go through impgpu_batch_decode_png_ex with IMPGPU_PNG_ALL (palette, 1/2/4-bit
    // gray, Adam7); none (the default) keeps the kinds impgpu_batch_decode_png takes.  Refusals are NOT_TAKEN either way.
    int png_accept = 0;
    // --png-inflate device: IMPGPU_PNG_DEVICE_INFLATE is ORed into that mask -- the uploads' zlib streams are inflated on the
    // device (one wavefront per stream) instead of on this thread and its helpers; the same files are taken and the same
    // answers given (the call then waits for the streams' verdicts).  host (the default) keeps the host inflate.  Independent
    // of --png-accept.
    int png_inflate = 0;
    // --jpeg-accept progressive: the batch's JPEG uploads go through impgpu_batch_decode_jpeg_prepared_begin_ex with
    // IMPGPU_JPEG_PROGRESSIVE, so a progressive upload (which the workers pass on whole) is answered instead of NOT_TAKEN;
    // none (the default) keeps impgpu_batch_decode_jpeg_prepared.
    int jpeg_accept = 0;
    // --webp-accept lossless: an IMPB_IN_FILE request whose bytes start RIFF....WEBP joins the batch's one
    // impgpu_batch_decode_webp call (lossless VP8L, decoded on the device); what that call refuses -- a lossy or animated
    // file, damage -- is NOT_TAKEN like the other decode refusals.  none (the default): such a file is NOT_TAKEN as before.
    // alpha: all, and IMPGPU_WEBP_ACCEPT_ALPHA too (VP8X + ALPH + `VP8 `); under all such a file stays NOT_TAKEN.
    int webp_accept = 0;                  // 1 lossless, 2 all: the lossy bit goes to that one call too (VP8 key frames), 3 alpha
    bool supervise = false;
    std::string ready_file;
};

struct Segment {
    uint8_t* base = nullptr;
    size_t bytes = 0;
    impb_header_fields* h = nullptr;
    impb_slot* slots = nullptr;
    uint8_t* data = nullptr;
    uint64_t slot_bytes = 0;
    uint64_t registered = 0;            // the first so many bytes of every slot's data area are page-locked (copies to the device start there)
    uint8_t* slot_data(int i) const { return data + (uint64_t)i * slot_bytes; }
};

std::atomic<bool> g_stop{false};
// where a batch's time goes (microseconds, summed over all batches; printed when the broker stops)
std::atomic<uint64_t> g_us_prepare{0}, g_us_decode{0}, g_us_ops{0}, g_us_answer{0}, g_us_idle{0};
void on_signal(int) { g_stop = true; }

long futex(volatile uint32_t* addr, int op, uint32_t val, const timespec* to) {
    return syscall(SYS_futex, addr, op, val, to, nullptr, 0);
}
bool pid_alive(uint32_t pid) { return pid != 0 && (kill((pid_t)pid, 0) == 0 || errno == EPERM); }
double now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e6 * (double)ts.tv_sec + 1e-3 * (double)ts.tv_nsec;
}
template <class T> T aload(volatile T* p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); }
template <class T> void astore(volatile T* p, T v) { __atomic_store_n(p, v, __ATOMIC_RELEASE); }

// ---- the segment: created, or adopted when one with the same geometry is already there (workers keep their mapping and
// their slots across a broker restart)
bool open_segment(const Options& o, Segment* S) {
    const uint64_t slot_bytes = (uint64_t)o.slot_mb << 20;
    const uint64_t slots_offset = sizeof(impb_header);
    const uint64_t data_offset = slots_offset + (uint64_t)o.slots * sizeof(impb_slot);
    const uint64_t total = data_offset + (uint64_t)o.slots * slot_bytes;
    bool fresh = false;
    int fd = shm_open(o.name.c_str(), O_RDWR, 0600);
    if (fd >= 0) {
        struct stat st;
        impb_header hdr;
        const bool same = fstat(fd, &st) == 0 && (uint64_t)st.st_size == total && pread(fd, &hdr, sizeof hdr, 0) == (ssize_t)sizeof hdr &&
                          hdr.f.magic == IMPB_MAGIC && hdr.f.version == IMPB_VERSION && hdr.f.nslots == (uint32_t)o.slots &&
                          hdr.f.slot_data_bytes == slot_bytes;
        if (same && pid_alive(hdr.f.broker_pid) && hdr.f.broker_pid != (uint32_t)getpid()) {
            std::fprintf(stderr, "impgpu_broker: %s is served by pid %u\n", o.name.c_str(), hdr.f.broker_pid);
            close(fd);
            return false;
        }
        if (!same) {                       // another layout: workers of the old one find a dead broker and re-open by name
            close(fd);
            shm_unlink(o.name.c_str());
            fd = -1;
        }
    }
    if (fd < 0) {
        fd = shm_open(o.name.c_str(), O_RDWR | O_CREAT | O_EXCL, 0600);
        if (fd < 0) { std::perror("impgpu_broker: shm_open"); return false; }
        if (ftruncate(fd, (off_t)total) != 0) { std::perror("impgpu_broker: ftruncate"); close(fd); shm_unlink(o.name.c_str()); return false; }
        fresh = true;
    }
    void* p = mmap(nullptr, total, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    close(fd);
    if (p == MAP_FAILED) { std::perror("impgpu_broker: mmap"); return false; }
    S->base = (uint8_t*)p; S->bytes = total;
    S->h = &((impb_header*)p)->f;
    S->slots = (impb_slot*)(S->base + slots_offset);
    S->data = S->base + data_offset;
    S->slot_bytes = slot_bytes;
    impb_header_fields* h = S->h;
    astore(&h->broker_pid, 0u);
    if (fresh) {
        h->magic = IMPB_MAGIC; h->version = IMPB_VERSION; h->nslots = (uint32_t)o.slots;
        h->slot_data_bytes = slot_bytes; h->slots_offset = slots_offset; h->data_offset = data_offset;
        h->epoch = 0;
    }
    __atomic_add_fetch(&h->epoch, 1u, __ATOMIC_SEQ_CST);
    h->device = (uint32_t)o.device;
    h->served = 0; h->batches = 0; h->sleepers = 0;
    // requests the previous broker died with: answered "device lost"; slots of dead workers: free
    for (int i = 0; i < o.slots; i++) {
        impb_slot_fields* s = &S->slots[i].f;
        const uint32_t st = aload(&s->state), owner = aload(&s->owner_pid);
        if (st == IMPB_FREE) continue;
        if (owner && !pid_alive(owner)) { astore(&s->owner_pid, 0u); astore(&s->state, (uint32_t)IMPB_FREE); continue; }
        if (st == IMPB_SUBMITTED || st == IMPB_TAKEN) {
            s->code = IMP_ERROR_DEVICE; s->step = IMP_STEP_START; s->out_bytes = 0; s->out_offset = 0;
            std::snprintf(s->error, sizeof s->error, "the broker was restarted");
            astore(&s->state, (uint32_t)IMPB_DONE);
            futex(&s->state, FUTEX_WAKE, 1, nullptr);
        }
    }
    return true;
}

// ---- one request, copied out of its slot
struct Req {
    int slot = -1;
    impb_slot_fields q;                 // private copy of the record (the strings included)
    const uint8_t* in = nullptr;        // the slot's data area (shared: read once by the decoder)
    impgpu_image* img = nullptr;
    int code = IMP_OK, step = IMP_STEP_START;
    bool done = false;                  // the answer is final (an error, NOT_TAKEN, a registration)
    std::string err;
    std::vector<const char*> filters;
    impgpu_job job{};
    impgpu_config cfg{};
    double t_taken = 0;
    // the answer, copied into the slot by finish() (the slot is shared memory: nothing here is read back from it)
    uint64_t out_offset = 0, out_bytes = 0;
    uint64_t cap = 0;                   // bytes from out_offset to the end of the slot's data area (0: none)
    int32_t out_w = 0, out_h = 0, out_c = 0, out_step = 0;
    int32_t out_frames = 0;
    uint64_t out_frame_stride = 0;
    float brightness = 0;
    std::vector<impb_gif_page> pages;   // IMPB_IN_GIF: the record table, copied out and checked (imp_broker_check.h)
    std::vector<impgpu_gif_page> gif;   // ... and as the library takes it: pointers into the slot's input
    bool fits(uint64_t need) const { return cap > 0 && cap >= need; }
};

struct Watermarks {
    std::mutex mu;
    std::vector<impgpu_image*> imgs;    // id - 1 -> frame (lives as long as the broker: a location's overlay)
} g_marks;

bool text_ok(const impb_slot_fields&, int at) { return at == -1 || (at >= 0 && at < IMPB_TEXT_BYTES); }

void fail(Req& r, int code, int step, const char* what) {
    r.code = code; r.step = step; r.done = true;
    r.err = what ? what : "";
}

// validate + build job / config out of the private copy
void prepare(Req& r, const Segment& S) {
    impb_slot_fields& q = r.q;
    q.text[IMPB_TEXT_BYTES - 1] = 0;
    if (q.in_bytes > S.slot_bytes) return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "in_bytes past the slot");
    if (q.in_kind > IMPB_IN_FI32 || q.out_kind > IMPB_OUT_FI) return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "unknown kind");
    if (q.filter_count < 0 || q.filter_count > IMPB_MAX_FILTERS || !text_ok(q, q.crop_at) || !text_ok(q, q.gravity_at) || !text_ok(q, q.resize_at) || !text_ok(q, q.ascii_at))
        return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "bad text offsets");
    for (int i = 0; i < q.filter_count; i++) {
        if (q.filter_at[i] < 0 || q.filter_at[i] >= IMPB_TEXT_BYTES) return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "bad filter offset");
        r.filters.push_back(q.text + q.filter_at[i]);
    }
    if (q.in_scan_bytes) {              // a JPEG whose scan the worker has unstuffed (impgpu_jpeg_unstuff)
        if (q.in_kind != IMPB_IN_FILE || q.in_head_bytes < 4 || q.in_head_bytes > q.in_scan_at || (q.in_scan_at & 255) || q.in_scan_at > q.in_bytes ||
            q.in_scan_bytes > q.in_bytes - q.in_scan_at || q.in_bytes - q.in_scan_at - q.in_scan_bytes < IMPGPU_JPEG_SCAN_TAIL)
            return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "prepared file: offsets past its bytes");
    }
    if (q.out_kind == IMPB_OUT_FI && q.quality != 24 && q.quality != 32) return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "a FreeImage answer is 24 or 32 bits");
    if (q.in_kind == IMPB_IN_GIF) {
        int frames = 0;
        uint64_t frame_bytes = 0;
        const impb::GifVerdict v = impb::check_gif(r.in, q.in_bytes, S.slot_bytes, q.in_pages, q.in_page, &r.pages, &frames, &frame_bytes);
        if (v == impb::GIF_INVALID) return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_DECODE, "GIF pages: a record does not match the input's bytes");
        if (v == impb::GIF_TOO_LARGE) return fail(r, IMP_ERROR_MALLOC_FAILED, IMP_STEP_ENCODE, "answer does not fit the slot");
        r.gif.resize(r.pages.size());
        for (size_t f = 0; f < r.pages.size(); f++) {
            const impb_gif_page& p = r.pages[f];
            r.gif[f] = impgpu_gif_page{r.in + p.indices_at, p.width, p.height, p.pitch, p.left, p.top, p.dispose, p.transparency_key, r.in + p.palette_at};
        }
    } else if (q.in_kind == IMPB_IN_FI32) {
        const long long need = (long long)q.in_step * q.in_h;
        if (q.in_w <= 0 || q.in_h <= 0 || (long long)q.in_step < (long long)q.in_w * 4 || need <= 0 || (unsigned long long)need > q.in_bytes)
            return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "bitmap geometry does not match its bytes");
    } else if (q.in_kind != IMPB_IN_FILE) {
        const long long need = (long long)q.in_step * q.in_h;
        if (q.in_w <= 0 || q.in_h <= 0 || (q.in_c != 1 && q.in_c != 3 && q.in_c != 4) || (long long)q.in_step < (long long)q.in_w * q.in_c ||
            need <= 0 || (unsigned long long)need > q.in_bytes)
            return fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_VALIDATE, "frame geometry does not match its bytes");
    }
    r.job.crop = q.crop_at >= 0 ? q.text + q.crop_at : nullptr;
    r.job.gravity = q.gravity_at >= 0 ? q.text + q.gravity_at : nullptr;
    r.job.resize = q.resize_at >= 0 ? q.text + q.resize_at : nullptr;
    r.job.simple = q.simple; r.job.need_flatten = q.need_flatten;
    r.job.filters = r.filters.data(); r.job.filter_count = q.filter_count;
    r.cfg.max_target_w = q.max_target_w; r.cfg.max_target_h = q.max_target_h;
    r.cfg.max_filters_count = q.max_filters_count; r.cfg.allow_experiments = q.allow_experiments;
    if (q.watermark_id) {
        std::lock_guard<std::mutex> lk(g_marks.mu);
        if (q.watermark_id < 0 || (size_t)q.watermark_id > g_marks.imgs.size())
            return fail(r, IMP_ERROR_NO_SUCH_WATERMARK, IMP_STEP_WATERMARK, "watermark id of another broker epoch");
        r.cfg.watermark = g_marks.imgs[(size_t)q.watermark_id - 1];
        r.cfg.watermark_opacity = q.watermark_opacity;
        r.cfg.watermark_gravity_x = q.watermark_gravity_x; r.cfg.watermark_gravity_y = q.watermark_gravity_y;
        r.cfg.watermark_offset_x = q.watermark_offset_x; r.cfg.watermark_offset_y = q.watermark_offset_y;
    }
}

bool is_jpeg(const uint8_t* p, uint64_t n) { return n >= 3 && p[0] == 0xFF && p[1] == 0xD8 && p[2] == 0xFF; }
bool is_webp(const uint8_t* p, uint64_t n) { return n >= 12 && !std::memcmp(p, "RIFF", 4) && !std::memcmp(p + 8, "WEBP", 4); }
bool is_png(const uint8_t* p, uint64_t n) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    return n >= 8 && !std::memcmp(p, sig, 8);
}

struct Worker {
    const Segment& S;
    const Options& O;
    int id;
    // scratch reused from batch to batch
    std::vector<Req> reqs;
    std::vector<impgpu_image*> imgs;
    std::vector<int> codes, steps;
    std::vector<size_t> jpegs, pngs, live;
    std::vector<impgpu_jpeg_prepared> pre;
    std::vector<const unsigned char*> png_blobs;
    std::vector<size_t> png_sizes;
    std::vector<impgpu_job> jobs;
    std::vector<const impgpu_config*> cfgs;
    std::vector<size_t> gifs;
    std::vector<impgpu_gif_set> gif_sets;

    Worker(const Segment& s, const Options& o, int i) : S(s), O(o), id(i) {}

    int take(std::vector<int>& mine, int start) {
        const int n = (int)S.h->nslots;
        int got = 0;
        for (int k = 0; k < n && (int)mine.size() < O.batch; k++) {
            const int i = (start + k) % n;
            impb_slot_fields* s = &S.slots[i].f;
            if (aload(&s->state) != IMPB_SUBMITTED) continue;
            uint32_t expect = IMPB_SUBMITTED;
            if (__atomic_compare_exchange_n(&s->state, &expect, (uint32_t)IMPB_TAKEN, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) {
                mine.push_back(i);
                got++;
            }
        }
        return got;
    }

    void finish(Req& r, int batch_size) {
        impb_slot_fields* s = &S.slots[r.slot].f;
        s->code = r.code; s->step = r.step;
        s->out_offset = r.out_offset; s->out_bytes = r.out_bytes;
        s->out_w = r.out_w; s->out_h = r.out_h; s->out_c = r.out_c; s->out_step = r.out_step;
        s->brightness = r.brightness;
        s->out_frames = r.out_frames; s->out_frame_stride = r.out_frame_stride;
        s->batch_size = (int32_t)batch_size;
        std::snprintf(s->error, sizeof s->error, "%s", r.err.c_str());
        s->broker_us = (uint32_t)(now_us() - r.t_taken);
        impgpu_image_release(&r.img);
        __atomic_add_fetch(&S.h->served, (uint64_t)1, __ATOMIC_RELAXED);
        if (aload(&s->owner_pid) == 0) { astore(&s->state, (uint32_t)IMPB_FREE); return; }     // abandoned by a worker that timed out
        astore(&s->state, (uint32_t)IMPB_DONE);
        futex(&s->state, FUTEX_WAKE, 1, nullptr);
    }

    // A decode call's verdicts: a file the device does not take goes back to the worker as NOT_TAKEN.
    void decoded(const std::vector<size_t>& who, int rc) {
        for (size_t j = 0; j < who.size(); j++) {
            Req& r = reqs[who[j]];
            const int c = rc != IMP_OK ? rc : codes[j];
            if (c == IMP_OK) { r.img = imgs[j]; continue; }
            if (c == IMP_ERROR_UNSUPPORTED || c == IMP_ERROR_DECODE_FAILED) fail(r, IMPB_NOT_TAKEN, IMP_STEP_DECODE, "not a file the device decodes");
            else fail(r, c, IMP_STEP_DECODE, impgpu_last_error());
        }
    }

    // The json exit (Info(), bridge.c:283-300) of the requests `who`: one impgpu_batch_calc_perceived_brightness -- one wait
    // for all of them instead of one each.  (A lane's batch is at most --batch <= 256 requests, which is what the call takes.)
    // A list of one keeps the lone call.  For the json exit that is also what the measurement says: at count 1 the batch
    // call loses the descriptor table's upload and the staging buffer (94 against 90 us), at count 2 it wins (95 against
    // 168; profiles/r09_info_batch_probe.jsonl).  For the text exit it is the rule alone -- a lone request keeps the path it
    // always had: the recorded count = 1 row has the batch call ahead (20 against 29 us; impgpu_ascii allocates twice and
    // waits on the stream itself).
    static constexpr size_t INFO_BATCH_MIN = 2, TEXT_BATCH_MIN = 2;
    void answer_info(const std::vector<size_t>& who) {
        if (who.size() < INFO_BATCH_MIN) {
            for (size_t k : who) {
                Req& r = reqs[k];
                float b = 0;
                const int rc = impgpu_calc_perceived_brightness(r.img, &b);
                if (rc != IMP_OK) { fail(r, rc, IMP_STEP_INFO, impgpu_last_error()); continue; }
                r.brightness = b;
                r.code = IMP_OK; r.done = true;
            }
            return;
        }
        const size_t m = who.size();
        std::vector<const impgpu_image*> im(m);
        std::vector<float> vals(m, 0.f);
        std::vector<int> cs(m, IMP_OK);
        for (size_t j = 0; j < m; j++) im[j] = reqs[who[j]].img;
        const int rc = impgpu_batch_calc_perceived_brightness(im.data(), (int)m, vals.data(), cs.data(), nullptr);
        for (size_t j = 0; j < m; j++) {
            Req& r = reqs[who[j]];
            const int c = rc != IMP_OK ? rc : cs[j];
            if (c != IMP_OK) { fail(r, c, IMP_STEP_INFO, impgpu_last_error()); continue; }
            r.brightness = vals[j];
            r.code = IMP_OK; r.done = true;
        }
    }

    // The text exit (ASCII(), bridge.c:668-676) of the requests `who` (each fits its slot: checked where they were collected):
    // one impgpu_batch_ascii, the texts straight into the slots at slot_data + out_offset.  The argument string comes from the
    // private copy in Req, never from the slot.
    void answer_text(const std::vector<size_t>& who) {
        auto arg_of = [](const Req& r) { return r.q.ascii_at >= 0 ? r.q.text + r.q.ascii_at : ""; };
        if (who.size() < TEXT_BATCH_MIN) {
            for (size_t k : who) {
                Req& r = reqs[k];
                const long need = (long)(r.out_w + 1) * r.out_h - 1;
                long len = 0;
                const int rc = impgpu_ascii(r.img, arg_of(r), S.slot_data(r.slot) + r.out_offset, need, &len);
                if (rc != IMP_OK) { fail(r, rc, IMP_STEP_INFO, rc == IMP_ERROR_DEVICE ? impgpu_last_error() : ""); continue; }
                r.out_bytes = (uint64_t)len;
                r.code = IMP_OK; r.done = true;
            }
            return;
        }
        const size_t m = who.size();
        std::vector<impgpu_image*> im(m);
        std::vector<const char*> args(m);
        std::vector<unsigned char*> outs(m);
        std::vector<long> caps(m), lens(m, 0);
        std::vector<int> cs(m, IMP_OK);
        for (size_t j = 0; j < m; j++) {
            const Req& r = reqs[who[j]];
            im[j] = r.img;
            args[j] = arg_of(r);
            outs[j] = S.slot_data(r.slot) + r.out_offset;
            caps[j] = (long)(r.out_w + 1) * r.out_h - 1;
        }
        const int rc = impgpu_batch_ascii(im.data(), args.data(), (int)m, outs.data(), caps.data(), lens.data(), cs.data(), nullptr);
        for (size_t j = 0; j < m; j++) {
            Req& r = reqs[who[j]];
            const int c = rc != IMP_OK ? rc : cs[j];
            if (c != IMP_OK) { fail(r, c, IMP_STEP_INFO, c == IMP_ERROR_DEVICE ? impgpu_last_error() : ""); continue; }
            r.out_bytes = (uint64_t)lens[j];
            r.code = IMP_OK; r.done = true;
        }
    }

    // One batched answer call for the requests `who`, from their placement in Req: call(images, count, outs, capacities,
    // steps, lengths, codes) -> IMP_*.  An answer that came back goes out with its length, a failure with the library's error.
    template <class Call>
    void answer(const std::vector<size_t>& who, Call call) {
        const size_t m = who.size();
        if (!m) return;
        std::vector<const impgpu_image*> im(m);
        std::vector<unsigned char*> outs(m);
        std::vector<size_t> caps(m), lens(m);
        std::vector<int> row_steps(m), cs(m, IMP_OK);
        for (size_t j = 0; j < m; j++) {
            const Req& r = reqs[who[j]];
            im[j] = r.img;
            outs[j] = S.slot_data(r.slot) + r.out_offset;
            caps[j] = (size_t)r.cap;
            row_steps[j] = r.out_step;
            lens[j] = (size_t)r.out_bytes;
        }
        const int rc = call(im.data(), (int)m, outs.data(), caps.data(), row_steps.data(), lens.data(), cs.data());
        for (size_t j = 0; j < m; j++) {
            Req& r = reqs[who[j]];
            const int c = rc != IMP_OK ? rc : cs[j];
            if (c != IMP_OK) { fail(r, c, IMP_STEP_ENCODE, impgpu_last_error()); continue; }
            r.out_bytes = lens[j];
            r.code = IMP_OK; r.step = IMP_STEP_ENCODE; r.done = true;
        }
    }

    void run(const std::vector<int>& mine) {
        const size_t n = mine.size();
        const double t0 = now_us();
        reqs.clear();
        reqs.resize(n);
        for (size_t k = 0; k < n; k++) {
            Req& r = reqs[k];
            r.slot = mine[k];
            std::memcpy(&r.q, (const void*)&S.slots[r.slot].f, sizeof r.q);
            r.in = S.slot_data(r.slot);
            r.t_taken = t0;
            prepare(r, S);
        }
        __atomic_add_fetch(&S.h->batches, (uint64_t)1, __ATOMIC_RELAXED);
        const double t1 = now_us();
        g_us_prepare += (uint64_t)(t1 - t0);

        // ---- decode (bridge.c:541-572): all JPEG files of the batch in one call, then all PNG files in one call
        jpegs.clear(); pre.clear();
        for (size_t k = 0; k < n; k++) {
            Req& r = reqs[k];
            if (r.done) continue;
            r.step = IMP_STEP_DECODE;
            if (r.q.in_kind != IMPB_IN_FILE || !is_jpeg(r.in, r.q.in_bytes)) continue;
            jpegs.push_back(k);
            impgpu_jpeg_prepared f{r.in, (size_t)r.q.in_bytes, nullptr, 0, 0};
            if (r.q.in_scan_bytes) {
                // (its bytes go to the device from the slot when they lie in its page-locked part; the worker sleeps until DONE)
                f.head_size = (size_t)r.q.in_head_bytes;
                f.scan = r.in + r.q.in_scan_at;
                f.scan_size = (size_t)r.q.in_scan_bytes;
                f.registered = r.q.in_scan_at + r.q.in_scan_bytes + IMPGPU_JPEG_SCAN_TAIL <= S.registered;
            }
            pre.push_back(f);
        }
        if (!jpegs.empty()) {
            imgs.assign(jpegs.size(), nullptr);
            codes.assign(jpegs.size(), IMP_OK);
            if (!O.jpeg_accept) decoded(jpegs, impgpu_batch_decode_jpeg_prepared(pre.data(), (int)jpegs.size(), imgs.data(), codes.data()));
            else {
                // (a lane's batch is at most --batch requests; the two-halves call takes 256 files)
                impgpu_jpeg_batch* jb = nullptr;
                int rc = jpegs.size() <= 256 ? impgpu_batch_decode_jpeg_prepared_begin_ex(pre.data(), (int)jpegs.size(), O.jpeg_accept, &jb) : IMP_ERROR_INVALID_ARGS;
                if (rc == IMP_OK) rc = impgpu_batch_decode_jpeg_finish(&jb, imgs.data(), codes.data());
                decoded(jpegs, rc);
            }
        }
        // (after the JPEG call: both are on the lane's stream, and the PNG call's inflates could overlap the JPEG kernels if
        // issued before it -- not done, DESIGN.md section 8 says why)
        pngs.clear();
        for (size_t k = 0; k < n; k++) {
            const Req& r = reqs[k];
            if (!r.done && !r.img && r.q.in_kind == IMPB_IN_FILE && is_png(r.in, r.q.in_bytes)) pngs.push_back(k);
        }
        if (!pngs.empty()) {
            const size_t m = pngs.size();
            png_blobs.resize(m);
            png_sizes.resize(m);
            imgs.assign(m, nullptr);
            codes.assign(m, IMP_OK);
            for (size_t j = 0; j < m; j++) {
                png_blobs[j] = reqs[pngs[j]].in;
                png_sizes[j] = (size_t)reqs[pngs[j]].q.in_bytes;
            }
            decoded(pngs, impgpu_batch_decode_png_ex(png_blobs.data(), png_sizes.data(), (int)m, O.png_accept | O.png_inflate, imgs.data(), codes.data(), nullptr));
        }
        // --webp-accept lossless: every WebP upload of the batch in ONE impgpu_batch_decode_webp call, behind the PNG call
        if (O.webp_accept) {
            std::vector<size_t> webps;
            for (size_t k = 0; k < n; k++) {
                const Req& r = reqs[k];
                if (!r.done && !r.img && r.q.in_kind == IMPB_IN_FILE && is_webp(r.in, r.q.in_bytes)) webps.push_back(k);
            }
            if (!webps.empty()) {
                const size_t m = webps.size();
                std::vector<const unsigned char*> blobs(m);
                std::vector<size_t> sizes(m);
                imgs.assign(m, nullptr);
                codes.assign(m, IMP_OK);
                for (size_t j = 0; j < m; j++) {
                    blobs[j] = reqs[webps[j]].in;
                    sizes[j] = (size_t)reqs[webps[j]].q.in_bytes;
                }
                decoded(webps, impgpu_batch_decode_webp_ex(blobs.data(), sizes.data(), (int)m, O.webp_accept == 3 ? IMPGPU_WEBP_ACCEPT_LOSSY | IMPGPU_WEBP_ACCEPT_ALPHA : O.webp_accept == 2 ? IMPGPU_WEBP_ACCEPT_LOSSY : 0, imgs.data(), codes.data(), nullptr));
            }
        }
        // every GIF of the batch: one upload of all their pages and ONE compose launch (advancedio.c:204-247), behind the file
        // decodes on the lane's stream.  The answer's image is the album; a page request (in_page >= 0) makes an album of one.
        gifs.clear();
        for (size_t k = 0; k < n; k++) if (!reqs[k].done && reqs[k].q.in_kind == IMPB_IN_GIF) gifs.push_back(k);
        if (!gifs.empty()) {
            const size_t m = gifs.size();
            gif_sets.resize(m);
            imgs.assign(m, nullptr);
            codes.assign(m, IMP_OK);
            for (size_t j = 0; j < m; j++) {
                const Req& r = reqs[gifs[j]];
                gif_sets[j] = impgpu_gif_set{r.gif.data(), (int)r.gif.size(), r.q.in_destructive, r.q.in_page};
            }
            // (a lane's batch is at most --batch <= 256 requests, which is what the call takes)
            const int rc = impgpu_batch_gif_compose(gif_sets.data(), (int)m, imgs.data(), codes.data(), nullptr);
            for (size_t j = 0; j < m; j++) {
                Req& r = reqs[gifs[j]];
                const int c = rc != IMP_OK ? rc : codes[j];
                if (c == IMP_OK) r.img = imgs[j];
                else fail(r, c, IMP_STEP_DECODE, c == IMP_ERROR_DEVICE ? impgpu_last_error() : "pages the compose call does not take");
            }
        }
        for (size_t k = 0; k < n; k++) {
            Req& r = reqs[k];
            if (r.done || r.img) continue;
            int rc = IMP_OK;
            if (r.q.in_kind == IMPB_IN_FILE) { fail(r, IMPB_NOT_TAKEN, IMP_STEP_DECODE, "neither JPEG nor PNG"); continue; }
            if (r.q.in_kind == IMPB_IN_FI32) rc = impgpu_image_upload_fi32(r.in, r.q.in_w, r.q.in_h, r.q.in_step, &r.img);      // LoadSingle, advancedio.c:310-318
            else rc = impgpu_image_upload(r.in, r.q.in_w, r.q.in_h, r.q.in_c, r.q.in_step, &r.img);
            if (rc != IMP_OK) { fail(r, rc, IMP_STEP_DECODE, impgpu_last_error()); continue; }
            if (r.q.in_kind == IMPB_IN_WATERMARK) {             // PrepareWatermark (bridge.c:199-237): kept, answered with its id
                std::lock_guard<std::mutex> lk(g_marks.mu);
                g_marks.imgs.push_back(r.img);
                r.img = nullptr;
                r.out_w = (int32_t)g_marks.imgs.size();
                r.code = IMP_OK; r.step = IMP_STEP_INFO; r.done = true;
            }
        }
        // a registered overlay must be complete before another lane's request reads it
        for (size_t k = 0; k < n; k++) if (reqs[k].q.in_kind == IMPB_IN_WATERMARK && reqs[k].code == IMP_OK) { (void)impgpu_sync(); break; }

        const double t2 = now_us();
        g_us_decode += (uint64_t)(t2 - t1);
        // ---- operators (bridge.c:574-656): every live request in ONE call -- the chains the mixed launch takes share a launch
        // per channel count, the rest run request by request inside it
        live.clear();
        for (size_t k = 0; k < n; k++) if (!reqs[k].done) live.push_back(k);
        if (!live.empty()) {
            const size_t m = live.size();
            imgs.resize(m);
            jobs.resize(m);
            cfgs.resize(m);
            codes.assign(m, IMP_OK);
            steps.assign(m, IMP_STEP_START);
            for (size_t j = 0; j < m; j++) {
                Req& r = reqs[live[j]];
                imgs[j] = r.img; jobs[j] = r.job; cfgs[j] = &r.cfg;
            }
            const int rc = impgpu_batch_run_ops(imgs.data(), jobs.data(), cfgs.data(), (int)m, codes.data(), steps.data(), nullptr);
            for (size_t j = 0; j < m; j++) {
                Req& r = reqs[live[j]];
                if (rc != IMP_OK) { fail(r, rc, IMP_STEP_START, impgpu_last_error()); continue; }
                r.img = imgs[j];
                if (codes[j] != IMP_OK) fail(r, codes[j], steps[j], codes[j] == IMP_ERROR_DEVICE ? impgpu_last_error() : "");
            }
        }

        const double t3 = now_us();
        g_us_ops += (uint64_t)(t3 - t2);
        // ---- answers (bridge.c:659-710): placed right behind the request's input in its slot
        std::map<int, std::vector<size_t>> by_quality;
        std::vector<size_t> raw, many, png, info, text;
        for (size_t k = 0; k < n; k++) {
            Req& r = reqs[k];
            if (r.done) continue;
            r.out_w = impgpu_image_width(r.img); r.out_h = impgpu_image_height(r.img); r.out_c = impgpu_image_channels(r.img);
            r.out_offset = (r.q.in_bytes + 63) & ~uint64_t(63);
            r.cap = r.out_offset < S.slot_bytes ? S.slot_bytes - r.out_offset : 0;
            if (r.q.out_kind == IMPB_OUT_INFO) {
                r.step = IMP_STEP_INFO;
                info.push_back(k);
            } else if (r.q.out_kind == IMPB_OUT_ASCII) {            // the text exit (bridge.c:669-670): (width + 1) * height - 1 characters
                r.step = IMP_STEP_INFO;
                const long need = (long)(r.out_w + 1) * r.out_h - 1;
                if (!r.fits((uint64_t)(need > 0 ? need : 1))) { fail(r, IMP_ERROR_MALLOC_FAILED, IMP_STEP_INFO, "answer does not fit the slot"); continue; }
                text.push_back(k);
            } else if (r.q.out_kind == IMPB_OUT_JPEG) {
                r.step = IMP_STEP_ENCODE;
                if (!r.fits(impgpu_jpeg_encode_bound(r.out_w, r.out_h, r.out_c))) { fail(r, IMP_ERROR_MALLOC_FAILED, IMP_STEP_ENCODE, "answer does not fit the slot"); continue; }
                by_quality[r.q.quality].push_back(k);
            } else if (r.q.out_kind == IMPB_OUT_PNG) {
                r.step = IMP_STEP_ENCODE;
                // levels 1..9 give one file (Z_RLE): every PNG answer of the batch goes into one call; the others are refused
                // here exactly as impgpu_image_encode_png refuses them
                if (r.q.quality == 0) { fail(r, IMP_ERROR_UNSUPPORTED, IMP_STEP_ENCODE, "PNG level 0 is encoded on the host"); continue; }
                if (r.q.quality < 1 || r.q.quality > 9) { fail(r, IMP_ERROR_INVALID_ARGS, IMP_STEP_ENCODE, "PNG level outside 0..9"); continue; }
                const size_t bound = impgpu_png_encode_bound(r.out_w, r.out_h, r.out_c);
                if (!bound) { fail(r, IMP_ERROR_UNSUPPORTED, IMP_STEP_ENCODE, "frame the device does not encode as PNG"); continue; }
                if (!r.fits(bound)) { fail(r, IMP_ERROR_MALLOC_FAILED, IMP_STEP_ENCODE, "answer does not fit the slot"); continue; }
                png.push_back(k);
            } else {
                // pixels: every frame of an album (an album of one, a single frame and a FreeImage answer alike: `many`),
                // a single frame for a host encoder as before (`raw`)
                r.step = IMP_STEP_ENCODE;
                const bool fi = r.q.out_kind == IMPB_OUT_FI;
                const uint64_t frames = (uint64_t)impgpu_album_count(r.img);
                const uint64_t row = fi ? (((uint64_t)r.out_w * (uint64_t)(r.q.quality / 8) + 3) & ~uint64_t(3)) : (uint64_t)impgpu_image_step(r.img);
                const uint64_t each = row * (uint64_t)r.out_h;
                if (!frames || !each || !r.fits(each) || frames > r.cap / each) { fail(r, IMP_ERROR_MALLOC_FAILED, IMP_STEP_ENCODE, "answer does not fit the slot"); continue; }
                r.out_step = (int32_t)row;
                r.out_bytes = each * frames;
                r.out_frames = (int32_t)frames; r.out_frame_stride = each;
                if (fi) r.out_c = r.q.quality / 8;
                if (fi || frames > 1) many.push_back(k);
                else raw.push_back(k);
            }
        }
        // one call per JPEG quality, the batch's most common one last; then the PNG answers, then pixels for host encoders
        int common = -1;
        size_t most = 0;
        for (auto& kv : by_quality) if (kv.second.size() > most) { most = kv.second.size(); common = kv.first; }
        auto jpeg = [](int quality) {
            return [quality](const impgpu_image* const* im, int m, unsigned char* const* outs, const size_t* caps, const int*, size_t* lens, int* cs) {
                return impgpu_batch_encode_jpeg(im, m, quality, outs, caps, lens, cs);
            };
        };
        for (auto& kv : by_quality)
            if (kv.first != common) answer(kv.second, jpeg(kv.first));
        answer(png, [](const impgpu_image* const* im, int m, unsigned char* const* outs, const size_t* caps, const int*, size_t* lens, int* cs) {
            return impgpu_batch_encode_png(im, m, 9, outs, caps, lens, cs);
        });
        answer(raw, [](const impgpu_image* const* im, int m, unsigned char* const* outs, const size_t*, const int* row_steps, size_t*, int*) {
            return impgpu_batch_download(im, m, outs, row_steps);
        });
        // album and FreeImage answers: the batch's FreeImage answers in one call, its many-frame albums in another -- every
        // frame of every request behind one transfer and one wait each (impgpu_batch_download_fi, impgpu_batch_album_download;
        // at most 256 handles a call)
        for (const bool fi : {true, false}) {
            std::vector<size_t> ks;
            for (size_t k : many) if ((reqs[k].q.out_kind == IMPB_OUT_FI) == fi) ks.push_back(k);
            for (size_t k0 = 0; k0 < ks.size(); k0 += 256) {
                const size_t m = std::min(ks.size() - k0, (size_t)256);
                std::vector<const impgpu_image*> imgs(m);
                std::vector<int> bpps(m), codes(m, IMP_OK), row_steps;
                std::vector<unsigned char*> at;
                for (size_t j = 0; j < m; j++) {
                    const Req& r = reqs[ks[k0 + j]];
                    imgs[j] = r.img;
                    bpps[j] = r.q.quality;
                    for (int32_t f = 0; f < r.out_frames; f++) {
                        at.push_back(S.slot_data(r.slot) + r.out_offset + (uint64_t)f * r.out_frame_stride);
                        row_steps.push_back(r.out_step);
                    }
                }
                const int rc = fi ? impgpu_batch_download_fi(imgs.data(), bpps.data(), (int)m, at.data(), row_steps.data(), codes.data(), nullptr)
                                  : impgpu_batch_album_download(imgs.data(), (int)m, at.data(), row_steps.data(), codes.data());
                for (size_t j = 0; j < m; j++) {
                    Req& r = reqs[ks[k0 + j]];
                    const int code = rc != IMP_OK ? rc : codes[j];
                    if (code != IMP_OK) { fail(r, code, IMP_STEP_ENCODE, impgpu_last_error()); continue; }
                    r.code = IMP_OK; r.done = true;
                }
            }
        }
        if (most) answer(by_quality[common], jpeg(common));
        // The json and text exits go LAST.  Each of the calls above and below ends in a wait of its own, and the lane's stream
        // is in order, so the order changes nobody's device time -- only how long the host sits in each wait.  The encoders'
        // calls carry most of a batch's device work; behind them the one-workgroup brightness walks and the texts are a short
        // tail, where in front they would hold back the enqueueing of everybody's encode (what the per-request calls in the
        // collecting loop used to do).  Nothing leaves before finish() below either way.
        answer_info(info);
        answer_text(text);
        for (size_t k = 0; k < n; k++) finish(reqs[k], (int)n);
        g_us_answer += (uint64_t)(now_us() - t3);
    }

    void loop() {
        impb_header_fields* h = S.h;
        std::vector<int> mine;
        int start = id * 7;
        while (!g_stop) {
            mine.clear();
            const uint32_t bell = __atomic_load_n(&h->doorbell, __ATOMIC_SEQ_CST);
            take(mine, start);
            if (mine.empty()) {
                const double idle0 = now_us();
                __atomic_add_fetch(&h->sleepers, 1u, __ATOMIC_SEQ_CST);
                take(mine, start);                          // (a submit between the scan and the count)
                if (mine.empty()) {
                    timespec tick{0, 100 * 1000 * 1000};
                    futex(&h->doorbell, FUTEX_WAIT, bell, &tick);
                }
                __atomic_sub_fetch(&h->sleepers, 1u, __ATOMIC_SEQ_CST);
                g_us_idle += (uint64_t)(now_us() - idle0);
                if (mine.empty()) continue;
            }
            if (O.gather_us > 0 && (int)mine.size() < O.batch) {
                // a few workers answered together come back together: give the stragglers of that wave a moment
                const double until = now_us() + O.gather_us;
                while (now_us() < until && (int)mine.size() < O.batch) {
                    if (!take(mine, start)) { timespec nap{0, 5000}; nanosleep(&nap, nullptr); }
                }
            }
            start = (start + 1) % (int)h->nslots;
            run(mine);
        }
    }
};

// slots of workers that are gone (killed between requests, or timed out and left): free again
void reap(const Segment& S) {
    for (uint32_t i = 0; i < S.h->nslots; i++) {
        impb_slot_fields* s = &S.slots[i].f;
        const uint32_t st = aload(&s->state), owner = aload(&s->owner_pid);
        if (st == IMPB_FREE || st == IMPB_TAKEN) continue;
        if (owner && !pid_alive(owner)) {
            uint32_t expect = owner;
            if (__atomic_compare_exchange_n(&s->owner_pid, &expect, 0u, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED) && st != IMPB_SUBMITTED)
                astore(&s->state, (uint32_t)IMPB_FREE);
            // (SUBMITTED: a broker thread takes it, finds no owner when it is done and frees it)
        } else if (!owner && st == IMPB_DONE) {
            astore(&s->state, (uint32_t)IMPB_FREE);
        }
    }
}

int serve(const Options& o) {
    Segment S;
    if (!open_segment(o, &S)) return 3;
    // a hardware queue per lane (the runtime's default is four per process; lanes that share a queue run one behind the
    // other: four threads served 16 workers at 10.6 k requests/s on four queues and at 12.4 k on eight)
    if (!getenv("GPU_MAX_HW_QUEUES")) setenv("GPU_MAX_HW_QUEUES", o.threads > 4 ? "16" : "8", 1);
    if (impgpu_env_start(o.device) != IMP_OK) {
        std::fprintf(stderr, "impgpu_broker: impgpu_env_start(%d): %s\n", o.device, impgpu_last_error());
        shm_unlink(o.name.c_str());                          // never served: workers must not find a segment nobody will answer on
        return 4;
    }
    (void)impgpu_env_bind_thread();
    // The front of every slot is page-locked: a JPEG a worker has unstuffed into it (glue/imp_gpu_client.c) goes to the device
    // from where it lies.  Files that reach past it are staged like any caller's.  (Locking allocates the pages: 8 MB a slot.)
    {
        const uint64_t want = std::min<uint64_t>(S.slot_bytes, (uint64_t)o.register_mb << 20);
        bool ok = want > 0;
        for (uint32_t i = 0; ok && i < S.h->nslots; i++) ok = impgpu_host_register(S.slot_data((int)i), (size_t)want) == IMP_OK;
        if (ok) S.registered = want;
        else if (want) std::fprintf(stderr, "impgpu_broker: the slots could not be page-locked (%s): prepared files are staged\n", impgpu_last_error());
    }
    std::vector<std::thread> threads;
    std::vector<Worker*> workers;
    for (int i = 0; i < o.threads; i++) {
        workers.push_back(new Worker(S, o, i));
        threads.emplace_back([w = workers.back()] { (void)impgpu_env_bind_thread(); w->loop(); });
    }
    astore(&S.h->broker_pid, (uint32_t)getpid());            // open for business
    if (!o.ready_file.empty()) { FILE* f = std::fopen(o.ready_file.c_str(), "w"); if (f) { std::fprintf(f, "%d\n", (int)getpid()); std::fclose(f); } }
    std::fprintf(stderr, "impgpu_broker: pid %d serves %s on device %d: %d slots of %ld MB, %d threads, epoch %u\n", (int)getpid(),
                 o.name.c_str(), impgpu_env_device(), o.slots, o.slot_mb, o.threads, S.h->epoch);
    int beats = 0;
    while (!g_stop) {
        timespec nap{0, 100 * 1000 * 1000};
        nanosleep(&nap, nullptr);
        __atomic_add_fetch(&S.h->heartbeat, 1u, __ATOMIC_RELAXED);
        if (++beats % 10 == 0) reap(S);
    }
    astore(&S.h->broker_pid, 0u);                            // closed: workers' next requests fail fast, waiting ones at their next tick
    futex(&S.h->doorbell, FUTEX_WAKE, 1 << 30, nullptr);
    for (auto& t : threads) t.join();
    for (Worker* w : workers) delete w;
    {
        const double nb = (double)(S.h->batches ? S.h->batches : 1);
        std::fprintf(stderr, "impgpu_broker: per batch, us: copy + validate %.0f, decode %.0f, operators %.0f, answers %.0f; idle per thread %.0f ms\n",
                     g_us_prepare.load() / nb, g_us_decode.load() / nb, g_us_ops.load() / nb, g_us_answer.load() / nb, g_us_idle.load() / 1e3 / o.threads);
    }
    std::fprintf(stderr, "impgpu_broker: served %llu requests in %llu batches\n", (unsigned long long)S.h->served, (unsigned long long)S.h->batches);
    {
        std::lock_guard<std::mutex> lk(g_marks.mu);
        for (impgpu_image*& m : g_marks.imgs) impgpu_image_release(&m);
    }
    impgpu_env_destroy();
    shm_unlink(o.name.c_str());                              // a clean stop leaves nothing in /dev/shm (a crash leaves the segment for the next child to adopt)
    return 0;
}

int supervise(const Options& o) {
    // this process never initialises HIP: every broker is a fork()ed child that starts from a clean slate
    int fast_deaths = 0;
    while (!g_stop) {
        const double t0 = now_us();
        const pid_t child = fork();
        if (child < 0) { std::perror("impgpu_broker: fork"); return 5; }
        if (child == 0) {
            Options c = o;
            c.supervise = false;
            _exit(serve(c));
        }
        int status = 0;
        while (waitpid(child, &status, 0) < 0 && errno == EINTR) {
            if (g_stop) kill(child, SIGTERM);
        }
        if (g_stop) break;
        const bool clean = WIFEXITED(status) && WEXITSTATUS(status) == 0;
        std::fprintf(stderr, "impgpu_broker: child %d ended (%s %d); starting a fresh one\n", (int)child,
                     WIFSIGNALED(status) ? "signal" : "status", WIFSIGNALED(status) ? WTERMSIG(status) : WEXITSTATUS(status));
        if (clean) break;
        fast_deaths = now_us() - t0 < 2e6 ? fast_deaths + 1 : 0;
        if (fast_deaths >= 5) { std::fprintf(stderr, "impgpu_broker: five brokers in a row died at once; giving up\n"); return 6; }
        timespec nap{0, 200 * 1000 * 1000};
        nanosleep(&nap, nullptr);
    }
    return 0;
}

}  // namespace

static const char USAGE[] =
    "usage: impgpu_broker [--name /impgpu-broker-0] [--device 0] [--slots 64] [--slot-mb 32] [--register-mb 8] [--threads 2] [--batch 64] "
    "[--gather-us 0] [--png-accept none|all] [--png-inflate host|device] [--jpeg-accept none|progressive] [--webp-accept none|lossless|all|alpha] [--supervise] [--ready-file PATH]\n";

int main(int argc, char** argv) {
    Options o;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char* what) -> const char* {
            if (i + 1 >= argc) { std::fprintf(stderr, "impgpu_broker: %s needs a value\n", what); std::exit(2); }
            return argv[++i];
        };
        if (a == "--name") o.name = val("--name");
        else if (a == "--device") o.device = std::atoi(val("--device"));
        else if (a == "--slots") o.slots = std::atoi(val("--slots"));
        else if (a == "--slot-mb") o.slot_mb = std::atol(val("--slot-mb"));
        else if (a == "--register-mb") o.register_mb = std::max(0l, std::atol(val("--register-mb")));
        else if (a == "--threads") o.threads = std::atoi(val("--threads"));
        else if (a == "--batch") o.batch = std::atoi(val("--batch"));
        else if (a == "--gather-us") o.gather_us = std::atoi(val("--gather-us"));
        else if (a == "--ready-file") o.ready_file = val("--ready-file");
        else if (a == "--png-accept") {
            const std::string v = val("--png-accept");
            if (v == "all") o.png_accept = IMPGPU_PNG_ALL;
            else if (v == "none") o.png_accept = 0;
            else { std::fprintf(stderr, "impgpu_broker: --png-accept takes all or none\n"); return 2; }
        }
        else if (a == "--png-inflate") {
            const std::string v = val("--png-inflate");
            if (v == "device") o.png_inflate = IMPGPU_PNG_DEVICE_INFLATE;
            else if (v == "host") o.png_inflate = 0;
            else { std::fprintf(stderr, "impgpu_broker: --png-inflate takes host or device\n"); std::fputs(USAGE, stderr); return 2; }
        }
        else if (a == "--jpeg-accept") {
            const std::string v = val("--jpeg-accept");
            if (v == "progressive") o.jpeg_accept = IMPGPU_JPEG_PROGRESSIVE;
            else if (v == "none") o.jpeg_accept = 0;
            else { std::fprintf(stderr, "impgpu_broker: --jpeg-accept takes progressive or none\n"); return 2; }
        }
        else if (a == "--webp-accept") {
            const std::string v = val("--webp-accept");
            if (v == "lossless") o.webp_accept = 1;
            else if (v == "all") o.webp_accept = 2;
            else if (v == "alpha") o.webp_accept = 3;
            else if (v == "none") o.webp_accept = 0;
            else { std::fprintf(stderr, "impgpu_broker: --webp-accept takes alpha, all, lossless or none\n"); std::fputs(USAGE, stderr); return 2; }
        }
        else if (a == "--supervise") o.supervise = true;
        else { std::fputs(USAGE, stderr); return 2; }
    }
    if (o.slots < 1 || o.slots > IMPB_MAX_SLOTS || o.slot_mb < 1 || o.slot_mb > 4096 || o.threads < 1 || o.threads > 32 || o.batch < 1 || o.batch > 256 ||
        o.name.empty() || o.name[0] != '/') {
        std::fprintf(stderr, "impgpu_broker: bad option value\n");
        return 2;
    }
    struct sigaction sa {};
    sa.sa_handler = on_signal;
    sigaction(SIGTERM, &sa, nullptr);
    sigaction(SIGINT, &sa, nullptr);
    signal(SIGPIPE, SIG_IGN);
    return o.supervise ? supervise(o) : serve(o);
}
