// imp_jpeg_api.cpp -- impgpu_image_decode_jpeg / impgpu_batch_decode_jpeg: the reference's cvDecodeImage(&rawencoded, -1)
// for JPEG blobs (bridge.c:545-552) with everything but marker parsing and FF00 unstuffing on the device (imp_jpeg.h).
// One file or many, the device sees the same thing: a table of jobs, one entropy launch, one pixel launch per sampling
// class, one wait for all verdicts.
#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "imp_host_pool.h"
#include "imp_jpeg_plan.h"
#include "imp_jpeg_prog.h"

using namespace imp;

namespace {

// Where the entropy stage of a launch runs.  The device's five launches cost about a quarter of a millisecond however small
// the file is; the calling thread's decoder takes 6 ns per byte.  One request at a time (tools/jpeg_tiny_probe.py,
// profiles/r04_jpeg_small_files.txt, frame complete, ms: device / calling thread / libjpeg-turbo on one core) -- 64x64 0.17 /
// 0.06 / 0.04, 160x120 0.21 / 0.09 / 0.09, 320x240 (22 KB) 0.24 / 0.17 / 0.23, 480x360 (50 KB) 0.26 / 0.31 / 0.45, 640x480
// (88 KB) 0.26 / 0.54 / 0.82, 1080p 0.37 / 3.4 / 5.4 -- they cross near 40 KB of entropy-coded data (round 3's stage, with its
// rounds: near 100 KB), so a launch smaller than that keeps its Huffman decoding on the thread that is about to sleep in the
// wait anyway (dequantisation, IDCT, upsampling and colour stay on the device either way), and everything larger -- every
// batch -- is the device's.  IMPGPU_JPEG_HUFF = device | host forces one (read per call: a getenv is nothing next to a decode).
// (`progressive`: the launch holds progressive files, taken because the caller asked for them on the device -- their scans
// are the device's whatever the launch weighs, so that a call's launches do not depend on how many files it holds)
bool entropy_on_device(size_t launch_bytes, bool progressive = false) {
    const char* s = std::getenv("IMPGPU_JPEG_HUFF");
    if (s && !std::strcmp(s, "host")) return false;
    if (s && !std::strcmp(s, "device")) return true;
    return progressive || launch_bytes >= (size_t(40) << 10);
}

// impgpu_jpeg_profile(1): every decode call leaves its stages' durations with the calling thread (impgpu_jpeg_stage_times) --
// the host's from its clock, the device's from events recorded between the kernels
std::atomic<int> g_profile{0};
// process-wide: files whose entropy stage ran on the device, of those refused by its verdict, of those with a chain wait
// that ran out (JPEG_ST_CHAIN_TIMEOUT: the file is then decoded by the caller's fallback -- a box that does this silently
// looks healthy and is not), files kept on the calling thread because their blocks are too long
constexpr int COUNT_PROG = 4 + JPEG_WHY_COUNT + 1, COUNT_PROG_LAUNCHES = COUNT_PROG + 1, COUNT_SLOTS = COUNT_PROG + 2;   // (impgpu_jpeg_counters [13], [14])
std::atomic<unsigned long long> g_count[COUNT_SLOTS];    // [4 + why]: files refused at their header, by reason; [4 + JPEG_WHY_COUNT]: damaged headers
thread_local double t_stage[16];

// IMPGPU_JPEG_TRACE=1: one line per call on stderr with the host's share of it, in microseconds
struct Stopwatch {
    bool on;
    std::chrono::steady_clock::time_point t0;
    double marks[8] = {};
    int n = 0;
    Stopwatch() : on(std::getenv("IMPGPU_JPEG_TRACE") != nullptr || g_profile.load(std::memory_order_relaxed)), t0(std::chrono::steady_clock::now()) {}
    void mark() {
        if (!on || n >= 8) return;
        const auto t = std::chrono::steady_clock::now();
        marks[n++] = std::chrono::duration<double, std::micro>(t - t0).count();
        t0 = t;
    }
};

constexpr int MAX_BATCH = 256;                      // verdicts of one launch fit the lane's pinned mailbox
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Prep {                                       // one file on its way to the device
    int code = IMP_OK;
    JpegHeader H;
    JpegFrame F;
    int dc_ids[2] = {-1, -1}, ac_ids[2] = {-1, -1};
    JpegScan scan;
    size_t nsegs = 0;
    size_t words_off = 0, words_cap = 0;            // bytes, in the staging buffer and in the device copy alike
    size_t coef_off = 0;                            // bytes in the coefficient area
    size_t side_tables = 0, side_qt = 0, side_meta = 0;   // byte offsets in the side blob
    size_t ctl_header = 0, ctl_records = 0, ctl_ext = 0;   // word offsets in the control area
    size_t work_off = 0;                            // bytes in the per-chunk work area (entry states, slot counts, DC sums)
    impgpu_image* im = nullptr;
    size_t scan_len = 0;                            // entropy-coded bytes: as the file has them, or unstuffed by the caller (prepared)
    const impgpu_jpeg_prepared* pre = nullptr;      // the caller has unstuffed the scan (impgpu_batch_decode_jpeg_prepared)
    bool given = false;                             // the frame has been handed to the caller ahead of its verdict (impgpu_batch_decode_jpeg_pending)
    bool direct = false;                            // ... into registered memory: its words go to the device from there
    size_t direct_off = 0;                          // bytes behind the staged part of the words' block
    // a progressive file (imp_jpeg_prog.h): its scans, its items as jpeg_prog_prepare cut them, its tables and scan records in the side blob
    JpegProg prog;
    bool is_prog = false;
    std::vector<JpegProgItem> items;
    std::vector<uint32_t> level_first;
    std::vector<JpegHuffDev> ptabs;
    size_t side_ptabs = 0, side_pscans = 0;
};

// A file whose blocks average more bits than this keeps its Huffman stage on the calling thread even inside a launch that is
// the device's: blocks that long seldom end inside a walk's overlap, so their chunks are reached one after the other by an
// explicit state (the host model, impgpu_jpeg_sync_stats: 4.5 % of the chunks at 210 bits per block, a quality-98 photograph; 25-70 % for
// white noise), and a 4 MB file of noise would hold a workgroup chain for most of a second where the host needs 25 ms.
constexpr size_t DENSE_BITS_PER_BLOCK = 200;
constexpr int CODE_DEFERRED = -0x7fff;              // internal: "decode this one in the host-entropy group"

// A group of files between the call that enqueued its decode and the call that reads its verdicts.  Everything the device
// works on (stream words, planes, tables, work areas) and the pinned words its verdicts arrive in belong to the group until
// group_finish; the caller's blobs must stay readable until then (a file deferred to the host-entropy group is read again).
constexpr int GROUP_SLOTS = 4;                      // groups in flight per calling thread: one slot of the lane's mailbox each
struct Group {
    std::vector<Prep> P;
    const unsigned char* const* blobs = nullptr;
    const size_t* sizes = nullptr;
    int count = 0;
    bool on_device = false, profile = false;
    bool one_block = false;                         // d_side and d_ctl lie inside d_words' block (one upload for all three)
    void *d_words = nullptr, *d_coef = nullptr, *d_side = nullptr, *d_ctl = nullptr, *d_work = nullptr;
    void* mark = nullptr;                           // the point of the group's stream where its last kernel was enqueued
    hipStream_t stream = nullptr;                   // the lane's stream, or its side stream (a batch begun ahead: its decode overlaps what the thread enqueues next)
    uint32_t* mailbox = nullptr;
    int slot = -1;
    size_t live = 0, ctl_total = 0;
    hipEvent_t ev[10] = {};                         // [8], [9]: around the progressive files' launches
    unsigned prog_files = 0, prog_launches = 0;
    Stopwatch sw;
    const void* owner = nullptr;                    // the thread that began the group (its slot, its lane): only it may finish it
    const impgpu_jpeg_prepared* prep = nullptr;     // per file, or nullptr: every blob is a whole file
};
thread_local char t_thread_tag;                     // its address names the calling thread
thread_local unsigned t_slots_busy = 0;             // bit k: mailbox slot k holds a group that has not been finished
std::atomic<int> g_groups_in_flight{0};             // over all threads: groups begun and not finished

// A prepared file as the file it came from (head, the scan with its 00s behind the FFs again, EOI): what the host's entropy
// decoder reads -- the A/B path and the files a device launch defers (dense blocks), never the common case.
std::vector<uint8_t> restuffed(const impgpu_jpeg_prepared& f) {
    std::vector<uint8_t> out;
    out.reserve(f.head_size + f.scan_size + f.scan_size / 64 + 16);
    out.insert(out.end(), f.head, f.head + f.head_size);
    for (size_t i = 0; i < f.scan_size; i++) {
        out.push_back(f.scan[i]);
        if (f.scan[i] == 0xFF) out.push_back(0);
    }
    out.push_back(0xFF);
    out.push_back(0xD9);
    return out;
}

void group_release(Group& G) {
    for (int i = 0; i < 10; i++) if (G.ev[i]) { (void)hipEventDestroy(G.ev[i]); G.ev[i] = nullptr; }
    void* blocks[5] = {G.d_words, G.d_coef, G.one_block ? nullptr : G.d_side, G.one_block ? nullptr : G.d_ctl, G.d_work};
    for (void* b : blocks)
        if (b) { if (G.stream && !on_lane_stream(G.stream)) dev_free_on(b, G.stream); else dev_free(b); }
    G.d_words = G.d_coef = G.d_side = G.d_ctl = G.d_work = nullptr;
    if (G.slot >= 0) { t_slots_busy &= ~(1u << G.slot); g_groups_in_flight.fetch_sub(1, std::memory_order_relaxed); }
    G.slot = -1;
}

// The pixel kernels' five instantiations: gray, 4:4:4, 4:2:2, 4:4:0, 4:2:0.  A launch and a tile map per class.
constexpr int NCLASSES = 5;
constexpr struct { int hs, vs, ncomp; } CLASSES[NCLASSES] = {{1, 1, 1}, {1, 1, 3}, {2, 1, 3}, {1, 2, 3}, {2, 2, 3}};
inline int class_of(const JpegFrame& F) { return F.ncomp == 1 ? 0 : (F.hs == 1 ? 1 : 2) + (F.vs == 1 ? 0 : 2); }
inline size_t tile_count(const JpegFrame& F) { return (size_t)((F.width + JPEG_TILE_W - 1) / JPEG_TILE_W) * ((F.height + JPEG_TILE_H - 1) / JPEG_TILE_H); }

struct FileTotals {                                 // over the files of a group that passed their headers, bytes
    size_t words = 0, coef = 0;                     // the staged scans; the coefficient planes
    size_t direct = 0;                              // the scans that go to the device from the caller's registered memory
    size_t launch_bytes = 0, prog_bytes = 0;        // entropy-coded: the sequential files' (what their chunking goes by), the progressive files'
};

// The side blob -- per job its tables, quantisers and interval arrays, then the job table and the workgroup maps -- with the
// sizes of what lies beside it: the control words ([0] ticket, then the jobs' headers, then their records) and the work area.
// (A file's own offsets are in its Prep.)
struct SidePlan {
    size_t jobs = 0, blocks = 0, sync = 0, pfiles = 0, pitems = 0, tile_map[NCLASSES] = {};    // byte offsets in the blob
    size_t bytes = 0;
    size_t njobs = 0, ctl_words = 4, work = 0;
    size_t total_blocks = 0, sync_blocks = 0, tiles[NCLASSES] = {};
    size_t prog_files = 0, prog_items = 0;
    int prog_levels = 0;
};

// What the phases of group_begin hand each other.
struct Begin {
    Group& G;
    int force_host, accept;
    FileTotals t;
    uint8_t* host = nullptr;                        // the pinned staging buffer
    void* token = nullptr;                          // ... and the claim on it, held until its upload is enqueued
    SidePlan side;
    size_t off_side = 0, off_ctl = 0, in_total = 0; // one block: where the side blob and the control words lie behind the words, and the end
    size_t direct_base = 0;                         // where the direct scans begin in the words' block
    std::vector<uint8_t> blob_mem;
    uint8_t* blob = nullptr;                        // the side blob as the host fills it: inside the staging buffer (one block) or blob_mem
    uint32_t* verdict_dev = nullptr;                // the device's view of the group's pinned verdict words
    std::vector<uint32_t> plevel_first;             // the progressive items' first index per level
};

// ---- open: the stream, the files, a slot of the lane's mailbox
int group_open(Group& G, const unsigned char* const* blobs, const size_t* sizes, int count, bool side, const impgpu_jpeg_prepared* prep) {
    hipStream_t s = side ? lane_side_stream() : nullptr;
    if (!s) s = env_stream();
    if (!s) return IMP_ERROR_DEVICE;
    G.stream = s;
    G.blobs = blobs; G.sizes = sizes; G.count = count; G.prep = prep;
    G.P.assign((size_t)count, Prep());
    for (int k = 0; k < GROUP_SLOTS && G.slot < 0; k++)
        if (!(t_slots_busy & (1u << k))) G.slot = k;
    if (G.slot < 0) { set_error_text("too many JPEG batches begun and not finished on this thread"); return IMP_ERROR_INVALID_ARGS; }
    t_slots_busy |= 1u << G.slot;
    G.owner = &t_thread_tag;
    g_groups_in_flight.fetch_add(1, std::memory_order_relaxed);
    return IMP_OK;
}

// ---- one file's header and geometry, and the sizes of everything it needs; a refusal is left in p.code and counted
void plan_file(Begin& B, Prep& p, const unsigned char* blob, size_t size, const impgpu_jpeg_prepared* pre) {
    if (!blob) { p.code = IMP_ERROR_INVALID_ARGS; return; }
    if (pre && pre->scan) p.pre = pre;
    // (a progressive file comes whole: a scan the caller unstuffed is a sequential file's)
    p.code = jpeg_parse_ex(blob, size, &p.H, (B.accept & IMPGPU_JPEG_PROGRESSIVE) && !p.pre ? &p.prog : nullptr);
    p.is_prog = !p.code && !p.prog.scans.empty();
    if (p.is_prog) for (int c = 0; c < p.H.ncomp; c++) p.H.comp[c].td = p.H.comp[c].ta = 0;      // (its tables belong to its scans)
    // (a prepared file: its head ends where its scan began, and nothing cuts the scan into intervals)
    if (!p.code && p.pre && (p.H.scan_begin != size || p.H.restart_interval || !p.pre->scan_size)) {
        set_error_text("prepared JPEG: the head does not end at its scan, or the file has a restart interval");
        p.code = IMP_ERROR_INVALID_ARGS;
        return;
    }
    if (!p.code) p.scan_len = p.is_prog ? p.prog.data_bytes : p.pre ? p.pre->scan_size : size - p.H.scan_begin;
    if (!p.code && !frame_fits(p.H.width, p.H.height, p.H.ncomp)) { p.code = IMP_ERROR_UNSUPPORTED; p.H.why = JPEG_WHY_OTHER; }
    if (p.code == IMP_ERROR_UNSUPPORTED) g_count[4 + (p.H.why > 0 && p.H.why < JPEG_WHY_COUNT ? p.H.why : JPEG_WHY_OTHER)].fetch_add(1, std::memory_order_relaxed);
    else if (p.code == IMP_ERROR_DECODE_FAILED) g_count[4 + JPEG_WHY_COUNT].fetch_add(1, std::memory_order_relaxed);
    if (!p.code) p.code = jpeg_frame_setup(p.H, &p.F, p.dc_ids, p.ac_ids);
    if (p.code) return;
    const size_t total_mcus = (size_t)p.H.mcux * p.H.mcuy;
    p.nsegs = p.H.restart_interval ? (total_mcus + p.H.restart_interval - 1) / p.H.restart_interval : 1;
    // Refused before anything is sized by what the header claims: an interval needs a data byte and its marker, a block a DC
    // code and an end-of-block code -- a few hundred bytes that announce 30000 x 30000 pixels, or a restart interval of one
    // MCU on a frame of 2^30, would otherwise have pinned and device memory allocated by the gigabyte before the decode fails.
    // (a progressive file's first DC scan spends a bit or more on every block of every component: nothing smaller holds the frame it announces)
    const size_t scan_bytes = p.scan_len, blocks = (size_t)p.F.total_slots / 64;
    if (p.is_prog ? blocks > 8 * scan_bytes + 64 : p.nsegs > scan_bytes / 3 + 1 || blocks > 4 * scan_bytes + 64) { p.code = IMP_ERROR_DECODE_FAILED; return; }
    p.words_cap = align_up(p.is_prog ? jpeg_prog_capacity(p.prog) : jpeg_scan_capacity(scan_bytes, p.nsegs), JPEG_CHUNK_BYTES_MAX);
    p.direct = !p.is_prog && p.pre && p.pre->registered && !B.force_host;
    if (p.direct) { p.direct_off = B.t.direct; B.t.direct += p.words_cap; }
    else { p.words_off = B.t.words; B.t.words += p.words_cap; }
    p.coef_off = B.t.coef;
    B.t.coef += align_up((size_t)p.F.total_slots * sizeof(int16_t), 256);
}

// ---- plan files: every header, then where the launch's entropy stage runs, and what follows from that
void plan_files(Begin& B) {
    Group& G = B.G;
    for (int i = 0; i < G.count; i++) plan_file(B, G.P[(size_t)i], G.blobs[i], G.sizes[i], G.prep ? &G.prep[i] : nullptr);
    unsigned nprog = 0;
    for (const Prep& p : G.P)
        if (!p.code) {
            if (p.is_prog) { B.t.prog_bytes += p.scan_len; nprog++; }
            else B.t.launch_bytes += p.scan_len;
        }
    G.on_device = !B.force_host && entropy_on_device(B.t.launch_bytes, nprog != 0);
    if (!G.on_device && B.t.direct) {                               // (a launch of under 40 KB: its files are staged after all)
        for (Prep& p : G.P) if (!p.code && p.direct) { p.direct = false; p.words_off = B.t.words; B.t.words += p.words_cap; }
        B.t.direct = 0;
    }
    if (G.on_device && !std::getenv("IMPGPU_JPEG_HUFF"))
        for (Prep& p : G.P)
            if (!p.code && !p.is_prog && p.scan_len * 8 > DENSE_BITS_PER_BLOCK * ((size_t)p.F.total_slots / 64)) {
                p.code = CODE_DEFERRED;
                g_count[3].fetch_add(1, std::memory_order_relaxed);
            }
}

// a file's scan on its way into the staging buffer (device entropy stage): unstuffed, cut into chunks, padded
void stage_scan(Begin& B, Prep& p, const unsigned char* blob, size_t size, bool busy) {
    if (p.is_prog) {
        p.ptabs.resize(p.prog.tables.size());
        for (size_t k = 0; k < p.ptabs.size() && !p.code; k++) p.code = jpeg_build_table(p.prog.tables[k], p.prog.table_is_dc[k] != 0, &p.ptabs[k]);
        if (!p.code) p.code = jpeg_prog_prepare(blob, size, p.H, p.prog, B.host + p.words_off, p.words_cap, &p.items, &p.level_first);
        return;
    }
    p.scan.chunk_bytes = jpeg_chunk_bytes_for(p.scan_len, B.t.launch_bytes, busy);
    if (!p.pre) { p.code = jpeg_prepare_scan(blob, size, p.H, B.host + p.words_off, p.words_cap, &p.scan); return; }
    // the caller's unstuffed bytes are one interval: what jpeg_prepare_scan would have left -- the bytes, 1-bits up to
    // the chunk boundary, one all-ones guard chunk (a registered scan brings them: IMPGPU_JPEG_SCAN_TAIL)
    const size_t CBY = p.scan.chunk_bytes, n = p.pre->scan_size, padded = (n + CBY - 1) / CBY * CBY;
    p.scan.seg_first_chunk.assign(1, 0u);
    p.scan.seg_bits.assign(1, (uint32_t)(n * 8));
    p.scan.nchunks = padded / CBY;
    if ((uint64_t)padded * 8 >= (1ull << 32)) { p.code = IMP_ERROR_UNSUPPORTED; return; }
    if (p.direct) return;
    uint8_t* out = B.host + p.words_off;
    std::memcpy(out, p.pre->scan, n);
    std::memset(out + n, 0xFF, padded - n + JPEG_CHUNK_BYTES);
}

// a file's whole entropy decoding into pinned coefficient planes (host entropy stage: small launches, the A/B path, deferred files)
void stage_coefficients(Begin& B, Prep& p, const unsigned char* blob, size_t size) {
    int16_t* planes = (int16_t*)(B.host + p.coef_off);
    std::memset(planes, 0, (size_t)p.F.total_slots * sizeof(int16_t));
    if (p.is_prog) p.code = jpeg_prog_reference(blob, size, p.H, p.prog, p.F, planes);     // (IMPGPU_JPEG_HUFF=host: the A/B path)
    else if (p.pre) {
        const std::vector<uint8_t> file = restuffed(*p.pre);
        p.code = jpeg_host_entropy(file.data(), file.size(), p.H, planes, p.F);
    } else p.code = jpeg_host_entropy(blob, size, p.H, planes, p.F);
}

// ---- stage: the compressed bytes -- FF00 unstuffing while they are copied into pinned memory, the only pass the host makes
// over them (device entropy stage), or the whole entropy decoding into pinned coefficient planes -- and a frame per live file
void stage_files(Begin& B) {
    Group& G = B.G;
    // The unstuffing copies of a batch are independent of each other (a file each, disjoint parts of the pinned buffer): from four
    // files and 256 KB on they are shared out to a few helper threads (host_pool) -- 31 us per 437 KB file on the calling thread
    // were 0.2 ms of a broker lane's 0.9-ms cycle at seven files a batch, and 2.0 of a one-thread stream's 5.8 ms per 64 files.
    // A lone request never gets here with more than one file, so an nginx worker that links the library never starts a thread.
    if (G.on_device) {
        std::vector<int> todo;
        for (int i = 0; i < G.count; i++) if (!G.P[(size_t)i].code) todo.push_back(i);
        const bool busy = g_groups_in_flight.load(std::memory_order_relaxed) > 1;    // (this group is counted already)
        auto prepare = [&](int i) { stage_scan(B, G.P[(size_t)i], G.blobs[i], G.sizes[i], busy); };
        host_parallel(todo, B.t.launch_bytes + B.t.prog_bytes, prepare);
    }
    for (int i = 0; i < G.count; i++) {
        Prep& p = G.P[(size_t)i];
        if (p.code) continue;
        if (!G.on_device) stage_coefficients(B, p, G.blobs[i], G.sizes[i]);
        else if (!p.is_prog) {
            p.F.nchunks = (unsigned)p.scan.nchunks;
            p.F.nsegs = (unsigned)p.scan.seg_first_chunk.size();
            p.F.chunk_bits = (unsigned)p.scan.chunk_bytes * 8;
            p.F.overlap_bits = jpeg_overlap_bits_for(p.F.chunk_bits, p.scan_len, (size_t)p.F.total_slots / 64);
            // k_jpeg_write decodes a chunk with two lanes, the second entering at the chunk's middle in the state the chunk's
            // true walk passed there: its chain is half as long and the synchronising phases are none the longer.  Where the
            // launch is a latency chain, that is (a lone 640 x 480: k_jpeg_write 65 -> 56 us, 4K 99 -> 89); a launch that fills
            // the device gains nothing from shorter chains and loses to the second round of workgroups its LDS forces
            // (64 files, 28 MB: 349 -> 415 us), so from 4 MB on -- where the chunks grow to 256 bytes -- a chunk keeps its
            // one lane.
            p.F.wsplit = B.t.launch_bytes > (size_t(4) << 20) ? 1u : 2u;
        }
        if (!p.code) p.code = image_new(p.H.width, p.H.height, p.H.ncomp, &p.im);
        if (!p.code) G.live++;
    }
}

// ---- plan side: every live file's place in the side blob, the control words and the work area, then the launch's own tables
void plan_side(Begin& B) {
    Group& G = B.G;
    SidePlan& S = B.side;
    auto take = [&S](size_t bytes) { const size_t at = S.bytes; S.bytes += align_up(bytes, 64); return at; };
    for (Prep& p : G.P) {
        if (p.code) continue;
        p.ctl_header = S.ctl_words;
        S.ctl_words += 4;
    }
    for (Prep& p : G.P) {
        if (p.code) continue;
        S.njobs++;
        if (G.on_device && p.is_prog) {
            p.side_ptabs = take((p.prog.tables.size() + 1) * sizeof(JpegHuffDev));
            p.side_pscans = take(p.prog.scans.size() * sizeof(JpegProgScanDev));
            S.prog_items += p.items.size();
            S.prog_levels = std::max(S.prog_levels, p.prog.nlevels);
            S.prog_files++;
        } else if (G.on_device) {
            p.side_tables = take(4 * sizeof(JpegHuffDev));
            p.side_meta = take((p.scan.nchunks + 2 * p.scan.seg_first_chunk.size()) * sizeof(uint32_t));
            p.ctl_records = S.ctl_words;
            S.ctl_words += (size_t)jpeg_sync_blocks(p.F.nchunks, p.F.bpm) * JPEG_CTL_REC;
            p.ctl_ext = S.ctl_words;
            S.ctl_words += 4;
            S.sync_blocks += jpeg_sync_blocks(p.F.nchunks, p.F.bpm);
            S.total_blocks += jpeg_entropy_blocks(p.F.nchunks * p.F.wsplit);
            p.work_off = S.work;
            S.work += jpeg_work_layout(p.F.nchunks, p.F.wsplit, p.F.bpm, p.F.total_slots).bytes;
        }
        p.side_qt = take(3 * 64 * sizeof(uint16_t));
        S.tiles[class_of(p.F)] += tile_count(p.F);
    }
    S.jobs = take(S.njobs * sizeof(JpegJob));
    S.blocks = take(S.total_blocks * sizeof(JpegMapEntry));
    S.sync = take(S.sync_blocks * sizeof(JpegMapEntry));
    S.pfiles = take(S.prog_files * sizeof(JpegProgFileDev));
    S.pitems = take(S.prog_items * sizeof(JpegProgItem));
    for (int k = 0; k < NCLASSES; k++) S.tile_map[k] = take(S.tiles[k] * sizeof(JpegMapEntry));
}

// ---- allocate: the device blocks
int allocate(Begin& B) {
    Group& G = B.G;
    const SidePlan& S = B.side;
    // The scan words, the side blob and the (zeroed) control area cross the link as ONE copy when the pinned buffer the
    // words were unstuffed into has room behind them (it is at least 8 MB): three commands on the stream -- two copies
    // and a fill -- were 30-40 us of a lone file's 220 (tools/jpeg_stage_probe.py), the bytes themselves 3.
    B.off_side = align_up(B.t.words, 256);
    B.off_ctl = B.off_side + align_up(S.bytes, 256);
    B.in_total = B.off_ctl + S.ctl_words * sizeof(uint32_t);
    G.one_block = G.on_device && stage_capacity(B.token) >= B.in_total;
    // (the scans a caller unstuffed into registered memory lie behind what is staged: each arrives by a copy of its own)
    B.direct_base = align_up(G.one_block ? B.in_total : B.t.words, 256);
    int rc;
    if (G.one_block) {
        rc = dev_alloc(B.direct_base + B.t.direct, &G.d_words);
        if (!rc) { G.d_side = (uint8_t*)G.d_words + B.off_side; G.d_ctl = (uint8_t*)G.d_words + B.off_ctl; }
    } else {
        rc = dev_alloc(S.bytes, &G.d_side);
        if (!rc && G.on_device) rc = dev_alloc(B.direct_base + B.t.direct, &G.d_words);
        if (!rc && G.on_device) rc = dev_alloc(S.ctl_words * sizeof(uint32_t), &G.d_ctl);
    }
    if (!rc) rc = dev_alloc(B.t.coef, &G.d_coef);
    if (!rc && G.on_device) rc = dev_alloc(S.work, &G.d_work);
    G.ctl_total = S.ctl_words;
    if (!rc) rc = stream_join(G.stream);                            // (side stream: the pool recycles in lane-stream order; the frames were allocated there too)
    return rc;
}

struct Fill {                                       // the tables of the side blob while they are filled: where each one's next entry goes
    JpegJob* jobs;
    JpegMapEntry *bmap, *smap, *tmap[NCLASSES];
    JpegProgFileDev* pfiles;
    size_t nb = 0, ns = 0, nt[NCLASSES] = {}, npf = 0;
    std::vector<JpegProgItem> pitems;               // every file's, by (level, kind): a launch per level, a decoder per wave
    std::vector<const JpegProg*> prog_of;           // per progressive file of the launch
    std::vector<uint32_t> meta;
};

// job j, a progressive file: its tables and scan records, its entry in the progressive files' table, its items
void fill_progressive(Begin& B, Fill& f, Prep& p, JpegJob& J, size_t j) {
    Group& G = B.G;
    if (!p.ptabs.empty()) std::memcpy(B.blob + p.side_ptabs, p.ptabs.data(), p.ptabs.size() * sizeof(JpegHuffDev));
    jpeg_prog_scans_dev(p.prog, (JpegProgScanDev*)(B.blob + p.side_pscans));
    J.header = (uint32_t*)G.d_ctl + p.ctl_header;
    JpegProgFileDev& D = f.pfiles[f.npf];
    jpeg_prog_file_dev(p.H, p.F, &D);
    D.coef = (int16_t*)((uint8_t*)G.d_coef + p.coef_off);
    D.words = (const uint32_t*)((uint8_t*)G.d_words + p.words_off);
    D.tables = (const JpegHuffDev*)((uint8_t*)G.d_side + p.side_ptabs);
    D.scans = (const JpegProgScanDev*)((uint8_t*)G.d_side + p.side_pscans);
    D.header = J.header;
    D.verdict = B.verdict_dev ? B.verdict_dev + 4 * j : nullptr;
    for (JpegProgItem it : p.items) { it.file = (uint32_t)f.npf; f.pitems.push_back(it); }
    f.prog_of.push_back(&p.prog);
    f.npf++;
}

// job j, a sequential file: its tables and interval arrays, what the entropy kernels are handed, its workgroups in their maps
void fill_sequential(Begin& B, Fill& f, Prep& p, JpegJob& J, size_t j) {
    Group& G = B.G;
    if (const int rc = jpeg_build_tables(p.H, p.dc_ids, p.ac_ids, (JpegHuffDev*)(B.blob + p.side_tables))) p.code = rc;      // (cannot happen after jpeg_parse; keeps the job inert)
    jpeg_scan_meta(p.scan, &f.meta);
    std::memcpy(B.blob + p.side_meta, f.meta.data(), f.meta.size() * sizeof(uint32_t));
    J.words = (const uint32_t*)((uint8_t*)G.d_words + (p.direct ? B.direct_base + p.direct_off : p.words_off));
    J.chunk_seg = (const uint32_t*)((uint8_t*)G.d_side + p.side_meta);
    J.seg_first_chunk = J.chunk_seg + p.F.nchunks;
    J.seg_bits = J.seg_first_chunk + p.F.nsegs;
    J.tables = (const JpegHuffDev*)((uint8_t*)G.d_side + p.side_tables);
    J.header = (uint32_t*)G.d_ctl + p.ctl_header;
    J.records = (uint32_t*)G.d_ctl + p.ctl_records;
    jpeg_job_bind_work(J, (uint8_t*)G.d_work + p.work_off, jpeg_work_layout(p.F.nchunks, p.F.wsplit, p.F.bpm, p.F.total_slots));
    J.ext_count = (uint32_t*)G.d_ctl + p.ctl_ext;
    for (unsigned b = 0; b < jpeg_entropy_blocks(p.F.nchunks * p.F.wsplit); b++) f.bmap[f.nb++] = JpegMapEntry{(uint32_t)j, b};
    for (unsigned b = 0; b < jpeg_sync_blocks(p.F.nchunks, p.F.bpm); b++) f.smap[f.ns++] = JpegMapEntry{(uint32_t)j, b};
}

// the progressive files' items as one list by (level, kind), and where each level begins in it
void fill_progressive_items(Begin& B, Fill& f) {
    B.plevel_first.assign((size_t)B.side.prog_levels + 1, 0u);
    if (!f.npf) return;
    // (each file's list is sorted already; the key is recomputed from the file's scans)
    auto key = [&](const JpegProgItem& it) { const JpegProgScan& sc = f.prog_of[it.file]->scans[it.scan]; return sc.level * 4 + sc.kind; };
    std::stable_sort(f.pitems.begin(), f.pitems.end(), [&](const JpegProgItem& a, const JpegProgItem& b) { return key(a) < key(b); });
    for (const JpegProgItem& it : f.pitems) B.plevel_first[(size_t)f.prog_of[it.file]->scans[it.scan].level + 1]++;
    for (int l = 0; l < B.side.prog_levels; l++) B.plevel_first[(size_t)l + 1] += B.plevel_first[(size_t)l];
    if (!f.pitems.empty()) std::memcpy(B.blob + B.side.pitems, f.pitems.data(), f.pitems.size() * sizeof(JpegProgItem));
}

// ---- fill: the side blob -- job table, maps, tables, quantisers, progressive files and items
void fill_side(Begin& B) {
    Group& G = B.G;
    const SidePlan& S = B.side;
    if (G.one_block) {
        B.blob = B.host + B.off_side;
        std::memset(B.host + B.t.words, 0, B.off_side - B.t.words);
        std::memset(B.host + B.off_side, 0, B.in_total - B.off_side);
    } else {
        B.blob_mem.assign(S.bytes, 0);
        B.blob = B.blob_mem.data();
    }
    if (G.on_device && hipHostGetDevicePointer((void**)&B.verdict_dev, G.mailbox, 0) != hipSuccess) { B.verdict_dev = nullptr; (void)hipGetLastError(); }
    Fill f;
    f.jobs = (JpegJob*)(B.blob + S.jobs);
    f.bmap = (JpegMapEntry*)(B.blob + S.blocks);
    f.smap = (JpegMapEntry*)(B.blob + S.sync);
    for (int k = 0; k < NCLASSES; k++) f.tmap[k] = (JpegMapEntry*)(B.blob + S.tile_map[k]);
    f.pfiles = (JpegProgFileDev*)(B.blob + S.pfiles);
    f.pitems.reserve(S.prog_items);
    size_t j = 0;
    for (Prep& p : G.P) {
        if (p.code) continue;
        JpegJob& J = f.jobs[j];
        std::memset(&J, 0, sizeof J);
        J.F = p.F;
        if (G.on_device && p.is_prog) fill_progressive(B, f, p, J, j);
        else if (G.on_device) fill_sequential(B, f, p, J, j);
        uint16_t* qt3 = (uint16_t*)(B.blob + p.side_qt);
        for (int c = 0; c < p.H.ncomp; c++) std::memcpy(qt3 + 64 * c, p.H.qt[p.H.comp[c].tq], 64 * sizeof(uint16_t));
        J.qt = (const uint16_t*)((uint8_t*)G.d_side + p.side_qt);
        J.coef = (int16_t*)((uint8_t*)G.d_coef + p.coef_off);
        J.dst = p.im->d;
        J.dstep = p.im->step;
        J.verdict = (G.on_device && B.verdict_dev) ? B.verdict_dev + 4 * j : nullptr;
        const int k = class_of(p.F);
        const uint32_t ntiles = (uint32_t)tile_count(p.F);
        for (uint32_t tl = 0; tl < ntiles; tl++) f.tmap[k][f.nt[k]++] = JpegMapEntry{(uint32_t)j, tl};
        j++;
    }
    fill_progressive_items(B, f);
    G.prog_files = (unsigned)f.npf;
}

// ---- upload and enqueue: the staged bytes, the side blob, the direct scans, the zeroed control words; then the kernels
int upload_and_enqueue(Begin& B) {
    Group& G = B.G;
    const SidePlan& S = B.side;
    const hipStream_t s = G.stream;
    const bool on_device = G.on_device, one = G.one_block;
    hipEvent_t* ev = G.ev;
    if (G.profile && on_device) {
        for (int i = 0; i < 10; i++) if (hipEventCreate(&ev[i]) != hipSuccess) { ev[i] = nullptr; G.profile = false; }
        if (G.profile) (void)hipEventRecord(ev[0], s);
    }
    int rc = stage_upload(B.token, on_device ? G.d_words : G.d_coef, one ? B.in_total : on_device ? B.t.words : B.t.coef);
    B.token = nullptr;
    if (!rc && !one) rc = upload_to(G.d_side, B.blob, S.bytes, s);  // (both copies ride the lane's stream; `s` is made to wait for them here)
    if (!rc && one) rc = stream_join(s);
    for (const Prep& p : G.P) {
        if (rc || p.code || !p.direct) continue;
        const hipError_t e = hipMemcpyAsync((uint8_t*)G.d_words + B.direct_base + p.direct_off, p.pre->scan, align_up(p.pre->scan_size, JPEG_CHUNK_BYTES_MAX) + JPEG_CHUNK_BYTES_MAX,
                                            hipMemcpyHostToDevice, s);
        if (e != hipSuccess) { set_error("hipMemcpyAsync(jpeg scan)", e); rc = IMP_ERROR_DEVICE; }
    }
    if (rc) return rc;
    const JpegJob* jobs = (const JpegJob*)((uint8_t*)G.d_side + S.jobs);
    auto map_at = [&G](size_t off) { return (const JpegMapEntry*)((uint8_t*)G.d_side + off); };
    if (on_device) {
        // (the coefficient planes are not cleared: k_jpeg_write stores whole blocks)
        if (!one && hipMemsetAsync(G.d_ctl, 0, S.ctl_words * sizeof(uint32_t), s) != hipSuccess) {
            set_error("hipMemsetAsync(jpeg)", hipGetLastError());
            return IMP_ERROR_DEVICE;
        }
        if (G.profile) (void)hipEventRecord(ev[1], s);
        // a launch too small to fill the device with any of its kernels runs walks, mend and select as ONE launch
        // (k_jpeg_entropy_small; measured, one file at a time, fused / five kernels: 640 x 480 0.221 / 0.235 ms, 720p equal,
        // 1080p 0.323 / 0.313, 4K 0.546 / 0.510 -- from a few hundred KB on every phase is bound by what it computes, not by
        // its launch, and a workgroup that waits inside a kernel holds slots a kernel boundary would have given to others).
        const bool small = B.t.launch_bytes <= (size_t(192) << 10);
        rc = launch_jpeg_entropy(jobs, map_at(S.sync), (unsigned)S.sync_blocks, map_at(S.blocks), (unsigned)S.total_blocks, (uint32_t*)G.d_ctl, s, G.profile ? ev + 2 : nullptr, small);
        if (rc) return rc;
        // the progressive files: the planes zeroed, a launch per level of the deepest scan script, their verdict words
        if (G.profile && G.prog_files) (void)hipEventRecord(ev[8], s);
        rc = launch_jpeg_prog((const JpegProgFileDev*)((uint8_t*)G.d_side + S.pfiles), G.prog_files, (const JpegProgItem*)((uint8_t*)G.d_side + S.pitems),
                              B.plevel_first.data(), S.prog_levels, s, nullptr, &G.prog_launches);
        if (rc) return rc;
        if (G.profile && G.prog_files) (void)hipEventRecord(ev[9], s);
        g_count[COUNT_PROG_LAUNCHES].fetch_add(G.prog_launches, std::memory_order_relaxed);
        // the kernel's verdicts (did every interval decode to exactly its MCUs?) are read before a frame is handed on:
        // k_jpeg_dcfix has written them into the pinned words; copied only where the device cannot address those
        if (!B.verdict_dev) {
            const hipError_t e = hipMemcpyAsync(G.mailbox, (uint32_t*)G.d_ctl + 4, S.njobs * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) { set_error("hipMemcpyAsync(jpeg verdicts)", e); return IMP_ERROR_DEVICE; }
        }
    }
    for (int k = 0; k < NCLASSES && !rc; k++) rc = launch_jpeg_pixels(CLASSES[k].hs, CLASSES[k].vs, CLASSES[k].ncomp, jobs, map_at(S.tile_map[k]), (unsigned)S.tiles[k], s);
    if (!rc && G.profile && on_device) (void)hipEventRecord(ev[7], s);
    return rc;
}

// the one way out of a group_begin that fails once frames or device blocks may exist
int group_abort(Begin& B, int rc) {
    Group& G = B.G;
    if (B.token) (void)stage_upload(B.token, nullptr, 0);
    (void)hipStreamSynchronize(G.stream);
    (void)lane_wait();                                              // nothing of this call may still be running when its buffers go back
    for (Prep& p : G.P) if (p.im) { image_delete(p.im); p.im = nullptr; }
    group_release(G);
    return rc;
}

// Everything up to the last enqueue: headers, the unstuffing copy (or the host's entropy decoding), job tables, uploads,
// the entropy and pixel kernels, the verdicts' copy.  Does NOT wait.  A non-zero return means nothing is in flight and
// nothing is held (codes[] of the caller are then filled by the caller from G.P where they are set, else with the return).
int group_begin(Group& G, const unsigned char* const* blobs, const size_t* sizes, int count, int force_host, bool side = false,
                const impgpu_jpeg_prepared* prep = nullptr, int accept = 0) {
    if (const int rc = group_open(G, blobs, sizes, count, side, prep)) return rc;
    Begin B{G, force_host, accept};
    plan_files(B);
    G.sw.mark();                                                    // [0] headers
    void* host = nullptr;
    if (const int rc = stage_begin(G.on_device ? B.t.words : B.t.coef, &host, &B.token)) { group_release(G); return rc; }
    B.host = (uint8_t*)host;
    stage_files(B);
    G.sw.mark();                                                    // [1] unstuffing copy / host entropy decoding
    G.profile = g_profile.load(std::memory_order_relaxed) != 0;
    G.mailbox = lane_mailbox() ? lane_mailbox() + 1024 * (1 + G.slot) : nullptr;      // (slot 0 of the mailbox is the other callers': brightness, the encoder)
    if (G.live == 0) { (void)stage_upload(B.token, nullptr, 0); return IMP_OK; }
    if (!G.mailbox) return group_abort(B, IMP_ERROR_DEVICE);
    plan_side(B);
    if (const int rc = allocate(B)) return group_abort(B, rc);
    fill_side(B);
    G.sw.mark();                                                    // [2] tables + job table
    if (const int rc = upload_and_enqueue(B)) return group_abort(B, rc);
    G.sw.mark();                                                    // [3] enqueue
    if (const int rc = lane_mark_on(G.stream, &G.mark)) return group_abort(B, rc);
    return IMP_OK;
}

// IMPGPU_JPEG_TRACE=2: the workgroups' clocks at their phase boundaries (the kernels' stamp()), microseconds since the launch's
// first workgroup started: wg: start | candidates loaded | twins | maps | scan + look-back | done (incl. the check of a guess), then
// the rounds of picking and the chunks the workgroup chased
void trace_clocks(const Group& G) {
    std::vector<uint32_t> ctl(G.ctl_total);
    if (hipMemcpy(ctl.data(), G.d_ctl, G.ctl_total * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return;
    uint32_t t0 = 0;
    bool have = false;
    for (const Prep& p : G.P)
        if (!p.code)
            for (unsigned b = 0; b < jpeg_sync_blocks(p.F.nchunks, p.F.bpm); b++) {
                const uint32_t v = ctl[p.ctl_records + (size_t)b * JPEG_CTL_REC + 20];
                if (!have || (int32_t)(v - t0) < 0) { t0 = v; have = true; }
            }
    auto us = [t0](uint32_t clock) { return (double)(int32_t)(clock - t0) / 100.0; };
    for (const Prep& p : G.P) {                                     // k_jpeg_write: every workgroup's start and end, and its walk's
        if (p.code) continue;
        const unsigned nb2 = jpeg_entropy_blocks(p.F.nchunks * p.F.wsplit);
        std::vector<int> wg((size_t)nb2 * 8);
        const size_t at = p.work_off + jpeg_work_layout(p.F.nchunks, p.F.wsplit, p.F.bpm, p.F.total_slots).wg_dc;
        if (hipMemcpy(wg.data(), (uint8_t*)G.d_work + at, wg.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) continue;
        for (unsigned b = 0; b < nb2; b++)
            std::fprintf(stderr, "ww %dx%d %u/%u: %.1f %.1f walk %.1f %.1f\n", p.H.width, p.H.height, b, nb2, us((uint32_t)wg[8 * b + 4]), us((uint32_t)wg[8 * b + 5]),
                         us((uint32_t)wg[8 * b + 6]), us((uint32_t)wg[8 * b + 7]));
    }
    for (const Prep& p : G.P) {
        if (p.code) continue;
        const unsigned nb = jpeg_sync_blocks(p.F.nchunks, p.F.bpm);
        for (unsigned b = 0; b < nb; b++) {
            const uint32_t* r = &ctl[p.ctl_records + (size_t)b * JPEG_CTL_REC + 20];
            std::fprintf(stderr, "wg %dx%d %u/%u:", p.H.width, p.H.height, b, nb);
            for (int k = 0; k <= 5; k++) std::fprintf(stderr, " %.1f", r[k] ? us(r[k]) : -1.0);
            std::fprintf(stderr, " rounds %u chased %u", r[9], r[10]);
            if (r[6]) std::fprintf(stderr, " | fused: start %.1f walks %.1f mend %.1f", us(r[6]), us(r[7]), us(r[8]));
            std::fprintf(stderr, "\n");
        }
    }
}

// IMPGPU_JPEG_TRACE=3: every chunk's entry state and slot count as k_jpeg_select left them ("ce <chunk> <state> <slots>": the
// host model prints the same)
void trace_entries(const Group& G) {
    for (const Prep& p : G.P) {
        if (p.code) continue;
        std::vector<uint64_t> ent(p.F.nchunks);
        std::vector<uint32_t> cn(p.F.nchunks);
        const JpegWorkLayout L = jpeg_work_layout(p.F.nchunks, p.F.wsplit, p.F.bpm, p.F.total_slots);
        const uint8_t* wk = (const uint8_t*)G.d_work + p.work_off;
        if (hipMemcpy(ent.data(), wk + L.chunk_entry, ent.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) continue;
        if (hipMemcpy(cn.data(), wk + L.chunk_n, cn.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) continue;
        for (size_t g = 0; g < ent.size(); g++) std::fprintf(stderr, "ce %zu %016llx %u\n", g, (unsigned long long)ent[g], cn[g]);
    }
}

// the device's verdict on every file of the group: counted, and a refusal left in the file's code
void read_verdicts(Group& G) {
    const uint32_t* mailbox = G.mailbox;
    const bool trace = G.sw.on && std::getenv("IMPGPU_JPEG_TRACE");
    size_t j = 0;
    for (Prep& p : G.P) {
        if (p.code) continue;
        const uint32_t status = mailbox[4 * j + 1];
        if (trace) std::fprintf(stderr, "jpeg %dx%d: %u chunks of %u bits (overlap %u), %u repair walks, %u chunks chased, %u walks in k_jpeg_select, status %u\n", p.H.width, p.H.height, p.F.nchunks, p.F.chunk_bits, p.F.overlap_bits, mailbox[4 * j + 2], mailbox[4 * j + 3], mailbox[4 * j + 0], status);
        g_count[0].fetch_add(1, std::memory_order_relaxed);
        if (status) g_count[1].fetch_add(1, std::memory_order_relaxed);
        if (status & JPEG_ST_CHAIN_TIMEOUT) g_count[2].fetch_add(1, std::memory_order_relaxed);
        if (p.is_prog && !status) g_count[COUNT_PROG].fetch_add(1, std::memory_order_relaxed);
        if (status) {
            char text[96];
            std::snprintf(text, sizeof text, "jpeg entropy stage refused the scan (status 0x%x)", status);
            set_error_text(text);
            p.code = IMP_ERROR_DECODE_FAILED;
        }
        j++;
    }
}

// the group's stages for impgpu_jpeg_stage_times (the host's from its clock, the device's from the events), and the call's trace line
void note_stage_times(const Group& G) {
    const Stopwatch& sw = G.sw;
    const bool events = G.profile && G.on_device;
    if (g_profile.load(std::memory_order_relaxed)) {
        for (int i = 0; i < 16; i++) t_stage[i] = 0;
        for (int i = 0; i < 5; i++) t_stage[i] = sw.marks[i];
        if (events && hipEventSynchronize(G.ev[7]) == hipSuccess)
            for (int i = 0; i < 7; i++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, G.ev[i], G.ev[i + 1]) == hipSuccess) t_stage[5 + i] = 1e3 * ms;
                else (void)hipGetLastError();                       // (a group of progressive files alone records no event between the sequential kernels)
            }
        t_stage[12] = (double)G.live;
        if (events && G.prog_files) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, G.ev[8], G.ev[9]) == hipSuccess) t_stage[13] = 1e3 * ms;
        }
        t_stage[14] = (double)G.prog_launches;
        t_stage[15] = (double)G.prog_files;
    }
    if (sw.on && std::getenv("IMPGPU_JPEG_TRACE"))
        std::fprintf(stderr, "jpeg x%d (%zu live): headers %.0f %s %.0f jobs %.0f enqueue %.0f wait %.0f us\n", G.count, G.live, sw.marks[0],
                     G.on_device ? "unstuff" : "host-entropy", sw.marks[1], sw.marks[2], sw.marks[3], sw.marks[4]);
}

// The other half: waits for the group's last kernel (not for whatever the thread enqueued after it), reads the verdicts,
// hands the frames out, gives the device memory back.
int group_finish(Group& G, impgpu_image** images, int* codes) {
    if (G.live) {
        const int rc = lane_wait_mark(G.mark);
        G.mark = nullptr;
        if (rc) {
            if (G.stream) (void)hipStreamSynchronize(G.stream);
            (void)lane_wait();                                      // nothing of this group may still be running when its buffers go back
            for (int i = 0; i < G.count; i++) {
                Prep& p = G.P[(size_t)i];
                if (p.im && !p.given) image_delete(p.im);
                images[i] = nullptr;
                codes[i] = p.code ? p.code : rc;
            }
            group_release(G);
            return rc;
        }
        if (G.on_device) {
            const char* tr = std::getenv("IMPGPU_JPEG_TRACE");
            if (tr && !std::strcmp(tr, "2")) trace_clocks(G);
            if (tr && !std::strcmp(tr, "3")) trace_entries(G);
            read_verdicts(G);
        }
        G.sw.mark();                                                // [4] wait for the verdicts
        note_stage_times(G);
    }
    for (int i = 0; i < G.count; i++) {
        Prep& p = G.P[(size_t)i];
        if (p.given) { images[i] = nullptr; codes[i] = p.code; continue; }      // (the caller has the frame: the code says whether it holds the file's pixels)
        if (p.code && p.im) { image_delete(p.im); p.im = nullptr; }
        images[i] = p.im;
        codes[i] = p.code;
    }
    group_release(G);
    return IMP_OK;
}

// codes[] after a group_begin that failed with `rc`: a file's own refusal where it has one, else the call's
void codes_of_failed_begin(const Group& G, int rc, int n, int* codes) {
    for (int i = 0; i < n; i++) codes[i] = G.P.size() > (size_t)i && G.P[(size_t)i].code ? G.P[(size_t)i].code : rc;
}

// files a device group deferred (dense blocks: CODE_DEFERRED) are decoded in a host-entropy group of their own
int group_deferred(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_image** images, int* codes, const impgpu_jpeg_prepared* prep = nullptr) {
    std::vector<int> late;
    for (int i = 0; i < count; i++) if (codes[i] == CODE_DEFERRED) late.push_back(i);
    if (late.empty()) return IMP_OK;
    std::vector<const unsigned char*> b2(late.size());
    std::vector<size_t> s2(late.size());
    std::vector<impgpu_image*> i2(late.size(), nullptr);
    std::vector<int> c2(late.size(), IMP_OK);
    std::vector<impgpu_jpeg_prepared> p2;
    for (size_t k = 0; k < late.size(); k++) { b2[k] = blobs[late[k]]; s2[k] = sizes[late[k]]; if (prep) p2.push_back(prep[late[k]]); }
    Group H;
    int rc = group_begin(H, b2.data(), s2.data(), (int)late.size(), 1, false, prep ? p2.data() : nullptr);
    if (!rc) rc = group_finish(H, i2.data(), c2.data());
    else codes_of_failed_begin(H, rc, (int)late.size(), c2.data());
    for (size_t k = 0; k < late.size(); k++) { images[late[k]] = rc ? nullptr : i2[k]; codes[late[k]] = rc ? rc : c2[k]; }
    if (rc) for (int i = 0; i < count; i++) if (images[i]) { impgpu_image_release(&images[i]); codes[i] = rc; }
    return rc;
}

// One group, begun and finished in one go -- except that a large group is cut in two and the second half is PREPARED (headers,
// unstuffing copy, job table: 2.3 of a 64-file call's 5.8 ms) while the device already works on the first: one calling thread
// went 11 -> 15 k requests/s with that.  When other threads keep the device busy anyway (four or more groups in flight) the
// group stays whole: two launches of half the size are the less efficient way to fill a device that is already full.
int decode_group(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_image** images, int* codes, int accept = 0) {
    const bool whole = std::getenv("IMPGPU_JPEG_WHOLE") != nullptr;      // measurements of ONE launch per batch (tools/jpeg_prof_r04.sh, bench.py's stage profile); read per call
    // (the two halves take a mailbox slot each: with batches begun and not finished on this thread -- impgpu_batch_decode_jpeg_begin --
    // holding three of the four, the group stays whole instead of failing for want of a second slot)
    const int free_slots = GROUP_SLOTS - __builtin_popcount(t_slots_busy & ((1u << GROUP_SLOTS) - 1));
    const int first = !whole && count >= 32 && free_slots >= 2 && g_groups_in_flight.load(std::memory_order_relaxed) < 4 ? count / 2 : count;
    Group A, B;
    int rc = group_begin(A, blobs, sizes, first, 0, false, nullptr, accept);
    if (rc) {
        codes_of_failed_begin(A, rc, first, codes);
        for (int i = 0; i < count; i++) { images[i] = nullptr; if (i >= first) codes[i] = rc; }
        return rc;
    }
    int rcb = IMP_OK;
    // Both halves on the lane's stream (the second half on the lane's side stream was measured on one box, two repetitions: the
    // same at 1, 2 and 8 threads, 7 % slower at 4 -- so it is not used here; impgpu_batch_decode_jpeg_begin does use it).
    if (first < count) rcb = group_begin(B, blobs + first, sizes + first, count - first, 0, false, nullptr, accept);
    rc = group_finish(A, images, codes);
    if (first < count) {
        if (!rcb) rcb = group_finish(B, images + first, codes + first);
        else for (int i = first; i < count; i++) { images[i] = nullptr; codes[i] = rcb; }
        if (!rc) rc = rcb;
    }
    if (rc) {
        for (int i = 0; i < count; i++) if (images[i]) { impgpu_image_release(&images[i]); codes[i] = rc; }
        return rc;
    }
    return group_deferred(blobs, sizes, count, images, codes);
}

// one group of files whose scans the caller has unstuffed: never cut in two, nothing accepted beyond baseline
int decode_prepared_group(const unsigned char* const* blobs, const size_t* sizes, const impgpu_jpeg_prepared* files, int n, impgpu_image** images, int* codes) {
    Group A;
    int rc = group_begin(A, blobs, sizes, n, 0, false, files);
    if (rc) codes_of_failed_begin(A, rc, n, codes);
    else rc = group_finish(A, images, codes);
    if (!rc) rc = group_deferred(blobs, sizes, n, images, codes, files);
    return rc;
}

// A call's files, MAX_BATCH at a time through `decode(at, n)`.  A slice that fails has seen to its own images and codes;
// the frames of the slices before it are released, the files behind it get the call's code.
template <class Decode>
int decode_in_slices(int count, impgpu_image** images, int* codes, Decode decode) {
    for (int at = 0; at < count; at += MAX_BATCH) {
        const int n = count - at < MAX_BATCH ? count - at : MAX_BATCH;
        if (const int rc = decode(at, n)) {
            for (int i = 0; i < at; i++) impgpu_image_release(&images[i]);
            for (int i = at + n; i < count; i++) { images[i] = nullptr; codes[i] = rc; }
            return rc;
        }
    }
    return IMP_OK;
}

// what every decode entry point does behind the check of its arguments (a macro: the range lives in the caller, the fault point returns from it)
#define JPEG_DECODE_ENTER()                                                                                  \
    if (!env_ready()) { set_error_text("impgpu_env_start has not been called"); return IMP_ERROR_DEVICE; }   \
    TraceRange tr("IMP_STEP_DECODE");                                                                        \
    IMP_FAULT_POINT(IMP_STEP_DECODE)

}  // namespace

struct impgpu_jpeg_batch {
    Group G;
    std::vector<impgpu_jpeg_prepared> files;        // impgpu_batch_decode_jpeg_prepared_begin: its own copy of the caller's array
    std::vector<const unsigned char*> blobs;
    std::vector<size_t> sizes;
};

extern "C" {

int impgpu_batch_decode_jpeg(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_image** images, int* codes) {
    return impgpu_batch_decode_jpeg_ex(blobs, sizes, count, 0, images, codes);
}

int impgpu_batch_decode_jpeg_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept, impgpu_image** images, int* codes) {
    if (count < 0 || (count && (!blobs || !sizes || !images || !codes))) return IMP_ERROR_INVALID_ARGS;
    JPEG_DECODE_ENTER();
    return decode_in_slices(count, images, codes, [&](int at, int n) { return decode_group(blobs + at, sizes + at, n, images + at, codes + at, accept); });
}

int impgpu_batch_decode_jpeg_begin(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_jpeg_batch** batch) {
    return impgpu_batch_decode_jpeg_begin_ex(blobs, sizes, count, 0, batch);
}

int impgpu_batch_decode_jpeg_begin_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept, impgpu_jpeg_batch** batch) {
    if (!batch) return IMP_ERROR_INVALID_ARGS;
    *batch = nullptr;
    if (count <= 0 || count > MAX_BATCH || !blobs || !sizes) return IMP_ERROR_INVALID_ARGS;
    JPEG_DECODE_ENTER();
    impgpu_jpeg_batch* b = new impgpu_jpeg_batch();
    // on the lane's side stream: what the thread enqueues before _finish overlaps it
    const int rc = group_begin(b->G, blobs, sizes, count, 0, true, nullptr, accept);
    if (rc) { delete b; return rc; }
    *batch = b;
    return IMP_OK;
}

int impgpu_batch_decode_jpeg_finish(impgpu_jpeg_batch** batch, impgpu_image** images, int* codes) {
    if (!batch || !*batch || !images || !codes) return IMP_ERROR_INVALID_ARGS;
    impgpu_jpeg_batch* b = *batch;
    // the slot, the mark event and the pool blocks belong to the beginning thread's lane: another thread would clear its own
    // slot bits and hand the event to its own lane.  Refused; the batch stays valid for its owner.
    if (b->G.owner != &t_thread_tag) { set_error_text("impgpu_batch_decode_jpeg_finish from another thread than _begin"); return IMP_ERROR_INVALID_ARGS; }
    *batch = nullptr;
    const unsigned char* const* blobs = b->G.blobs;
    const size_t* sizes = b->G.sizes;
    const int count = b->G.count;
    int rc = group_finish(b->G, images, codes);
    if (!rc) rc = group_deferred(blobs, sizes, count, images, codes, b->G.prep);
    delete b;
    return rc;
}

int impgpu_batch_decode_jpeg_pending(impgpu_jpeg_batch* batch, impgpu_image** images) {
    if (!batch || !images) return IMP_ERROR_INVALID_ARGS;
    Group& G = batch->G;
    if (G.owner != &t_thread_tag) { set_error_text("impgpu_batch_decode_jpeg_pending from another thread than _begin"); return IMP_ERROR_INVALID_ARGS; }
    // (only a batch whose kernels are on the thread's OWN stream: what the caller enqueues on the frames runs behind them)
    if (G.stream && !on_lane_stream(G.stream)) { set_error_text("impgpu_batch_decode_jpeg_pending: the batch runs on the thread's second stream"); return IMP_ERROR_INVALID_ARGS; }
    for (int i = 0; i < G.count; i++) {
        Prep& p = G.P[(size_t)i];
        images[i] = nullptr;
        if (p.code || !p.im || p.given) continue;               // refused at its header, deferred to the host's Huffman stage, or handed out already
        images[i] = p.im;
        p.given = true;
    }
    return IMP_OK;
}

int impgpu_batch_decode_jpeg_prepared_begin(const impgpu_jpeg_prepared* files, int count, impgpu_jpeg_batch** batch) {
    return impgpu_batch_decode_jpeg_prepared_begin_ex(files, count, 0, batch);
}

int impgpu_batch_decode_jpeg_prepared_begin_ex(const impgpu_jpeg_prepared* files, int count, int accept, impgpu_jpeg_batch** batch) {
    if (!batch) return IMP_ERROR_INVALID_ARGS;
    *batch = nullptr;
    if (count <= 0 || count > MAX_BATCH || !files) return IMP_ERROR_INVALID_ARGS;
    JPEG_DECODE_ENTER();
    impgpu_jpeg_batch* b = new impgpu_jpeg_batch();
    b->files.assign(files, files + count);
    b->blobs.resize((size_t)count);
    b->sizes.resize((size_t)count);
    for (int i = 0; i < count; i++) { b->blobs[(size_t)i] = files[i].head; b->sizes[(size_t)i] = files[i].head_size; }
    const int rc = group_begin(b->G, b->blobs.data(), b->sizes.data(), count, 0, false, b->files.data(), accept);
    if (rc) { delete b; return rc; }
    *batch = b;
    return IMP_OK;
}

int impgpu_batch_decode_jpeg_prepared(const impgpu_jpeg_prepared* files, int count, impgpu_image** images, int* codes) {
    if (count < 0 || (count && (!files || !images || !codes))) return IMP_ERROR_INVALID_ARGS;
    JPEG_DECODE_ENTER();
    std::vector<const unsigned char*> blobs((size_t)count);
    std::vector<size_t> sizes((size_t)count);
    for (int i = 0; i < count; i++) { blobs[(size_t)i] = files[i].head; sizes[(size_t)i] = files[i].head_size; images[i] = nullptr; codes[i] = IMP_OK; }
    return decode_in_slices(count, images, codes, [&](int at, int n) { return decode_prepared_group(blobs.data() + at, sizes.data() + at, files + at, n, images + at, codes + at); });
}

int impgpu_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return IMP_ERROR_INVALID_ARGS;
    if (!env_ready() || !env_stream()) { set_error_text("impgpu_env_start has not been called"); return IMP_ERROR_DEVICE; }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) { set_error("hipHostRegister", e); (void)hipGetLastError(); return IMP_ERROR_DEVICE; }
    return IMP_OK;
}

int impgpu_host_unregister(void* p) {
    if (!p) return IMP_ERROR_INVALID_ARGS;
    const hipError_t e = hipHostUnregister(p);
    if (e != hipSuccess) { set_error("hipHostUnregister", e); (void)hipGetLastError(); return IMP_ERROR_DEVICE; }
    return IMP_OK;
}

int impgpu_jpeg_counters(unsigned long long* counters, int n) {
    if (!counters || n < 0) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < n; i++) counters[i] = i < COUNT_SLOTS ? g_count[i].load(std::memory_order_relaxed) : 0ull;
    return IMP_OK;
}

int impgpu_jpeg_profile(int on) {
    return g_profile.exchange(on ? 1 : 0);
}

int impgpu_jpeg_stage_times(double* microseconds, int n) {
    if (!microseconds || n < 0) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < n; i++) microseconds[i] = i < 16 ? t_stage[i] : 0.0;
    return IMP_OK;
}

int impgpu_image_decode_jpeg(const unsigned char* blob, size_t size, impgpu_image** out) {
    return impgpu_image_decode_jpeg_ex(blob, size, 0, out);
}

int impgpu_image_decode_jpeg_ex(const unsigned char* blob, size_t size, int accept, impgpu_image** out) {
    if (!blob || !out) return IMP_ERROR_INVALID_ARGS;
    *out = nullptr;
    int code = IMP_OK;
    const int rc = impgpu_batch_decode_jpeg_ex(&blob, &size, 1, accept, out, &code);
    return rc ? rc : code;
}

}  // extern "C"
