// imp_webp_dec.cpp -- lossless WebP uploads in: impgpu_batch_decode_webp reads every file's front on the host
// (imp_webp_dec_host.h: the container, the header, the transforms with their sub-images, the cache size, the entropy
// image, the code lengths), lays the files it took out in one device block a group -- descriptors, the table launch's
// items, then per file the compressed words, the code lengths, the entropy image and the transforms' data, uploaded once
// from one pinned block; behind them the status words (zeroed) and per file the codes, their sorted symbols and the
// residual plane, which never cross the link -- runs the three launches of imp_webp_dec.hip on it and waits ONCE per
// call, for the status words of all its groups.  impgpu_webp_decode_host is the same decoder with no device.
// The _ex calls with IMPGPU_WEBP_ACCEPT_LOSSY take VP8 key frames too (imp_vp8_dec_host.h, imp_vp8_dec.hip): a lossy file
// puts a descriptor and its chunk's bytes into the same upload, its planes and contexts behind it, and its status word
// behind the lossless files' -- a group launches each kind's kernels only if it holds that kind.
// With IMPGPU_WEBP_ACCEPT_ALPHA too a lossy file may bring an alpha plane (imp_webp_alpha.h): raw bytes that join the
// upload, or a VP8L stream that is one more item of the lossless launches, decoded into a scratch plane behind the upload
// with a status word of its own; k_webp_alpha (imp_webp_alpha.hip) then writes byte 3 of the frame.
#include <algorithm>
#include "imp_internal.h"
#include "imp_enc_host.h"
#include "imp_webp_dec_host.h"
#include "imp_vp8_dec_host.h"

namespace imp {

int launch_vp8_decode(uint8_t* mem, const VdFileDesc* files, uint32_t* status, int nfiles, hipStream_t s);
int launch_webp_decode(uint8_t* mem, const WdFileDesc* files, const WdCodeItem* items, long long nitems, uint32_t* status, int nfiles, hipStream_t s);
int launch_webp_alpha(uint8_t* mem, const WaFileDesc* files, const uint32_t* status, int nfiles, hipStream_t s);

namespace {

struct WdEntry {
    int entry;                            // its index in the call's arrays
    WdPlan plan;
    bool lossy = false;
    VdPlan vplan;
    VaPlane alpha;                        // of a lossy file; method 1: `plan` is its VP8L stream's
    size_t upload, device;                // what it puts into the group's upload, and behind it
};

size_t wd_upload_bytes(const WdPlan& P) {
    size_t n = up256(P.words.size() * 4u) + up256(P.lens.size()) + up256(P.meta.size() * 4u);
    for (int i = 0; i < P.ntrans; i++) n += up256(P.trdata[i].size() * 4u);
    return n + up256(sizeof(WdFileDesc)) + up256((size_t)P.ngroups * WD_CODES * sizeof(WdCodeItem));
}
size_t wd_device_bytes(const WdPlan& P) {
    return up256((size_t)P.ngroups * WD_CODES * sizeof(WdCode)) + up256((size_t)P.ngroups * wd_sorted_stride(P.cache_bits) * 2u) +
           up256((size_t)P.w * (size_t)P.h * 4u) + 256u;
}

size_t vd_upload_bytes(const VdPlan& P) { return up256(sizeof(VdFileDesc)) + up256(P.chunk.size()); }
size_t vd_device_bytes(const VdPlan& P) {
    const size_t mbw = (size_t)P.hdr.mbw, mbh = (size_t)P.hdr.mbh;
    return up256(mbw * mbh * 256u) + 2u * up256(mbw * mbh * 64u) + up256(mbw * mbh * 4u) + up256(mbw * 6u) + 256u;
}

size_t va_upload_bytes(const WdEntry& e) {
    if (!e.alpha.present) return 0;
    return up256(sizeof(WaFileDesc)) + (e.alpha.method ? wd_upload_bytes(e.plan) : up256((size_t)e.plan.w * (size_t)e.plan.h));
}
size_t va_device_bytes(const WdEntry& e) {                               // a VP8L plane: the stream's own blocks and the scratch plane it decodes into
    return e.alpha.present && e.alpha.method ? wd_device_bytes(e.plan) + up256((size_t)e.plan.w * (size_t)e.plan.h * 4u) : 0;
}

struct WdGroupRun {                       // a group in flight: its block lives until the call's one wait is over
    DevBlock block;
    std::vector<int> entries;             // the entry of every status word: a lossy file with a VP8L plane has two
    uint32_t* status = nullptr;
    int piece = -1;
};

// one group: upload and launches, nothing waited for
int decode_group(const std::vector<WdEntry*>& all, impgpu_image** images, WdGroupRun* run) {
    hipStream_t s = env_stream();
    // the lossless files, the VP8L alpha planes (lossless items too), then the lossy files: the order of the status words
    std::vector<WdEntry*> group, lossy, planes;
    for (WdEntry* e : all) (e->lossy ? lossy : group).push_back(e);
    const int nreal = (int)group.size();                                // those that decode into an image
    for (WdEntry* e : lossy)
        if (e->alpha.present) {
            planes.push_back(e);
            if (e->alpha.method) group.push_back(e);
        }
    const int nf = (int)group.size(), ny = (int)lossy.size(), na = (int)planes.size();
    run->entries.clear();
    for (const WdEntry* e : group) run->entries.push_back(e->entry);
    for (const WdEntry* e : lossy) run->entries.push_back(e->entry);
    std::vector<WaFileDesc> afd((size_t)na);
    std::vector<VdFileDesc> vfd((size_t)ny);
    std::vector<WdFileDesc> fd((size_t)nf);
    std::vector<WdCodeItem> items;
    BlockLayout L;
    const size_t o_fd = L.take((size_t)nf * sizeof(WdFileDesc));
    size_t nitems = 0;
    for (const WdEntry* e : group) nitems += (size_t)e->plan.ngroups * WD_CODES;
    if (nitems > 0x7fffffffull) return IMP_ERROR_UNSUPPORTED;
    const size_t o_items = L.take(nitems * sizeof(WdCodeItem));
    std::vector<size_t> o_tr((size_t)nf * 4u, 0);
    for (int f = 0; f < nf; f++) {
        const WdPlan& P = group[(size_t)f]->plan;
        WdFileDesc& d = fd[(size_t)f];
        std::memset(&d, 0, sizeof d);
        d.in_off = (long long)L.take(P.words.size() * 4u);
        d.lens_off = (long long)L.take(P.lens.size());
        d.meta_off = (long long)L.take(P.meta.size() * 4u);
        d.ntrans = P.ntrans;
        for (int i = 0; i < P.ntrans; i++) {
            d.tr[i] = P.tr[i];
            d.tr[i].data_off = (long long)(o_tr[(size_t)f * 4u + (size_t)i] = L.take(P.trdata[i].size() * 4u));
        }
        d.bitpos = P.bitpos;
        d.in_size = P.in_size; d.in_cap = (uint32_t)(P.words.size() * 4u); d.ngroups = P.ngroups;
        d.w = P.w; d.h = P.h; d.cw = P.cw; d.alpha_used = P.alpha_used;
        d.cache_bits = P.cache_bits; d.meta_bits = P.meta_bits; d.meta_w = P.meta_w;
        d.img = f < nreal ? images[group[(size_t)f]->entry]->d : nullptr;   // a plane's scratch: placed below
        for (uint32_t g = 0; g < P.ngroups; g++)
            for (int k = 0; k < WD_CODES; k++) items.push_back(WdCodeItem{f, g, k, 0});
    }
    const size_t o_vfd = L.take((size_t)ny * sizeof(VdFileDesc));
    for (int f = 0; f < ny; f++) {
        VdFileDesc& d = vfd[(size_t)f];
        std::memset(&d, 0, sizeof d);
        d.hdr = lossy[(size_t)f]->vplan.hdr;
        d.chunk_off = (long long)L.take(lossy[(size_t)f]->vplan.chunk.size());
        d.img = images[lossy[(size_t)f]->entry]->d;
    }
    const size_t o_afd = L.take((size_t)na * sizeof(WaFileDesc));
    for (int f = 0, k = nreal; f < na; f++) {
        const WdEntry* e = planes[(size_t)f];
        WaFileDesc& d = afd[(size_t)f];
        std::memset(&d, 0, sizeof d);
        d.img = images[e->entry]->d;
        d.w = e->plan.w; d.h = e->plan.h; d.filter = e->alpha.filter; d.method = e->alpha.method;
        d.status_frame = nf + (int)(std::find(lossy.begin(), lossy.end(), e) - lossy.begin());
        d.status_stream = e->alpha.method ? k++ : d.status_frame;
        if (!e->alpha.method) d.src_off = (long long)L.take((size_t)d.w * (size_t)d.h);
    }
    const size_t upload = L.size();                                     // where the upload ends
    const size_t o_status = L.take((size_t)(nf + ny) * 4u);
    for (int f = 0; f < ny; f++) {
        VdFileDesc& d = vfd[(size_t)f];
        const size_t nmb = (size_t)d.hdr.mbw * (size_t)d.hdr.mbh;
        d.y_off = (long long)L.take(nmb * 256u);
        d.u_off = (long long)L.take(nmb * 64u);
        d.v_off = (long long)L.take(nmb * 64u);
        d.finfo_off = (long long)L.take(nmb * 4u);
        d.ctx_off = (long long)L.take((size_t)d.hdr.mbw * 6u);
    }
    for (int f = 0; f < nf; f++) {
        const WdPlan& P = group[(size_t)f]->plan;
        fd[(size_t)f].codes_off = (long long)L.take((size_t)P.ngroups * WD_CODES * sizeof(WdCode));
        fd[(size_t)f].sorted_off = (long long)L.take((size_t)P.ngroups * wd_sorted_stride(P.cache_bits) * 2u);
        fd[(size_t)f].plane_off = (long long)L.take((size_t)P.w * (size_t)P.h * 4u);
    }
    std::vector<size_t> o_scratch((size_t)na, 0);
    for (int f = 0; f < na; f++)
        if (afd[(size_t)f].method) afd[(size_t)f].src_off = (long long)(o_scratch[(size_t)f] = L.take((size_t)afd[(size_t)f].w * (size_t)afd[(size_t)f].h * 4u));
    if (int rc = dev_alloc(L.size(), &run->block.p)) return rc;
    uint8_t* m = run->block.bytes();
    for (int f = 0; f < na; f++)
        if (afd[(size_t)f].method) fd[(size_t)afd[(size_t)f].status_stream].img = m + o_scratch[(size_t)f];
    void *host = nullptr, *token = nullptr;
    if (int rc = stage_begin(upload, &host, &token)) return rc;
    uint8_t* hp = (uint8_t*)host;
    if (nf) std::memcpy(hp + o_fd, fd.data(), fd.size() * sizeof(WdFileDesc));
    if (!items.empty()) std::memcpy(hp + o_items, items.data(), items.size() * sizeof(WdCodeItem));
    if (ny) std::memcpy(hp + o_vfd, vfd.data(), vfd.size() * sizeof(VdFileDesc));
    if (na) std::memcpy(hp + o_afd, afd.data(), afd.size() * sizeof(WaFileDesc));
    for (int f = 0; f < na; f++)
        if (!afd[(size_t)f].method) std::memcpy(hp + afd[(size_t)f].src_off, planes[(size_t)f]->alpha.data, (size_t)afd[(size_t)f].w * (size_t)afd[(size_t)f].h);
    for (int f = 0; f < ny; f++) std::memcpy(hp + vfd[(size_t)f].chunk_off, lossy[(size_t)f]->vplan.chunk.data(), lossy[(size_t)f]->vplan.chunk.size());
    for (int f = 0; f < nf; f++) {
        const WdPlan& P = group[(size_t)f]->plan;
        const WdFileDesc& d = fd[(size_t)f];
        std::memcpy(hp + d.in_off, P.words.data(), P.words.size() * 4u);
        std::memcpy(hp + d.lens_off, P.lens.data(), P.lens.size());
        if (!P.meta.empty()) std::memcpy(hp + d.meta_off, P.meta.data(), P.meta.size() * 4u);
        for (int i = 0; i < P.ntrans; i++)
            if (!P.trdata[i].empty()) std::memcpy(hp + o_tr[(size_t)f * 4u + (size_t)i], P.trdata[i].data(), P.trdata[i].size() * 4u);
    }
    int rc = stage_upload(token, m, upload);
    if (!rc) {
        const hipError_t e = hipMemsetAsync(m + o_status, 0, up256((size_t)(nf + ny) * 4u), s);
        if (e != hipSuccess) { set_error("hipMemsetAsync(webp decode)", e); rc = IMP_ERROR_DEVICE; }
    }
    run->status = (uint32_t*)(m + o_status);
    if (!rc && nf) rc = launch_webp_decode(m, (const WdFileDesc*)(m + o_fd), (const WdCodeItem*)(m + o_items), (long long)nitems, run->status, nf, s);
    if (!rc && ny) rc = launch_vp8_decode(m, (const VdFileDesc*)(m + o_vfd), run->status + nf, ny, s);
    if (!rc && na) rc = launch_webp_alpha(m, (const WaFileDesc*)(m + o_afd), run->status, na, s);
    return rc;
}

int batch_decode(const unsigned char* const* blobs, const size_t* sizes, int count, int accept, impgpu_image** images, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!blobs || !sizes || !images || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) images[i] = nullptr;
    if (count == 0) return IMP_OK;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    const unsigned long long launched = t_launches;
    const size_t cap = stage_cap();
    std::vector<std::unique_ptr<WdEntry>> taken;
    std::unique_ptr<WdMem> mem(new WdMem());
    for (int i = 0; i < count; i++) {
        if (!blobs[i]) { codes[i] = IMP_ERROR_INVALID_ARGS; continue; }
        std::unique_ptr<WdEntry> e(new WdEntry());
        e->entry = i;
        const uint8_t* payload = nullptr;
        uint32_t psize = 0;
        int lossy = 0;
        if ((codes[i] = vd_route(blobs[i], sizes[i], accept, &payload, &psize, &lossy, &e->alpha)) != IMP_OK) continue;
        if (lossy) {
            e->lossy = true;
            if ((codes[i] = vd_plan(payload, psize, &e->vplan)) != IMP_OK) continue;
            e->plan.w = e->vplan.hdr.w; e->plan.h = e->vplan.hdr.h;
            if (e->alpha.present && e->alpha.method && (codes[i] = va_parse_stream(e->alpha, e->plan.w, e->plan.h, &e->plan, mem.get())) != IMP_OK) continue;
            e->upload = vd_upload_bytes(e->vplan) + va_upload_bytes(*e);
            e->device = vd_device_bytes(e->vplan) + va_device_bytes(*e);
        } else {
            if ((codes[i] = wd_parse(blobs[i], sizes[i], &e->plan, mem.get())) != IMP_OK) continue;
            e->upload = wd_upload_bytes(e->plan);
            e->device = wd_device_bytes(e->plan);
        }
        if (cap && e->upload + e->device > cap) { codes[i] = IMP_ERROR_MALLOC_FAILED; continue; }   // a file that does not fit under the stage cap
        if ((codes[i] = image_new(e->plan.w, e->plan.h, 4, &images[i])) != IMP_OK) { images[i] = nullptr; continue; }
        taken.push_back(std::move(e));
    }
    // the groups: as many files as the stage cap takes; all are enqueued before the one wait
    std::vector<std::unique_ptr<WdGroupRun>> runs;
    AnswerFetch words;
    std::vector<WdEntry*> group;
    size_t bytes = 0;
    auto fail = [&](const std::vector<WdEntry*>& g, int rc) {
        for (const WdEntry* e : g) { codes[e->entry] = rc; image_delete(images[e->entry]); images[e->entry] = nullptr; }
    };
    int hard = IMP_OK;                                                   // a failure behind enqueued work: drain before the blocks go
    auto flush = [&]() {
        if (group.empty()) return;
        std::unique_ptr<WdGroupRun> run(new WdGroupRun());
        const int rc = decode_group(group, images, run.get());
        if (rc) {
            fail(group, rc);
            hard = rc;
        } else {
            run->piece = words.add(run->status, run->entries.size() * 4u);
        }
        runs.push_back(std::move(run));
        group.clear();
        bytes = 0;
    };
    for (auto& e : taken) {
        if (!group.empty() && cap && bytes + e->upload + e->device > cap) flush();
        group.push_back(e.get());
        bytes += e->upload + e->device;
    }
    flush();
    int rc = words.run("hipMemcpyAsync(webp decode status)");            // the call's one wait
    if (hard && !rc) (void)drained(hard);
    for (auto& run : runs) {
        if (run->piece < 0) continue;
        const uint32_t* st = (const uint32_t*)words.at(run->piece);
        for (size_t k = 0; k < run->entries.size(); k++) codes[run->entries[k]] = IMP_OK;
        for (size_t k = 0; k < run->entries.size(); k++) {                // a file fails if any of its status words is set
            const int i = run->entries[k];
            const int code = rc ? rc : st[k] ? IMP_ERROR_DECODE_FAILED : IMP_OK;
            if (code) codes[i] = code;
        }
        for (int i : run->entries)
            if (codes[i] && images[i]) { image_delete(images[i]); images[i] = nullptr; }
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" {

int impgpu_webp_info(const unsigned char* blob, size_t size, int* width, int* height, int* channels) {
    int w = 0, h = 0, alpha = 0;
    if (int rc = wd_info(blob, size, &w, &h, &alpha)) return rc;
    if (width) *width = w;
    if (height) *height = h;
    if (channels) *channels = 4;
    return IMP_OK;
}

int impgpu_webp_decode_host(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, int* width, int* height, int* info) {
    return wd_decode_host(blob, size, out, capacity, width, height, info);
}

int impgpu_batch_decode_webp(const unsigned char* const* blobs, const size_t* sizes, int count, impgpu_image** images, int* codes, int* launches) {
    return batch_decode(blobs, sizes, count, 0, images, codes, launches);
}

int impgpu_image_decode_webp(const unsigned char* blob, size_t size, impgpu_image** out) {
    if (out) *out = nullptr;
    if (!blob || !out) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = batch_decode(&blob, &size, 1, 0, out, &code, nullptr)) return rc;
    return code;
}

int impgpu_webp_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels) {
    int w = 0, h = 0;
    if (int rc = vd_info(blob, size, accept, &w, &h)) return rc;
    if (width) *width = w;
    if (height) *height = h;
    if (channels) *channels = 4;
    return IMP_OK;
}

int impgpu_webp_alpha_info(const unsigned char* blob, size_t size, int info[4]) { return va_info(blob, size, info); }

int impgpu_webp_decode_host_ex(const unsigned char* blob, size_t size, int accept, unsigned char* out, size_t capacity, int* width, int* height, int* info) {
    return vd_decode_host_any(blob, size, accept, out, capacity, width, height, info);
}

int impgpu_batch_decode_webp_ex(const unsigned char* const* blobs, const size_t* sizes, int count, int accept, impgpu_image** images, int* codes, int* launches) {
    return batch_decode(blobs, sizes, count, accept, images, codes, launches);
}

int impgpu_image_decode_webp_ex(const unsigned char* blob, size_t size, int accept, impgpu_image** out) {
    if (out) *out = nullptr;
    if (!blob || !out) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = batch_decode(&blob, &size, 1, accept, out, &code, nullptr)) return rc;
    return code;
}

}  // extern "C"
