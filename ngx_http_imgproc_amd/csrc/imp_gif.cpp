// imp_gif.cpp -- GIF files in: the container walk (include/impgpu_gif.h) on the host, the LZW pages and LoadGIF's
// compositing loop on the device.  impgpu_batch_decode_gif lays every accepted file's page table, output pointers,
// palettes and COMPRESSED pages out in one staging blob -- impgpu_batch_gif_compose's layout with the sub-block payloads
// where the index planes were -- and reserves the planes behind it in the same device block: one upload, k_gif_lzw
// (imp_gif.hip) decodes every page into its plane, k_gif_compose_mix (imp_geom.hip) follows on the same stream, and the
// call waits once, for the pages' status words.  With IMPGPU_GIF_SPLIT three launches stand where k_gif_lzw is one: the
// pages are cut at their clear codes and a wavefront decodes every segment; the segment tables lie behind the planes.
#include "imp_internal.h"
#include "imp_gif.h"
#include "../../include/impgpu_gif.h"

namespace imp {
static size_t up16(size_t v) { return (v + 15) & ~size_t(15); }
// a file whose index planes pass this goes back to the host decoder (4096 pages of 4096 x 4096 would be 64 GB)
static constexpr size_t GIF_PLANES_MAX = size_t(1) << 30;

static void gif_palette(const unsigned char* blob, const impgpu_gif_desc& d, uint8_t* out) {      // 256 x B,G,R,0; missing entries 0
    std::memset(out, 0, 1024);
    for (int k = 0; k < d.palette_entries; k++) {
        const unsigned char* q = blob + d.palette_at + 3 * (size_t)k;
        out[4 * k] = q[2]; out[4 * k + 1] = q[1]; out[4 * k + 2] = q[0];
    }
}

struct GifPlan {
    int entry, npages, nout, destructive, only, cw, ch;
    size_t first_desc;               // its pages in `descs`
    size_t up_bytes, plane_bytes;    // what it puts into the upload, and behind it
    int slot0;                       // its first status word
    long long seg_slots;             // IMPGPU_GIF_SPLIT: the segment slots of its pages (gif_seg_cap each)
};

}  // namespace imp

using namespace imp;

extern "C" {

int impgpu_gif_info(const unsigned char* blob, size_t size, int* count, int* canvas_width, int* canvas_height) {
    return impgpu_gif_walk(blob, size, nullptr, 0, count, canvas_width, canvas_height);
}

int impgpu_gif_pages(const unsigned char* blob, size_t size, int how, unsigned char* out, size_t capacity, size_t* length) {
    return gif_pages_host(blob, size, how, out, capacity, length);
}

int impgpu_gif_pages_split(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, size_t* length,
                           int* segments, int pages_capacity) {
    return gif_pages_split_host(blob, size, out, capacity, length, segments, pages_capacity);
}

int impgpu_batch_decode_gif_ex(const unsigned char* const* blobs, const size_t* sizes, const int* destructive, const int* page,
                               int count, int flags, impgpu_image** albums, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (flags & ~IMPGPU_GIF_SPLIT) return IMP_ERROR_INVALID_ARGS;
    const bool split = (flags & IMPGPU_GIF_SPLIT) != 0;
    if (count < 0 || count > 256 || (count > 0 && (!blobs || !sizes || !destructive || !page || !albums || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) albums[i] = nullptr;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    const unsigned long long launched = t_launches;
    auto head_bytes = [](int npages, int nout) { return up16((size_t)npages * sizeof(GifPageDev) + (size_t)nout * sizeof(uint8_t*)); };
    // every file judged as its lone call judges it: the container walk, then the page rules of impgpu_gif_compose_album
    std::vector<GifPlan> plans;
    std::vector<impgpu_gif_desc> descs, walked((size_t)IMPB_MAX_GIF_PAGES);
    int slots = 0;
    for (int i = 0; i < count; i++) {
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!blobs[i] || page[i] < -1) continue;
        int n = 0, cw = 0, ch = 0;
        if ((codes[i] = impgpu_gif_walk(blobs[i], sizes[i], walked.data(), (int)walked.size(), &n, &cw, &ch)) != IMP_OK) continue;
        int only = page[i], destr = destructive[i] ? 1 : 0;
        if (only != -1) {                                          // (gif_compose: a page request walks destructively, past the end = page 0)
            destr = 1;
            if (only > n - 1) only = 0;
        }
        GifPlan pl{i, only >= 0 ? only + 1 : n, only >= 0 ? 1 : n, destr, only, cw, ch, descs.size(), 0, 0, slots, 0};
        pl.up_bytes = head_bytes(pl.npages, pl.nout);
        bool huge = false;
        for (int f = 0; f < pl.npages; f++) {                      // pages behind the requested one are neither decoded nor judged
            huge = huge || walked[f].data_bytes >= GIF_DATA_MAX;
            pl.up_bytes += 1024 + up16(walked[f].data_bytes);
            pl.plane_bytes += up16((size_t)gif_pitch(walked[f].width) * walked[f].height);
            if (!huge) pl.seg_slots += gif_seg_cap((uint32_t)walked[f].data_bytes);
        }
        if (huge || pl.plane_bytes > GIF_PLANES_MAX) { codes[i] = IMP_ERROR_UNSUPPORTED; continue; }
        codes[i] = image_new_album(cw, ch, 4, pl.nout, &albums[i]);
        if (codes[i] != IMP_OK) continue;
        descs.insert(descs.end(), walked.begin(), walked.begin() + pl.npages);
        slots += pl.npages;
        plans.push_back(pl);
    }
    if (plans.empty()) return IMP_OK;
    hipStream_t s = env_stream();
    void* status_dev = nullptr;
    int rc_all = dev_alloc((size_t)slots * sizeof(uint32_t), &status_dev);
    const size_t cap = stage_cap();
    std::vector<char> ran(plans.size(), 0);
    for (size_t g0 = 0; g0 < plans.size();) {
        // the group [g0, g1): as many files as the staging cap and the grid take (impgpu_batch_gif_compose's cut)
        size_t g1 = g0, bytes = 0, planes = 0;
        long long blocks = 0, nslots = 0;
        int npages = 0;
        // (IMPGPU_GIF_SPLIT: the pages' GifSplitPage and the slot table travel behind the LZW descriptors)
        auto split_off = [&](int n, int pages) { return gif_mix_table_bytes(n) + up16((size_t)pages * sizeof(GifLzwDesc)); };
        auto front = [&](int n, int pages, long long nsl) {
            return split_off(n, pages) + (split ? up16((size_t)pages * sizeof(GifSplitPage)) + up16((size_t)nsl * sizeof(GifSegSlot)) : 0);
        };
        while (g1 < plans.size()) {
            const GifPlan& pl = plans[g1];
            const long long nb = ((long long)pl.cw * pl.ch + 255) / 256;
            if (g1 > g0 && ((cap && front((int)(g1 - g0 + 1), npages + pl.npages, nslots + pl.seg_slots) + bytes + pl.up_bytes > cap) ||
                            (blocks + nb) * 8 > 0x7fffffffLL || (split && nslots + pl.seg_slots > 0x7fffffffLL))) break;
            bytes += pl.up_bytes;
            planes += pl.plane_bytes;
            npages += pl.npages;
            blocks += nb;
            nslots += pl.seg_slots;
            g1++;
        }
        const int n = (int)(g1 - g0);
        const size_t lzw_off = gif_mix_table_bytes(n);
        const size_t pages_off = split_off(n, npages), slots_off = pages_off + up16((size_t)npages * sizeof(GifSplitPage));
        const size_t upload = front(n, npages, nslots) + bytes;
        // behind the planes, with the flag: every page's segment block, GifSeg[cap + 1] (the device's own; never uploaded)
        const size_t total = upload + planes + (split ? ((size_t)nslots + (size_t)npages) * sizeof(GifSeg) : 0);
        int rc = rc_all;
        // pass 1: where everything goes; the LZW descriptors, dealt
        std::vector<GifMixItem> items((size_t)n);
        std::vector<GifLzwDesc> lzw;
        lzw.reserve((size_t)npages);
        std::vector<size_t> pal_at((size_t)npages), data_at((size_t)npages), plane_at((size_t)npages);
        size_t off = front(n, npages, nslots), poff = upload;
        int q = 0;
        for (int k = 0; k < n; k++) {
            const GifPlan& pl = plans[g0 + (size_t)k];
            const impgpu_image* im = albums[pl.entry];
            GifMixItem& it = items[(size_t)k];
            it.pages_off = off;
            it.outs_off = off + (size_t)pl.npages * sizeof(GifPageDev);
            it.npages = pl.npages; it.cw = im->w; it.ch = im->h; it.ostep = im->step; it.destructive = pl.destructive; it.only = pl.only;
            off += head_bytes(pl.npages, pl.nout);
            for (int f = 0; f < pl.npages; f++, q++) {
                const impgpu_gif_desc& d = descs[pl.first_desc + (size_t)f];
                pal_at[(size_t)q] = off; off += 1024;
                data_at[(size_t)q] = off; off += up16(d.data_bytes);
                plane_at[(size_t)q] = poff; poff += up16((size_t)gif_pitch(d.width) * d.height);
                GifLzwDesc z{};
                z.data_off = (long long)data_at[(size_t)q]; z.plane_off = (long long)plane_at[(size_t)q];
                z.data_bytes = (uint32_t)d.data_bytes;
                z.w = d.width; z.h = d.height; z.pitch = gif_pitch(d.width); z.mcs = d.min_code_size; z.interlaced = d.interlaced;
                z.slot = pl.slot0 + f;
                z.nblk = 1;
                lzw.push_back(z);
            }
        }
        std::vector<GifLzwDesc> sorted;
        MixIndex ix{};
        int most = 0;
        mix_deal(lzw, [](GifLzwDesc& d) -> GifLzwDesc& { return d; }, [](GifLzwDesc& d) { return (long long)d.data_bytes + (long long)d.w * d.h; },
                 &sorted, &ix, &most);
        // pass 2: the blob, built in the pinned buffer and sent in pieces while the next files are copied in
        MixStaged up{};
        if (!rc) rc = stage_begin(upload, &up.host, &up.token);
        if (!rc && (rc = dev_alloc(total, &up.dev)) != IMP_OK) (void)stage_upload_part(up.token, 0, nullptr, 0, true);
        uint8_t* const whole = (uint8_t*)up.host;
        size_t sent = lzw_off;
        if (!rc) std::memcpy(whole + lzw_off, sorted.data(), sorted.size() * sizeof(GifLzwDesc));
        if (!rc && split) {                                         // per dealt descriptor: its segment block and its slots
            GifSplitPage* sp = (GifSplitPage*)(whole + pages_off);
            GifSegSlot* slot = (GifSegSlot*)(whole + slots_off);
            for (size_t i = 0; i < sorted.size(); i++) {
                const uint32_t scap = gif_seg_cap(sorted[i].data_bytes);
                sp[i] = GifSplitPage{(long long)poff, scap, 0};
                poff += ((size_t)scap + 1) * sizeof(GifSeg);
                for (uint32_t k = 0; k < scap; k++) *slot++ = GifSegSlot{(int)i, (int)k};
            }
        }
        q = 0;
        for (int k = 0; k < n && !rc; k++) {
            const GifPlan& pl = plans[g0 + (size_t)k];
            const impgpu_image* im = albums[pl.entry];
            const unsigned char* blob = blobs[pl.entry];
            GifPageDev* meta = (GifPageDev*)(whole + items[(size_t)k].pages_off);
            uint8_t** optr = (uint8_t**)(whole + items[(size_t)k].outs_off);
            for (int o = 0; o < pl.nout; o++) optr[o] = im->d + (size_t)o * im->fstride;
            size_t end = items[(size_t)k].pages_off + head_bytes(pl.npages, pl.nout);
            for (int f = 0; f < pl.npages; f++, q++) {
                const impgpu_gif_desc& d = descs[pl.first_desc + (size_t)f];
                gif_palette(blob, d, whole + pal_at[(size_t)q]);
                impgpu_gif_gather(blob, &d, whole + data_at[(size_t)q]);
                meta[f].pal_off = (long long)pal_at[(size_t)q];
                meta[f].idx_off = (long long)plane_at[(size_t)q];
                meta[f].w = d.width; meta[f].h = d.height; meta[f].pitch = gif_pitch(d.width); meta[f].left = d.left; meta[f].top = d.top;
                meta[f].dispose = d.dispose; meta[f].key = d.transparency_key; meta[f].pad = 0;
                end = data_at[(size_t)q] + up16(d.data_bytes);
            }
            if (end - sent >= (size_t(2) << 20) || k == n - 1) {
                rc = stage_upload_part(up.token, sent, (uint8_t*)up.dev + sent, end - sent, false);
                if (rc) { (void)stage_upload_part(up.token, 0, up.dev, 0, true); dev_free(up.dev); }
                sent = end;
            }
        }
        if (!rc) {
            rc = split ? launch_gif_lzw_split((uint8_t*)up.dev, lzw_off, pages_off, slots_off, ix, most, nslots, (uint32_t*)status_dev, s)
                       : launch_gif_lzw((uint8_t*)up.dev, lzw_off, ix, most, (uint32_t*)status_dev, s);
            if (rc) { (void)stage_upload_part(up.token, 0, up.dev, 0, true); dev_free(up.dev); }
        }
        if (!rc) rc = launch_gif_compose_mixed(items.data(), n, up, total, s);     // (sends its table, fences the buffer, frees up.dev)
        for (size_t k = g0; k < g1; k++) {
            if (rc == IMP_OK) { ran[k] = 1; continue; }
            image_delete(albums[plans[k].entry]);                   // this group's files fail together; the others stand
            albums[plans[k].entry] = nullptr;
            codes[plans[k].entry] = rc;
        }
        g0 = g1;
    }
    // the one wait: every page's status word
    if (!rc_all) {
        void *host = nullptr, *token = nullptr;
        int rc = stage_begin((size_t)slots * sizeof(uint32_t), &host, &token);
        if (!rc) {
            const hipError_t e = hipMemcpyAsync(host, status_dev, (size_t)slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) { set_error("hipMemcpyAsync(batch_decode_gif)", e); rc = IMP_ERROR_DEVICE; }
        }
        dev_free(status_dev);
        const int rcw = lane_wait();
        if (!rc) rc = rcw;
        for (size_t k = 0; k < plans.size(); k++) {
            if (!ran[k]) continue;
            const GifPlan& pl = plans[k];
            int code = rc;
            for (int f = 0; f < pl.npages && !code; f++)
                if (((const uint32_t*)host)[pl.slot0 + f] != GIF_LZW_OK) code = IMP_ERROR_DECODE_FAILED;
            if (!code) continue;
            image_delete(albums[pl.entry]);
            albums[pl.entry] = nullptr;
            codes[pl.entry] = code;
        }
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

int impgpu_batch_decode_gif(const unsigned char* const* blobs, const size_t* sizes, const int* destructive, const int* page,
                            int count, impgpu_image** albums, int* codes, int* launches) {
    return impgpu_batch_decode_gif_ex(blobs, sizes, destructive, page, count, 0, albums, codes, launches);
}

int impgpu_image_decode_gif_ex(const unsigned char* blob, size_t size, int destructive, int page, int flags, impgpu_image** album) {
    if (!blob || !album) return IMP_ERROR_INVALID_ARGS;
    *album = nullptr;
    int code = IMP_ERROR_INVALID_ARGS;
    const int rc = impgpu_batch_decode_gif_ex(&blob, &size, &destructive, &page, 1, flags, album, &code, nullptr);
    return rc ? rc : code;
}

int impgpu_image_decode_gif(const unsigned char* blob, size_t size, int destructive, int page, impgpu_image** album) {
    return impgpu_image_decode_gif_ex(blob, size, destructive, page, 0, album);
}

}  // extern "C"
