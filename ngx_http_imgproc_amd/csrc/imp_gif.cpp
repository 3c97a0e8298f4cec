// imp_gif.cpp -- GIF files in: the container walk (include/impgpu_gif.h) on the host, the LZW pages and LoadGIF's
// compositing loop on the device.  The compose calls take pages the host has decoded: impgpu_gif_compose(_album) lays one
// file's page table, output pointers, palettes and index planes out in one blob, impgpu_batch_gif_compose many files' in
// one staging blob behind the compose launch's descriptor table.  impgpu_batch_decode_gif lays every accepted file out
// the same way with the COMPRESSED pages -- the sub-block payloads -- where the index planes were, and reserves the planes
// behind it in the same device block: one upload, k_gif_lzw (imp_gif.hip) decodes every page into its plane,
// k_gif_compose_mix (imp_geom.hip) follows on the same stream, and the call waits once, for the pages' status words.  With
// IMPGPU_GIF_SPLIT three launches stand where k_gif_lzw is one: the pages are cut at their clear codes and a wavefront
// decodes every segment; the segment tables lie behind the planes.  Where everything lies is imp_gif_plan.h's to say.
#include "imp_internal.h"
#include "imp_gif.h"
#include "imp_gif_plan.h"
#include "../../include/impgpu_gif.h"

namespace imp {
// a file whose index planes pass this goes back to the host decoder (4096 pages of 4096 x 4096 would be 64 GB)
static constexpr size_t GIF_PLANES_MAX = size_t(1) << 30;

static void gif_palette(const unsigned char* blob, const impgpu_gif_desc& d, uint8_t* out) {      // 256 x B,G,R,0; missing entries 0
    std::memset(out, 0, 1024);
    for (int k = 0; k < d.palette_entries; k++) {
        const unsigned char* q = blob + d.palette_at + 3 * (size_t)k;
        out[4 * k] = q[2]; out[4 * k + 1] = q[1]; out[4 * k + 2] = q[0];
    }
}

static void album_outs(uint8_t** optr, const impgpu_image* album, int nout) {
    for (int o = 0; o < nout; o++) optr[o] = album->d + (size_t)o * album->fstride;
}

// ---------------------------------------------------------------- pages the host has decoded (the compose calls)
// what an entry of these pages puts into the blob; 0: a page breaks the page rule (pages behind a requested one are not judged)
static size_t compose_entry_bytes(const impgpu_gif_page* pages, const GifRequest& rq) {
    GifCursor c{0};
    c.entry(rq);
    for (int f = 0; f < rq.npages; f++) {
        if (!gif_page_ok(pages[f])) return 0;
        c.page((size_t)pages[f].pitch * pages[f].height);
    }
    return c.at;
}

// the cursor's next page: palette and index plane into `blob`, and its record
static GifPageDev compose_page(uint8_t* blob, GifCursor& c, const impgpu_gif_page& p) {
    const GifCursor::Page at = c.page((size_t)p.pitch * p.height);
    std::memcpy(blob + at.pal_at, p.palette, 1024);
    std::memcpy(blob + at.payload_at, p.indices, (size_t)p.pitch * p.height);
    return gif_page_dev(p.width, p.height, p.pitch, p.left, p.top, p.dispose, p.transparency_key, at.pal_at, at.payload_at);
}

static int gif_compose(const impgpu_gif_page* pages, int count, int destructive, int page, bool as_album, impgpu_image** frames) {
    if (!pages || !frames || count <= 0 || page < -1) return IMP_ERROR_INVALID_ARGS;   // page < -1: the reference reads Frames[page] below the array
    const GifRequest rq = gif_request(count, destructive, page);
    if (int rc = need_env()) return rc;
    const int cw = pages[0].width, ch = pages[0].height;           // advancedio.c:133-136: canvas = first page
    if (cw <= 0 || ch <= 0) return IMP_ERROR_INVALID_ARGS;
    const size_t bytes = compose_entry_bytes(pages, rq);
    if (!bytes) return IMP_ERROR_INVALID_ARGS;
    std::vector<impgpu_image*> imgs((size_t)rq.nout, nullptr);
    auto drop = [&]() { for (impgpu_image* im : imgs) if (im) image_delete(im); };
    if (as_album) {                                                // every output frame in one block behind one handle
        imgs.resize(1);
        if (int rc = image_new_album(cw, ch, 4, rq.nout, &imgs[0])) return rc;
    } else {
        for (int i = 0; i < rq.nout; i++)
            if (int rc = image_new(cw, ch, 4, &imgs[i])) { drop(); return rc; }
    }
    std::vector<uint8_t> blob(bytes, 0);                           // one entry at base 0
    GifCursor c{0};
    const GifMixItem it = c.entry(rq);
    GifPageDev* meta = (GifPageDev*)(blob.data() + it.pages_off);
    uint8_t** optr = (uint8_t**)(blob.data() + it.outs_off);
    if (as_album) album_outs(optr, imgs[0], rq.nout);
    else for (int i = 0; i < rq.nout; i++) optr[i] = imgs[i]->d;
    for (int f = 0; f < rq.npages; f++) meta[f] = compose_page(blob.data(), c, pages[f]);
    void* dev = nullptr;
    hipStream_t s = env_stream();
    if (int rc = upload_small(blob.data(), blob.size(), &dev, s)) { drop(); return rc; }
    const uint8_t* d = (const uint8_t*)dev;
    int rc = launch_gif_compose(d, (const GifPageDev*)(d + it.pages_off), (uint8_t* const*)(d + it.outs_off), rq.npages, cw, ch, imgs[0]->step,
                                rq.destructive, rq.only, s);
    dev_free(dev);                                                 // stream-ordered: after the kernel
    if (rc) { drop(); return rc; }
    for (size_t i = 0; i < imgs.size(); i++) frames[i] = imgs[i];
    return IMP_OK;
}

// One group of impgpu_batch_gif_compose: built in the pinned staging buffer itself, leaving in pieces while the next
// entries are still being copied in (one pass over the pages, the copy to the device beside it: built in a vector and
// uploaded whole, 16 files of 40 MB took four times the lone calls' loop).
static int compose_group(const impgpu_gif_set* sets, impgpu_image* const* albums, const GifEntry* plans, const GifGroup& g, hipStream_t s) {
    const GifFront F = gif_front(gif_mix_table_bytes(g.n), 0, 0, false);
    const size_t total = g.upload(F);
    std::vector<GifMixItem> items((size_t)g.n);
    GifSender up;
    int rc = up.begin(total, total, F.bytes);
    GifCursor c{F.bytes};
    for (int k = 0; k < g.n && !rc; k++) {
        const GifEntry& pl = plans[k];
        const GifMixItem& it = items[(size_t)k] = c.entry(pl.rq, albums[pl.entry]);
        album_outs((uint8_t**)up.at(it.outs_off), albums[pl.entry], pl.rq.nout);
        GifPageDev* meta = (GifPageDev*)up.at(it.pages_off);
        for (int f = 0; f < pl.rq.npages; f++) meta[f] = compose_page(up.at(0), c, sets[pl.entry].pages[f]);
        rc = up.send(c.at, k == g.n - 1);
    }
    if (!rc) rc = launch_gif_compose_mixed(items.data(), g.n, MixStaged{up.host, up.token, up.dev}, total, s);     // (sends the table, fences the buffer, frees up.dev)
    return rc;
}

// ---------------------------------------------------------------- files (impgpu_batch_decode_gif_ex, in phases)
struct GifCall {                     // what the phases share
    const unsigned char* const* blobs;
    impgpu_image** albums;
    int* codes;
    bool split;
    std::vector<GifEntry> files;     // the accepted ones, their pages' descriptors, and how many status words: one per page
    std::vector<impgpu_gif_desc> descs;
    int slots;
};
struct GifPlaced {                   // a group, cut and placed
    GifGroup g;
    GifFront F;
    size_t upload, total;
    std::vector<GifMixItem> items;
    std::vector<GifLzwDesc> sorted;  // the LZW descriptors, dealt (mix_deal)
    MixIndex ix;
    int most;
};
struct GifSpot { size_t pal_at, data_at, plane_at; };
// where the cursors' next page goes: `up` walks the upload, `planes` the planes behind it (both passes place through this)
static GifSpot place_page(GifCursor& up, GifCursor& planes, const impgpu_gif_desc& d) {
    const GifCursor::Page p = up.page(d.data_bytes);
    return GifSpot{p.pal_at, p.payload_at, planes.take((size_t)gif_pitch(d.width) * d.height)};
}

// every file judged as its lone call judges it: the container walk, then the page rules of impgpu_gif_compose_album
static void judge_files(GifCall& C, const size_t* sizes, const int* destructive, const int* page, int count) {
    std::vector<impgpu_gif_desc> walked((size_t)IMPB_MAX_GIF_PAGES);
    for (int i = 0; i < count; i++) {
        C.codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!C.blobs[i] || page[i] < -1) continue;
        int n = 0, cw = 0, ch = 0;
        if ((C.codes[i] = impgpu_gif_walk(C.blobs[i], sizes[i], walked.data(), (int)walked.size(), &n, &cw, &ch)) != IMP_OK) continue;
        GifEntry e{i, gif_request(n, destructive[i], page[i]), GifLoad{}, C.descs.size(), C.slots};
        GifCursor up{0}, planes{0};
        up.entry(e.rq);
        bool huge = false;
        for (int f = 0; f < e.rq.npages; f++) {                    // pages behind the requested one are neither decoded nor judged
            huge = huge || walked[f].data_bytes >= GIF_DATA_MAX;
            (void)place_page(up, planes, walked[f]);
            if (!huge) e.load.slots += gif_seg_cap((uint32_t)walked[f].data_bytes);
        }
        e.load.bytes = up.at; e.load.planes = planes.at; e.load.lzw_pages = e.rq.npages; e.load.blocks = gif_canvas_blocks(cw, ch);
        if (huge || e.load.planes > GIF_PLANES_MAX) { C.codes[i] = IMP_ERROR_UNSUPPORTED; continue; }
        C.codes[i] = image_new_album(cw, ch, 4, e.rq.nout, &C.albums[i]);
        if (C.codes[i] != IMP_OK) continue;
        C.descs.insert(C.descs.end(), walked.begin(), walked.begin() + e.rq.npages);
        C.slots += e.rq.npages;
        C.files.push_back(e);
    }
}

// pass 1: where everything of the group that starts at file g0 goes; the LZW descriptors, dealt
static void place_group(const GifCall& C, size_t g0, GifPlaced& P) {
    P.F = gif_front(gif_mix_table_bytes(P.g.n), P.g.lzw_pages, P.g.slots, C.split);
    P.upload = P.g.upload(P.F);
    P.total = P.g.total(P.F, C.split);
    P.items.resize((size_t)P.g.n);
    std::vector<GifLzwDesc> lzw;
    lzw.reserve((size_t)P.g.lzw_pages);
    GifCursor up{P.F.bytes}, planes{P.upload};
    for (int k = 0; k < P.g.n; k++) {
        const GifEntry& fl = C.files[g0 + (size_t)k];
        P.items[(size_t)k] = up.entry(fl.rq, C.albums[fl.entry]);
        for (int f = 0; f < fl.rq.npages; f++) {
            const impgpu_gif_desc& d = C.descs[fl.first_desc + (size_t)f];
            const GifSpot at = place_page(up, planes, d);
            GifLzwDesc z{};
            z.data_off = (long long)at.data_at; z.plane_off = (long long)at.plane_at;
            z.data_bytes = (uint32_t)d.data_bytes;
            z.w = d.width; z.h = d.height; z.pitch = gif_pitch(d.width); z.mcs = d.min_code_size; z.interlaced = d.interlaced;
            z.slot = fl.slot0 + f;
            z.nblk = 1;
            lzw.push_back(z);
        }
    }
    mix_deal(lzw, [](GifLzwDesc& d) -> GifLzwDesc& { return d; }, [](GifLzwDesc& d) { return (long long)d.data_bytes + (long long)d.w * d.h; },
             &P.sorted, &P.ix, &P.most);
}

// pass 2: the blob, built in the pinned buffer and sent in pieces while the next files are copied in
static int fill_and_send(const GifCall& C, size_t g0, const GifPlaced& P, GifSender& out) {
    std::memcpy(out.at(P.F.lzw_off), P.sorted.data(), P.sorted.size() * sizeof(GifLzwDesc));
    if (C.split) {                                                 // per dealt descriptor: its segment block and its slots
        GifSplitPage* sp = (GifSplitPage*)out.at(P.F.pages_off);
        GifSegSlot* slot = (GifSegSlot*)out.at(P.F.slots_off);
        GifCursor segs{P.upload + P.g.planes};
        for (size_t i = 0; i < P.sorted.size(); i++) {
            const uint32_t scap = gif_seg_cap(P.sorted[i].data_bytes);
            sp[i] = GifSplitPage{(long long)segs.take(((size_t)scap + 1) * sizeof(GifSeg)), scap, 0};
            for (uint32_t k = 0; k < scap; k++) *slot++ = GifSegSlot{(int)i, (int)k};
        }
    }
    GifCursor up{P.F.bytes}, planes{P.upload};
    int rc = IMP_OK;
    for (int k = 0; k < P.g.n && !rc; k++) {
        const GifEntry& fl = C.files[g0 + (size_t)k];
        const unsigned char* blob = C.blobs[fl.entry];
        const GifMixItem it = up.entry(fl.rq);
        album_outs((uint8_t**)out.at(it.outs_off), C.albums[fl.entry], fl.rq.nout);
        GifPageDev* meta = (GifPageDev*)out.at(it.pages_off);
        for (int f = 0; f < fl.rq.npages; f++) {
            const impgpu_gif_desc& d = C.descs[fl.first_desc + (size_t)f];
            const GifSpot at = place_page(up, planes, d);
            gif_palette(blob, d, out.at(at.pal_at));
            impgpu_gif_gather(blob, &d, out.at(at.data_at));
            meta[f] = gif_page_dev(d.width, d.height, gif_pitch(d.width), d.left, d.top, d.dispose, d.transparency_key, at.pal_at, at.plane_at);
        }
        rc = out.send(up.at, k == P.g.n - 1);
    }
    return rc;
}

static int launch_group(const GifCall& C, const GifPlaced& P, GifSender& out, uint32_t* status, hipStream_t s) {
    const int rc = C.split ? launch_gif_lzw_split((uint8_t*)out.dev, P.F.lzw_off, P.F.pages_off, P.F.slots_off, P.ix, P.most, P.g.slots, status, s)
                           : launch_gif_lzw((uint8_t*)out.dev, P.F.lzw_off, P.ix, P.most, status, s);
    if (rc) { out.abandon(); return rc; }
    return launch_gif_compose_mixed(P.items.data(), P.g.n, MixStaged{out.host, out.token, out.dev}, P.total, s);     // (sends its table, fences the buffer, frees out.dev)
}

// the one wait: every page's status word
static void read_verdicts(const GifCall& C, const std::vector<char>& ran, void* status_dev, hipStream_t s) {
    void *host = nullptr, *token = nullptr;
    int rc = stage_begin((size_t)C.slots * sizeof(uint32_t), &host, &token);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(host, status_dev, (size_t)C.slots * sizeof(uint32_t), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { set_error("hipMemcpyAsync(batch_decode_gif)", e); rc = IMP_ERROR_DEVICE; }
    }
    dev_free(status_dev);
    const int rcw = lane_wait();
    if (!rc) rc = rcw;
    for (size_t k = 0; k < C.files.size(); k++) {
        if (!ran[k]) continue;
        const GifEntry& fl = C.files[k];
        int code = rc;
        for (int f = 0; f < fl.rq.npages && !code; f++)
            if (((const uint32_t*)host)[fl.slot0 + f] != GIF_LZW_OK) code = IMP_ERROR_DECODE_FAILED;
        if (!code) continue;
        image_delete(C.albums[fl.entry]);
        C.albums[fl.entry] = nullptr;
        C.codes[fl.entry] = code;
    }
}

}  // namespace imp

using namespace imp;

extern "C" {

int impgpu_gif_compose(const impgpu_gif_page* pages, int count, int destructive, int page, impgpu_image** frames) {
    return gif_compose(pages, count, destructive, page, false, frames);
}

int impgpu_gif_compose_album(const impgpu_gif_page* pages, int count, int destructive, int page, impgpu_image** album) {
    return gif_compose(pages, count, destructive, page, true, album);
}

// Many files, one compose launch.  Every entry is judged as gif_compose judges it alone; the accepted ones' page tables,
// output pointers, palettes and index planes are laid out in ONE blob behind the descriptor table (launch_gif_compose_mixed),
// which is one upload and one launch.  A blob that would pass the staging cap is cut at an entry boundary: one upload and
// one launch per group, in entry order.
int impgpu_batch_gif_compose(const impgpu_gif_set* sets, int count, impgpu_image** albums, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!sets || !albums || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) albums[i] = nullptr;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    std::vector<GifEntry> plans;
    for (int i = 0; i < count; i++) {
        const impgpu_gif_set& st = sets[i];
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!st.pages || st.count <= 0 || st.page < -1) continue;
        if (st.pages[0].width <= 0 || st.pages[0].height <= 0) continue;
        GifEntry e{i, gif_request(st.count, st.destructive, st.page), GifLoad{}, 0, 0};
        e.load.bytes = compose_entry_bytes(st.pages, e.rq);
        e.load.blocks = gif_canvas_blocks(st.pages[0].width, st.pages[0].height);
        if (!e.load.bytes) continue;
        codes[i] = image_new_album(st.pages[0].width, st.pages[0].height, 4, e.rq.nout, &albums[i]);
        if (codes[i] == IMP_OK) plans.push_back(e);
    }
    const size_t cap = stage_cap();
    hipStream_t s = env_stream();
    int issued = 0;
    for (size_t g0 = 0; g0 < plans.size();) {
        GifGroup g;
        const size_t g1 = gif_cut(plans, g0, cap, false, gif_mix_table_bytes, &g);
        const int rc = compose_group(sets, albums, plans.data() + g0, g, s);
        if (rc == IMP_OK) issued++;
        else
            for (size_t k = g0; k < g1; k++) {                      // this group's entries fail together; the others stand
                image_delete(albums[plans[k].entry]);
                albums[plans[k].entry] = nullptr;
                codes[plans[k].entry] = rc;
            }
        g0 = g1;
    }
    if (launches) *launches = issued;
    return IMP_OK;
}

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
    if (count < 0 || count > 256 || (count > 0 && (!blobs || !sizes || !destructive || !page || !albums || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) albums[i] = nullptr;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    const unsigned long long launched = t_launches;
    GifCall C{blobs, albums, codes, (flags & IMPGPU_GIF_SPLIT) != 0, {}, {}, 0};
    judge_files(C, sizes, destructive, page, count);
    if (C.files.empty()) return IMP_OK;
    hipStream_t s = env_stream();
    void* status_dev = nullptr;
    const int rc_all = dev_alloc((size_t)C.slots * sizeof(uint32_t), &status_dev);
    const size_t cap = stage_cap();
    std::vector<char> ran(C.files.size(), 0);
    for (size_t g0 = 0; g0 < C.files.size();) {
        // the group [g0, g1): as many files as the staging cap and the grids take; placed, filled and sent, launched
        GifPlaced P;
        const size_t g1 = gif_cut(C.files, g0, cap, C.split, gif_mix_table_bytes, &P.g);
        place_group(C, g0, P);
        GifSender out;
        int rc = rc_all;
        if (!rc) rc = out.begin(P.upload, P.total, P.F.lzw_off);
        if (!rc) rc = fill_and_send(C, g0, P, out);
        if (!rc) rc = launch_group(C, P, out, (uint32_t*)status_dev, s);
        for (size_t k = g0; k < g1; k++) {
            if (rc == IMP_OK) { ran[k] = 1; continue; }
            image_delete(albums[C.files[k].entry]);                 // this group's files fail together; the others stand
            albums[C.files[k].entry] = nullptr;
            codes[C.files[k].entry] = rc;
        }
        g0 = g1;
    }
    if (!rc_all) read_verdicts(C, ran, status_dev, s);
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
