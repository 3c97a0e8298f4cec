// imp_gif_plan.h -- the device blob k_gif_compose / k_gif_compose_mix (and, in front of them, the k_gif_lzw kernels) read,
// said once for the three calls of imp_gif.cpp that build it: which pages a request walks, what a page must look like, the
// order of the regions and their roundings, where a call's entries are cut into groups, and when a piece of the pinned
// buffer leaves.  tests/c/gif_plan_check.cpp runs it under AddressSanitizer.  Host only; include it after imp_internal.h.
//
//   [0, front)           the group's FRONT: the compose launch's descriptor table (table_bytes; sent last, by the launch);
//                        the decode call puts GifLzwDesc[pages] behind it, and with IMPGPU_GIF_SPLIT GifSplitPage[pages]
//                        and GifSegSlot[slots]
//   [front, upload)      per entry: GifPageDev[npages] | output pointers[nout], rounded up to 16 together; then per page its
//                        palette (1024 bytes) and its payload rounded up to 16 -- the index plane (compose calls) or the
//                        compressed bytes (decode call)
//   [upload, total)      decode call only, never uploaded: every page's index plane, rounded up to 16; with the flag every
//                        page's segment block GifSeg[cap + 1] behind them, in the order of the dealt table
#pragma once
#include "imp_gif.h"

namespace imp {

inline size_t up16(size_t v) { return (v + 15) & ~size_t(15); }

// advancedio.c:111-116: a page request is always a destructive walk, and a page past the end is page 0; the walk stops at
// the requested page (:249-251), which is the one frame that comes out.  (count > 0 and page >= -1: the caller's refusals.)
struct GifRequest { int npages, nout, destructive, only; };
inline GifRequest gif_request(int count, int destructive, int page) {
    if (page != -1) {
        destructive = 1;
        if (page > count - 1) page = 0;
    }
    return GifRequest{page >= 0 ? page + 1 : count, page >= 0 ? 1 : count, destructive ? 1 : 0, page};
}

inline bool gif_page_ok(const impgpu_gif_page& p) { return p.indices && p.palette && p.width > 0 && p.height > 0 && p.pitch >= p.width; }
inline size_t gif_head_bytes(int npages, int nout) { return up16((size_t)npages * sizeof(GifPageDev) + (size_t)nout * sizeof(uint8_t*)); }
inline long long gif_canvas_blocks(int cw, int ch) { return ((long long)cw * ch + 255) / 256; }     // k_gif_compose_mix's workgroups

inline GifPageDev gif_page_dev(int w, int h, int pitch, int left, int top, int dispose, int key, size_t pal_off, size_t idx_off) {
    return GifPageDev{(long long)idx_off, (long long)pal_off, w, h, pitch, left, top, dispose, key, 0};
}

// A running offset into the blob.  One walks [front, upload): entry() per entry, page() per page of it.  The decode call
// runs a second one from `upload`: take() per plane, then per segment block.
struct GifCursor {
    size_t at;
    struct Page { size_t pal_at, payload_at; };
    size_t take(size_t bytes) { const size_t was = at; at += up16(bytes); return was; }
    GifMixItem entry(const GifRequest& rq, const impgpu_image* album = nullptr) {
        GifMixItem it{};
        it.pages_off = take(gif_head_bytes(rq.npages, rq.nout));
        it.outs_off = it.pages_off + (size_t)rq.npages * sizeof(GifPageDev);
        it.npages = rq.npages; it.destructive = rq.destructive; it.only = rq.only;
        if (album) { it.cw = album->w; it.ch = album->h; it.ostep = album->step; }
        return it;
    }
    Page page(size_t payload_bytes) {
        const size_t pal_at = take(1024);
        return Page{pal_at, take(payload_bytes)};
    }
};

struct GifFront { size_t lzw_off, pages_off, slots_off, bytes; };
// `lzw_pages`: the pages that have an LZW descriptor (the compose call has none: its front is the table alone)
inline GifFront gif_front(size_t table_bytes, int lzw_pages, long long slots, bool split) {
    GifFront F;
    F.lzw_off = table_bytes;
    F.pages_off = F.lzw_off + up16((size_t)lzw_pages * sizeof(GifLzwDesc));
    F.slots_off = F.pages_off + up16((size_t)lzw_pages * sizeof(GifSplitPage));
    F.bytes = split ? F.slots_off + up16((size_t)slots * sizeof(GifSegSlot)) : F.pages_off;
    return F;
}

// What an accepted entry weighs, and the entry itself as the calls keep it between judging and filling.
struct GifLoad {
    size_t bytes, planes;            // what it puts into [front, upload), and behind it
    long long blocks, slots;         // gif_canvas_blocks of its canvas; IMPGPU_GIF_SPLIT: gif_seg_cap of every page
    int lzw_pages;
};
struct GifEntry {
    int entry;                       // its index in the call's arrays
    GifRequest rq;
    GifLoad load;
    size_t first_desc;               // decode call: its pages in the call's descriptors ...
    int slot0;                       // ... and its first status word
};

// A group of entries that share one upload and one set of launches: as many as the staging cap (0: none), the compose
// launch's grid and, with the flag, the slot launches' grid take.  The first entry is always taken -- an entry past the cap
// by itself goes alone, as its lone call would.  `table_next` is the table of a group one entry larger.
struct GifGroup {
    int n = 0, lzw_pages = 0;
    size_t bytes = 0, planes = 0;
    long long blocks = 0, slots = 0;
    bool takes(const GifLoad& e, size_t table_next, size_t cap, bool split) const {
        if (n == 0) return true;
        return !((cap && gif_front(table_next, lzw_pages + e.lzw_pages, slots + e.slots, split).bytes + bytes + e.bytes > cap) ||
                 (blocks + e.blocks) * 8 > 0x7fffffffLL || (split && slots + e.slots > 0x7fffffffLL));
    }
    void add(const GifLoad& e) { n++; lzw_pages += e.lzw_pages; bytes += e.bytes; planes += e.planes; blocks += e.blocks; slots += e.slots; }
    size_t upload(const GifFront& F) const { return F.bytes + bytes; }
    size_t total(const GifFront& F, bool split) const { return upload(F) + planes + (split ? ((size_t)slots + (size_t)lzw_pages) * sizeof(GifSeg) : 0); }
};
// the group [g0, returned) of `entries`; `table_bytes` is gif_mix_table_bytes (a parameter: it lives beside the kernel)
inline size_t gif_cut(const std::vector<GifEntry>& entries, size_t g0, size_t cap, bool split, size_t (*table_bytes)(int), GifGroup* g) {
    size_t g1 = g0;
    *g = GifGroup{};
    while (g1 < entries.size() && g->takes(entries[g1].load, table_bytes(g->n + 1), cap, split)) g->add(entries[g1++].load);
    return g1;
}

// The group's pinned buffer and device block, and how far the buffer has been sent.  The blob is built in the buffer
// itself and leaves in pieces while the next entries are still being copied in; a piece ends where an entry ends.  What
// lies in front of `first` (the table) is launch_gif_compose_mixed's to send: the last piece, the one that fences the buffer.
constexpr size_t GIF_PIECE = size_t(2) << 20;
struct GifSender {
    void *host = nullptr, *token = nullptr, *dev = nullptr;
    size_t sent = 0;
    int begin(size_t upload, size_t total, size_t first) {
        sent = first;
        int rc = stage_begin(upload, &host, &token);
        if (!rc && (rc = dev_alloc(total, &dev)) != IMP_OK) (void)stage_upload_part(token, 0, nullptr, 0, true);
        return rc;
    }
    uint8_t* at(size_t off) const { return (uint8_t*)host + off; }
    // [sent, end) leaves once it is a piece, or when nothing follows; a failure abandons the group
    int send(size_t end, bool last) {
        if (end - sent < GIF_PIECE && !last) return IMP_OK;
        const int rc = stage_upload_part(token, sent, (uint8_t*)dev + sent, end - sent, false);
        sent = end;
        if (rc) abandon();
        return rc;
    }
    // after a failure behind begin(): the pieces already sent are fenced and the block goes back
    void abandon() {
        (void)stage_upload_part(token, 0, dev, 0, true);
        dev_free(dev);
    }
};

}  // namespace imp
