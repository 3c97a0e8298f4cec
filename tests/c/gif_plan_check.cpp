// gif_plan_check.cpp -- the GIF compose / decode calls' device blob (csrc/imp_gif_plan.h) under AddressSanitizer + UBSan
// (tests/test_gif_plan_host.py builds and runs it; CPU only).  For a sweep of entries per group, pages per entry, page
// sizes and pitches, page requests, table sizes and -- on the decode route -- compressed sizes with and without
// IMPGPU_GIF_SPLIT, a group is laid out and filled through the header the way imp_gif.cpp's callers do it, into heap blocks
// of exactly `upload` and `total` bytes, and checked: every offset and both sizes are what commit 0a35b10 computed by hand
// (imp_api.cpp:671-838, imp_gif.cpp:64-204, restated here as plain arithmetic); every region lies inside its zone, apart
// from the others and aligned; every region is written whole; the pieces leave where the old loops sent them.  The group
// cut is swept over caps of 0, 1 MB and the default against the old loops.  stage_begin, dev_alloc, stage_upload_part and
// dev_free are stubs over malloc: a piece is COPIED from the one block into the other, so a piece past either is
// AddressSanitizer's to report.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ngx_http_imgproc_amd/csrc/imp_internal.h"
#include "../../ngx_http_imgproc_amd/csrc/imp_gif_plan.h"

using namespace imp;

namespace {
struct Part { size_t off, bytes; bool last; const void* dev; };
struct Stub {
    uint8_t *host = nullptr, *dev = nullptr;
    size_t host_bytes = 0, dev_bytes = 0;
    std::vector<Part> parts;
    int frees = 0;
    bool fail_alloc = false;
} S;
void stub_reset() {
    std::free(S.host);
    S = Stub{};
}
}  // namespace

namespace imp {
int stage_begin(size_t bytes, void** host, void** token) {
    S.host = (uint8_t*)std::malloc(bytes);
    S.host_bytes = bytes;
    *host = S.host; *token = &S;
    return S.host ? IMP_OK : IMP_ERROR_MALLOC_FAILED;
}
int dev_alloc(size_t bytes, void** out) {
    if (S.fail_alloc) return IMP_ERROR_MALLOC_FAILED;
    S.dev = (uint8_t*)std::malloc(bytes);
    S.dev_bytes = bytes;
    *out = S.dev;
    return S.dev ? IMP_OK : IMP_ERROR_MALLOC_FAILED;
}
void dev_free(void* p) {
    if (p == S.dev) S.frees++;
    std::free(p);
    S.dev = nullptr;
}
int stage_upload_part(void* token, size_t offset, void* dev, size_t bytes, bool last) {
    if (token != &S) return IMP_ERROR_INVALID_ARGS;
    S.parts.push_back(Part{offset, bytes, last, dev});
    if (bytes) std::memcpy(dev, S.host + offset, bytes);
    return IMP_OK;
}
}  // namespace imp

namespace {

size_t r16(size_t v) { return (v + 15) & ~size_t(15); }                // the old code's rounding, spelt as it was
size_t table_of(size_t per_entry, int n) { return per_entry * (size_t)n; }
size_t g_table_unit = 16;                                              // the stand-in for gif_mix_table_bytes: 16 or 4096 bytes an entry
size_t table_bytes(int n) { return table_of(g_table_unit, n); }

struct Case { int n, pages, w, h, pitch, request; size_t unit; bool decode; size_t data_bytes; bool split; };
int fail(const char* what, const Case& c, long long a = 0, long long b = 0) {
    std::printf("FAIL %s (%lld vs %lld): entries %d pages %d page %dx%d pitch %d request %d table %zu decode %d data %zu split %d\n", what, a, b, c.n,
                c.pages, c.w, c.h, c.pitch, c.request, c.unit, (int)c.decode, c.data_bytes, (int)c.split);
    return 1;
}

// zone 0: [front, upload), in the pinned block; zone 1: [upload, total), device only; zone 2: the front's own tables
struct Region { const char* name; size_t off, bytes, align; int zone; };

// commit 0a35b10's page request, as all three callers spelt it
void old_request(int count, int destructive, int page, int* npages, int* nout, int* destr, int* only) {
    if (page != -1) {
        destructive = 1;
        if (page > count - 1) page = 0;
    }
    *npages = page >= 0 ? page + 1 : count;
    *nout = page >= 0 ? 1 : count;
    *destr = destructive ? 1 : 0;
    *only = page;
}

int check(const Case& c) {
    g_table_unit = c.unit;
    int bad = 0;
    impgpu_image album;
    album.w = c.w; album.h = c.h; album.step = c.w * 4;
    const GifRequest rq = gif_request(c.pages, 0, c.request);
    int npages, nout, destr, only;
    old_request(c.pages, 0, c.request, &npages, &nout, &destr, &only);
    if (rq.npages != npages || rq.nout != nout || rq.destructive != destr || rq.only != only) return fail("request", c);
    const size_t payload = c.decode ? c.data_bytes : (size_t)c.pitch * c.h;
    const size_t plane = c.decode ? (size_t)gif_pitch(c.w) * c.h : 0;

    // ---- through the header, as the callers do: an entry's weight from a cursor at 0, the group, its front and sizes
    GifEntry e{0, rq, GifLoad{}, 0, 0};
    GifCursor size{0}, psize{0};
    size.entry(rq);
    for (int f = 0; f < npages; f++) {
        size.page(payload);
        psize.take(plane);
        if (c.decode) e.load.slots += gif_seg_cap((uint32_t)c.data_bytes);
    }
    e.load.bytes = size.at; e.load.planes = psize.at; e.load.lzw_pages = c.decode ? npages : 0; e.load.blocks = gif_canvas_blocks(c.w, c.h);
    std::vector<GifEntry> entries((size_t)c.n, e);
    GifGroup g;
    if (gif_cut(entries, 0, 0, c.split, table_bytes, &g) != (size_t)c.n || g.n != c.n) return fail("uncapped cut", c);
    const GifFront F = gif_front(table_bytes(c.n), g.lzw_pages, g.slots, c.split);
    const size_t upload = g.upload(F), total = g.total(F, c.split);

    // ---- the same as commit 0a35b10 spelt it
    const size_t head = ((size_t)npages * sizeof(GifPageDev) + (size_t)nout * sizeof(uint8_t*) + 15) & ~size_t(15);
    const size_t up_bytes = head + (size_t)npages * (1024 + r16(payload));
    const int all_pages = c.decode ? c.n * npages : 0;
    const long long nslots = c.decode ? (long long)all_pages * gif_seg_cap((uint32_t)c.data_bytes) : 0;
    const size_t lzw_off = table_bytes(c.n), split_off = lzw_off + r16((size_t)all_pages * sizeof(GifLzwDesc));
    const size_t slots_off = split_off + r16((size_t)all_pages * sizeof(GifSplitPage));
    const size_t front = split_off + (c.split ? r16((size_t)all_pages * sizeof(GifSplitPage)) + r16((size_t)nslots * sizeof(GifSegSlot)) : 0);
    const size_t old_upload = front + (size_t)c.n * up_bytes;
    const size_t old_total = old_upload + (size_t)all_pages * r16(plane) + (c.split ? ((size_t)nslots + (size_t)all_pages) * sizeof(GifSeg) : 0);
    if (e.load.bytes != up_bytes) bad |= fail("entry bytes", c, (long long)e.load.bytes, (long long)up_bytes);
    if (F.lzw_off != lzw_off || F.pages_off != split_off || F.slots_off != slots_off || F.bytes != front) bad |= fail("front", c, (long long)F.bytes, (long long)front);
    if (upload != old_upload || total != old_total) bad |= fail("sizes", c, (long long)total, (long long)old_total);
    if (bad) return bad;

    // ---- fill and send: the blocks are exactly `upload` and `total` bytes
    stub_reset();
    GifSender out;
    if (out.begin(upload, total, F.lzw_off) != IMP_OK || S.host_bytes != upload || S.dev_bytes != total) return fail("begin", c);
    std::vector<Region> R;
    std::vector<Part> old_parts;
    auto put = [&](const char* name, size_t off, size_t bytes, size_t align, int zone) {
        R.push_back(Region{name, off, bytes, align, zone});
        std::memset(zone == 1 ? S.dev + off : out.at(off), 0xA5, bytes);          // written whole: a byte outside is ASan's
    };
    if (c.decode) {
        put("lzw table", F.lzw_off, (size_t)all_pages * sizeof(GifLzwDesc), 8, 2);
        if (c.split) {
            put("split pages", F.pages_off, (size_t)all_pages * sizeof(GifSplitPage), 8, 2);
            put("slots", F.slots_off, (size_t)nslots * sizeof(GifSegSlot), 8, 2);
            GifCursor segs{upload + g.planes};
            size_t old_seg = old_upload + (size_t)all_pages * r16(plane);
            for (int q = 0; q < all_pages; q++) {
                const size_t block = ((size_t)gif_seg_cap((uint32_t)c.data_bytes) + 1) * sizeof(GifSeg);
                const size_t at = segs.take(block);
                if (at != old_seg) bad |= fail("segment block", c, (long long)at, (long long)old_seg);
                old_seg += block;
                put("segment block", at, block, 8, 1);
            }
        }
    }
    GifCursor up{F.bytes}, planes{upload};
    size_t off = front, poff = old_upload, sent = lzw_off;              // the old loops' running offsets
    for (int k = 0; k < c.n; k++) {
        const GifMixItem it = up.entry(rq, &album);
        if (it.pages_off != off || it.outs_off != off + (size_t)npages * sizeof(GifPageDev)) bad |= fail("item offsets", c, (long long)it.pages_off, (long long)off);
        if (it.npages != npages || it.cw != c.w || it.ch != c.h || it.ostep != album.step || it.destructive != destr || it.only != only) bad |= fail("item", c);
        off += head;
        put("page table", it.pages_off, (size_t)npages * sizeof(GifPageDev), 8, 0);
        put("output pointers", it.outs_off, (size_t)nout * sizeof(uint8_t*), 8, 0);
        GifPageDev* meta = (GifPageDev*)out.at(it.pages_off);
        for (int f = 0; f < npages; f++) {
            const GifCursor::Page at = up.page(payload);
            const size_t plane_at = c.decode ? planes.take(plane) : 0;
            const size_t old_pal = off, old_payload = off + 1024, old_plane = poff;
            off += 1024 + r16(payload);
            poff += r16(plane);
            if (at.pal_at != old_pal || at.payload_at != old_payload || (c.decode && plane_at != old_plane)) bad |= fail("page offsets", c, (long long)at.pal_at, (long long)old_pal);
            put("palette", at.pal_at, 1024, 16, 0);
            put("payload", at.payload_at, payload, 16, 0);
            if (c.decode) put("plane", plane_at, plane, 16, 1);
            meta[f] = gif_page_dev(c.w, c.h, c.pitch, 1, 2, 3, 4, at.pal_at, c.decode ? plane_at : at.payload_at);
            const GifPageDev& m = meta[f];
            if (m.pal_off != (long long)old_pal || m.idx_off != (long long)(c.decode ? old_plane : old_payload) || m.w != c.w || m.h != c.h || m.pitch != c.pitch ||
                m.left != 1 || m.top != 2 || m.dispose != 3 || m.key != 4 || m.pad != 0)
                bad |= fail("page record", c);
        }
        if (up.at != off) bad |= fail("entry end", c, (long long)up.at, (long long)off);
        if (off - sent >= (size_t(2) << 20) || k == c.n - 1) {           // the old piece rule
            old_parts.push_back(Part{sent, off - sent, false, S.dev + sent});
            sent = off;
        }
        if (out.send(up.at, k == c.n - 1) != IMP_OK) bad |= fail("send", c);
    }
    if (up.at != upload || (c.decode && planes.at != upload + g.planes)) bad |= fail("cursor ends", c, (long long)up.at, (long long)upload);
    if (S.parts.size() != old_parts.size()) bad |= fail("piece count", c, (long long)S.parts.size(), (long long)old_parts.size());
    for (size_t i = 0; i < S.parts.size() && i < old_parts.size(); i++)
        if (S.parts[i].off != old_parts[i].off || S.parts[i].bytes != old_parts[i].bytes || S.parts[i].last || S.parts[i].dev != old_parts[i].dev)
            bad |= fail("piece", c, (long long)S.parts[i].off, (long long)old_parts[i].off);
    if (out.sent != upload) bad |= fail("sent mark", c, (long long)out.sent, (long long)upload);
    // ---- the failure dance: one fencing piece of no bytes onto the block, and the block goes back
    const size_t before = S.parts.size();
    const void* block = S.dev;
    out.abandon();
    if (S.parts.size() != before + 1 || !S.parts.back().last || S.parts.back().bytes || S.parts.back().off || S.parts.back().dev != block || S.frees != 1)
        bad |= fail("abandon", c);

    // ---- zones, alignment, overlap
    for (const Region& r : R) {
        const size_t lo = r.zone == 0 ? F.bytes : r.zone == 1 ? upload : F.lzw_off, hi = r.zone == 0 ? upload : r.zone == 1 ? total : F.bytes;
        if (r.off < lo || r.off > hi || r.bytes > hi - r.off) bad |= fail("outside its zone", c, (long long)r.off, (long long)hi);
        if (r.off % r.align) bad |= fail("alignment", c, (long long)r.off, (long long)r.align);
    }
    std::sort(R.begin(), R.end(), [](const Region& a, const Region& b) { return a.off != b.off ? a.off < b.off : a.bytes < b.bytes; });    // (an empty payload shares its offset)
    for (size_t i = 0; i + 1 < R.size(); i++)
        if (R[i].off + R[i].bytes > R[i + 1].off) bad |= fail("overlap", c, (long long)R[i].off, (long long)R[i + 1].off);

    // ---- the lone compose call: the same entry on a cursor that starts at 0 (imp_api.cpp:683-692)
    if (!c.decode && c.n == 1) {
        GifCursor lone{0};
        const GifMixItem it = lone.entry(rq);
        size_t o = (size_t)npages * sizeof(GifPageDev) + (size_t)nout * sizeof(uint8_t*);
        o = (o + 15) & ~size_t(15);
        if (it.pages_off != 0 || it.outs_off != (size_t)npages * sizeof(GifPageDev)) bad |= fail("lone item", c);
        for (int f = 0; f < npages; f++) {
            const GifCursor::Page at = lone.page(payload);
            if (at.pal_at != o || at.payload_at != o + 1024) bad |= fail("lone page", c, (long long)at.pal_at, (long long)o);
            o += 1024 + (((size_t)c.pitch * c.h + 15) & ~size_t(15));
        }
        if (lone.at != o || lone.at != e.load.bytes) bad |= fail("lone size", c, (long long)lone.at, (long long)o);
    }

    // ---- the cut: this case's entries, one past the cap by itself among them, against the old loops
    for (size_t cap : {size_t(0), size_t(1) << 20, size_t(512) << 20}) {
        std::vector<GifEntry> list((size_t)c.n + 3, e);
        GifEntry& big = list[(size_t)c.n / 2 + 1];
        big.load.bytes += (cap ? cap : size_t(1) << 20) + 16;           // (the cut reads the weights only)
        for (size_t g0 = 0; g0 < list.size();) {
            size_t g1 = g0, bytes = 0;
            long long blocks = 0, nsl = 0;
            int np = 0;
            auto old_front = [&](int n, int pages, long long sl) {
                return table_bytes(n) + (c.decode ? r16((size_t)pages * sizeof(GifLzwDesc)) : 0) +
                       (c.split ? r16((size_t)pages * sizeof(GifSplitPage)) + r16((size_t)sl * sizeof(GifSegSlot)) : 0);
            };
            while (g1 < list.size()) {
                const GifLoad& l = list[g1].load;
                if (g1 > g0 && ((cap && old_front((int)(g1 - g0 + 1), np + l.lzw_pages, nsl + l.slots) + bytes + l.bytes > cap) ||
                                (blocks + l.blocks) * 8 > 0x7fffffffLL || (c.split && nsl + l.slots > 0x7fffffffLL))) break;
                bytes += l.bytes; np += l.lzw_pages; blocks += l.blocks; nsl += l.slots;
                g1++;
            }
            GifGroup cut;
            const size_t got = gif_cut(list, g0, cap, c.split, table_bytes, &cut);
            if (got != g1 || cut.n != (int)(g1 - g0) || cut.bytes != bytes || cut.lzw_pages != np || cut.blocks != blocks || cut.slots != nsl)
                bad |= fail("cut", c, (long long)got, (long long)g1);
            g0 = g1;
        }
    }
    return bad;
}

// the grid terms of the cut, which no real page of the sweep reaches, and a block that cannot be had
int check_limits() {
    int bad = 0;
    g_table_unit = 16;
    GifEntry e{0, gif_request(1, 0, -1), GifLoad{}, 0, 0};
    e.load.bytes = 1040; e.load.lzw_pages = 1;
    std::vector<GifEntry> list(5, e);
    GifGroup g;
    for (GifEntry& x : list) x.load.blocks = (0x7fffffffLL / 8) / 2;                    // two fit the compose grid, three do not
    if (gif_cut(list, 0, 0, false, table_bytes, &g) != 2 || gif_cut(list, 2, 0, false, table_bytes, &g) != 4) bad = 1;
    for (GifEntry& x : list) { x.load.blocks = 1; x.load.slots = 0x7fffffffLL / 3; }    // three fit the slot grid -- which counts under the flag only
    if (gif_cut(list, 0, 0, true, table_bytes, &g) != 3 || gif_cut(list, 0, 0, false, table_bytes, &g) != 5) bad = 1;
    list[0].load.blocks = 0x7fffffffLL;                                                 // past the grid by itself: it goes alone
    if (gif_cut(list, 0, 0, false, table_bytes, &g) != 1) bad = 1;
    // begin() when the device block cannot be had: the pinned buffer is fenced, nothing is freed
    stub_reset();
    S.fail_alloc = true;
    GifSender out;
    if (out.begin(64, 64, 16) == IMP_OK || S.parts.size() != 1 || !S.parts[0].last || S.parts[0].dev || S.parts[0].bytes || S.frees) bad = 1;
    // the page rule
    const impgpu_gif_page ok{(const unsigned char*)"", 3, 5, 4, 0, 0, 0, -1, (const unsigned char*)""};
    impgpu_gif_page p = ok;
    if (!gif_page_ok(p)) bad = 1;
    p = ok; p.indices = nullptr; if (gif_page_ok(p)) bad = 1;
    p = ok; p.palette = nullptr; if (gif_page_ok(p)) bad = 1;
    p = ok; p.width = 0; if (gif_page_ok(p)) bad = 1;
    p = ok; p.height = 0; if (gif_page_ok(p)) bad = 1;
    p = ok; p.pitch = 2; if (gif_page_ok(p)) bad = 1;
    if (bad) std::printf("FAIL limits\n");
    return bad;
}

}  // namespace

int main() {
    const int entries[] = {1, 2, 7}, pages[] = {1, 3, 40};
    const int sizes[][2] = {{1, 1}, {3, 5}, {257, 3}, {300, 200}};
    const size_t units[] = {16, 4096}, data[] = {0, 1, 15, 16, 17, 70001};
    int bad = check_limits(), n = 0;
    for (int ne : entries)
        for (int np : pages)
            for (const int* wh : sizes)
                for (int wide = 0; wide < 2; wide++)
                    for (int request : {-1, 0, np - 1, np})
                        for (size_t unit : units) {
                            const int pitch = wide ? (wh[0] + 3) & ~3 : wh[0];
                            bad |= check(Case{ne, np, wh[0], wh[1], pitch, request, unit, false, 0, false});
                            n++;
                            for (size_t db : data)
                                for (int split = 0; split < 2; split++) {
                                    bad |= check(Case{ne, np, wh[0], wh[1], gif_pitch(wh[0]), request, unit, true, db, split != 0});
                                    n++;
                                }
                        }
    stub_reset();
    std::printf("%s %d layouts\n", bad ? "FAILED" : "ok", n);
    return bad;
}
