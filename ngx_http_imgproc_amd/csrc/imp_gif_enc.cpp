// imp_gif_enc.cpp -- GIF answers out: impgpu_batch_encode_gif lays the frames of every accepted album out in one device
// block (descriptors and item tables in front, uploaded once; records, colour sets, tables, index planes, segment slots
// and framed streams behind), runs the five launches of imp_gif_enc.hip on it and waits twice: once for the frames'
// records (the verdicts, the table sizes, the streams' lengths -- what the files' sizes depend on), once for the tables
// and streams of the files that fit their callers' buffers.  The host writes only the container around them
// (gif_enc_write_file).  impgpu_gif_encode_host is the same pipeline with no device: imp_gif_enc.h's lane code on one thread.
// The _ex calls take flags: under IMPGPU_GIF_ENC_QUANTIZE a group's block also holds a pool of histogram slots, eight launches
// run, and the albums the pool had no room for are encoded in further groups (impgpu_batch_encode_gif_ex).
// The _ex2 calls also take IMPGPU_GIF_ENC_DELTA: the block then holds a candidate word and a window record per frame, a
// second colour set and the candidates' held planes, k_gif_enc_delta runs ahead of the other launches, and the windows come
// back with the records in the first wait.
#include "imp_internal.h"
#include "imp_enc_host.h"
#include "imp_gif_enc.h"

namespace imp {
namespace {

// ---------------------------------------------------------------- the device route: one group of albums
struct EncPlan { int entry, first, frames; };
struct EncDeferred { int entry; uint32_t need; };        // an album whose overflowed frames got no histogram slots, and how many it wants

// flags & IMPGPU_GIF_ENC_QUANTIZE: a pool of `nslots` histogram slots lies in the block, and three launches more run
// (claim, hist, cut); an album the pool had no room for comes back in `deferred` with nothing written for it.
int encode_group(const std::vector<EncPlan>& plans, const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                 const int* loop_counts, uint32_t segment, int flags, int nslots, std::vector<EncDeferred>* deferred, unsigned char* const* outs,
                 const size_t* caps, size_t* lens, int* codes) {
    hipStream_t s = env_stream();
    const int na = (int)plans.size();
    int nf = 0;
    for (const EncPlan& p : plans) nf += p.frames;
    std::vector<GifEncFrameDesc> fd((size_t)nf);
    std::vector<GifEncAlbumDesc> ad((size_t)na);
    std::vector<GifEncItem> px_items, seg_items, pack_items;
    const bool delta = (flags & IMPGPU_GIF_ENC_DELTA) != 0;
    std::vector<GifDeltaDesc> dd(delta ? (size_t)nf : 0);
    size_t planes = 0, scratch = 0, outb = 0, heldw = 0;
    uint64_t nsegs = 0;
    for (int a = 0; a < na; a++) {
        const impgpu_image* im = albums[plans[(size_t)a].entry];
        ad[(size_t)a] = GifEncAlbumDesc{plans[(size_t)a].first, plans[(size_t)a].frames};
        const uint32_t total = (uint32_t)im->w * (uint32_t)im->h;
        const uint32_t out_cap = gif_enc_framed_size((uint32_t)gif_enc_stream_bound(total));
        const int* dis = dispose ? dispose[plans[(size_t)a].entry] : nullptr;
        auto keeps = [&](int q) { const int d = dis ? dis[q] : 0; return d == 0 || d == 1; };
        for (int q = 0; q < im->frames; q++) {
            const int f = plans[(size_t)a].first + q;
            if (delta) {                                                    // a candidate: a held plane, 16 pixels a word
                const bool cand = q >= 1 && keeps(q - 1) && keeps(q);
                dd[(size_t)f] = GifDeltaDesc{cand ? f - 1 : -1, (uint32_t)heldw};
                if (cand) heldw += up256(((size_t)total + 15) / 16 * 2) / 2;
            }
            GifEncFrameDesc& d = fd[(size_t)f];
            d.src = im->d + (size_t)q * im->fstride;
            d.w = im->w; d.h = im->h; d.c = im->c; d.step = im->step; d.album = a;
            d.wide = (im->c == 4 && (((uintptr_t)d.src | (uintptr_t)im->step) & 3) == 0) ? 1 : 0;
            d.total = total; d.segment = segment;
            d.nseg = gif_enc_segments(total, segment);
            d.seg0 = (uint32_t)nsegs; nsegs += d.nseg;
            d.slot_words = gif_enc_slot_words(segment < total ? segment : total);
            d.out_cap = out_cap;
            d.plane_off = (long long)planes; planes += up256(total);
            d.scratch_off = (long long)scratch; scratch += up256((size_t)d.nseg * d.slot_words * 4u);
            d.out_off = (long long)outb; outb += up256(out_cap);
            for (uint32_t k = 0; k < (total + GIF_ENC_PX_BLOCK - 1) / GIF_ENC_PX_BLOCK; k++) px_items.push_back(GifEncItem{f, (int)k});
            for (uint32_t k = 0; k < d.nseg; k++) seg_items.push_back(GifEncItem{f, (int)k});
            const uint32_t sb = (uint32_t)gif_enc_stream_bound(total);
            for (uint32_t k = 0; k < (sb + GIF_ENC_PACK_BLOCK - 1) / GIF_ENC_PACK_BLOCK; k++) pack_items.push_back(GifEncItem{f, (int)k});
        }
    }
    if (nsegs > 0x7fffffffull) return IMP_ERROR_UNSUPPORTED;
    // the block: what is uploaded | records + album words + sets + pool (zeroed) | tables | segment lengths | planes | slots | streams
    const bool quant = (flags & IMPGPU_GIF_ENC_QUANTIZE) != 0;
    const size_t ns = quant ? (size_t)nslots : 0;
    BlockLayout L;
    const size_t o_fd = L.take(fd.size() * sizeof(GifEncFrameDesc));    // the frames
    const size_t o_ad = L.take(ad.size() * sizeof(GifEncAlbumDesc));    // the albums
    const size_t o_px = L.take(px_items.size() * sizeof(GifEncItem));   // the items of the pixel launches
    const size_t o_seg = L.take(seg_items.size() * sizeof(GifEncItem)); // ... of k_gif_enc_lzw
    const size_t o_pack = L.take(pack_items.size() * sizeof(GifEncItem));   // ... of k_gif_enc_pack
    const size_t o_dd = L.take(dd.size() * sizeof(GifDeltaDesc));       // delta: the candidates (none without the bit)
    const size_t o_rec = L.take((size_t)nf * sizeof(GifEncRec));        // the records: where the upload ends and the zeroed stretch begins
    const size_t o_win = delta ? L.take((size_t)nf * sizeof(GifDeltaRec)) : L.size();     // delta: the frames' windows
    const size_t o_need = quant ? L.take((size_t)na * 4) : L.size();    // quantise: a word an album, the slots it got none of
    const size_t o_set = L.take((size_t)nf * sizeof(GifColourSet));     // the colour sets
    const size_t o_seta = delta ? L.take((size_t)nf * sizeof(GifColourSet)) : L.size();   // delta: the second sets
    const size_t o_sframe = L.take(ns * 4);                             // the pool: a slot's frame,
    const size_t o_strans = L.take(ns * 4);                             // ... its transparency,
    const size_t o_hist = L.take_exact(ns * GIF_Q_HIST_WORDS * 4);      // ... its histogram
    const size_t o_slotof = quant ? L.take((size_t)nf * 4) : L.size();  // quantise: a frame's slot; where the zeroed stretch ends under the flag,
    const size_t o_cmap = L.take_exact(ns * GIF_Q_CELLS);               // the slots' cell maps
    const size_t o_tab = L.take((size_t)nf * 1024);                     // the tables: ... and where it ends without
    const size_t o_bits = L.take((size_t)nsegs * 4);                    // the segments' lengths
    const size_t o_held = L.take(heldw * 2);                            // delta: the candidates' held planes
    const size_t o_plane = L.take_exact(planes);                        // the index planes
    const size_t o_scr = L.take_exact(scratch);                         // the segment slots
    const size_t o_out = L.take_exact(outb);                            // the framed streams
    for (GifEncFrameDesc& d : fd) { d.plane_off += (long long)o_plane; d.scratch_off += (long long)o_scr; d.out_off += (long long)o_out; }
    DevBlock block;
    if (int rc = dev_alloc(L.size(), &block.p)) return rc;
    uint8_t* m = block.bytes();
    std::vector<uint8_t> head(o_rec, 0);
    head_put(head, o_fd, fd);
    head_put(head, o_ad, ad);
    head_put(head, o_px, px_items);
    head_put(head, o_seg, seg_items);
    head_put(head, o_pack, pack_items);
    head_put(head, o_dd, dd);
    int rc = upload_to(m, head.data(), head.size(), s);
    if (!rc) {
        const hipError_t e = hipMemsetAsync(m + o_rec, 0, (quant ? o_slotof : o_tab) - o_rec, s);
        if (e != hipSuccess) { set_error("hipMemsetAsync(gif encode)", e); rc = IMP_ERROR_DEVICE; }
    }
    GifEncDev D;
    D.mem = m;
    D.frames = (const GifEncFrameDesc*)(m + o_fd); D.albums = (const GifEncAlbumDesc*)(m + o_ad);
    D.px_items = (const GifEncItem*)(m + o_px); D.seg_items = (const GifEncItem*)(m + o_seg); D.pack_items = (const GifEncItem*)(m + o_pack);
    D.flags = flags; D.nslots = (int)ns;
    D.slot_of = quant ? (int*)(m + o_slotof) : nullptr; D.slot_frame = quant ? (uint32_t*)(m + o_sframe) : nullptr;
    D.slot_trans = quant ? (uint32_t*)(m + o_strans) : nullptr; D.hist = quant ? (uint32_t*)(m + o_hist) : nullptr;
    D.cmaps = quant ? m + o_cmap : nullptr; D.album_need = quant ? (uint32_t*)(m + o_need) : nullptr;
    D.ddesc = delta ? (const GifDeltaDesc*)(m + o_dd) : nullptr; D.wins = delta ? (GifDeltaRec*)(m + o_win) : nullptr;
    D.held = delta ? (uint16_t*)(m + o_held) : nullptr; D.sets_a = delta ? (GifColourSet*)(m + o_seta) : nullptr;
    D.sets = (GifColourSet*)(m + o_set); D.tabs = (uint32_t*)(m + o_tab); D.recs = (GifEncRec*)(m + o_rec); D.segbits = (uint32_t*)(m + o_bits);
    if (!rc) rc = launch_gif_encode(D, (long long)px_items.size(), (long long)seg_items.size(), (long long)pack_items.size(), na, s);
    // the first wait: the records (and, behind them, the frames' windows and the albums' words)
    if (rc) return drained(rc);
    const size_t rec_bytes = quant ? (o_need - o_rec) + (size_t)na * 4 : delta ? (o_win - o_rec) + (size_t)nf * sizeof(GifDeltaRec)
                                                                               : (size_t)nf * sizeof(GifEncRec);
    std::vector<uint8_t> back(rec_bytes);
    if ((rc = fetch_records(D.recs, rec_bytes, back.data(), "hipMemcpyAsync(gif encode records)"))) return rc;
    const GifEncRec* recs = (const GifEncRec*)back.data();
    const GifDeltaRec* wins = delta ? (const GifDeltaRec*)(back.data() + (o_win - o_rec)) : nullptr;
    const uint32_t* album_need = quant ? (const uint32_t*)(back.data() + (o_need - o_rec)) : nullptr;
    // the files' sizes; what fits is fetched: per frame its table (local tables; the first frame's for a global one) and its stream
    AnswerFetch pieces;
    std::vector<int> tab_at((size_t)nf, -1), str_at((size_t)nf, -1);
    for (int a = 0; a < na; a++) {
        const EncPlan& p = plans[(size_t)a];
        const int i = p.entry;
        const GifEncRec* r0 = &recs[(size_t)p.first];
        if (r0->mode == GIF_ENC_REFUSED && quant && album_need[a]) { deferred->push_back(EncDeferred{i, album_need[a]}); continue; }
        if (r0->mode == GIF_ENC_REFUSED) { codes[i] = IMP_ERROR_UNSUPPORTED; lens[i] = 0; continue; }
        bool sane = true;
        size_t file_bytes = 13 + (loop_counts[i] >= 0 ? 19 : 0) + 1 + (r0->mode == GIF_ENC_GLOBAL ? gif_enc_table_bytes(r0->nkeys) : 0);
        for (int q = 0; q < p.frames; q++) {
            const GifEncRec& r = r0[q];
            sane = sane && r.nkeys >= 1 && r.nkeys <= GIF_SET_MAX && gif_enc_framed_size(r.stream_bytes) <= fd[(size_t)(p.first + q)].out_cap;
            if (delta) {
                const GifDeltaRec& wr = wins[(size_t)(p.first + q)];
                sane = sane && wr.ww >= 1 && wr.wh >= 1 && wr.x0 + wr.ww <= (uint32_t)albums[i]->w && wr.y0 + wr.wh <= (uint32_t)albums[i]->h;
            }
            file_bytes += 8 + 10 + 1 + gif_enc_framed_size(r.stream_bytes) + (r.mode == GIF_ENC_LOCAL ? gif_enc_table_bytes(r.nkeys) : 0);
        }
        if (!sane) { codes[i] = IMP_ERROR_DEVICE; lens[i] = 0; set_error_text("gif encode: a stream outgrew its bound"); continue; }
        if (!answer_fits(file_bytes, caps[i], &codes[i], &lens[i])) continue;
        for (int q = 0; q < p.frames; q++) {
            const size_t f = (size_t)(p.first + q);
            if (r0->mode == GIF_ENC_LOCAL || q == 0) tab_at[f] = pieces.add(D.tabs + f * 256, (size_t)r0[q].nkeys * 4);
            str_at[f] = pieces.add(m + fd[f].out_off, gif_enc_framed_size(r0[q].stream_bytes));
        }
    }
    rc = pieces.run("hipMemcpyAsync(gif encode download)");             // the second wait: the files
    std::vector<GifEncPage> pages;
    for (int a = 0; a < na && !rc; a++) {
        const EncPlan& p = plans[(size_t)a];
        const int i = p.entry;
        if (str_at[(size_t)p.first] < 0) continue;                      // refused, deferred or too long for its buffer
        pages.clear();
        for (int q = 0; q < p.frames; q++) {
            const size_t f = (size_t)(p.first + q), tf = tab_at[f] >= 0 ? f : (size_t)p.first;     // its own table, or the album's
            pages.push_back(GifEncPage{&recs[f], (const uint32_t*)pieces.at(tab_at[tf]), pieces.at(str_at[f])});
        }
        gif_enc_write_file(outs[i], pages.data(), p.frames, albums[i]->w, albums[i]->h, time_ms ? time_ms[i] : nullptr,
                           dispose ? dispose[i] : nullptr, loop_counts[i], delta ? wins + p.first : nullptr);
    }
    return rc;
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" {

size_t impgpu_gif_encode_bound(int width, int height, int frames) { return gif_enc_file_bound(width, height, frames); }

int impgpu_gif_encode_host(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                           const int* time_ms, const int* dispose, int loop_count, int segment, unsigned char* out, size_t capacity,
                           size_t* length) {
    return gif_encode_host(frames, count, width, height, channels, step, time_ms, dispose, loop_count, segment, out, capacity, length);
}

int impgpu_gif_encode_host_ex(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                              const int* time_ms, const int* dispose, int loop_count, int segment, int flags, unsigned char* out,
                              size_t capacity, size_t* length) {
    return gif_encode_host_ex(frames, count, width, height, channels, step, time_ms, dispose, loop_count, segment, flags, out, capacity, length);
}

int impgpu_gif_encode_host_ex2(const unsigned char* const* frames, int count, int width, int height, int channels, int step,
                               const int* time_ms, const int* dispose, int loop_count, int segment, int flags, unsigned char* out,
                               size_t capacity, size_t* length) {
    return gif_encode_host_ex2(frames, count, width, height, channels, step, time_ms, dispose, loop_count, segment, flags, out, capacity, length);
}

int impgpu_gif_quantize_host(const unsigned char* frame, int width, int height, int channels, int step, unsigned char* table,
                             int* entries, int* transparent_index, unsigned char* indices) {
    return gif_quantize_host(frame, width, height, channels, step, table, entries, transparent_index, indices);
}

int impgpu_batch_encode_gif(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                            const int* loop_counts, int count, int segment, unsigned char* const* outs, const size_t* capacities,
                            size_t* lengths, int* codes, int* launches) {
    return impgpu_batch_encode_gif_ex(albums, time_ms, dispose, loop_counts, count, segment, 0, outs, capacities, lengths, codes, launches);
}

int impgpu_batch_encode_gif_ex(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                               const int* loop_counts, int count, int segment, int flags, unsigned char* const* outs,
                               const size_t* capacities, size_t* lengths, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (flags & ~IMPGPU_GIF_ENC_QUANTIZE) return IMP_ERROR_INVALID_ARGS;
    return impgpu_batch_encode_gif_ex2(albums, time_ms, dispose, loop_counts, count, segment, flags, outs, capacities, lengths, codes, launches);
}

int impgpu_batch_encode_gif_ex2(const impgpu_image* const* albums, const int* const* time_ms, const int* const* dispose,
                                const int* loop_counts, int count, int segment, int flags, unsigned char* const* outs,
                                const size_t* capacities, size_t* lengths, int* codes, int* launches) {
    if (launches) *launches = 0;
    if (flags & ~(IMPGPU_GIF_ENC_QUANTIZE | IMPGPU_GIF_ENC_DELTA)) return IMP_ERROR_INVALID_ARGS;
    if (count < 0 || count > 256 || (count > 0 && (!albums || !loop_counts || !outs || !capacities || !lengths || !codes))) return IMP_ERROR_INVALID_ARGS;
    if (int rc = gif_enc_check_args(0, nullptr, 0, segment)) return rc;
    for (int i = 0; i < count; i++) lengths[i] = 0;
    if (count == 0) return IMP_OK;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    TraceRange tr("IMP_STEP_ENCODE");
    const unsigned long long launched = t_launches;
    const uint32_t seg = segment ? (uint32_t)segment : (uint32_t)IMPGPU_GIF_ENC_SEGMENT;
    const size_t cap = stage_cap();
    // the pool of a group: the histogram slots that fit under the cap (256 MB where there is none), one at least, never
    // more than the group has frames; a group of deferred albums gets what they need
    const size_t pool = std::max<size_t>(1, (cap ? cap : (size_t)256 << 20) / GIF_Q_SLOT_BYTES);
    std::vector<EncPlan> group;
    std::vector<EncDeferred> deferred, again;
    size_t bytes = 0, want = 0;
    int first = 0;
    auto run = [&](std::vector<EncDeferred>* left, size_t slots) {
        if (group.empty()) return;
        const int rc = encode_group(group, albums, time_ms, dispose, loop_counts, seg, flags, (int)std::min<size_t>(slots, (size_t)first), left, outs,
                                    capacities, lengths, codes);
        if (rc)
            for (const EncPlan& p : group) { codes[p.entry] = rc; lengths[p.entry] = 0; }
        group.clear();
        bytes = 0;
        want = 0;
        first = 0;
    };
    for (int i = 0; i < count; i++) {
        const impgpu_image* im = albums[i];
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!im || !outs[i]) continue;
        if ((codes[i] = gif_enc_check_geometry(im->w, im->h, im->c, im->frames)) != IMP_OK) continue;
        if ((codes[i] = gif_enc_check_args(im->frames, dispose ? dispose[i] : nullptr, loop_counts[i], segment)) != IMP_OK) continue;
        if (fault_hit(IMP_STEP_ENCODE)) { codes[i] = IMP_ERROR_DEVICE; continue; }
        const size_t bound = gif_enc_file_bound(im->w, im->h, im->frames);
        if (!group.empty() && cap && bytes + bound > cap) run(&deferred, pool);    // a call past the staging cap goes in groups
        group.push_back(EncPlan{i, first, im->frames});
        first += im->frames;
        bytes += bound;
    }
    run(&deferred, pool);
    for (const EncDeferred& d : deferred) {                             // the albums the pools had no room for: further groups
        const impgpu_image* im = albums[d.entry];
        const size_t bound = gif_enc_file_bound(im->w, im->h, im->frames);
        if (!group.empty() && ((cap && bytes + bound > cap) || want + d.need > pool)) run(&again, want);
        group.push_back(EncPlan{d.entry, first, im->frames});
        first += im->frames;
        bytes += bound;
        want += d.need;
    }
    run(&again, want);
    for (const EncDeferred& d : again) {                                // (a group that holds what its albums need defers none)
        codes[d.entry] = IMP_ERROR_DEVICE; lengths[d.entry] = 0;
        set_error_text("gif encode: an album was deferred twice");
    }
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

// one album: the _ex2 batch call with arrays of one, behind the checks of a lone call; `allowed` = the flags of the entry point
static int album_encode(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment, int flags, int allowed,
                        unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (flags & ~allowed) return IMP_ERROR_INVALID_ARGS;
    if (!album || !out || !length) return IMP_ERROR_INVALID_ARGS;
    if (int rc = gif_enc_check_args(album->frames <= GIF_ENC_MAX_FRAMES ? album->frames : 0, dispose, loop_count, segment)) return rc;
    int code = IMP_OK;
    if (int rc = impgpu_batch_encode_gif_ex2(&album, &time_ms, &dispose, &loop_count, 1, segment, flags, &out, &capacity, length, &code, nullptr)) return rc;
    return code;
}

int impgpu_album_encode_gif(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment,
                            unsigned char* out, size_t capacity, size_t* length) {
    return album_encode(album, time_ms, dispose, loop_count, segment, 0, 0, out, capacity, length);
}

int impgpu_album_encode_gif_ex(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment, int flags,
                               unsigned char* out, size_t capacity, size_t* length) {
    return album_encode(album, time_ms, dispose, loop_count, segment, flags, IMPGPU_GIF_ENC_QUANTIZE, out, capacity, length);
}

int impgpu_album_encode_gif_ex2(const impgpu_image* album, const int* time_ms, const int* dispose, int loop_count, int segment, int flags,
                                unsigned char* out, size_t capacity, size_t* length) {
    return album_encode(album, time_ms, dispose, loop_count, segment, flags, IMPGPU_GIF_ENC_QUANTIZE | IMPGPU_GIF_ENC_DELTA, out, capacity, length);
}

}  // extern "C"
