// imp_webp_enc.cpp -- lossless WebP answers out: impgpu_batch_encode_webp lays every accepted frame of the call out in one
// device block (descriptors, item tables and forced modes in front, uploaded once; records, the frames' work areas and
// their zeroed files behind, then the items' bit counts and offsets, the modes and the residuals), runs the six launches of
// imp_webp_enc.hip on it and waits twice: once for the frames' records (the files' lengths), once for the files that fit
// their callers' buffers, which leave the device complete -- container, sizes and pad byte included.
// impgpu_webp_encode_host is the same pipeline with no device: imp_webp_enc.h's lane code on one thread.
// With IMPGPU_WEBP_ENC_BACKREFS (the _flags calls) the block also holds a WebpLz per frame behind the work areas (zeroed
// with them) and the token planes behind the residuals, a file's region is sized by the flagged bound, and there are seven
// launches; with flags 0 the block and the launches are the flag-less call's.
#include "imp_internal.h"
#include "imp_enc_host.h"
#include "imp_webp_enc.h"

namespace imp {
namespace {

// what a frame takes of a group's device block, for the stage cap: its file, its residuals, its work area
size_t webp_frame_bytes(const impgpu_image* im, int flags) {
    const size_t plane = up256((size_t)im->w * im->h * 4u);
    const size_t plain = up256(webp_file_bound_flags(im->w, im->h, im->c, flags)) + plane + up256(sizeof(WebpWork));
    return flags & IMPGPU_WEBP_ENC_BACKREFS ? plain + plane + up256(sizeof(WebpLz)) : plain;     // the token plane, the WebpLz
}

// ---------------------------------------------------------------- the device route: one group of frames
int encode_group(const std::vector<int>& entries, const impgpu_image* const* images, const unsigned char* const* forced, unsigned char* const* outs,
                 const size_t* caps, size_t* lens, int* codes, int flags) {
    hipStream_t s = env_stream();
    const bool lz = (flags & IMPGPU_WEBP_ENC_BACKREFS) != 0;
    const int nf = (int)entries.size();
    const int tb = IMPGPU_WEBP_TILE_BITS;
    std::vector<WebpFrameDesc> fd((size_t)nf);
    std::vector<WebpItem> items;
    std::vector<WebpTileItem> tile_items;
    std::vector<uint8_t> forced_bytes;
    size_t outb = 0, modesb = 0, residb = 0, tokb = 0;
    for (int f = 0; f < nf; f++) {
        const impgpu_image* im = images[entries[(size_t)f]];
        WebpFrameDesc& d = fd[(size_t)f];
        d.src = im->d;
        d.w = im->w; d.h = im->h; d.c = im->c; d.step = im->step;
        d.tiles_x = webp_tiles(im->w, tb); d.tiles_y = webp_tiles(im->h, tb);
        d.npix = (uint32_t)im->w * (uint32_t)im->h;
        d.ntiles = (uint32_t)d.tiles_x * (uint32_t)d.tiles_y;
        d.item0 = (uint32_t)items.size();
        items.push_back(WebpItem{f, WEBP_IT_HDR_A, 0u});
        for (uint32_t k = 0; k < webp_item_count(d.ntiles); k++) items.push_back(WebpItem{f, WEBP_IT_MODES, k});
        items.push_back(WebpItem{f, WEBP_IT_HDR_B, 0u});
        for (uint32_t k = 0; k < webp_item_count(d.npix); k++) items.push_back(WebpItem{f, WEBP_IT_PIXELS, k});
        d.nitems = (uint32_t)items.size() - d.item0;
        for (uint32_t k = 0; k < (d.ntiles + 3u) / 4u; k++) tile_items.push_back(WebpTileItem{f, k});
        const size_t region = up256(webp_file_bound_flags(im->w, im->h, im->c, flags));
        d.out_words = (uint32_t)(region / 4u);
        d.out_off = (long long)outb; outb += region;
        d.modes_off = (long long)modesb; modesb += up256(d.ntiles);
        d.resid_off = (long long)residb; residb += up256((size_t)d.npix * 4u);
        d.tok_off = (long long)tokb;
        if (lz) tokb += up256((size_t)d.npix * 4u);
        const unsigned char* fm = forced ? forced[entries[(size_t)f]] : nullptr;
        d.has_forced = fm ? 1u : 0u;
        d.forced_off = (long long)forced_bytes.size();
        if (fm) {
            forced_bytes.insert(forced_bytes.end(), fm, fm + d.ntiles);
            forced_bytes.resize(up256(forced_bytes.size()), 0);
        }
    }
    if (items.size() > 0x7fffffffull || tile_items.size() > 0x7fffffffull) return IMP_ERROR_UNSUPPORTED;
    // the block: what is uploaded | records | work areas [+ WebpLz's] + files (zeroed) | item bits | item offsets | modes | residuals
    // [| token planes]
    BlockLayout L;
    const size_t o_fd = L.take(fd.size() * sizeof(WebpFrameDesc));      // the frames
    const size_t o_items = L.take(items.size() * sizeof(WebpItem));     // the items of k_webp_measure / _scan / _emit
    const size_t o_tiles = L.take(tile_items.size() * sizeof(WebpTileItem));   // the items of k_webp_modes
    const size_t o_forced = L.take(forced_bytes.size());                // the forced modes
    const size_t o_rec = L.take((size_t)nf * sizeof(WebpRec));          // the records: where the upload ends and the zeroed stretch begins
    const size_t o_work = L.take((size_t)nf * sizeof(WebpWork));        // the work areas
    const size_t o_lz = lz ? L.take((size_t)nf * sizeof(WebpLz)) : L.size();      // back references: a WebpLz a frame
    const size_t o_out = L.take_exact(outb);                            // the files
    const size_t o_bits = L.take(items.size() * 4u);                    // the items' bit counts: where the zeroed stretch ends
    const size_t o_off = L.take(items.size() * 8u);                     // the items' offsets
    const size_t o_modes = L.take_exact(modesb);                        // the modes
    const size_t o_resid = L.take_exact(residb);                        // the residuals
    const size_t o_tok = L.take_exact(tokb);                            // the token planes
    for (WebpFrameDesc& d : fd) {
        d.out_off += (long long)o_out; d.modes_off += (long long)o_modes; d.resid_off += (long long)o_resid; d.forced_off += (long long)o_forced;
        d.tok_off += (long long)o_tok;
    }
    DevBlock block;
    if (int rc = dev_alloc(L.size(), &block.p)) return rc;
    uint8_t* m = block.bytes();
    std::vector<uint8_t> head(o_rec, 0);
    head_put(head, o_fd, fd);
    head_put(head, o_items, items);
    head_put(head, o_tiles, tile_items);
    head_put(head, o_forced, forced_bytes);
    int rc = upload_to(m, head.data(), head.size(), s);
    if (!rc) {
        const hipError_t e = hipMemsetAsync(m + o_rec, 0, o_bits - o_rec, s);
        if (e != hipSuccess) { set_error("hipMemsetAsync(webp encode)", e); rc = IMP_ERROR_DEVICE; }
    }
    WebpDev D;
    D.mem = m;
    D.frames = (const WebpFrameDesc*)(m + o_fd); D.items = (const WebpItem*)(m + o_items); D.tile_items = (const WebpTileItem*)(m + o_tiles);
    D.works = (WebpWork*)(m + o_work); D.recs = (WebpRec*)(m + o_rec); D.item_bits = (uint32_t*)(m + o_bits); D.item_off = (uint64_t*)(m + o_off);
    D.tile_bits = tb;
    D.lz = lz ? (WebpLz*)(m + o_lz) : nullptr;
    if (!rc) rc = launch_webp_encode(D, (long long)tile_items.size(), (long long)items.size(), nf, s);
    if (rc) return drained(rc);
    std::vector<WebpRec> recs((size_t)nf);
    if ((rc = fetch_records(D.recs, recs.size() * sizeof(WebpRec), recs.data(), "hipMemcpyAsync(webp encode records)"))) return rc;   // the first wait
    // the files' sizes; what fits is fetched
    AnswerFetch files;
    std::vector<int> piece((size_t)nf, -1);
    for (int f = 0; f < nf; f++) {
        const int i = entries[(size_t)f];
        const size_t len = (size_t)recs[(size_t)f].file_len;
        if (len < 20 || len > (size_t)fd[(size_t)f].out_words * 4u) {
            codes[i] = IMP_ERROR_DEVICE; lens[i] = 0; set_error_text("webp encode: a file outgrew its bound");
            continue;
        }
        if (answer_fits(len, caps[i], &codes[i], &lens[i])) piece[(size_t)f] = files.add(m + fd[(size_t)f].out_off, len);
    }
    rc = files.run("hipMemcpyAsync(webp encode download)");            // the second wait
    for (int f = 0; f < nf && !rc; f++)
        if (piece[(size_t)f] >= 0) std::memcpy(outs[entries[(size_t)f]], files.at(piece[(size_t)f]), (size_t)recs[(size_t)f].file_len);
    return rc;
}

int batch_encode(const impgpu_image* const* images, const unsigned char* const* forced, int count, unsigned char* const* outs, const size_t* capacities,
                 size_t* lengths, int* codes, int* launches, int flags = 0) {
    if (launches) *launches = 0;
    if (flags & ~IMPGPU_WEBP_ENC_BACKREFS) return IMP_ERROR_INVALID_ARGS;
    if (count < 0 || count > 256 || (count > 0 && (!images || !outs || !capacities || !lengths || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) lengths[i] = 0;
    const int tb = IMPGPU_WEBP_TILE_BITS;
    for (int i = 0; i < count && forced; i++) {                         // a forced mode above 13: before a device is looked for
        const impgpu_image* im = images[i];
        if (!forced[i] || !im || im->frames != 1 || webp_check_geometry(im->w, im->h, im->c) != IMP_OK) continue;
        const size_t ntiles = (size_t)webp_tiles(im->w, tb) * (size_t)webp_tiles(im->h, tb);
        for (size_t t = 0; t < ntiles; t++)
            if (forced[i][t] >= WEBP_MODES) return IMP_ERROR_INVALID_ARGS;
    }
    if (count == 0) return IMP_OK;
    if (int rc = need_env()) {
        for (int i = 0; i < count; i++) codes[i] = rc;
        return rc;
    }
    TraceRange tr("IMP_STEP_ENCODE");
    const unsigned long long launched = t_launches;
    const size_t cap = stage_cap();
    std::vector<int> group;
    size_t bytes = 0;
    auto run = [&]() {
        if (group.empty()) return;
        const int rc = encode_group(group, images, forced, outs, capacities, lengths, codes, flags);
        if (rc)
            for (int i : group) { codes[i] = rc; lengths[i] = 0; }
        group.clear();
        bytes = 0;
    };
    for (int i = 0; i < count; i++) {
        const impgpu_image* im = images[i];
        codes[i] = IMP_ERROR_INVALID_ARGS;
        if (!im || !outs[i]) continue;
        if (im->frames != 1) { codes[i] = IMP_ERROR_UNSUPPORTED; continue; }                    // an album
        if ((codes[i] = webp_check_geometry(im->w, im->h, im->c)) != IMP_OK) continue;
        if (!im->d || !view_fits(im->w, im->h, im->c, im->step)) { codes[i] = IMP_ERROR_INVALID_ARGS; continue; }
        if (fault_hit(IMP_STEP_ENCODE)) { codes[i] = IMP_ERROR_DEVICE; continue; }
        const size_t need = webp_frame_bytes(im, flags);
        if (cap && need > cap) { codes[i] = IMP_ERROR_MALLOC_FAILED; continue; }                // a frame that does not fit under the stage cap
        if (!group.empty() && cap && bytes + need > cap) run();                                 // a call past the cap goes in groups
        group.push_back(i);
        bytes += need;
    }
    run();
    if (launches) *launches = (int)(t_launches - launched);
    return IMP_OK;
}

}  // namespace
}  // namespace imp

using namespace imp;

extern "C" {

size_t impgpu_webp_encode_bound(int width, int height, int channels) { return webp_file_bound(width, height, channels); }

int impgpu_webp_encode_host(const unsigned char* frame, int width, int height, int channels, int step, const unsigned char* forced_modes,
                            unsigned char* out, size_t capacity, size_t* length) {
    return webp_encode_host(frame, width, height, channels, step, forced_modes, out, capacity, length);
}

int impgpu_batch_encode_webp(const impgpu_image* const* images, int count, unsigned char* const* outs, const size_t* capacities, size_t* lengths,
                             int* codes, int* launches) {
    return batch_encode(images, nullptr, count, outs, capacities, lengths, codes, launches);
}

int impgpu_image_encode_webp_ex(const impgpu_image* image, const unsigned char* forced_modes, unsigned char* out, size_t capacity, size_t* length) {
    return impgpu_image_encode_webp_flags(image, 0, forced_modes, out, capacity, length);
}

size_t impgpu_webp_encode_bound_flags(int width, int height, int channels, int flags) {
    return flags & ~IMPGPU_WEBP_ENC_BACKREFS ? 0 : webp_file_bound_flags(width, height, channels, flags);
}

int impgpu_webp_encode_host_flags(const unsigned char* frame, int width, int height, int channels, int step, int flags, const unsigned char* forced_modes,
                                  unsigned char* out, size_t capacity, size_t* length) {
    return webp_encode_host(frame, width, height, channels, step, forced_modes, out, capacity, length, flags);
}

int impgpu_batch_encode_webp_flags(const impgpu_image* const* images, int count, int flags, unsigned char* const* outs, const size_t* capacities,
                                   size_t* lengths, int* codes, int* launches) {
    return batch_encode(images, nullptr, count, outs, capacities, lengths, codes, launches, flags);
}

int impgpu_image_encode_webp_flags(const impgpu_image* image, int flags, const unsigned char* forced_modes, unsigned char* out, size_t capacity,
                                   size_t* length) {
    if (length) *length = 0;
    if (!image || !out || !length || (flags & ~IMPGPU_WEBP_ENC_BACKREFS)) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = batch_encode(&image, forced_modes ? &forced_modes : nullptr, 1, &out, &capacity, length, &code, nullptr, flags)) return rc;
    return code;
}

int impgpu_image_encode_webp(const impgpu_image* image, unsigned char* out, size_t capacity, size_t* length) {
    return impgpu_image_encode_webp_ex(image, nullptr, out, capacity, length);
}

}  // extern "C"
