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
#include "imp_webp_enc.h"

namespace imp {
namespace {

size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

int need_env() {
    if (!env_ready()) { set_error("impgpu_env_start has not been called", hipErrorNotInitialized); return IMP_ERROR_DEVICE; }
    return IMP_OK;
}

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
    const size_t o_fd = 0, o_items = o_fd + up256(fd.size() * sizeof(WebpFrameDesc)), o_tiles = o_items + up256(items.size() * sizeof(WebpItem)),
                 o_forced = o_tiles + up256(tile_items.size() * sizeof(WebpTileItem)), o_rec = o_forced + up256(forced_bytes.size()),
                 o_work = o_rec + up256((size_t)nf * sizeof(WebpRec)), o_lz = o_work + up256((size_t)nf * sizeof(WebpWork)), o_out = o_lz + (lz ? up256((size_t)nf * sizeof(WebpLz)) : 0), o_bits = o_out + outb,
                 o_off = o_bits + up256(items.size() * 4u), o_modes = o_off + up256(items.size() * 8u), o_resid = o_modes + modesb,
                 o_tok = o_resid + residb, o_end = o_tok + tokb;
    for (WebpFrameDesc& d : fd) {
        d.out_off += (long long)o_out; d.modes_off += (long long)o_modes; d.resid_off += (long long)o_resid; d.forced_off += (long long)o_forced;
        d.tok_off += (long long)o_tok;
    }
    void* mem = nullptr;
    if (int rc = dev_alloc(o_end, &mem)) return rc;
    uint8_t* m = (uint8_t*)mem;
    std::vector<uint8_t> head(o_rec, 0);
    std::memcpy(head.data() + o_fd, fd.data(), fd.size() * sizeof(WebpFrameDesc));
    std::memcpy(head.data() + o_items, items.data(), items.size() * sizeof(WebpItem));
    std::memcpy(head.data() + o_tiles, tile_items.data(), tile_items.size() * sizeof(WebpTileItem));
    if (!forced_bytes.empty()) std::memcpy(head.data() + o_forced, forced_bytes.data(), forced_bytes.size());
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
    // the first wait: the records
    std::vector<WebpRec> recs((size_t)nf);
    void *pin = nullptr, *token = nullptr;
    if (!rc) rc = stage_begin(recs.size() * sizeof(WebpRec), &pin, &token);
    if (!rc) {
        const hipError_t e = hipMemcpyAsync(pin, D.recs, recs.size() * sizeof(WebpRec), hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { set_error("hipMemcpyAsync(webp encode records)", e); rc = IMP_ERROR_DEVICE; }
    }
    if (rc) { (void)hipStreamSynchronize(s); dev_free(mem); return rc; }
    stage_hold(token, true);
    rc = lane_wait();
    if (!rc) std::memcpy(recs.data(), pin, recs.size() * sizeof(WebpRec));
    stage_hold(token, false);
    if (rc) { dev_free(mem); return rc; }
    // the files' sizes; what fits is fetched
    std::vector<size_t> at((size_t)nf, 0);
    std::vector<char> fetch((size_t)nf, 0);
    size_t total = 0;
    for (int f = 0; f < nf; f++) {
        const int i = entries[(size_t)f];
        const size_t len = (size_t)recs[(size_t)f].file_len;
        if (len < 20 || len > (size_t)fd[(size_t)f].out_words * 4u) {
            codes[i] = IMP_ERROR_DEVICE; lens[i] = 0; set_error_text("webp encode: a file outgrew its bound");
            continue;
        }
        lens[i] = len;
        if (len > caps[i]) { codes[i] = IMP_ERROR_MALLOC_FAILED; continue; }
        codes[i] = IMP_OK;
        fetch[(size_t)f] = 1;
        at[(size_t)f] = total;
        total += (len + 63) & ~size_t(63);
    }
    if (total) {
        if ((rc = stage_begin(total, &pin, &token))) { dev_free(mem); return rc; }
        hipError_t e = hipSuccess;
        for (int f = 0; f < nf && e == hipSuccess; f++)
            if (fetch[(size_t)f])
                e = hipMemcpyAsync((uint8_t*)pin + at[(size_t)f], m + fd[(size_t)f].out_off, (size_t)recs[(size_t)f].file_len, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) { set_error("hipMemcpyAsync(webp encode download)", e); (void)hipStreamSynchronize(s); dev_free(mem); return IMP_ERROR_DEVICE; }
        stage_hold(token, true);
        rc = lane_wait();                                               // the second wait: the files
        if (!rc)
            for (int f = 0; f < nf; f++)
                if (fetch[(size_t)f]) std::memcpy(outs[entries[(size_t)f]], (const uint8_t*)pin + at[(size_t)f], (size_t)recs[(size_t)f].file_len);
        stage_hold(token, false);
    }
    dev_free(mem);
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
    if (length) *length = 0;
    if (!image || !out || !length) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = batch_encode(&image, forced_modes ? &forced_modes : nullptr, 1, &out, &capacity, length, &code, nullptr)) return rc;
    return code;
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
