// imp_webp_lossy.cpp -- lossy WebP answers out: impgpu_batch_encode_webp_lossy lays every accepted frame of the call out in
// one device block (descriptors and the macroblock-row table in front, uploaded once; records and work areas behind,
// zeroed; then per frame the padded planes, the alpha plane, the levels, the info words, the token records and their
// counts, the coded partitions and the file), runs the five launches of imp_webp_lossy.hip on it and waits twice: once for
// the frames' records (the files' lengths), once for the files that fit their callers' buffers, which leave the device
// complete.  impgpu_webp_lossy_encode_host is the same pipeline with no device: imp_webp_lossy.h's lane code on one thread.
#include "imp_internal.h"
#include "imp_enc_host.h"
#include "imp_webp_lossy.h"

namespace imp {
namespace {

// a frame's regions behind the shared front of a group's block, in the order they are taken
struct Vp8Regions { size_t y, u, v, alpha, lev, info, rec, nrec, first, part[8], out, end; };
Vp8Regions vp8_regions(int w, int h, int c, size_t at) {
    const int mbw = vp8_mbs(w), mbh = vp8_mbs(h), np = vp8_partitions(mbh);
    const size_t nmb = (size_t)mbw * (size_t)mbh;
    BlockLayout L;
    L.end = at;
    Vp8Regions r{};
    r.y = L.take(nmb * 256u); r.u = L.take(nmb * 64u); r.v = L.take(nmb * 64u);
    r.alpha = L.take(c == 4 ? (size_t)w * (size_t)h : 0u);
    r.lev = L.take(nmb * 800u); r.info = L.take(nmb * 4u);
    r.rec = L.take(nmb * VP8_MB_RECORDS * 2u); r.nrec = L.take(nmb * 4u);
    r.first = L.take(vp8_first_bound((uint32_t)nmb));
    for (int p = 0; p < 8; p++) r.part[p] = L.take(p < np ? vp8_partition_bound(mbw, mbh, np, p) : 0u);
    r.out = L.take(vp8_file_bound(w, h, c));
    r.end = L.size();
    return r;
}
// what a frame takes of a group's device block, for the stage cap
size_t vp8_frame_bytes(const impgpu_image* im) { return vp8_regions(im->w, im->h, im->c, 0).end + up256(sizeof(Vp8Work)); }

// ---------------------------------------------------------------- the device route: one group of frames
int encode_group(const std::vector<int>& entries, const impgpu_image* const* images, const int* qualities, unsigned char* const* outs, const size_t* caps,
                 size_t* lens, int* codes) {
    hipStream_t s = env_stream();
    const int nf = (int)entries.size();
    std::vector<Vp8FrameDesc> fd((size_t)nf);
    std::vector<Vp8RowItem> rows;
    for (int f = 0; f < nf; f++) {
        const impgpu_image* im = images[entries[(size_t)f]];
        for (int r = 0; r < vp8_mbs(im->h); r++) rows.push_back(Vp8RowItem{f, r});
    }
    // the block: what is uploaded | records | work areas (zeroed) | the frames' regions
    BlockLayout L;
    const size_t o_fd = L.take(fd.size() * sizeof(Vp8FrameDesc));
    const size_t o_rows = L.take(rows.size() * sizeof(Vp8RowItem));
    const size_t o_rec = L.take((size_t)nf * sizeof(Vp8Rec));           // where the upload ends and the zeroed stretch begins
    const size_t o_work = L.take((size_t)nf * sizeof(Vp8Work));
    const size_t o_frames = L.size();                                   // where the zeroed stretch ends
    int max_wpad = 0;
    uint32_t max_nmb = 0;
    for (int f = 0; f < nf; f++) {
        const impgpu_image* im = images[entries[(size_t)f]];
        Vp8FrameDesc& d = fd[(size_t)f];
        d.src = im->d;
        d.w = im->w; d.h = im->h; d.c = im->c; d.step = im->step;
        d.mbw = vp8_mbs(im->w); d.mbh = vp8_mbs(im->h); d.nparts = vp8_partitions(d.mbh);
        d.qi = vp8_quant_index(qualities[entries[(size_t)f]]);
        d.nmb = (uint32_t)d.mbw * (uint32_t)d.mbh;
        const Vp8Regions r = vp8_regions(im->w, im->h, im->c, L.size());
        d.y_off = (long long)r.y; d.u_off = (long long)r.u; d.v_off = (long long)r.v; d.alpha_off = (long long)r.alpha;
        d.lev_off = (long long)r.lev; d.info_off = (long long)r.info; d.rec_off = (long long)r.rec; d.nrec_off = (long long)r.nrec;
        d.first_off = (long long)r.first;
        for (int p = 0; p < 8; p++) d.part_off[p] = (long long)r.part[p];
        d.out_off = (long long)r.out;
        d.out_bytes = (unsigned long long)vp8_file_bound(im->w, im->h, im->c);
        L.end = r.end;
        max_wpad = std::max(max_wpad, d.mbw * 16);
        max_nmb = std::max(max_nmb, d.nmb);
    }
    DevBlock block;
    if (int rc = dev_alloc(L.size(), &block.p)) return rc;
    uint8_t* m = block.bytes();
    std::vector<uint8_t> head(o_rec, 0);
    head_put(head, o_fd, fd);
    head_put(head, o_rows, rows);
    int rc = upload_to(m, head.data(), head.size(), s);
    if (!rc) {
        const hipError_t e = hipMemsetAsync(m + o_rec, 0, o_frames - o_rec, s);
        if (e != hipSuccess) { set_error("hipMemsetAsync(webp lossy encode)", e); rc = IMP_ERROR_DEVICE; }
    }
    Vp8Dev D;
    D.mem = m;
    D.frames = (const Vp8FrameDesc*)(m + o_fd); D.rows = (const Vp8RowItem*)(m + o_rows);
    D.works = (Vp8Work*)(m + o_work); D.recs = (Vp8Rec*)(m + o_rec);
    D.nframes = nf;
    if (!rc) rc = launch_vp8_encode(D, (long long)rows.size(), max_wpad, max_nmb, s);
    if (rc) return drained(rc);
    std::vector<Vp8Rec> recs((size_t)nf);
    if ((rc = fetch_records(D.recs, recs.size() * sizeof(Vp8Rec), recs.data(), "hipMemcpyAsync(webp lossy encode records)"))) return rc;   // the first wait
    AnswerFetch files;
    std::vector<int> piece((size_t)nf, -1);
    for (int f = 0; f < nf; f++) {
        const int i = entries[(size_t)f];
        const uint64_t len = recs[(size_t)f].file_len;
        if (len == 0) { codes[i] = IMP_ERROR_UNSUPPORTED; lens[i] = 0; continue; }     // sizes the format cannot say
        if (len < 30 || len > (uint64_t)fd[(size_t)f].out_bytes) {
            codes[i] = IMP_ERROR_DEVICE; lens[i] = 0; set_error_text("webp lossy encode: a file outgrew its bound");
            continue;
        }
        if (answer_fits((size_t)len, caps[i], &codes[i], &lens[i])) piece[(size_t)f] = files.add(m + fd[(size_t)f].out_off, (size_t)len);
    }
    rc = files.run("hipMemcpyAsync(webp lossy encode download)");       // the second wait
    for (int f = 0; f < nf && !rc; f++)
        if (piece[(size_t)f] >= 0) std::memcpy(outs[entries[(size_t)f]], files.at(piece[(size_t)f]), (size_t)recs[(size_t)f].file_len);
    return rc;
}

int batch_encode(const impgpu_image* const* images, int count, const int* qualities, unsigned char* const* outs, const size_t* capacities, size_t* lengths,
                 int* codes, int* launches) {
    if (launches) *launches = 0;
    if (count < 0 || count > 256 || (count > 0 && (!images || !qualities || !outs || !capacities || !lengths || !codes))) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++)
        if (qualities[i] < 0 || qualities[i] > 100) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) lengths[i] = 0;
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
        const int rc = encode_group(group, images, qualities, outs, capacities, lengths, codes);
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
        if ((codes[i] = vp8_check_geometry(im->w, im->h, im->c)) != IMP_OK) continue;
        if (!im->d || !view_fits(im->w, im->h, im->c, im->step)) { codes[i] = IMP_ERROR_INVALID_ARGS; continue; }
        if (fault_hit(IMP_STEP_ENCODE)) { codes[i] = IMP_ERROR_DEVICE; continue; }
        const size_t need = vp8_frame_bytes(im);
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

size_t impgpu_webp_lossy_encode_bound(int width, int height, int channels) { return vp8_file_bound(width, height, channels); }

int impgpu_webp_lossy_encode_host(const unsigned char* frame, int width, int height, int channels, int step, int quality, unsigned char* out,
                                  size_t capacity, size_t* length) {
    return vp8_encode_host(frame, width, height, channels, step, quality, out, capacity, length, nullptr, nullptr, nullptr, nullptr, nullptr);
}

int impgpu_webp_lossy_encode_host_ex(const unsigned char* frame, int width, int height, int channels, int step, int quality, unsigned char* out,
                                     size_t capacity, size_t* length, unsigned char* modes, short* levels, unsigned char* recon_y,
                                     unsigned char* recon_u, unsigned char* recon_v) {
    return vp8_encode_host(frame, width, height, channels, step, quality, out, capacity, length, modes, levels, recon_y, recon_u, recon_v);
}

int impgpu_batch_encode_webp_lossy(const impgpu_image* const* images, int count, const int* qualities, unsigned char* const* outs,
                                   const size_t* capacities, size_t* lengths, int* codes, int* launches) {
    return batch_encode(images, count, qualities, outs, capacities, lengths, codes, launches);
}

int impgpu_image_encode_webp_lossy(const impgpu_image* image, int quality, unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (!image || !out || !length) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = batch_encode(&image, 1, &quality, &out, &capacity, length, &code, nullptr)) return rc;
    return code;
}

}  // extern "C"
