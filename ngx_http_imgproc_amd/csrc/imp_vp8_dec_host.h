// imp_vp8_dec_host.h -- the host front of the lossy WebP decoder, and its host model.  The host walks the container, reads
// the 10-byte frame tag and, with the lanes' own boolean decoder (imp_vp8_dec.h), the frame header at the head of the first
// partition -- segments, filter, partition count, quantisers, probability updates, the skip probability -- and the
// partition table.  What comes out is a VdPlan: a VdHdr and the chunk's bytes, which go into the group's one upload.
// vd_decode_host goes on from there with no device, the lanes one after the other -- impgpu_webp_decode_host_ex.
// With IMPGPU_WEBP_ACCEPT_ALPHA the front also finds a file's ALPH chunk (va_container, va_plane) and the host model
// puts the plane into byte 3 (va_decode_host: imp_webp_alpha.h's lanes, a VP8L plane by the lossless front's wd_parse_stream).
// Host only, no HIP: tests/c/vp8_dec_test.cpp and tests/c/webp_alpha_test.cpp build it with g++ under AddressSanitizer / UBSan.
#pragma once
#include <cstring>
#include <vector>
#include "imp_vp8_dec.h"
#include "imp_webp_alpha.h"
#include "imp_webp_dec_host.h"

namespace imp {

struct VdPlan {
    VdHdr hdr;
    std::vector<uint8_t> chunk;                   // the VP8 chunk's payload, a heap block of exactly its size
};

// The container as wd_container walks it, but a VP8 chunk is an image too: *lossy says which one was found.
inline int vd_container(const uint8_t* blob, size_t size, const uint8_t** payload, uint32_t* psize, int* lossy) {
    *lossy = 0;
    if (!blob || size < 12 || std::memcmp(blob, "RIFF", 4) != 0 || std::memcmp(blob + 8, "WEBP", 4) != 0) return IMP_ERROR_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)wd_le32(blob + 4) + 8u;
    const size_t end = riff_end < (uint64_t)size ? (size_t)riff_end : size;
    size_t at = 12;
    for (;;) {
        if (at + 8 > end) return IMP_ERROR_DECODE_FAILED;
        const uint8_t* c = blob + at;
        const uint64_t n = wd_le32(c + 4);
        if (!std::memcmp(c, "ANIM", 4) || !std::memcmp(c, "ANMF", 4) || !std::memcmp(c, "ALPH", 4)) return IMP_ERROR_UNSUPPORTED;
        if ((uint64_t)at + 8u + n > (uint64_t)end) return IMP_ERROR_DECODE_FAILED;
        if (!std::memcmp(c, "VP8X", 4) && n >= 1 && (c[8] & 0x02)) return IMP_ERROR_UNSUPPORTED;
        if (!std::memcmp(c, "VP8L", 4) || !std::memcmp(c, "VP8 ", 4)) {
            *lossy = c[3] == ' ';
            *payload = c + 8;
            *psize = (uint32_t)n;
            // libwebp is handed an odd VP8 chunk WITH its pad byte (the demuxer's payload), and its last partition runs to
            // the end of what it is handed: the pad byte is stream data
            if (*lossy && (n & 1u) && (uint64_t)at + 8u + n + 1u <= (uint64_t)end) *psize += 1u;
            return IMP_OK;
        }
        at += 8 + (size_t)n + (size_t)(n & 1u);
    }
}

// the frame tag and the key frame's start code and size (libwebp: VP8GetInfo and the head of VP8GetHeaders)
inline int vd_tag(const uint8_t* p, uint32_t n, int* w, int* h, uint32_t* first_size) {
    if (n < 10) return IMP_ERROR_DECODE_FAILED;
    const uint32_t bits = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    if (bits & 1u) return IMP_ERROR_UNSUPPORTED;                              // an inter frame
    if (((bits >> 1) & 7u) > 3u) return IMP_ERROR_DECODE_FAILED;
    if (!((bits >> 4) & 1u)) return IMP_ERROR_UNSUPPORTED;                    // show_frame 0
    if (p[3] != 0x9d || p[4] != 0x01 || p[5] != 0x2a) return IMP_ERROR_DECODE_FAILED;
    *w = (int)(((uint32_t)p[6] | (uint32_t)p[7] << 8) & 0x3fffu);             // the scale bits are ignored
    *h = (int)(((uint32_t)p[8] | (uint32_t)p[9] << 8) & 0x3fffu);
    *first_size = bits >> 5;
    if (*w == 0 || *h == 0) return IMP_ERROR_DECODE_FAILED;
    if ((uint64_t)*w * (uint64_t)*h > (uint64_t)IMPGPU_WEBP_DEC_MAX_PIXELS) return IMP_ERROR_UNSUPPORTED;
    if (*first_size > n - 10u) return IMP_ERROR_DECODE_FAILED;                // a first partition that runs past the chunk
    return IMP_OK;
}

inline int vd_clip_q(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// the frame header -> IMP_*
inline int vd_parse(const uint8_t* p, uint32_t n, VdHdr* H) {
    std::memset(H, 0, sizeof *H);
    uint32_t first = 0;
    if (int rc = vd_tag(p, n, &H->w, &H->h, &first)) return rc;
    H->mbw = vp8_mbs(H->w); H->mbh = vp8_mbs(H->h);
    H->first_off = 10u; H->first_size = first;
    uint32_t feat = 0;
    if (H->w & 15) feat |= IMPGPU_VP8_DEC_F_CROP_W;
    if (H->h & 15) feat |= IMPGPU_VP8_DEC_F_CROP_H;
    VdBool br;
    vd_bool_begin(br, p + 10, first);
    (void)vd_value(br, 2);                                                    // colour space, clamp type: ignored
    int use_segment = vd_bit(br, 128), absolute = 1, seg_q[4] = {0, 0, 0, 0}, seg_lf[4] = {0, 0, 0, 0};
    H->seg_prob[0] = H->seg_prob[1] = H->seg_prob[2] = 255;
    if (use_segment) {
        feat |= IMPGPU_VP8_DEC_F_SEGMENTS;
        H->update_map = (uint8_t)vd_bit(br, 128);
        if (vd_bit(br, 128)) {
            absolute = vd_bit(br, 128);
            for (int s = 0; s < 4; s++) seg_q[s] = vd_bit(br, 128) ? vd_signed_value(br, 7) : 0;
            for (int s = 0; s < 4; s++) seg_lf[s] = vd_bit(br, 128) ? vd_signed_value(br, 6) : 0;
            if (!absolute) feat |= IMPGPU_VP8_DEC_F_DELTA_VALUES;
        }
        if (H->update_map) {
            feat |= IMPGPU_VP8_DEC_F_MAP_UPDATE;
            for (int s = 0; s < 3; s++) H->seg_prob[s] = vd_bit(br, 128) ? (uint8_t)vd_value(br, 8) : 255;
        }
    }
    if (br.eof) return IMP_ERROR_DECODE_FAILED;
    const int simple = vd_bit(br, 128), level = vd_value(br, 6), sharpness = vd_value(br, 3), use_lf_delta = vd_bit(br, 128);
    int ref_delta[4] = {0, 0, 0, 0}, mode_delta[4] = {0, 0, 0, 0};
    if (use_lf_delta && vd_bit(br, 128)) {
        for (int i = 0; i < 4; i++) if (vd_bit(br, 128)) ref_delta[i] = vd_signed_value(br, 6);
        for (int i = 0; i < 4; i++) if (vd_bit(br, 128)) mode_delta[i] = vd_signed_value(br, 6);
    }
    if (br.eof) return IMP_ERROR_DECODE_FAILED;
    H->filter_type = level == 0 ? 0 : (simple ? 1 : 2);                       // frame level 0: off, whatever the segments say
    if (H->filter_type == 1) feat |= IMPGPU_VP8_DEC_F_SIMPLE;
    if (H->filter_type == 2) feat |= IMPGPU_VP8_DEC_F_NORMAL;
    if (H->filter_type && sharpness) feat |= IMPGPU_VP8_DEC_F_SHARPNESS;
    if (H->filter_type && use_lf_delta) feat |= IMPGPU_VP8_DEC_F_LF_DELTA;
    for (int s = 0; s < 4; s++) {
        int base = level;
        if (use_segment) { base = seg_lf[s]; if (!absolute) base += level; }
        for (int i4 = 0; i4 < 2; i4++) {
            int lv = base;
            if (use_lf_delta) { lv += ref_delta[0]; if (i4) lv += mode_delta[0]; }
            lv = lv < 0 ? 0 : (lv > 63 ? 63 : lv);
            uint8_t* f = H->fstr[s][i4];
            f[0] = f[1] = f[2] = 0;
            if (lv > 0 && H->filter_type) {
                int il = lv;
                if (sharpness > 0) {
                    il >>= sharpness > 4 ? 2 : 1;
                    if (il > 9 - sharpness) il = 9 - sharpness;
                }
                if (il < 1) il = 1;
                f[0] = (uint8_t)(2 * lv + il); f[1] = (uint8_t)il; f[2] = (uint8_t)(lv >= 40 ? 2 : (lv >= 15 ? 1 : 0));
            }
            f[3] = (uint8_t)i4;
        }
    }
    // the partitions: sizes past the end are cut to it; a last partition of no bytes fails
    const int pbits = vd_value(br, 2);
    H->nparts = 1 << pbits;
    if (pbits) feat |= IMPGPU_VP8_DEC_F_PARTS2 << (pbits - 1);
    const uint32_t rest = n - 10u - first, table = 3u * (uint32_t)(H->nparts - 1);
    if (rest < table) return IMP_ERROR_DECODE_FAILED;
    uint32_t at = 10u + first + table, left = rest - table;
    for (int i = 0; i < H->nparts; i++) {
        uint32_t ps = left;
        if (i + 1 < H->nparts) {
            const uint8_t* sz = p + 10u + first + 3u * (uint32_t)i;
            ps = (uint32_t)sz[0] | (uint32_t)sz[1] << 8 | (uint32_t)sz[2] << 16;
            if (ps > left) ps = left;
        }
        H->part_off[i] = at; H->part_size[i] = ps;
        at += ps; left -= ps;
    }
    for (int i = H->nparts; i < 8; i++) { H->part_off[i] = at; H->part_size[i] = 0; }
    if (H->part_size[H->nparts - 1] == 0) return IMP_ERROR_DECODE_FAILED;
    // the quantisers
    const int base_q = vd_value(br, 7);
    int dqd[5];
    for (int i = 0; i < 5; i++) {
        dqd[i] = vd_bit(br, 128) ? vd_signed_value(br, 4) : 0;
        if (dqd[i]) feat |= IMPGPU_VP8_DEC_F_DQ_Y1DC << i;
    }
    for (int s = 0; s < 4; s++) {
        int q = base_q;
        if (use_segment) { q = seg_q[s]; if (!absolute) q += base_q; }
        uint16_t* m = H->dq[s];
        m[0] = (uint16_t)vp8_dc_step(vd_clip_q(q + dqd[0], 127));
        m[1] = (uint16_t)vp8_ac_step(vd_clip_q(q, 127));
        m[2] = (uint16_t)(vp8_dc_step(vd_clip_q(q + dqd[1], 127)) * 2);
        m[3] = (uint16_t)((vp8_ac_step(vd_clip_q(q + dqd[2], 127)) * 101581) >> 16);
        if (m[3] < 8) m[3] = 8;
        m[4] = (uint16_t)vp8_dc_step(vd_clip_q(q + dqd[3], 117));
        m[5] = (uint16_t)vp8_ac_step(vd_clip_q(q + dqd[4], 127));
    }
    (void)vd_bit(br, 128);                                                    // refresh_entropy_probs: nothing follows a key frame
    for (int t = 0; t < 4; t++)
        for (int b = 0; b < 8; b++)
            for (int c = 0; c < 3; c++)
                for (int k = 0; k < 11; k++) {
                    const int i = ((t * 8 + b) * 3 + c) * 11 + k;
                    if (vd_bit(br, vp8_update_prob(i))) { H->prob[t][b][c][k] = (uint8_t)vd_value(br, 8); feat |= IMPGPU_VP8_DEC_F_PROB_UPDATE; }
                    else H->prob[t][b][c][k] = vp8_coef_prob(t, b, c, k);
                }
    H->use_skip = (uint8_t)vd_bit(br, 128);
    if (H->use_skip) H->skip_p = (uint8_t)vd_value(br, 8);
    else feat |= IMPGPU_VP8_DEC_F_SKIP_OFF;
    H->feat = feat;
    H->br_pos = br.pos; H->br_value = br.value; H->br_range = br.range; H->br_bits = br.bits; H->br_eof = br.eof;
    return IMP_OK;
}

inline int vd_plan(const uint8_t* payload, uint32_t n, VdPlan* P) {
    if (int rc = vd_parse(payload, n, &P->hdr)) return rc;
    P->chunk.assign(payload, payload + n);
    return IMP_OK;
}

// ---------------------------------------------------------------- the alpha plane (IMPGPU_WEBP_ACCEPT_ALPHA)
struct VaChunk {                                  // what the container walk found
    const uint8_t* p = nullptr;                   // the ALPH chunk's payload, its header byte first
    uint32_t n = 0;
    int canvas_w = 0, canvas_h = 0;               // VP8X's
};
struct VaPlane {                                  // the plane a file's frame gets; present 0: none, A stays 255
    int present = 0, method = 0, filter = 0, pre = 0;
    const uint8_t* data = nullptr;                // behind the header byte: w * h raw bytes (what follows is ignored), or the VP8L stream
    uint32_t size = 0;
};

// The container with both bits set.  The canonical layout is taken: VP8X with the alpha flag (and no animation flag), ONE
// ALPH chunk in front of the one `VP8 ` chunk, other chunks skipped (a second VP8X among them: the first one speaks).  An ALPH chunk anywhere else -- without VP8X or its
// flag, a second one, in front of VP8L, behind the image chunk -- is IMP_ERROR_UNSUPPORTED: libwebp's plain decode and its
// demuxer disagree about those, and the host decoder judges them as before.  A file without ALPH gets vd_container's verdict.
inline int va_container(const uint8_t* blob, size_t size, const uint8_t** payload, uint32_t* psize, int* lossy, VaChunk* A) {
    *lossy = 0;
    *A = VaChunk{};
    if (!blob || size < 12 || std::memcmp(blob, "RIFF", 4) != 0 || std::memcmp(blob + 8, "WEBP", 4) != 0) return IMP_ERROR_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)wd_le32(blob + 4) + 8u;
    const size_t end = riff_end < (uint64_t)size ? (size_t)riff_end : size;
    size_t at = 12;
    bool image = false, flagged = false, vp8x = false;
    for (;;) {
        if (at + 8 > end) return image ? IMP_OK : IMP_ERROR_DECODE_FAILED;
        const uint8_t* c = blob + at;
        const uint64_t n = wd_le32(c + 4);
        const bool alph = !std::memcmp(c, "ALPH", 4);
        if (image) {                                                          // behind the image only an ALPH is looked at
            if (alph) return IMP_ERROR_UNSUPPORTED;
            if ((uint64_t)at + 8u + n > (uint64_t)end) return IMP_OK;
            at += 8 + (size_t)n + (size_t)(n & 1u);
            continue;
        }
        if (!std::memcmp(c, "ANIM", 4) || !std::memcmp(c, "ANMF", 4)) return IMP_ERROR_UNSUPPORTED;
        if (alph && (!flagged || A->p)) return IMP_ERROR_UNSUPPORTED;
        if ((uint64_t)at + 8u + n > (uint64_t)end) return IMP_ERROR_DECODE_FAILED;
        if (!std::memcmp(c, "VP8X", 4)) {
            if (n >= 1 && (c[8] & 0x02)) return IMP_ERROR_UNSUPPORTED;
            if (!vp8x) flagged = n >= 10 && (c[8] & 0x10);
            if (!vp8x && n >= 10) {
                A->canvas_w = 1 + (int)((uint32_t)c[12] | (uint32_t)c[13] << 8 | (uint32_t)c[14] << 16);
                A->canvas_h = 1 + (int)((uint32_t)c[15] | (uint32_t)c[16] << 8 | (uint32_t)c[17] << 16);
            }
            vp8x = true;                                                      // a repeated VP8X is skipped like any other chunk: the first one's flag and canvas hold
        }
        if (alph) { A->p = c + 8; A->n = (uint32_t)n; }
        if (!std::memcmp(c, "VP8L", 4) || !std::memcmp(c, "VP8 ", 4)) {
            *lossy = c[3] == ' ';
            if (A->p && !*lossy) return IMP_ERROR_UNSUPPORTED;
            *payload = c + 8;
            *psize = (uint32_t)n;
            if (*lossy && (n & 1u) && (uint64_t)at + 8u + n + 1u <= (uint64_t)end) *psize += 1u;   // the pad byte: see vd_container
            image = true;
        }
        at += 8 + (size_t)n + (size_t)(n & 1u);
    }
}

// The ALPH chunk of a w x h frame -> IMP_OK and the plane, IMP_ERROR_UNSUPPORTED (a canvas that is not the frame) or
// IMP_ERROR_DECODE_FAILED: fewer than 2 bytes, a method above 1, pre-processing above 1, a reserved bit, a raw plane
// shorter than w * h.
inline int va_plane(const VaChunk& A, int w, int h, VaPlane* P) {
    *P = VaPlane{};
    if (!A.p) return IMP_OK;
    if (A.canvas_w != w || A.canvas_h != h) return IMP_ERROR_UNSUPPORTED;
    if (A.n < 2u) return IMP_ERROR_DECODE_FAILED;
    const uint32_t b = A.p[0];
    P->method = (int)(b & 3u); P->filter = (int)((b >> 2) & 3u); P->pre = (int)((b >> 4) & 3u);
    if (P->method > 1 || P->pre > 1 || (b >> 6)) return IMP_ERROR_DECODE_FAILED;
    P->data = A.p + 1; P->size = A.n - 1u;
    if (P->method == 0 && (uint64_t)P->size < (uint64_t)w * (uint64_t)h) return IMP_ERROR_DECODE_FAILED;
    P->present = 1;
    return IMP_OK;
}

// Which decoder a file goes to, for every _ex call alike.  Without the lossy bit: the lossless one, whose own container
// walk gives the codes of the calls without _ex (*lossy = 0, nothing else looked at).  With it: vd_container's verdict is
// the file's -- a `VP8 ` chunk that runs past the file is IMP_ERROR_DECODE_FAILED like any other chunk that does.  With
// the alpha bit too: va_container's, and for a file with an ALPH chunk the frame tag's and va_plane's -- the one order of
// the checks for the info call, the host model and the device path.
inline int vd_route(const uint8_t* blob, size_t size, int accept, const uint8_t** payload, uint32_t* psize, int* lossy, VaPlane* alpha) {
    *lossy = 0;
    *alpha = VaPlane{};
    if (!(accept & IMPGPU_WEBP_ACCEPT_LOSSY)) return IMP_OK;
    if (!(accept & IMPGPU_WEBP_ACCEPT_ALPHA)) return vd_container(blob, size, payload, psize, lossy);
    VaChunk A;
    if (int rc = va_container(blob, size, payload, psize, lossy, &A)) return rc;
    if (!A.p) return IMP_OK;
    int w = 0, h = 0;
    uint32_t first = 0;
    if (int rc = vd_tag(*payload, *psize, &w, &h, &first)) return rc;
    return va_plane(A, w, h, alpha);
}

// the geometry alone
inline int vd_info(const uint8_t* blob, size_t size, int accept, int* w, int* h) {
    const uint8_t* p = nullptr;
    uint32_t n = 0, first = 0;
    int lossy = 0, alpha = 0;
    VaPlane plane;
    if (int rc = vd_route(blob, size, accept, &p, &n, &lossy, &plane)) return rc;
    if (!lossy) return wd_info(blob, size, w, h, &alpha);
    return vd_tag(p, n, w, h, &first);
}

// A VP8L alpha stream's front: the lossless parse entered without container and header -> IMP_OK or IMP_ERROR_DECODE_FAILED
inline int va_parse_stream(const VaPlane& A, int w, int h, WdPlan* P, WdMem* m) {
    P->w = w; P->h = h; P->alpha_used = 1;
    return wd_parse_stream(A.data, A.size, 0, P, m) ? IMP_ERROR_DECODE_FAILED : IMP_OK;
}

// The plane into byte 3 of the w x h frame `out`, with no device; *feat (may be null): a VP8L stream's feature word.
// out == nullptr: the feature word alone -- the stream's entropy-coded image is still walked (back references and
// distance codes show only there), into one buffer of w * h words; no inverse transform, no frame.
inline int va_decode_host(const VaPlane& A, int w, int h, uint8_t* out, uint32_t* feat) {
    if (feat) *feat = 0;
    if (A.method == 0) {
        if (out) wa_unfilter_host(WaSrc{A.data, 1, 0}, out, w, h, A.filter);
        return IMP_OK;
    }
    std::unique_ptr<WdMem> m(new WdMem());
    WdPlan P;
    if (int rc = va_parse_stream(A, w, h, &P, m.get())) return rc;
    std::vector<uint32_t> a, b;
    const uint32_t* argb = nullptr;
    int info[IMPGPU_WEBP_DEC_INFO_WORDS] = {0};
    info[0] = (int)P.feat;
    const int rc = out ? wd_pixels_host(P, m.get(), info, &a, &b, &argb) : wd_coded_host(P, m.get(), info, &a);
    if (feat) *feat = (uint32_t)info[0];
    if (rc) return rc;
    if (out) wa_unfilter_host(WaSrc{(const uint8_t*)argb, 4, 1}, out, w, h, A.filter);
    return IMP_OK;
}

struct VdHostMem {
    std::vector<uint8_t> y, u, v, ctx;
    std::vector<uint32_t> finfo;
    VdWalk walk;
    VdMb mb;
    VdPlanes planes;
};
inline void vd_host_mem(const VdHdr& H, VdHostMem* m) {
    const size_t mbw = (size_t)H.mbw, mbh = (size_t)H.mbh;
    m->y.assign(mbw * 16u * mbh * 16u, 0); m->u.assign(mbw * 8u * mbh * 8u, 0); m->v.assign(mbw * 8u * mbh * 8u, 0);
    m->ctx.assign(mbw * 6u, 0);
    m->finfo.assign(mbw * mbh, 0);
    m->walk.top_nz = m->ctx.data(); m->walk.top_dc = m->ctx.data() + mbw; m->walk.top_modes = m->ctx.data() + 2u * mbw;
    m->planes = VdPlanes{m->y.data(), m->u.data(), m->v.data(), H.mbw * 16, H.mbw * 8};
}

// impgpu_webp_decode_host_ex for a lossy file
inline int vd_decode_host(const uint8_t* payload, uint32_t n, uint8_t* out, size_t capacity, int* width, int* height, int* info) {
    VdPlan P;
    const int rc = vd_plan(payload, n, &P);
    const VdHdr& H = P.hdr;
    if (rc != IMP_OK && rc != IMP_ERROR_DECODE_FAILED) return rc;
    if (width) *width = H.w;
    if (height) *height = H.h;
    if (rc) return rc;
    if (info) { info[0] = (int)H.feat; info[2] = H.nparts; info[3] = H.mbw; info[4] = H.mbh; info[7] = 1; }
    const size_t npix = (size_t)H.w * (size_t)H.h;
    if (!out || capacity < npix * 4u) return IMP_ERROR_MALLOC_FAILED;
    VdHostMem m;
    vd_host_mem(H, &m);
    const int status = vd_decode_mbs(H, P.chunk.data(), m.walk, m.mb, m.planes, m.finfo.data());
    if (info) { info[0] = (int)(H.feat | m.walk.feat); info[1] = (int)m.walk.mode_mask; info[5] = status; }
    if (status) return IMP_ERROR_DECODE_FAILED;
    if (H.filter_type)
        for (int my = 0; my < H.mbh; my++)
            for (int mx = 0; mx < H.mbw; mx++)
                for (int step = 0; step < VD_FILTER_STEPS; step++)
                    for (int lane = 0; lane < VD_FILTER_LANES; lane++)
                        vd_filter_step(H, m.planes, m.finfo[(size_t)my * (size_t)H.mbw + (size_t)mx], mx, my, step, lane);
    for (int y = 0; y < H.h; y++)
        for (int x = 0; x < H.w; x++) {
            const uint32_t px = vd_frame_pixel(m.planes, H.w, H.h, x, y);
            std::memcpy(out + ((size_t)y * (size_t)H.w + (size_t)x) * 4u, &px, 4);
        }
    return IMP_OK;
}

// impgpu_webp_decode_host_ex
inline int vd_decode_host_any(const uint8_t* blob, size_t size, int accept, uint8_t* out, size_t capacity, int* width, int* height, int* info) {
    const uint8_t* p = nullptr;
    uint32_t n = 0;
    int lossy = 0;
    VaPlane alpha;
    int rc = vd_route(blob, size, accept, &p, &n, &lossy, &alpha);
    if (rc || lossy) {
        if (info) std::memset(info, 0, sizeof(int) * IMPGPU_WEBP_DEC_INFO_WORDS);
        if (rc) return rc;
        int w = 0, h = 0;
        rc = vd_decode_host(p, n, out, capacity, &w, &h, info);
        if (width) *width = w;
        if (height) *height = h;
        if (rc == IMP_OK && alpha.present) rc = va_decode_host(alpha, w, h, out, nullptr);
        return rc;
    }
    return wd_decode_host(blob, size, out, capacity, width, height, info);
}

// impgpu_webp_alpha_info
inline int va_info(const uint8_t* blob, size_t size, int* info) {
    const uint8_t* p = nullptr;
    uint32_t n = 0, first = 0, feat = 0;
    int lossy = 0, w = 0, h = 0;
    VaPlane alpha;
    if (int rc = vd_route(blob, size, IMPGPU_WEBP_ACCEPT_LOSSY | IMPGPU_WEBP_ACCEPT_ALPHA, &p, &n, &lossy, &alpha)) return rc;
    if (!lossy || !alpha.present) return IMP_ERROR_UNSUPPORTED;
    if (int rc = vd_tag(p, n, &w, &h, &first)) return rc;
    if (alpha.method == 1)
        if (int rc = va_decode_host(alpha, w, h, nullptr, &feat)) return rc;
    if (info) { info[0] = alpha.method; info[1] = alpha.filter; info[2] = alpha.pre; info[3] = (int)feat; }
    return IMP_OK;
}

}  // namespace imp
