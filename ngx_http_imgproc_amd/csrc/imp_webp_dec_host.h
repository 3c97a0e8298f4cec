// imp_webp_dec_host.h -- the host front of the lossless WebP decoder, and the host model.  VP8L interleaves its headers
// with small entropy-coded sub-images, so the host reads everything in front of the main image's pixel stream -- the
// container and the header, the transforms with their sub-images (predictor modes, colour-transform elements, the
// delta-coded palette), the cache size, the entropy image, the code lengths of every group's five codes -- with the
// decoder functions the lanes use (imp_webp_dec.h), one lane after the other.  What comes out is a WdPlan: the blocks a
// file puts into the call's one upload, each a heap block of exactly its size.  wd_decode_host goes on from there with
// no device: tables, the main image's rounds, the inverse transforms -- impgpu_webp_decode_host.
// Host only, no HIP: tests/c/webp_dec_test.cpp builds it with g++ under AddressSanitizer / UBSan.
#pragma once
#include <cstring>
#include <memory>
#include <vector>
#include "../../include/impgpu.h"
#include "imp_webp_dec.h"

namespace imp {

struct WdPlan {
    int w = 0, h = 0, alpha_used = 0;
    int cw = 0;                                   // the coded width: what the transforms leave of w
    int cache_bits = 0, meta_bits = 0, meta_w = 0;
    uint32_t ngroups = 1;
    std::vector<uint32_t> words;                  // the VP8L chunk's bytes, zero-padded to words
    uint32_t in_size = 0;
    uint64_t bitpos = 0;                          // of the main image's first symbol
    std::vector<uint8_t> lens;                    // [ngroups][wd_sorted_stride]: the code lengths
    std::vector<uint32_t> meta;                   // the entropy image
    int ntrans = 0;
    WdTransform tr[4];
    std::vector<uint32_t> trdata[4];              // modes / elements / the palette (deltas added up)
    uint32_t feat = 0;
};

inline uint32_t wd_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// The container: a RIFF / WEBP file whose image is one VP8L chunk, alone or behind VP8X; other chunks are skipped.
inline int wd_container(const uint8_t* blob, size_t size, const uint8_t** payload, uint32_t* psize) {
    if (!blob || size < 12 || std::memcmp(blob, "RIFF", 4) != 0 || std::memcmp(blob + 8, "WEBP", 4) != 0) return IMP_ERROR_UNSUPPORTED;
    const uint64_t riff_end = (uint64_t)wd_le32(blob + 4) + 8u;
    const size_t end = riff_end < (uint64_t)size ? (size_t)riff_end : size;
    size_t at = 12;
    for (;;) {
        if (at + 8 > end) return IMP_ERROR_DECODE_FAILED;                     // no image chunk before the end
        const uint8_t* c = blob + at;
        const uint64_t n = wd_le32(c + 4);
        if (!std::memcmp(c, "VP8 ", 4) || !std::memcmp(c, "ANIM", 4) || !std::memcmp(c, "ANMF", 4) || !std::memcmp(c, "ALPH", 4)) return IMP_ERROR_UNSUPPORTED;
        if ((uint64_t)at + 8u + n > (uint64_t)end) return IMP_ERROR_DECODE_FAILED;   // a chunk that runs past the file
        if (!std::memcmp(c, "VP8X", 4) && n >= 1 && (c[8] & 0x02)) return IMP_ERROR_UNSUPPORTED;   // the animation flag
        if (!std::memcmp(c, "VP8L", 4)) {
            *payload = c + 8;
            *psize = (uint32_t)n;
            return IMP_OK;
        }
        at += 8 + (size_t)n + (size_t)(n & 1u);
    }
}

// the five header bytes: signature, 14 + 14 bits of size, alpha_is_used, 3 bits of version
inline int wd_header(const uint8_t* p, uint32_t n, int* w, int* h, int* alpha) {
    if (n < 5 || p[0] != 0x2f) return IMP_ERROR_DECODE_FAILED;
    const uint32_t v = wd_le32(p + 1);
    *w = (int)(v & 0x3fffu) + 1;
    *h = (int)((v >> 14) & 0x3fffu) + 1;
    *alpha = (int)((v >> 28) & 1u);
    if ((v >> 29) != 0u) return IMP_ERROR_UNSUPPORTED;
    if ((uint64_t)*w * (uint64_t)*h > (uint64_t)WD_MAX_PIXELS) return IMP_ERROR_UNSUPPORTED;
    return IMP_OK;
}

inline int wd_info(const uint8_t* blob, size_t size, int* w, int* h, int* alpha) {
    const uint8_t* p = nullptr;
    uint32_t n = 0;
    if (int rc = wd_container(blob, size, &p, &n)) return rc;
    return wd_header(p, n, w, h, alpha);
}

// one prefix code's lengths (the simple or the normal form) -> WD_*
inline int wd_read_code_lens(WdBits* b, uint64_t in_bits, uint8_t* lens, int alphabet, uint32_t* feat) {
    std::memset(lens, 0, (size_t)alphabet);
    if (wd_read(b, 1)) {
        *feat |= WD_F_SIMPLE;
        const int n = (int)wd_read(b, 1) + 1;
        const uint32_t s0 = wd_read(b, wd_read(b, 1) ? 8 : 1);
        if (s0 < (uint32_t)alphabet) lens[s0] = 1;
        if (n == 2) {
            const uint32_t s1 = wd_read(b, 8);
            if (s1 < (uint32_t)alphabet) lens[s1] = 1;
        }
        return wd_bits_pos(*b) > in_bits ? WD_SHORT : WD_OK;
    }
    static const uint8_t order[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    uint8_t cl[19] = {0};
    const int ncl = (int)wd_read(b, 4) + 4;
    for (int i = 0; i < ncl; i++) cl[order[i]] = (uint8_t)wd_read(b, 3);
    if (wd_bits_pos(*b) > in_bits) return WD_SHORT;
    WdCode clc;
    uint16_t clsorted[19];
    if (!wd_build_host(&clc, cl, 19, clsorted)) return WD_DAMAGED;
    int max_symbol = alphabet;
    if (wd_read(b, 1)) {
        const int nb = 2 + 2 * (int)wd_read(b, 3);
        max_symbol = 2 + (int)wd_read(b, nb);
        if (max_symbol > alphabet) return WD_DAMAGED;
    }
    int sym = 0, prev = 8;
    while (sym < alphabet) {
        if (max_symbol-- == 0) break;
        const int c = wd_read_sym(b, &clc, clsorted);
        if (c < 0) return WD_DAMAGED;
        if (wd_bits_pos(*b) > in_bits) return WD_SHORT;
        if (c < 16) {
            lens[sym++] = (uint8_t)c;
            if (c) prev = c;
            continue;
        }
        const int extra = c == 16 ? 2 : c == 17 ? 3 : 7, base = c == 18 ? 11 : 3;
        const int rep = (int)wd_read(b, extra) + base;
        if (sym + rep > alphabet) return WD_DAMAGED;
        std::memset(lens + sym, c == 16 ? prev : 0, (size_t)rep);
        sym += rep;
    }
    return wd_bits_pos(*b) > in_bits ? WD_SHORT : WD_OK;
}

// an optional colour cache's size -> WD_*
inline int wd_read_cache_bits(WdBits* b, int* cache_bits) {
    *cache_bits = 0;
    if (!wd_read(b, 1)) return WD_OK;
    *cache_bits = (int)wd_read(b, 4);
    return *cache_bits >= 1 && *cache_bits <= WD_MAX_CACHE_BITS ? WD_OK : WD_DAMAGED;
}

// `ngroups` groups' tables from their code lengths, by the lanes' build -> false: a code libwebp refuses
inline bool wd_tables_host(const uint8_t* lens, uint32_t ngroups, int cache_bits, std::vector<WdCode>* codes, std::vector<uint16_t>* sorted) {
    const uint32_t stride = wd_sorted_stride(cache_bits);
    codes->assign((size_t)ngroups * WD_CODES, WdCode{});
    sorted->assign((size_t)ngroups * stride, 0);
    for (uint32_t g = 0; g < ngroups; g++)
        for (int k = 0; k < WD_CODES; k++) {
            const size_t at = (size_t)g * stride + wd_sorted_at(k, cache_bits);
            if (!wd_build_host(&(*codes)[(size_t)g * WD_CODES + (size_t)k], lens + at, (int)wd_alphabet(k, cache_bits), sorted->data() + at)) return false;
        }
    return true;
}

// A sub-image between the headers: its cache size, its one group's codes, its pixels -- the lanes' rounds on the host.
inline int wd_sub_image(const WdPlan& P, WdBits* b, int w, int h, std::vector<uint32_t>* out, WdMem* m, uint32_t* feat) {
    const uint64_t in_bits = (uint64_t)P.in_size * 8u;
    int cache_bits = 0;
    if (int rc = wd_read_cache_bits(b, &cache_bits)) return rc;
    if (cache_bits) *feat |= WD_F_CACHE;
    const uint32_t stride = wd_sorted_stride(cache_bits);
    std::vector<uint8_t> lens(stride);
    for (int k = 0; k < WD_CODES; k++)
        if (int rc = wd_read_code_lens(b, in_bits, lens.data() + wd_sorted_at(k, cache_bits), (int)wd_alphabet(k, cache_bits), feat)) return rc;
    std::vector<WdCode> codes;
    std::vector<uint16_t> sorted;
    if (!wd_tables_host(lens.data(), 1, cache_bits, &codes, &sorted)) return WD_DAMAGED;
    out->assign((size_t)w * (size_t)h, 0);
    WdImage im{};
    im.in = (const uint8_t*)P.words.data(); im.in_size = P.in_size; im.in_cap = (uint32_t)(P.words.size() * 4u);
    im.w = w; im.h = h; im.npix = (uint32_t)w * (uint32_t)h;
    im.cache_bits = cache_bits;
    im.codes = codes.data(); im.sorted = sorted.data();
    im.sorted_stride = stride; im.green_n = wd_green_n(cache_bits); im.ngroups = 1;
    im.out = out->data();
    uint64_t endbit = 0;
    if (int rc = wd_rounds_host(im, wd_bits_pos(*b), m, feat, &endbit)) return rc;
    wd_bits_begin(b, P.words.data(), (int)P.words.size(), 0, endbit);
    return WD_OK;
}

// Everything in front of the main image's pixel stream, of a stream whose first bit is bit `bitpos` of `payload` and whose
// size P->w x P->h the caller has set: 40 behind the five header bytes of a VP8L chunk, 0 for the headerless stream of an
// ALPH chunk (imp_vp8_dec_host.h) -> IMP_*
inline int wd_parse_stream(const uint8_t* payload, uint32_t n, uint64_t bitpos, WdPlan* P, WdMem* m) {
    P->in_size = n;
    P->words.assign(((size_t)n + 3) / 4, 0);
    if (n) std::memcpy(P->words.data(), payload, n);
    const uint64_t in_bits = (uint64_t)n * 8u;
    WdBits b;
    wd_bits_begin(&b, P->words.data(), (int)P->words.size(), 0, bitpos);
    int xsize = P->w;
    unsigned seen = 0;
    while (wd_read(&b, 1)) {
        const int type = (int)wd_read(&b, 2);
        if (wd_bits_pos(b) > in_bits || (seen & (1u << type)) || P->ntrans >= 4) return IMP_ERROR_DECODE_FAILED;   // a transform twice
        seen |= 1u << type;
        WdTransform& t = P->tr[P->ntrans];
        std::vector<uint32_t>& data = P->trdata[P->ntrans];
        t = WdTransform{type, 0, xsize, 0u, 0};
        P->ntrans++;
        P->feat |= 1u << type;
        if (type == WD_TR_PREDICTOR || type == WD_TR_COLOR) {
            t.bits = (int)wd_read(&b, 3) + 2;
            if (wd_sub_image(*P, &b, wd_sub_size(xsize, t.bits), wd_sub_size(P->h, t.bits), &data, m, &P->feat)) return IMP_ERROR_DECODE_FAILED;
        } else if (type == WD_TR_INDEXING) {
            t.ncolors = wd_read(&b, 8) + 1u;
            t.bits = t.ncolors > 16u ? 0 : t.ncolors > 4u ? 1 : t.ncolors > 2u ? 2 : 3;
            if (wd_sub_image(*P, &b, (int)t.ncolors, 1, &data, m, &P->feat)) return IMP_ERROR_DECODE_FAILED;
            for (uint32_t i = 1; i < t.ncolors; i++) data[i] = wd_add_px(data[i], data[i - 1]);
            xsize = wd_sub_size(xsize, t.bits);
            P->feat |= WD_F_BUNDLE_0 << t.bits;
        }
    }
    P->cw = xsize;
    if (wd_read_cache_bits(&b, &P->cache_bits)) return IMP_ERROR_DECODE_FAILED;
    if (P->cache_bits) P->feat |= WD_F_CACHE;
    if (wd_read(&b, 1)) {
        P->meta_bits = (int)wd_read(&b, 3) + 2;
        P->meta_w = wd_sub_size(xsize, P->meta_bits);
        if (wd_bits_pos(b) > in_bits) return IMP_ERROR_DECODE_FAILED;
        if (wd_sub_image(*P, &b, P->meta_w, wd_sub_size(P->h, P->meta_bits), &P->meta, m, &P->feat)) return IMP_ERROR_DECODE_FAILED;
        uint32_t top = 0;
        for (uint32_t v : P->meta) top = std::max(top, (v >> 8) & 0xffffu);
        P->ngroups = top + 1u;
        if (P->ngroups > 1u) P->feat |= WD_F_GROUPS;
    }
    if (wd_bits_pos(b) > in_bits) return IMP_ERROR_DECODE_FAILED;
    const uint32_t stride = wd_sorted_stride(P->cache_bits);
    for (uint32_t g = 0; g < P->ngroups; g++) {
        P->lens.resize((size_t)(g + 1u) * stride);
        for (int k = 0; k < WD_CODES; k++)
            if (wd_read_code_lens(&b, in_bits, P->lens.data() + (size_t)g * stride + wd_sorted_at(k, P->cache_bits), (int)wd_alphabet(k, P->cache_bits), &P->feat))
                return IMP_ERROR_DECODE_FAILED;
    }
    P->bitpos = wd_bits_pos(b);
    return IMP_OK;
}

// the same of a file: the container and the five header bytes first
inline int wd_parse(const uint8_t* blob, size_t size, WdPlan* P, WdMem* m) {
    const uint8_t* payload = nullptr;
    uint32_t n = 0;
    if (int rc = wd_container(blob, size, &payload, &n)) return rc;
    if (int rc = wd_header(payload, n, &P->w, &P->h, &P->alpha_used)) return rc;
    return wd_parse_stream(payload, n, 40, P, m);
}

// the main image as the lanes see it; `out` holds cw * h pixels
inline WdImage wd_main_image(const WdPlan& P, const WdCode* codes, const uint16_t* sorted, uint32_t* out) {
    WdImage im{};
    im.in = (const uint8_t*)P.words.data(); im.in_size = P.in_size; im.in_cap = (uint32_t)(P.words.size() * 4u);
    im.w = P.cw; im.h = P.h; im.npix = (uint32_t)P.cw * (uint32_t)P.h;
    im.cache_bits = P.cache_bits;
    im.meta_bits = P.meta_bits; im.meta_w = P.meta_w; im.meta = P.meta.empty() ? nullptr : P.meta.data();
    im.codes = codes; im.sorted = sorted;
    im.sorted_stride = wd_sorted_stride(P.cache_bits); im.green_n = wd_green_n(P.cache_bits); im.ngroups = P.ngroups;
    im.out = out;
    return im;
}

// The transforms undone last to first, the lanes one after the other.  `a` holds the coded plane and, like `b`, w * h
// pixels; -> the buffer that holds the result.
inline uint32_t* wd_inverse_host(const WdPlan& P, uint32_t* a, uint32_t* b) {
    uint32_t *cur = a, *other = b;
    const int L = WD_LANES;
    for (int i = P.ntrans - 1; i >= 0; i--) {
        const WdTransform& t = P.tr[i];
        const uint32_t* data = P.trdata[i].data();
        const int w = t.xsize;
        const uint32_t npix = (uint32_t)w * (uint32_t)P.h;
        if (t.type == WD_TR_SUB_GREEN) {
            for (int j = 0; j < L; j++) wd_inv_add_green(cur, npix, (uint32_t)j, (uint32_t)L);
        } else if (t.type == WD_TR_COLOR) {
            for (int j = 0; j < L; j++) wd_inv_color(cur, w, P.h, t.bits, data, (uint32_t)j, (uint32_t)L);
        } else if (t.type == WD_TR_INDEXING) {
            for (int j = 0; j < L; j++) wd_inv_index(cur, other, w, P.h, t.bits, data, t.ncolors, (uint32_t)j, (uint32_t)L);
            std::swap(cur, other);
        } else {
            const int band = P.h < WD_INV_LANES ? P.h : WD_INV_LANES;       // the device's bands: the same rows are a band's first
            for (int row0 = 0; row0 < P.h; row0 += band)
                for (int s = 0; s < wd_pred_steps(w, band); s++)
                    for (int j = 0; j < band; j++) wd_inv_pred_step(cur, w, P.h, t.bits, data, row0, s, j);
        }
    }
    return cur;
}

// A parsed stream's coded plane: tables and the main image's rounds, the lanes one after the other, into a (w * h words;
// cw * h are written).  info (may be null): words 0, 5, 6, 7 -- the feature word is complete behind this.
inline int wd_coded_host(const WdPlan& P, WdMem* m, int* info, std::vector<uint32_t>* a) {
    const size_t npix = (size_t)P.w * (size_t)P.h;
    std::vector<WdCode> codes;
    std::vector<uint16_t> sorted;
    if (!wd_tables_host(P.lens.data(), P.ngroups, P.cache_bits, &codes, &sorted)) return IMP_ERROR_DECODE_FAILED;
    a->assign(npix, 0);
    const WdImage im = wd_main_image(P, codes.data(), sorted.data(), a->data());
    uint64_t endbit = 0;
    uint32_t feat = P.feat;
    int rounds = 0, longest = 0;
    const int status = wd_rounds_host(im, P.bitpos, m, &feat, &endbit, &rounds);
    for (uint8_t l : P.lens) longest = std::max(longest, (int)l);
    if (info) { info[0] = (int)feat; info[5] = status; info[6] = rounds; info[7] = longest; }
    return status ? IMP_ERROR_DECODE_FAILED : IMP_OK;
}

// A parsed stream's pixels: the coded plane, then the inverse transforms.  a / b: w * h words each; *dst is the one that
// holds the frame's ARGB words.
inline int wd_pixels_host(const WdPlan& P, WdMem* m, int* info, std::vector<uint32_t>* a, std::vector<uint32_t>* b, const uint32_t** dst) {
    const size_t npix = (size_t)P.w * (size_t)P.h;
    if (int rc = wd_coded_host(P, m, info, a)) return rc;
    b->assign(npix, 0);
    uint32_t* cur = wd_inverse_host(P, a->data(), b->data());
    uint32_t* out = cur == a->data() ? b->data() : a->data();
    for (int j = 0; j < WD_LANES; j++) wd_finish(cur, out, (uint32_t)npix, P.alpha_used, (uint32_t)j, (uint32_t)WD_LANES);
    *dst = out;
    return IMP_OK;
}

// impgpu_webp_decode_host
inline int wd_decode_host(const uint8_t* blob, size_t size, uint8_t* out, size_t capacity, int* width, int* height, int* info) {
    if (info) std::memset(info, 0, sizeof(int) * IMPGPU_WEBP_DEC_INFO_WORDS);
    std::unique_ptr<WdMem> m(new WdMem());
    WdPlan P;
    const int rc = wd_parse(blob, size, &P, m.get());
    if (rc != IMP_OK && rc != IMP_ERROR_DECODE_FAILED) return rc;
    if (width) *width = P.w;
    if (height) *height = P.h;
    if (rc) return rc;
    if (info) { info[0] = (int)P.feat; info[1] = (int)P.ngroups; info[2] = P.cache_bits; info[3] = P.ntrans; info[4] = P.cw; }
    const size_t npix = (size_t)P.w * (size_t)P.h;
    if (!out || capacity < npix * 4u) return IMP_ERROR_MALLOC_FAILED;
    std::vector<uint32_t> a, b;
    const uint32_t* dst = nullptr;
    if (int rc2 = wd_pixels_host(P, m.get(), info, &a, &b, &dst)) return rc2;
    std::memcpy(out, dst, npix * 4u);
    return IMP_OK;
}

}  // namespace imp
