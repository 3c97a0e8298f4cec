// imp_webp_enc.h -- the lane code of the lossless WebP encoder: what the launches of imp_webp_enc.hip run per lane, and what
// impgpu_webp_encode_host (imp_webp_enc.cpp) runs one lane after the other (and under the sanitizers,
// tests/c/webp_enc_fuzz.cpp).  The file is defined in include/impgpu.h ("WEBP ANSWERS") and pinned by tests/webp_writer.py.
//
//   MODES    a wavefront per tile of 2^IMPGPU_WEBP_TILE_BITS pixels a side: every lane sums the 14 predictors' costs over
//            its pixels of the tile (webp_tile_costs_lane), the wave adds them up, the cheapest mode wins (webp_pick_mode).
//   RESID    a lane per pixel: the green-subtracted pixel minus its prediction (webp_residual_at), counted in four
//            256-bin histograms.
//   CODES    a lane per prefix code (webp_code_lane: zlib's build_tree from imp_png_deflate.h, the length list by zlib's
//            send_tree), then one lane strings the two header pieces together (webp_headers) and knows the file's size.
//   ITEMS    the stream is a row of ITEMS of up to 1024 symbols of at most 60 bits each: the header in front of the mode
//            image, the mode image's tiles, the header in front of the pixels, the pixels (webp_item_symbols, webp_symbol).
//            An item's bits are measured, the items' offsets are an exclusive scan (64-bit), and an item is put together
//            where its lanes can OR into it (webp_emit_put) before whole dwords leave.
//
//   PARSE    with IMPGPU_WEBP_ENC_BACKREFS alone: a pixel item's 1024 residuals are parsed greedily against 24 neighbours
//            (webp_lz_distance).  Per candidate the item's equality bits are 32 words (webp_lz_equal), a match's length
//            is the distance to the next zero bit (webp_lz_skips, webp_lz_length), the longest match of at least
//            IMPGPU_WEBP_MIN_MATCH wins (webp_lz_token); the tokens reached from the item's first position are written to
//            the token plane and counted (webp_lz_count), and webp_symbol_lz codes them.
//
// Safe by construction: every index into a frame is built from x < w and y < h; a store into the file checks the dword's
// index against the region's size.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../include/impgpu.h"

#if defined(__HIPCC__)
#define IMP_WEBP_HD __host__ __device__ __forceinline__
#else
#define IMP_WEBP_HD inline
#ifndef IMP_HD
#define IMP_HD
#endif
#endif
#include "imp_png_deflate.h"

namespace imp {

constexpr int WEBP_MODES = 14, WEBP_MAX_SIDE = 16384;
constexpr uint32_t WEBP_ITEM = 1024;                                   // symbols an item holds at most
constexpr int WEBP_SYMBOL_BITS = 60;                                   // four codes of at most 15 bits
constexpr int WEBP_STRIP_WORDS = 72;                                   // one prefix code's header: at most 63 + 7 * 280 bits
constexpr int WEBP_HDR_WORDS = 272;                                    // a header piece: at most 7 + four such headers
constexpr int WEBP_EMIT_WORDS = (int)(WEBP_ITEM * WEBP_SYMBOL_BITS / 32) + 4;
constexpr uint32_t WEBP_HDR_A_MAX = 40 + 3 + 6 + 1 + 2023 + 3 * 11 + 4, WEBP_HDR_B_MAX = 3 + 4 * 2023 + 4;
enum : uint32_t { WEBP_IT_HDR_A = 0, WEBP_IT_MODES = 1, WEBP_IT_HDR_B = 2, WEBP_IT_PIXELS = 3 };
// the codes of a frame: 0..3 = green, red, blue, alpha of the pixels' residuals; 4 = the mode image's green
constexpr int WEBP_CODES = 5, WEBP_CODE_MODES = 4;

struct WebpFrame { const uint8_t* src; int w, h, c, step; };

// what a frame's launches share in device memory (the host encoder holds one on the heap)
struct WebpWork {
    uint32_t hist[WEBP_CODES][256];                                    // zeroed before the launches
    uint32_t alpha_seen;                                               // zeroed: some alpha is not 255
    uint32_t strip_bits[WEBP_CODES];
    uint32_t hdr_bits[2];
    uint32_t tab[WEBP_CODES][256];                                     // code | length << 16
    uint32_t strip[WEBP_CODES][WEBP_STRIP_WORDS];
    uint32_t hdr[2][WEBP_HDR_WORDS];
    png::BlockTrees trees[WEBP_CODES];
};
struct WebpRec { uint64_t file_len; uint64_t payload_bits; };
// backward references: 24 candidates; the green code grows to its 280 symbols, the distance code has 40
constexpr int WEBP_LZ_CANDS = 24, WEBP_LZ_GREEN = 280, WEBP_LZ_DIST = 40, WEBP_LZ_SYMS = WEBP_LZ_GREEN + WEBP_LZ_DIST;
constexpr uint32_t WEBP_TOK_LITERAL = 0x80000000u;                     // the token plane: 0 covered, this, or length | k << 16
constexpr uint32_t WEBP_HDR_DIST_MAX = 63 + 7 * WEBP_LZ_DIST;          // the distance code's header in the normal form
// what a frame's launches share beside its WebpWork under IMPGPU_WEBP_ENC_BACKREFS: the green code (its strip and tree stay
// WebpWork's code 0, whose 256-bin histogram and table rest) and the distance code, green first in `hist` and `tab`
struct WebpLz {
    uint32_t hist[WEBP_LZ_SYMS];                                       // zeroed before the launches
    unsigned long long extra_bits;                                     // zeroed: the extra bits of every length and distance
    uint32_t tab[WEBP_LZ_SYMS];
    uint32_t strip_bits;
    uint32_t strip[WEBP_STRIP_WORDS];                                  // the distance code's header
    png::BlockTrees tree;
};
// A call's device block (imp_webp_enc.cpp lays it out): the frames, the item tables -- `tile_items` for k_webp_modes (four
// tiles each), `items` in stream order for the others -- and, by offsets from `mem`, each frame's modes (a byte a tile),
// residuals (a dword a pixel), forced modes (the _ex diagnostic) and file (out_words zeroed dwords).
struct WebpFrameDesc {
    const uint8_t* src;
    int w, h, c, step, tiles_x, tiles_y;
    uint32_t npix, ntiles, item0, nitems, out_words, has_forced;
    long long modes_off, resid_off, out_off, forced_off;
    long long tok_off;                                                 // the token plane (a dword a pixel), with `lz` alone
};
struct WebpItem { int frame; uint32_t kind, k; };
struct WebpTileItem { int frame; uint32_t k; };
struct WebpDev {
    uint8_t* mem;
    const WebpFrameDesc* frames;
    const WebpItem* items;
    const WebpTileItem* tile_items;
    WebpWork* works;
    WebpRec* recs;
    uint32_t* item_bits;
    uint64_t* item_off;
    int tile_bits;
    WebpLz* lz;                                                        // IMPGPU_WEBP_ENC_BACKREFS: a WebpLz per frame; else null
};

IMP_WEBP_HD void webp_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}
IMP_WEBP_HD void webp_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicAdd(p, v);
#else
    *p += v;
#endif
}

// ---------------------------------------------------------------- geometry and sizes
IMP_WEBP_HD int webp_tiles(int side, int tile_bits) { return (side + (1 << tile_bits) - 1) >> tile_bits; }
inline int webp_check_geometry(int w, int h, int c) {
    if (w <= 0 || h <= 0) return IMP_ERROR_INVALID_ARGS;
    if ((c != 1 && c != 3 && c != 4) || w > WEBP_MAX_SIDE || h > WEBP_MAX_SIDE) return IMP_ERROR_UNSUPPORTED;
    return IMP_OK;
}
// impgpu_webp_encode_bound: both header pieces at their longest, 15 bits a tile, 60 bits a pixel, the container, the pad byte
inline size_t webp_file_bound(int w, int h, int c) {
    if (webp_check_geometry(w, h, c) != IMP_OK) return 0;
    const uint64_t ntiles = (uint64_t)webp_tiles(w, IMPGPU_WEBP_TILE_BITS) * (uint64_t)webp_tiles(h, IMPGPU_WEBP_TILE_BITS);
    const uint64_t bits = WEBP_HDR_A_MAX + WEBP_HDR_B_MAX + 15u * ntiles + (uint64_t)WEBP_SYMBOL_BITS * (uint64_t)w * (uint64_t)h;
    return (size_t)(20u + (bits + 7u) / 8u + 1u);
}
// impgpu_webp_encode_bound_flags: with backward references the distance code's header may be the normal form (a reference
// is at most 15 + 8 + 15 + 3 bits for at least three positions: less than the literals it stands for are bounded by)
inline size_t webp_file_bound_flags(int w, int h, int c, int flags) {
    const size_t plain = webp_file_bound(w, h, c);
    return plain && (flags & IMPGPU_WEBP_ENC_BACKREFS) ? plain + (WEBP_HDR_DIST_MAX - 4u + 7u) / 8u : plain;
}

// ---------------------------------------------------------------- pixels: A << 24 | R << 16 | G << 8 | B
IMP_WEBP_HD uint32_t webp_argb(const WebpFrame& f, int x, int y) {
    const uint8_t* p = f.src + (size_t)y * (size_t)f.step + (size_t)x * (size_t)f.c;
    if (f.c == 1) return 0xff000000u | (uint32_t)p[0] * 0x010101u;
    if (f.c == 3) return 0xff000000u | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | (uint32_t)p[0];
    if (((((uintptr_t)f.src) | (uintptr_t)(uint32_t)f.step) & 3u) == 0u) return *(const uint32_t*)p;
    return (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | (uint32_t)p[0];
}
IMP_WEBP_HD uint32_t webp_sub_green(uint32_t p) {
    const uint32_t g = (p >> 8) & 255u;
    const uint32_t rb = 0xff00ff00u + (p & 0x00ff00ffu) - (g << 16 | g);
    return (p & 0xff00ff00u) | (rb & 0x00ff00ffu);
}
IMP_WEBP_HD uint32_t webp_px(const WebpFrame& f, int x, int y) { return webp_sub_green(webp_argb(f, x, y)); }
// per channel a - b mod 256
IMP_WEBP_HD uint32_t webp_sub(uint32_t a, uint32_t b) {
    const uint32_t ag = 0x00ff00ffu + (a & 0xff00ff00u) - (b & 0xff00ff00u);
    const uint32_t rb = 0xff00ff00u + (a & 0x00ff00ffu) - (b & 0x00ff00ffu);
    return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}
IMP_WEBP_HD uint32_t webp_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
IMP_WEBP_HD int webp_ch(uint32_t p, int k) { return (int)((p >> (8 * k)) & 255u); }
IMP_WEBP_HD uint32_t webp_clamp(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
IMP_WEBP_HD uint32_t webp_select(uint32_t L, uint32_t T, uint32_t TL) {
    int to_l = 0, to_t = 0;                                            // with p = L + T - TL: sum |p - L| and sum |p - T|
    for (int k = 0; k < 4; k++) {
        const int dl = webp_ch(T, k) - webp_ch(TL, k), dt = webp_ch(L, k) - webp_ch(TL, k);
        to_l += dl < 0 ? -dl : dl;
        to_t += dt < 0 ? -dt : dt;
    }
    return to_l < to_t ? L : T;
}
IMP_WEBP_HD uint32_t webp_add_sub_full(uint32_t L, uint32_t T, uint32_t TL) {
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) r |= webp_clamp(webp_ch(L, k) + webp_ch(T, k) - webp_ch(TL, k)) << (8 * k);
    return r;
}
IMP_WEBP_HD uint32_t webp_add_sub_half(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) {
        const int x = webp_ch(a, k);
        r |= webp_clamp(x + (x - webp_ch(b, k)) / 2) << (8 * k);       // C division: toward zero
    }
    return r;
}
struct WebpNb { uint32_t L, T, TL, TR; };
IMP_WEBP_HD uint32_t webp_predict(int mode, const WebpNb& n) {
    switch (mode) {
        case 0: return 0xff000000u;
        case 1: return n.L;
        case 2: return n.T;
        case 3: return n.TR;
        case 4: return n.TL;
        case 5: return webp_avg2(webp_avg2(n.L, n.TR), n.T);
        case 6: return webp_avg2(n.L, n.TL);
        case 7: return webp_avg2(n.L, n.T);
        case 8: return webp_avg2(n.TL, n.T);
        case 9: return webp_avg2(n.T, n.TR);
        case 10: return webp_avg2(webp_avg2(n.L, n.TL), webp_avg2(n.T, n.TR));
        case 11: return webp_select(n.L, n.T, n.TL);
        case 12: return webp_add_sub_full(n.L, n.T, n.TL);
        default: return webp_add_sub_half(webp_avg2(n.L, n.T), n.TL);
    }
}
// The prediction the edge rules fix at (x, y), if they do; otherwise the four neighbours.
IMP_WEBP_HD bool webp_edge(const WebpFrame& f, int x, int y, uint32_t* pred, WebpNb* n) {
    if (y == 0) { *pred = x == 0 ? 0xff000000u : webp_px(f, x - 1, 0); return true; }
    if (x == 0) { *pred = webp_px(f, 0, y - 1); return true; }
    n->L = webp_px(f, x - 1, y);
    n->T = webp_px(f, x, y - 1);
    n->TL = webp_px(f, x - 1, y - 1);
    n->TR = x + 1 < f.w ? webp_px(f, x + 1, y - 1) : webp_px(f, 0, y);
    return false;
}
IMP_WEBP_HD uint32_t webp_cost(uint32_t r) {
    uint32_t s = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t v = (r >> (8 * k)) & 255u;
        s += v < 256u - v ? v : 256u - v;
    }
    return s;
}

// MODES: lane `lane` of `nlanes` adds its pixels of tile (tx, ty) to cost[0 .. 14); returns whether it saw an alpha != 255
IMP_WEBP_HD bool webp_tile_costs_lane(const WebpFrame& f, int tile_bits, int tx, int ty, int lane, int nlanes, uint32_t* cost) {
    const int t = 1 << tile_bits, x0 = tx << tile_bits, y0 = ty << tile_bits;
    const int tw = f.w - x0 < t ? f.w - x0 : t, th = f.h - y0 < t ? f.h - y0 : t;
    bool alpha = false;
    for (int i = lane; i < tw * th; i += nlanes) {
        const int x = x0 + i % tw, y = y0 + i / tw;
        const uint32_t p = webp_argb(f, x, y), cur = webp_sub_green(p);
        alpha = alpha || (p >> 24) != 255u;
        uint32_t pred = 0;
        WebpNb n{0, 0, 0, 0};
        if (webp_edge(f, x, y, &pred, &n)) {
            const uint32_t c = webp_cost(webp_sub(cur, pred));
            for (int m = 0; m < WEBP_MODES; m++) cost[m] += c;
        } else {
            for (int m = 0; m < WEBP_MODES; m++) cost[m] += webp_cost(webp_sub(cur, webp_predict(m, n)));
        }
    }
    return alpha;
}
IMP_WEBP_HD int webp_pick_mode(const uint32_t* cost) {
    int best = 0;
    for (int m = 1; m < WEBP_MODES; m++)
        if (cost[m] < cost[best]) best = m;                            // a tie stays with the lowest mode
    return best;
}

// RESID: pixel `pix` of the frame (raster order) under the tiles' modes
IMP_WEBP_HD uint32_t webp_residual_at(const WebpFrame& f, const uint8_t* modes, int tile_bits, int tiles_x, uint32_t pix) {
    const int x = (int)(pix % (uint32_t)f.w), y = (int)(pix / (uint32_t)f.w);
    uint32_t pred = 0;
    WebpNb n{0, 0, 0, 0};
    if (!webp_edge(f, x, y, &pred, &n)) pred = webp_predict(modes[(size_t)(y >> tile_bits) * (size_t)tiles_x + (size_t)(x >> tile_bits)], n);
    return webp_sub(webp_px(f, x, y), pred);
}
IMP_WEBP_HD void webp_count(uint32_t* hist /* [4][256] */, uint32_t r) {
    webp_add(&hist[0 * 256 + ((r >> 8) & 255u)], 1u);
    webp_add(&hist[1 * 256 + ((r >> 16) & 255u)], 1u);
    webp_add(&hist[2 * 256 + (r & 255u)], 1u);
    webp_add(&hist[3 * 256 + (r >> 24)], 1u);
}

// ---------------------------------------------------------------- CODES
IMP_WEBP_HD int webp_cl_order(int i) {
    const uint8_t o[19] = {17, 18, 0, 1, 2, 3, 4, 5, 16, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
    return o[i];
}
IMP_WEBP_HD void webp_put_simple(png::BitWords& o, uint32_t symbol) { o.put(5u | symbol << 3, 11); }   // 1, 0, 1, the 8-bit symbol
// Code k of the frame: its table (code | length << 16 per symbol) and its header's bits in strip[k].  One used symbol: the
// simple form; otherwise lengths by build_tree (at most 15 bits), the length list by scan_tree / send_tree over the WHOLE
// alphabet (no max_symbol), the code-length code by build_tree again (at most 7 bits).
IMP_WEBP_HD void webp_code_lane(WebpWork* W, int k) {
    const uint32_t* hist = W->hist[k];
    const int nsym = k == WEBP_CODE_MODES ? WEBP_MODES : 256, alphabet = (k == 0 || k == WEBP_CODE_MODES) ? 280 : 256;
    uint32_t* tab = W->tab[k];
    for (int i = 0; i < WEBP_STRIP_WORDS; i++) W->strip[k][i] = 0;
    png::BitWords o{W->strip[k], 0};
    int used = 0, last = 0;
    for (int n = 0; n < nsym; n++)
        if (hist[n]) { used++; last = n; }
    for (int n = 0; n < 256; n++) tab[n] = 0;
    if (used <= 1) {
        webp_put_simple(o, (uint32_t)last);
    } else {
        png::BlockTrees& T = W->trees[k];
        for (int n = 0; n < png::L_CODES; n++) T.lf[n] = n < nsym ? hist[n] : 0u;
        for (int n = 0; n < png::BL_CODES; n++) T.bf[n] = 0;
        T.opt_len = T.static_len = 0;
        png::build_tree(T, 0);
        png::scan_tree(T, T.ll, alphabet - 1);
        png::build_tree(T, 2);
        int count = png::BL_CODES;
        while (count > 4 && T.blen[webp_cl_order(count - 1)] == 0) count--;
        o.put(0u, 1);
        o.put((uint32_t)(count - 4), 4);
        for (int i = 0; i < count; i++) o.put(T.blen[webp_cl_order(i)], 3);
        o.put(0u, 1);
        png::send_tree(o, T, T.ll, alphabet - 1);
        for (int n = 0; n < nsym; n++)
            if (T.ll[n] && n <= T.lmax) tab[n] = (uint32_t)T.lcode[n] | (uint32_t)T.ll[n] << 16;
    }
    W->strip_bits[k] = (uint32_t)o.at;
}
// The same for a code of `nsym` <= L_CODES symbols counted in `hist`, of an alphabet of `alphabet` >= nsym, wherever its
// pieces lie: with backward references the green code over its 280 symbols and the distance code over its 40 as well.
// `none_is_0`: a code nobody uses is the bits 1,0,0,0.  (webp_code_lane above stays beside it as it was written, so that
// the flag-less launch's device code does not change with the flag's.)
IMP_WEBP_HD void webp_code_build(png::BlockTrees& T, const uint32_t* hist, int nsym, int alphabet, uint32_t* tab, uint32_t* strip, uint32_t* strip_bits,
                                 bool none_is_0) {
    for (int i = 0; i < WEBP_STRIP_WORDS; i++) strip[i] = 0;
    png::BitWords o{strip, 0};
    int used = 0, last = 0;
    for (int n = 0; n < nsym; n++) {
        if (hist[n]) { used++; last = n; }
        tab[n] = 0;
    }
    if (used == 0 && none_is_0) {
        o.put(1u, 4);
    } else if (used <= 1) {
        webp_put_simple(o, (uint32_t)last);                            // (a lone green symbol is a literal's: position 0 is one)
    } else {
        for (int n = 0; n < png::L_CODES; n++) T.lf[n] = n < nsym ? hist[n] : 0u;
        for (int n = 0; n < png::BL_CODES; n++) T.bf[n] = 0;
        T.opt_len = T.static_len = 0;
        png::build_tree(T, 0);
        png::scan_tree(T, T.ll, alphabet - 1);
        png::build_tree(T, 2);
        int count = png::BL_CODES;
        while (count > 4 && T.blen[webp_cl_order(count - 1)] == 0) count--;
        o.put(0u, 1);
        o.put((uint32_t)(count - 4), 4);
        for (int i = 0; i < count; i++) o.put(T.blen[webp_cl_order(i)], 3);
        o.put(0u, 1);
        png::send_tree(o, T, T.ll, alphabet - 1);
        for (int n = 0; n < nsym; n++)
            if (T.ll[n] && n <= T.lmax) tab[n] = (uint32_t)T.lcode[n] | (uint32_t)T.ll[n] << 16;
    }
    *strip_bits = (uint32_t)o.at;
}
// CODES with backward references: lane 0 the green code, 1..4 as ever, 5 the distance code -- where each lane's pieces lie
// is picked first, so that the six lanes of a wavefront walk ONE body side by side, not three one after the other
IMP_WEBP_HD void webp_code_lane_lz(WebpWork* W, WebpLz* L, int k) {
    const bool green = k == 0, dist = k == WEBP_CODES;
    const int kk = dist ? 0 : k;
    png::BlockTrees& T = dist ? L->tree : W->trees[kk];
    const uint32_t* hist = green ? L->hist : dist ? L->hist + WEBP_LZ_GREEN : W->hist[kk];
    uint32_t* tab = green ? L->tab : dist ? L->tab + WEBP_LZ_GREEN : W->tab[kk];
    const int nsym = green ? WEBP_LZ_GREEN : dist ? WEBP_LZ_DIST : k == WEBP_CODE_MODES ? WEBP_MODES : 256;
    const int alphabet = green || k == WEBP_CODE_MODES ? WEBP_LZ_GREEN : dist ? WEBP_LZ_DIST : 256;
    webp_code_build(T, hist, nsym, alphabet, tab, dist ? L->strip : W->strip[kk], dist ? &L->strip_bits : &W->strip_bits[kk], dist);
}
IMP_WEBP_HD void webp_put_strip(png::BitWords& o, const uint32_t* words, uint32_t bits) {
    for (uint32_t at = 0; at < bits; at += 32u) {
        const uint32_t n = bits - at < 32u ? bits - at : 32u;
        o.put(n == 32u ? words[at >> 5] : words[at >> 5] & ((1u << n) - 1u), (int)n);
    }
}
// the two header pieces, the stream's length, the container's 20 bytes (five dwords at `out32`, which holds them)
// `L` (null without backward references): the distance code's strip stands where the bits 1,0,0,0 stood, the green symbols
// are counted over 280 bins, and the extra bits of the lengths and distances are part of the payload
IMP_WEBP_HD void webp_headers(WebpWork* W, int w, int h, int c, int tile_bits, WebpRec* rec, uint32_t* out32, const WebpLz* L = nullptr) {
    for (int i = 0; i < WEBP_HDR_WORDS; i++) W->hdr[0][i] = W->hdr[1][i] = 0;
    png::BitWords a{W->hdr[0], 0};
    a.put(0x2fu, 8);
    a.put((uint32_t)(w - 1), 14);
    a.put((uint32_t)(h - 1), 14);
    a.put(c == 4 && W->alpha_seen ? 1u : 0u, 1);
    a.put(0u, 3);
    a.put(1u | 2u << 1, 3);                                            // a transform: subtract-green
    a.put(1u | 0u << 1, 3);                                            // a transform: predictor
    a.put((uint32_t)(tile_bits - 2), 3);
    a.put(0u, 1);                                                      // the mode image: no colour cache
    webp_put_strip(a, W->strip[WEBP_CODE_MODES], W->strip_bits[WEBP_CODE_MODES]);
    webp_put_simple(a, 0u);
    webp_put_simple(a, 0u);
    webp_put_simple(a, 255u);
    a.put(1u, 4);                                                      // the distance code: 1, 0, 0, 0
    W->hdr_bits[0] = (uint32_t)a.at;
    png::BitWords b{W->hdr[1], 0};
    b.put(0u, 1);                                                      // no further transform
    b.put(0u, 2);                                                      // no colour cache, no meta prefix image
    for (int k = 0; k < 4; k++) webp_put_strip(b, W->strip[k], W->strip_bits[k]);
    if (L) webp_put_strip(b, L->strip, L->strip_bits);
    else b.put(1u, 4);
    W->hdr_bits[1] = (uint32_t)b.at;
    uint64_t bits = a.at + b.at;
    if (L) {
        bits += L->extra_bits;
        for (int n = 0; n < WEBP_LZ_SYMS; n++) bits += (uint64_t)L->hist[n] * (uint64_t)(L->tab[n] >> 16);
    }
    for (int k = 0; k < WEBP_CODES; k++)
        for (int n = 0; n < 256; n++) bits += (uint64_t)W->hist[k][n] * (uint64_t)(W->tab[k][n] >> 16);
    const uint64_t payload = (bits + 7u) >> 3;
    rec->payload_bits = bits;
    rec->file_len = 20u + payload + (payload & 1u);
    out32[0] = 0x46464952u;                                            // "RIFF"
    out32[1] = (uint32_t)(rec->file_len - 8u);
    out32[2] = 0x50424557u;                                            // "WEBP"
    out32[3] = 0x4c385056u;                                            // "VP8L"
    out32[4] = (uint32_t)payload;
}

// ---------------------------------------------------------------- ITEMS
IMP_WEBP_HD uint32_t webp_item_count(uint32_t n) { return (n + WEBP_ITEM - 1u) / WEBP_ITEM; }
IMP_WEBP_HD uint32_t webp_item_symbols(uint32_t kind, uint32_t k, const WebpWork* W, uint32_t ntiles, uint32_t npix) {
    if (kind == WEBP_IT_HDR_A || kind == WEBP_IT_HDR_B) return (W->hdr_bits[kind == WEBP_IT_HDR_B] + 31u) >> 5;
    const uint32_t n = kind == WEBP_IT_MODES ? ntiles : npix;
    return n - k * WEBP_ITEM < WEBP_ITEM ? n - k * WEBP_ITEM : WEBP_ITEM;
}
// symbol i of the item as up to four parts of at most 32 bits each, in stream order: code[q]'s low len[q] bits (a part
// that is not there has len 0); the symbol's bits returned.  `tab`: the frame's five tables (W->tab, or a copy of it)
IMP_WEBP_HD uint32_t webp_symbol(uint32_t kind, uint32_t k, uint32_t i, const WebpWork* W, const uint32_t* tab, const uint8_t* modes,
                                 const uint32_t* resid, uint32_t* code, uint32_t* len) {
    code[1] = code[2] = code[3] = 0u;
    len[1] = len[2] = len[3] = 0u;
    if (kind == WEBP_IT_HDR_A || kind == WEBP_IT_HDR_B) {
        const int p = kind == WEBP_IT_HDR_B;
        const uint32_t left = W->hdr_bits[p] - 32u * i, n = left < 32u ? left : 32u;
        code[0] = n == 32u ? W->hdr[p][i] : W->hdr[p][i] & ((1u << n) - 1u);
        len[0] = n;
        return n;
    }
    if (kind == WEBP_IT_MODES) {
        const uint32_t t = tab[WEBP_CODE_MODES * 256 + modes[(size_t)k * WEBP_ITEM + i]];
        code[0] = t & 0xffffu;
        len[0] = t >> 16;
        return len[0];
    }
    const uint32_t r = resid[(size_t)k * WEBP_ITEM + i];
    const uint32_t t0 = tab[(r >> 8) & 255u], t1 = tab[256 + ((r >> 16) & 255u)], t2 = tab[512 + (r & 255u)], t3 = tab[768 + (r >> 24)];
    code[0] = t0 & 0xffffu; len[0] = t0 >> 16;
    code[1] = t1 & 0xffffu; len[1] = t1 >> 16;
    code[2] = t2 & 0xffffu; len[2] = t2 >> 16;
    code[3] = t3 & 0xffffu; len[3] = t3 >> 16;
    return len[0] + len[1] + len[2] + len[3];
}
// `n` bits (at most 32) of v at bit `pos` of `words`, which the lanes of the item share
IMP_WEBP_HD void webp_emit_put(uint32_t* words, uint32_t pos, uint32_t v, uint32_t n) {
    if (n == 0u) return;
    const uint32_t sh = pos & 31u, wi = pos >> 5;
    webp_or(&words[wi], v << sh);
    if (sh + n > 32u) webp_or(&words[wi + 1], v >> (32u - sh));       // (then sh >= 1)
}
// word j of the `nwords` an item has put together, into the file (a region of `out_words` zeroed dwords; the payload
// starts at dword 5): the item's first and last dword may be shared with its neighbours and are ORed, the others are its own
IMP_WEBP_HD void webp_emit_store(uint32_t* out32, uint32_t out_words, uint64_t off, uint32_t j, uint32_t nwords, uint32_t v) {
    const uint64_t at = 5u + (off >> 5) + j;
    if (at >= out_words) return;
    if (j == 0 || j + 1u == nwords) webp_or(&out32[at], v);
    else out32[at] = v;
}
IMP_WEBP_HD uint32_t webp_emit_words(uint64_t off, uint32_t bits) { return bits ? (uint32_t)(((off & 31u) + bits + 31u) >> 5) : 0u; }

// ---------------------------------------------------------------- PARSE (IMPGPU_WEBP_ENC_BACKREFS)
// candidate k = 1 .. 24: the k-th entry of VP8L's distance map as a distance in a frame `w` wide (below 1: usable nowhere)
IMP_WEBP_HD int webp_lz_distance(int k, int w) {
    const int8_t xi[WEBP_LZ_CANDS] = {0, 1, 1, -1, 0, 2, 1, -1, 2, -2, 2, -2, 0, 3, 1, -1, 3, -3, 2, -2, 3, -3, 0, 4};
    const int8_t yi[WEBP_LZ_CANDS] = {1, 0, 1, 1, 2, 0, 2, 2, 1, 1, 2, 2, 3, 0, 3, 3, 1, 1, 3, 3, 2, 2, 4, 0};
    return xi[k - 1] + yi[k - 1] * w;
}
// VP8L's prefix coding of a value v >= 1 (a length, a plane code): the symbol, its extra bits and their count
IMP_WEBP_HD void webp_lz_prefix(uint32_t v, uint32_t* sym, uint32_t* extra, uint32_t* nbits) {
    if (v <= 4u) { *sym = v - 1u; *extra = 0u; *nbits = 0u; return; }
    const uint32_t u = v - 1u, hb = 31u - (uint32_t)__builtin_clz(u);
    *sym = 2u * hb + ((u >> (hb - 1u)) & 1u);
    *nbits = hb - 1u;
    *extra = u & ((1u << (hb - 1u)) - 1u);
}
// position p of the plane (of the item that ends at e) under distance d: does it repeat the residual d positions back?
IMP_WEBP_HD bool webp_lz_equal(const uint32_t* resid, uint32_t p, uint32_t e, int d) {
    return p < e && d >= 1 && (uint32_t)d <= p && resid[p] == resid[p - (uint32_t)d];
}
// skip[j], j = 0 .. 32: the first of a candidate's 32 words `eq` at or after j that has a zero bit; 32: none
IMP_WEBP_HD void webp_lz_skips(const uint32_t* eq, uint8_t* skip) {
    skip[32] = 32;
    for (int j = 31; j >= 0; j--) skip[j] = eq[j] != 0xffffffffu ? (uint8_t)j : skip[j + 1];
}
// the match at position i < 1024 of the item: the distance to the next zero bit at or after i (the bits of positions past
// the item's end are zero)
IMP_WEBP_HD uint32_t webp_lz_length(const uint32_t* eq, const uint8_t* skip, uint32_t i) {
    const uint32_t j = i >> 5, z = ~eq[j] >> (i & 31u);
    if (z) return (uint32_t)__builtin_ctz(z);
    const uint32_t j2 = skip[j + 1u];
    if (j2 >= 32u) return WEBP_ITEM - i;
    return j2 * 32u - i + (uint32_t)__builtin_ctz(~eq[j2]);
}
// the token of a position whose longest match is `best` under candidate k (the lowest k of that length)
IMP_WEBP_HD uint32_t webp_lz_token(uint32_t best, uint32_t k) { return best >= (uint32_t)IMPGPU_WEBP_MIN_MATCH ? best | k << 16 : WEBP_TOK_LITERAL; }
IMP_WEBP_HD uint32_t webp_lz_step(uint32_t tok) { return tok == WEBP_TOK_LITERAL ? 1u : tok & 0xffffu; }
// a token (of residual r) into the histograms: `lz` as WebpLz::hist, `rba` the red, blue and alpha bins (WebpWork::hist[1]..),
// `extra` a count of extra bits
IMP_WEBP_HD void webp_lz_count(uint32_t tok, uint32_t r, uint32_t* lz, uint32_t* rba, uint32_t* extra) {
    if (tok == WEBP_TOK_LITERAL) {
        webp_add(&lz[(r >> 8) & 255u], 1u);
        webp_add(&rba[0 * 256 + ((r >> 16) & 255u)], 1u);
        webp_add(&rba[1 * 256 + (r & 255u)], 1u);
        webp_add(&rba[2 * 256 + (r >> 24)], 1u);
        return;
    }
    uint32_t ls, lx, ln, ds, dx, dn;
    webp_lz_prefix(tok & 0xffffu, &ls, &lx, &ln);
    webp_lz_prefix(tok >> 16, &ds, &dx, &dn);
    webp_add(&lz[256u + ls], 1u);
    webp_add(&lz[WEBP_LZ_GREEN + ds], 1u);
    if (ln + dn) webp_add(extra, ln + dn);
}
// webp_symbol with a token plane: a covered position is no bits, a literal its four symbols with green from the 280-entry
// table, a reference the length's symbol, its extra bits, the distance's symbol, its extra bits.  `lztab` as WebpLz::tab
IMP_WEBP_HD uint32_t webp_symbol_lz(uint32_t kind, uint32_t k, uint32_t i, const WebpWork* W, const uint32_t* tab, const uint32_t* lztab, const uint8_t* modes,
                                    const uint32_t* resid, const uint32_t* tok, uint32_t* code, uint32_t* len) {
    if (kind != WEBP_IT_PIXELS) return webp_symbol(kind, k, i, W, tab, modes, resid, code, len);
    const uint32_t t = tok[(size_t)k * WEBP_ITEM + i];
    code[0] = code[1] = code[2] = code[3] = 0u;
    len[0] = len[1] = len[2] = len[3] = 0u;
    if (t == 0u) return 0u;
    if (t == WEBP_TOK_LITERAL) {
        const uint32_t r = resid[(size_t)k * WEBP_ITEM + i];
        const uint32_t t0 = lztab[(r >> 8) & 255u], t1 = tab[256 + ((r >> 16) & 255u)], t2 = tab[512 + (r & 255u)], t3 = tab[768 + (r >> 24)];
        code[0] = t0 & 0xffffu; len[0] = t0 >> 16;
        code[1] = t1 & 0xffffu; len[1] = t1 >> 16;
        code[2] = t2 & 0xffffu; len[2] = t2 >> 16;
        code[3] = t3 & 0xffffu; len[3] = t3 >> 16;
    } else {
        uint32_t ls, ds;
        webp_lz_prefix(t & 0xffffu, &ls, &code[1], &len[1]);
        webp_lz_prefix(t >> 16, &ds, &code[3], &len[3]);
        const uint32_t t0 = lztab[256u + ls], t2 = lztab[WEBP_LZ_GREEN + ds];
        code[0] = t0 & 0xffffu; len[0] = t0 >> 16;
        code[2] = t2 & 0xffffu; len[2] = t2 >> 16;
    }
    return len[0] + len[1] + len[2] + len[3];
}
// PARSE on one thread: item k of a plane of npix residuals, as k_webp_parse does it -- the candidates' equality words, the
// lengths from them -- but walking from token to token instead of marking the reachable positions.  `tok` starts zeroed.
inline void webp_parse_item_host(const uint32_t* resid, uint32_t npix, int w, uint32_t k, uint32_t* tok, WebpWork* W, WebpLz* L) {
    const uint32_t s = k * WEBP_ITEM, e = npix - s < WEBP_ITEM ? npix : s + WEBP_ITEM;
    uint32_t eq[WEBP_LZ_CANDS][32];
    uint8_t skip[WEBP_LZ_CANDS][33];
    for (int c = 0; c < WEBP_LZ_CANDS; c++) {
        const int d = webp_lz_distance(c + 1, w);
        for (uint32_t j = 0; j < 32u; j++) {
            uint32_t bits = 0;
            for (uint32_t b = 0; b < 32u; b++) bits |= (uint32_t)webp_lz_equal(resid, s + j * 32u + b, e, d) << b;
            eq[c][j] = bits;
        }
        webp_lz_skips(eq[c], skip[c]);
    }
    uint32_t extra = 0;
    for (uint32_t i = 0; s + i < e;) {
        uint32_t best = 0, bk = 0;
        for (int c = 0; c < WEBP_LZ_CANDS; c++) {
            const uint32_t n = webp_lz_length(eq[c], skip[c], i);
            if (n > best) { best = n; bk = (uint32_t)c + 1u; }         // a tie stays with the lowest k
        }
        const uint32_t t = webp_lz_token(best, bk);
        tok[s + i] = t;
        webp_lz_count(t, resid[s + i], L->hist, &W->hist[1][0], &extra);
        i += webp_lz_step(t);
    }
    L->extra_bits += extra;
}

// ---------------------------------------------------------------- impgpu_webp_encode_host: the lanes one after the other
inline int webp_encode_host(const unsigned char* frame, int width, int height, int channels, int step, const unsigned char* forced_modes,
                            unsigned char* out, size_t capacity, size_t* length, int flags = 0) {
    if (length) *length = 0;
    if (!frame || !length || (flags & ~IMPGPU_WEBP_ENC_BACKREFS)) return IMP_ERROR_INVALID_ARGS;
    const bool lz = (flags & IMPGPU_WEBP_ENC_BACKREFS) != 0;
    if (int rc = webp_check_geometry(width, height, channels)) return rc;
    if ((long long)step < (long long)width * channels) return IMP_ERROR_INVALID_ARGS;
    const int tb = IMPGPU_WEBP_TILE_BITS, tiles_x = webp_tiles(width, tb), tiles_y = webp_tiles(height, tb);
    const uint32_t ntiles = (uint32_t)tiles_x * (uint32_t)tiles_y, npix = (uint32_t)width * (uint32_t)height;
    if (forced_modes)
        for (uint32_t t = 0; t < ntiles; t++)
            if (forced_modes[t] >= WEBP_MODES) return IMP_ERROR_INVALID_ARGS;
    const WebpFrame f{frame, width, height, channels, step};
    std::vector<WebpWork> work(1);
    WebpWork* W = work.data();
    memset(W->hist, 0, sizeof(W->hist));
    W->alpha_seen = 0;
    std::vector<uint8_t> modes(ntiles);
    for (uint32_t t = 0; t < ntiles; t++) {                            // MODES
        uint32_t cost[WEBP_MODES] = {0};
        for (int lane = 0; lane < 64; lane++)
            if (webp_tile_costs_lane(f, tb, (int)(t % (uint32_t)tiles_x), (int)(t / (uint32_t)tiles_x), lane, 64, cost)) W->alpha_seen = 1;
        modes[t] = forced_modes ? forced_modes[t] : (uint8_t)webp_pick_mode(cost);
        W->hist[WEBP_CODE_MODES][modes[t]]++;
    }
    std::vector<uint32_t> resid(npix);
    for (uint32_t p = 0; p < npix; p++) {                              // RESID
        resid[p] = webp_residual_at(f, modes.data(), tb, tiles_x, p);
        if (!lz) webp_count(&W->hist[0][0], resid[p]);
    }
    std::vector<WebpLz> lzwork(lz ? 1 : 0);
    std::vector<uint32_t> tok(lz ? npix : 0u, 0u);
    WebpLz* L = lz ? lzwork.data() : nullptr;
    if (lz) {
        for (uint32_t k = 0; k < webp_item_count(npix); k++) webp_parse_item_host(resid.data(), npix, width, k, tok.data(), W, L);   // PARSE
        for (int k = 0; k <= WEBP_CODES; k++) webp_code_lane_lz(W, L, k);
    } else {
        for (int k = 0; k < WEBP_CODES; k++) webp_code_lane(W, k);     // CODES
    }
    WebpRec rec{};
    uint32_t riff[5];
    webp_headers(W, width, height, channels, tb, &rec, riff, L);
    *length = (size_t)rec.file_len;
    if (rec.file_len > capacity || !out) return IMP_ERROR_MALLOC_FAILED;
    const uint32_t out_words = (uint32_t)((rec.file_len + 3u) / 4u);
    std::vector<uint32_t> file(out_words, 0u), words((size_t)WEBP_EMIT_WORDS);
    for (int i = 0; i < 5; i++) file[(size_t)i] = riff[i];
    uint64_t off = 0;
    const uint32_t kinds[4] = {WEBP_IT_HDR_A, WEBP_IT_MODES, WEBP_IT_HDR_B, WEBP_IT_PIXELS};
    const uint32_t counts[4] = {1u, webp_item_count(ntiles), 1u, webp_item_count(npix)};
    for (int q = 0; q < 4; q++)
        for (uint32_t k = 0; k < counts[q]; k++) {                     // ITEMS: measured and put together in one go
            const uint32_t ns = webp_item_symbols(kinds[q], k, W, ntiles, npix);
            std::fill(words.begin(), words.end(), 0u);
            uint32_t bits = 0;
            for (uint32_t i = 0; i < ns; i++) {
                uint32_t code[4], len[4];
                if (lz) webp_symbol_lz(kinds[q], k, i, W, &W->tab[0][0], L->tab, modes.data(), resid.data(), tok.data(), code, len);
                else webp_symbol(kinds[q], k, i, W, &W->tab[0][0], modes.data(), resid.data(), code, len);
                for (int part = 0; part < 4; part++) {
                    webp_emit_put(words.data(), (uint32_t)(off & 31u) + bits, code[part], len[part]);
                    bits += len[part];
                }
            }
            const uint32_t nw = webp_emit_words(off, bits);
            for (uint32_t j = 0; j < nw; j++) webp_emit_store(file.data(), out_words, off, j, nw, words[j]);
            off += bits;
        }
    if (off != rec.payload_bits) return IMP_ERROR_DEVICE;              // (the histograms and the stream disagree: never)
    memcpy(out, file.data(), (size_t)rec.file_len);
    return IMP_OK;
}

}  // namespace imp
