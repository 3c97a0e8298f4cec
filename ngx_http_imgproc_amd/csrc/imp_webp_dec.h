// imp_webp_dec.h -- lossless WebP (VP8L) in: the lanes' logic, shared by the kernels of imp_webp_dec.hip, by the host front
// (imp_webp_dec_host.h reads everything in front of the main image's pixel stream with these same functions) and by the
// host model impgpu_webp_decode_host, which runs the same rounds one lane after the other (and under the sanitizers,
// tests/c/webp_dec_test.cpp).  Depends on nothing but <stdint.h>: every function here is __host__ __device__.
//
// An entropy-coded image (WdImage: the main image, or on the host one of the small sub-images between the headers) is
// decoded by ONE wavefront in ROUNDS:
//   1. the wave stages WD_IN_WORDS words of the compressed bytes, from the word the next bit lies in (wd_stage: nothing
//      at or past in_size is kept, nothing at or past in_cap is read);
//   2. symbols are decoded (wd_decode; wave-uniform: every lane computes the same, lane 0 writes) into a token list -- a
//      literal ARGB, a colour-cache key, or length + distance with their extra bits added and the distance already
//      mapped to pixels -- with every token's pixel position, until the list is full, the staged words run low, the
//      image is complete, the token's pixel lies in a tile of another prefix-code group (the wave then loads that
//      group's five codes, wd_group_load, and goes on in the same round) or something is wrong with the next token;
//   3. the tokens are emitted into the plane in global memory IN TOKEN ORDER, a run of tokens that are not matches at a
//      time (wd_emit_run: side by side, one lane per token, in a file without a colour cache; by lane 0, which also
//      keeps the cache, in a file with one -- a cache token's colour is whatever its slot holds at that moment), then
//      the match behind the run by the whole wave (wd_emit_copy: lane j writes pixels j, j + 64, ... reading pixel
//      j mod distance of the source, which lies before the match -- written by an earlier step, never by this one;
//      there is no ring: a match may reach back to the first pixel, so the source is the plane itself).  With a cache
//      the copied pixels enter it behind the copy: every lane stamps its pixels' slots with their positions
//      (wd_cache_stamp: the largest position wins, as the last insertion does) and the winners write (wd_cache_put).
// Between two steps whose second reads what the first stored the device puts a workgroup barrier (the kernel says why
// that orders global stores before loads); the host runs the lanes of a step one after the other.
//
// A prefix code is built by the whole wave (wd_build_*, after inf_build_*): lane l counts the symbols of length l, the
// counts are scanned and JUDGED by libwebp's rules (no symbol at all: refused; exactly one symbol of length 1..14: a
// code of ZERO bits whatever else has length 15; otherwise the code must be exactly complete -- over-subscribed and
// incomplete codes are refused), lane l writes the symbols of length l in order, the lanes fill the 10-bit lookup table.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IMP_WD_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IMP_WD_HD inline
#endif

namespace imp {

// A value every lane holds alike, read from memory: on the device it is moved to a scalar register, so that what is
// computed from it (the bit buffer, the table indices) runs on the scalar unit; on the host it is the value.
IMP_WD_HD uint32_t wd_uniform(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
#else
    return v;
#endif
}

enum : int { WD_OK = 0, WD_DAMAGED = 1, WD_SHORT = 2 };     // a file's status word; anything but 0 is IMP_ERROR_DECODE_FAILED
constexpr int WD_LANES = 64;
constexpr int WD_IN_WORDS = 512;                            // staged per round
constexpr int WD_TOKENS = 512;
constexpr int WD_FAST = 10;                                 // bits of a code's direct-lookup table
constexpr int WD_MAX_SIDE = 16384;                          // the format's own limit (14 bits)
constexpr uint32_t WD_MAX_PIXELS = 1u << 26;                // what a file may hold here (IMPGPU_WEBP_DEC_MAX_PIXELS)
constexpr int WD_GREEN = 256 + 24, WD_DIST = 40, WD_CODES = 5;
constexpr int WD_MAX_CACHE_BITS = 11;
constexpr uint16_t WD_T_LITERAL = 0, WD_T_CACHE = 0xffffu;  // tlen[]: these, or a match's length (1..4096)
// the feature word (info[0] of impgpu_webp_decode_host; IMPGPU_WEBP_DEC_F_* in impgpu.h)
enum : uint32_t {
    WD_F_PREDICTOR = 1u << 0, WD_F_COLOR = 1u << 1, WD_F_SUB_GREEN = 1u << 2, WD_F_INDEXING = 1u << 3,
    WD_F_CACHE = 1u << 4, WD_F_GROUPS = 1u << 5, WD_F_BACKREF = 1u << 6, WD_F_SIMPLE = 1u << 7,
    WD_F_DIST_ABOVE_24 = 1u << 8, WD_F_DIST_CLAMPED = 1u << 9,
    WD_F_BUNDLE_0 = 1u << 10,                                // << width bits: 0 none, 1 two, 2 four, 3 eight pixels a value
    WD_F_ALL = (1u << 14) - 1u,
};
enum : int { WD_TR_PREDICTOR = 0, WD_TR_COLOR = 1, WD_TR_SUB_GREEN = 2, WD_TR_INDEXING = 3 };

// one canonical prefix code: per length the count, the first code, where its symbols start in its sorted[] and the
// left-aligned (15-bit) limit below which a 15-bit peek belongs to a code of at most that length; the lookup table
// (symbol << 4 | length, 0: not a code of at most WD_FAST bits)
struct WdCode {
    uint16_t count[16], first[16], offs[16], lim[16];
    uint16_t fast[1 << WD_FAST];
    int32_t single;                      // >= 0: the code of zero bits for this symbol; -2 between scan and fill
    uint32_t nsym;
    uint32_t ok, pad;
};

// What one image's wave works on.  In LDS on the device (about 34 KB), an ordinary object on the host.
struct WdMem {
    uint32_t in[WD_IN_WORDS];
    uint32_t tval[WD_TOKENS];            // literal: ARGB; cache token: the key; match: the distance in pixels
    uint32_t tpos[WD_TOKENS];            // the token's first pixel
    uint16_t tlen[WD_TOKENS];
    uint32_t cache[1 << WD_MAX_CACHE_BITS];
    uint32_t stamp[1 << WD_MAX_CACHE_BITS];   // position + 1 of the last copied pixel that claimed the slot
    WdCode g[WD_CODES];                  // the loaded group: green, red, blue, alpha, distance
};

// an entropy-coded image.  `in` is 4-byte aligned and in_cap (a multiple of 4, >= in_size) bytes of it may be read
struct WdImage {
    const uint8_t* in;
    uint32_t in_size, in_cap;
    int w, h;
    uint32_t npix;
    int cache_bits;                      // 0: none
    int meta_bits, meta_w;               // meta_bits 0: one group
    const uint32_t* meta;                // the entropy image: group = (pixel >> 8) & 0xffff
    const WdCode* codes;                 // [ngroups][WD_CODES]
    const uint16_t* sorted;              // [ngroups][sorted_stride]: green_n | 256 | 256 | 256 | 40
    uint32_t sorted_stride, green_n, ngroups;
    uint32_t* out;                       // npix pixels
};

struct WdState {                         // wave-uniform: the decoder between two rounds
    uint64_t bitpos;
    uint32_t pos;
    int status, done, group;
    uint32_t feat;
};
struct WdBits {                          // wave-uniform: the bit reader over `nw` words; a word past them reads as zero
    const uint32_t* w;
    int nw, widx, bn;                    // widx: words moved into bb
    uint32_t nx;                         // w[widx], read ahead: a refill never waits for its word
    uint64_t bb, base;                   // base: stream bit offset of w[0]
};
struct WdRound {                         // wave-uniform: what a round decoded
    uint32_t pos;                        // behind the last token
    int ntok, err, want;                 // want: the group of the token that comes next
    uint64_t bitpos;
};

IMP_WD_HD uint32_t wd_rev15(uint32_t x) {
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
    x = ((x & 0x00ffu) << 8) | ((x >> 8) & 0x00ffu);
    return (x >> 1) & 0x7fffu;
}
IMP_WD_HD int wd_sub_size(int size, int bits) { return (size + (1 << bits) - 1) >> bits; }
IMP_WD_HD uint32_t wd_green_n(int cache_bits) { return (uint32_t)WD_GREEN + (cache_bits ? 1u << cache_bits : 0u); }
IMP_WD_HD uint32_t wd_sorted_stride(int cache_bits) { return wd_green_n(cache_bits) + 3u * 256u + (uint32_t)WD_DIST; }
IMP_WD_HD uint32_t wd_alphabet(int k, int cache_bits) { return k == 0 ? wd_green_n(cache_bits) : k == 4 ? (uint32_t)WD_DIST : 256u; }
IMP_WD_HD uint32_t wd_sorted_at(int k, int cache_bits) { return k == 0 ? 0u : wd_green_n(cache_bits) + 256u * (uint32_t)(k - 1); }

// ---------------------------------------------------------------- bits
IMP_WD_HD void wd_refill(WdBits* b) {
    if (b->bn <= 32) {
        b->bb |= (uint64_t)b->nx << b->bn;
        b->bn += 32;
        b->widx++;
        b->nx = b->widx < b->nw ? wd_uniform(b->w[b->widx]) : 0u;
    }
}
IMP_WD_HD uint32_t wd_take(WdBits* b, int n) {              // n <= 32, after a refill
    const uint32_t v = (uint32_t)(b->bb & ((1ull << n) - 1ull));
    b->bb >>= n;
    b->bn -= n;
    return v;
}
IMP_WD_HD uint32_t wd_read(WdBits* b, int n) { wd_refill(b); return wd_take(b, n); }
IMP_WD_HD uint64_t wd_bits_pos(const WdBits& b) { return b.base + (uint64_t)b.widx * 32u - (uint64_t)b.bn; }
// the reader at stream bit `bitpos` (>= base)
IMP_WD_HD void wd_bits_begin(WdBits* b, const uint32_t* words, int nw, uint64_t base, uint64_t bitpos) {
    b->w = words; b->nw = nw;
    b->bb = 0; b->bn = 0;
    b->base = base;
    b->widx = (int)((bitpos - base) >> 5);
    b->nx = b->widx < b->nw ? wd_uniform(b->w[b->widx]) : 0u;
    wd_refill(b);
    (void)wd_take(b, (int)((bitpos - base) & 31u));
}

// Step 1, lane `lane`'s words: in[] from the word that holds bit `bitpos`; a byte at or past in_size reads as zero
IMP_WD_HD void wd_stage(WdMem* m, const WdImage& im, uint64_t bitpos, int lane) {
    const uint32_t w0 = (uint32_t)(bitpos >> 5);
    for (int k = lane; k < WD_IN_WORDS; k += WD_LANES) {
        const uint64_t off = ((uint64_t)w0 + (uint64_t)k) * 4u;
        uint32_t w = 0;
        if (off + 4u <= (uint64_t)im.in_cap) {
            w = ((const uint32_t*)im.in)[w0 + (uint32_t)k];
            if (off + 4u > (uint64_t)im.in_size) {
                const uint32_t keep = off < (uint64_t)im.in_size ? im.in_size - (uint32_t)off : 0u;
                w = keep ? (w & ((1u << (8u * keep)) - 1u)) : 0u;
            }
        }
        m->in[k] = w;
    }
}

// One symbol of code `c` from the next 15 bits (`peek`, the stream's first bit in bit 0), or -1
IMP_WD_HD int wd_sym(const WdCode* c, const uint16_t* sorted, uint32_t peek, int* len) {
    const uint32_t e = wd_uniform(c->fast[peek & ((1u << WD_FAST) - 1u)]);    // (both reads before the first use: one wait)
    const int single = (int)wd_uniform((uint32_t)c->single);
    if (single >= 0) { *len = 0; return single; }
    if (e) { *len = (int)(e & 15u); return (int)(e >> 4); }
    const uint32_t v = wd_rev15(peek);
    for (int l = WD_FAST + 1; l <= 15; l++) {
        if (v < wd_uniform(c->lim[l])) {
            const uint32_t idx = wd_uniform((uint32_t)c->offs[l] + (v >> (15 - l)) - (uint32_t)c->first[l]), n = wd_uniform(c->nsym);
            *len = l;
            return (int)wd_uniform(sorted[idx < n ? idx : n - 1u]);
        }
    }
    return -1;
}
IMP_WD_HD int wd_read_sym(WdBits* b, const WdCode* c, const uint16_t* sorted) {
    wd_refill(b);
    int l = 0;
    const int s = wd_sym(c, sorted, (uint32_t)b->bb & 0x7fffu, &l);
    if (s >= 0) (void)wd_take(b, l);
    return s;
}

// ---------------------------------------------------------------- a code built by the whole wave from n code lengths
IMP_WD_HD void wd_build_count(WdCode* c, const uint8_t* lens, int n, int lane) {
    if (lane < 16) {
        int cnt = 0;
        for (int i = 0; i < n; i++) cnt += lens[i] == lane ? 1 : 0;
        c->count[lane] = (uint16_t)cnt;
    }
    for (int i = lane; i < (1 << WD_FAST); i += WD_LANES) c->fast[i] = 0;
}
// scan and verdict (wave-uniform; lane 0 writes): false = refused
IMP_WD_HD bool wd_build_scan(WdCode* c, int n, int lane) {
    int left = 1, used14 = 0;
    bool ok = true;
    uint32_t code = 0, off = 0;
    for (int l = 1; l <= 15; l++) {
        const int cnt = c->count[l];
        left = (left << 1) - cnt;
        if (left < 0) { ok = false; left = 0; }
        if (l < 15) used14 += cnt;
        if (lane == 0) {
            c->first[l] = (uint16_t)code;
            c->offs[l] = (uint16_t)off;
            c->lim[l] = (uint16_t)(ok ? (code + (uint32_t)cnt) << (15 - l) : 0u);
        }
        code = (code + (uint32_t)cnt) << 1;
        off += (uint32_t)cnt;
    }
    const bool none = (int)c->count[0] == n;
    const bool single = !none && used14 == 1;
    if (single) ok = true;
    else if (none || left != 0) ok = false;
    if (lane == 0) {
        c->single = single && ok ? -2 : -1;
        c->nsym = (uint32_t)n;
        c->ok = ok ? 1u : 0u;
        c->pad = 0;
    }
    return ok;
}
IMP_WD_HD void wd_build_sort(const WdCode* c, const uint8_t* lens, int n, uint16_t* sorted, int lane) {
    if (lane < 1 || lane > 15) return;
    uint32_t k = c->offs[lane];
    for (int i = 0; i < n; i++)
        if (lens[i] == lane && k < (uint32_t)n) sorted[k++] = (uint16_t)i;
}
IMP_WD_HD void wd_build_fill(WdCode* c, const uint16_t* sorted, int lane) {
    if (c->single == -2) {
        if (lane == 0) c->single = (int32_t)sorted[0];
        return;
    }
    const int used = (int)c->offs[WD_FAST + 1];                  // the symbols of at most WD_FAST bits
    for (int p = lane; p < used; p += WD_LANES) {
        int l = 1;
        while (l < WD_FAST && p >= (int)c->offs[l] + (int)c->count[l]) l++;
        const uint32_t code = (uint32_t)c->first[l] + (uint32_t)(p - (int)c->offs[l]);
        const uint32_t rev = wd_rev15(code << (15 - l));
        const uint16_t e = (uint16_t)(((uint32_t)sorted[p] << 4) | (uint32_t)l);
        for (uint32_t i = rev; i < (1u << WD_FAST); i += 1u << l) c->fast[i] = e;
    }
}

// ---------------------------------------------------------------- values
// the prefix coding of lengths and distances: symbol -> value, its extra bits read
IMP_WD_HD uint32_t wd_prefix_value(WdBits* b, int sym) {
    if (sym < 4) return (uint32_t)sym + 1u;
    const int eb = (sym - 2) >> 1;
    const uint32_t off = (2u + ((uint32_t)sym & 1u)) << eb;
    return off + wd_read(b, eb) + 1u;
}
// The distance map: codes 1..120 name a neighbour (xi, yi) -- xi columns to the left, yi rows up -- in this order (the
// specification's list), here as xi + 7 | yi << 4; the distance is xi + yi * width, and below 1 it is 1.  Codes above
// 120 are the distance + 120.
IMP_WD_HD uint32_t wd_distance(uint32_t code, int width, bool* clamped) {
    const uint8_t nb[120] = {
        23, 8, 24, 22, 39, 9, 40, 38, 25, 21, 41, 37, 55, 10, 56, 54, 26, 20, 57, 53, 42, 36, 71, 11, 72, 70, 27, 19, 58, 52,
        73, 69, 43, 35, 87, 74, 68, 59, 51, 12, 88, 86, 28, 18, 89, 85, 44, 34, 75, 67, 90, 84, 60, 50, 103, 13, 104, 102, 29, 17,
        105, 101, 45, 33, 91, 83, 76, 66, 106, 100, 61, 49, 119, 14, 120, 118, 92, 82, 30, 16, 107, 99, 77, 65, 121, 117, 46, 32, 122, 116,
        62, 48, 108, 98, 93, 81, 15, 123, 115, 78, 64, 31, 47, 109, 97, 63, 124, 114, 94, 80, 79, 125, 113, 110, 96, 95, 126, 112, 111, 127};
    *clamped = false;
    if (code > 120u) return code - 120u;
    const int e = nb[code - 1u];
    const int d = ((e & 15) - 7) + (e >> 4) * width;
    if (d < 1) { *clamped = true; return 1u; }
    return (uint32_t)d;
}
IMP_WD_HD uint32_t wd_hash(uint32_t argb, int bits) { return (argb * 0x1e35a7bdu) >> (32 - bits); }

// ---------------------------------------------------------------- the rounds
IMP_WD_HD void wd_start(WdState* s, const WdImage& im, uint64_t bitpos) {
    s->bitpos = bitpos;
    s->pos = 0;
    s->status = WD_OK; s->done = 0; s->group = -1;
    s->feat = 0;
    if (bitpos > (uint64_t)im.in_size * 8u) { s->status = WD_SHORT; s->done = 1; }
}
// lane `lane`'s part of clearing the cache (once, before the first round)
IMP_WD_HD void wd_cache_clear(WdMem* m, int lane) {
    for (int i = lane; i < (1 << WD_MAX_CACHE_BITS); i += WD_LANES) { m->cache[i] = 0; m->stamp[i] = 0; }
}
IMP_WD_HD void wd_round_begin(WdRound* r, const WdState& s) {
    r->pos = s.pos;
    r->ntok = 0; r->err = 0;
    r->want = s.group;
    r->bitpos = s.bitpos;
}
IMP_WD_HD uint32_t wd_group_at(const WdImage& im, uint32_t pos) {
    if (!im.meta_bits) return 0u;
    const uint32_t y = pos / (uint32_t)im.w, x = pos - y * (uint32_t)im.w;
    const uint32_t g = (wd_uniform(im.meta[(size_t)(y >> im.meta_bits) * (size_t)im.meta_w + (x >> im.meta_bits)]) >> 8) & 0xffffu;
    return g < im.ngroups ? g : im.ngroups - 1u;
}
// the first pixel behind `pos` that may belong to another group: the end of the tile's piece of the row
IMP_WD_HD uint32_t wd_group_end(const WdImage& im, uint32_t pos) {
    if (!im.meta_bits) return im.npix;
    const uint32_t y = pos / (uint32_t)im.w, x = pos - y * (uint32_t)im.w;
    const uint32_t xe = ((x >> im.meta_bits) + 1u) << im.meta_bits;
    return pos + ((xe < (uint32_t)im.w ? xe : (uint32_t)im.w) - x);
}
// lane `lane`'s words of group `g`'s five codes, into the wave's memory
IMP_WD_HD void wd_group_load(WdMem* m, const WdImage& im, int g, int lane) {
    const uint32_t* src = (const uint32_t*)(im.codes + (size_t)g * WD_CODES);
    uint32_t* dst = (uint32_t*)m->g;
    for (int i = lane; i < (int)(sizeof(WdCode) * WD_CODES / 4u); i += WD_LANES) dst[i] = src[i];
}

// Step 2.  Wave-uniform; lane 0 writes the list.  Goes on from r->pos / r->ntok with group s->group loaded; stops with
// r->want != s->group where the next token belongs to another group.
IMP_WD_HD void wd_decode(WdMem* m, const WdImage& im, WdState* s, WdBits* b, WdRound* r, int lane) {
    uint32_t pos = r->pos;
    int ntok = r->ntok;
    const uint64_t in_bits = (uint64_t)im.in_size * 8u;
    const uint16_t* srt = im.sorted + (size_t)(s->group < 0 ? 0 : s->group) * im.sorted_stride;
    const uint32_t gn = im.green_n;
    uint32_t gend = 0;
    for (;;) {
        r->bitpos = wd_bits_pos(*b);
        if (pos >= im.npix) break;
        if (ntok >= WD_TOKENS || b->widx > WD_IN_WORDS - 4) break;
        if (pos >= gend) {                                   // a group holds to the end of its tile's piece of the row
            const int gi = (int)wd_group_at(im, pos);
            r->want = gi;
            if (gi != s->group) break;
            gend = wd_group_end(im, pos);
        }
        const int g = wd_read_sym(b, &m->g[0], srt);
        if (g < 0) { r->err = WD_DAMAGED; break; }
        uint32_t val, step = 1;
        uint16_t kind;
        if (g < 256) {
            const int red = wd_read_sym(b, &m->g[1], srt + gn);
            const int blue = wd_read_sym(b, &m->g[2], srt + gn + 256u);
            const int alpha = wd_read_sym(b, &m->g[3], srt + gn + 512u);
            if (red < 0 || blue < 0 || alpha < 0) { r->err = WD_DAMAGED; break; }
            val = (uint32_t)alpha << 24 | ((uint32_t)red & 255u) << 16 | (uint32_t)g << 8 | ((uint32_t)blue & 255u);
            kind = WD_T_LITERAL;
        } else if (g < WD_GREEN) {
            const uint32_t len = wd_prefix_value(b, g - 256);
            const int ds = wd_read_sym(b, &m->g[4], srt + gn + 768u);
            if (ds < 0 || ds >= WD_DIST) { r->err = WD_DAMAGED; break; }
            const uint32_t code = wd_prefix_value(b, ds);
            bool clamped = false;
            const uint32_t dist = wd_distance(code, im.w, &clamped);
            if (wd_bits_pos(*b) > in_bits) { r->err = WD_SHORT; break; }
            if (dist > pos || im.npix - pos < len) { r->err = WD_DAMAGED; break; }   // before the first pixel; past the image
            s->feat |= WD_F_BACKREF | (code > 24u ? WD_F_DIST_ABOVE_24 : 0u) | (clamped ? WD_F_DIST_CLAMPED : 0u);
            val = dist;
            kind = (uint16_t)len;
            step = len;
        } else {
            const uint32_t key = (uint32_t)g - (uint32_t)WD_GREEN;
            if (!im.cache_bits || key >= (1u << im.cache_bits)) { r->err = WD_DAMAGED; break; }
            val = key;
            kind = WD_T_CACHE;
        }
        if (wd_bits_pos(*b) > in_bits) { r->err = WD_SHORT; break; }
        if (lane == 0) { m->tval[ntok] = val; m->tpos[ntok] = pos; m->tlen[ntok] = kind; }
        ntok++;
        pos += step;
    }
    r->ntok = ntok;
    r->pos = pos;
}

// Step 3.  The first match at or behind token t0 (wave-uniform)
IMP_WD_HD int wd_run_end(const WdMem* m, int t0, int ntok) {
    int t = t0;
    while (t < ntok && (m->tlen[t] == WD_T_LITERAL || m->tlen[t] == WD_T_CACHE)) t++;
    return t;
}
IMP_WD_HD void wd_emit_run(WdMem* m, const WdImage& im, int t0, int t1, int lane) {
    if (!im.cache_bits) {
        for (int t = t0 + lane; t < t1; t += WD_LANES) im.out[m->tpos[t]] = m->tval[t];
        return;
    }
    if (lane != 0) return;
    for (int t = t0; t < t1; t++) {
        const uint32_t v = m->tlen[t] == WD_T_CACHE ? m->cache[m->tval[t] & ((1u << WD_MAX_CACHE_BITS) - 1u)] : m->tval[t];
        im.out[m->tpos[t]] = v;
        m->cache[wd_hash(v, im.cache_bits)] = v;
    }
}
IMP_WD_HD void wd_emit_copy(const WdMem* m, const WdImage& im, int t, int lane) {
    const uint32_t len = m->tlen[t], dist = m->tval[t], pos = m->tpos[t];
    if (!dist || dist > pos || len > im.npix - pos) return;
    for (uint32_t j = (uint32_t)lane; j < len; j += WD_LANES) {
        const uint32_t from = dist >= len ? j : j % dist;
        im.out[pos + j] = im.out[pos - dist + from];
    }
}
IMP_WD_HD void wd_cache_stamp(WdMem* m, const WdImage& im, int t, int lane) {
    const uint32_t len = m->tlen[t], pos = m->tpos[t];
    if (len > im.npix - pos) return;
    for (uint32_t j = (uint32_t)lane; j < len; j += WD_LANES) {
        const uint32_t h = wd_hash(im.out[pos + j], im.cache_bits), mine = pos + j + 1u;
#if defined(__HIP_DEVICE_COMPILE__)
        atomicMax(&m->stamp[h], mine);
#else
        if (m->stamp[h] < mine) m->stamp[h] = mine;
#endif
    }
}
IMP_WD_HD void wd_cache_put(WdMem* m, const WdImage& im, int t, int lane) {
    const uint32_t len = m->tlen[t], pos = m->tpos[t];
    if (len > im.npix - pos) return;
    for (uint32_t j = (uint32_t)lane; j < len; j += WD_LANES) {
        const uint32_t v = im.out[pos + j], h = wd_hash(v, im.cache_bits);
        if (m->stamp[h] == pos + j + 1u) m->cache[h] = v;
    }
}
IMP_WD_HD void wd_round_end(WdState* s, const WdImage& im, const WdRound& r) {
    s->pos = r.pos;
    s->bitpos = r.bitpos;
    if (r.err) { s->status = r.err; s->done = 1; return; }
    if (s->pos >= im.npix) { s->status = WD_OK; s->done = 1; }
}

// ---------------------------------------------------------------- the inverse transforms (lane `lane` of `nlanes`)
IMP_WD_HD uint32_t wd_add_px(uint32_t a, uint32_t b) {     // per channel a + b mod 256
    const uint32_t ag = (a & 0xff00ff00u) + (b & 0xff00ff00u), rb = (a & 0x00ff00ffu) + (b & 0x00ff00ffu);
    return (ag & 0xff00ff00u) | (rb & 0x00ff00ffu);
}
IMP_WD_HD void wd_inv_add_green(uint32_t* p, uint32_t npix, uint32_t lane, uint32_t nlanes) {
    for (uint32_t i = lane; i < npix; i += nlanes) {
        const uint32_t v = p[i], g = (v >> 8) & 255u;
        p[i] = (v & 0xff00ff00u) | (((v & 0x00ff00ffu) + (g << 16 | g)) & 0x00ff00ffu);
    }
}
IMP_WD_HD int wd_color_delta(uint32_t t, uint32_t c) { return ((int)(int8_t)t * (int)(int8_t)c) >> 5; }
IMP_WD_HD void wd_inv_color(uint32_t* p, int w, int h, int bits, const uint32_t* elems, uint32_t lane, uint32_t nlanes) {
    const int ew = wd_sub_size(w, bits);
    const uint32_t npix = (uint32_t)w * (uint32_t)h;
    for (uint32_t i = lane; i < npix; i += nlanes) {
        const uint32_t y = i / (uint32_t)w, x = i - y * (uint32_t)w;
        const uint32_t e = elems[(size_t)(y >> bits) * (size_t)ew + (x >> bits)];
        const uint32_t v = p[i], green = (v >> 8) & 255u;
        uint32_t red = (v >> 16) & 255u, blue = v & 255u;
        red = (red + (uint32_t)wd_color_delta(e & 255u, green)) & 255u;
        blue = (blue + (uint32_t)wd_color_delta((e >> 8) & 255u, green) + (uint32_t)wd_color_delta((e >> 16) & 255u, red)) & 255u;
        p[i] = (v & 0xff00ff00u) | red << 16 | blue;
    }
}
// colour indexing: `src` holds wd_sub_size(w, bits) values a row, 1 << bits indices in a value's green byte, the first
// in the low bits; an index past the palette gives 0
IMP_WD_HD void wd_inv_index(const uint32_t* src, uint32_t* dst, int w, int h, int bits, const uint32_t* pal, uint32_t ncolors, uint32_t lane,
                            uint32_t nlanes) {
    const uint32_t sw = (uint32_t)wd_sub_size(w, bits), npix = (uint32_t)w * (uint32_t)h;
    const uint32_t per = 8u >> bits, mask = (1u << per) - 1u;
    for (uint32_t i = lane; i < npix; i += nlanes) {
        const uint32_t y = i / (uint32_t)w, x = i - y * (uint32_t)w;
        const uint32_t v = (src[(size_t)y * sw + (x >> bits)] >> 8) & 255u;
        const uint32_t idx = (v >> ((x & ((1u << bits) - 1u)) * per)) & mask;
        dst[i] = idx < ncolors ? pal[idx] : 0u;
    }
}
IMP_WD_HD uint32_t wd_avg2(uint32_t a, uint32_t b) { return (((a ^ b) & 0xfefefefeu) >> 1) + (a & b); }
IMP_WD_HD int wd_ch(uint32_t p, int k) { return (int)((p >> (8 * k)) & 255u); }
IMP_WD_HD uint32_t wd_clamp(int v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }
IMP_WD_HD uint32_t wd_predict(int mode, uint32_t L, uint32_t T, uint32_t TL, uint32_t TR) {
    switch (mode) {
        case 1: return L;
        case 2: return T;
        case 3: return TR;
        case 4: return TL;
        case 5: return wd_avg2(wd_avg2(L, TR), T);
        case 6: return wd_avg2(L, TL);
        case 7: return wd_avg2(L, T);
        case 8: return wd_avg2(TL, T);
        case 9: return wd_avg2(T, TR);
        case 10: return wd_avg2(wd_avg2(L, TL), wd_avg2(T, TR));
        case 11: {                                           // Select: with p = L + T - TL, L when sum |p - L| < sum |p - T|
            int to_l = 0, to_t = 0;
            for (int k = 0; k < 4; k++) {
                const int dl = wd_ch(T, k) - wd_ch(TL, k), dt = wd_ch(L, k) - wd_ch(TL, k);
                to_l += dl < 0 ? -dl : dl;
                to_t += dt < 0 ? -dt : dt;
            }
            return to_l < to_t ? L : T;
        }
        case 12: {
            uint32_t r = 0;
            for (int k = 0; k < 4; k++) r |= wd_clamp(wd_ch(L, k) + wd_ch(T, k) - wd_ch(TL, k)) << (8 * k);
            return r;
        }
        case 13: {
            const uint32_t a = wd_avg2(L, T);
            uint32_t r = 0;
            for (int k = 0; k < 4; k++) {
                const int x = wd_ch(a, k);
                r |= wd_clamp(x + (x - wd_ch(TL, k)) / 2) << (8 * k);
            }
            return r;
        }
        default: return 0xff000000u;                         // 0, and the two values past 13 the four mode bits can hold
    }
}
// The predictor's inverse runs rows SKEWED: in a band of `nlanes` rows from row0, lane j works on row row0 + j and at
// step s on pixel x = s - 2 j, two pixels behind the lane above -- whose pixels through x + 1 (TR) an earlier step
// stored.  A band takes w + 2 (nlanes - 1) steps; in place: the residual at (x, y) becomes the pixel.
IMP_WD_HD int wd_pred_steps(int w, int nlanes) { return w + 2 * (nlanes - 1); }
constexpr int WD_INV_LANES = 256;                           // k_webp_dec_inverse's workgroup: a band is min(h, this) rows, on the host too
IMP_WD_HD void wd_inv_pred_step(uint32_t* p, int w, int h, int bits, const uint32_t* modes, int row0, int step, int lane) {
    const int y = row0 + lane, x = step - 2 * lane;
    if (y >= h || x < 0 || x >= w) return;
    uint32_t* row = p + (size_t)y * (size_t)w;
    uint32_t pred;
    if (y == 0) pred = x == 0 ? 0xff000000u : row[x - 1];
    else if (x == 0) pred = row[x - w];
    else {
        const int mode = (int)((modes[(size_t)(y >> bits) * (size_t)wd_sub_size(w, bits) + (size_t)(x >> bits)] >> 8) & 15u);
        const uint32_t TR = x + 1 < w ? row[x + 1 - w] : row[0];
        pred = wd_predict(mode, row[x - 1], row[x - w], row[x - 1 - w], TR);
    }
    row[x] = wd_add_px(row[x], pred);
}
// the frame: B,G,R,A bytes are the ARGB word's; A is 255 unless the header's alpha_is_used bit is set
IMP_WD_HD void wd_finish(const uint32_t* src, uint32_t* dst, uint32_t npix, int alpha_used, uint32_t lane, uint32_t nlanes) {
    const uint32_t force = alpha_used ? 0u : 0xff000000u;
    for (uint32_t i = lane; i < npix; i += nlanes) dst[i] = src[i] | force;
}

// what the inverse works through: the transforms in the order the file gives them (undone last to first)
struct WdTransform {
    int type, bits, xsize;               // xsize: the image's width when the transform was read
    uint32_t ncolors;
    long long data_off;                  // its sub-image (modes, elements) or its palette: an offset, or on the host an index
};

// ---------------------------------------------------------------- what the kernels read (imp_webp_dec.hip)
// a file of a group; the offsets are into the group's device block
struct WdFileDesc {
    long long in_off, lens_off, meta_off, codes_off, sorted_off, plane_off;
    uint8_t* img;                        // the frame: w * 4 bytes a row
    uint64_t bitpos;                     // of the main image's first symbol
    uint32_t in_size, in_cap, ngroups, pad;
    int w, h, cw, alpha_used, cache_bits, meta_bits, meta_w, ntrans;
    WdTransform tr[4];
};
struct WdCodeItem { int file; uint32_t group; int k, pad; };      // one wavefront of k_webp_dec_tables

// ---------------------------------------------------------------- the host's run of the rounds
inline bool wd_build_host(WdCode* c, const uint8_t* lens, int n, uint16_t* sorted) {
    for (int j = 0; j < WD_LANES; j++) wd_build_count(c, lens, n, j);
    const bool ok = wd_build_scan(c, n, 0);
    if (!ok) return false;
    for (int j = 0; j < WD_LANES; j++) wd_build_sort(c, lens, n, sorted, j);
    for (int j = 0; j < WD_LANES; j++) wd_build_fill(c, sorted, j);
    return true;
}

inline int wd_rounds_host(const WdImage& im, uint64_t bitpos, WdMem* m, uint32_t* feat, uint64_t* endbit, int* rounds = nullptr) {
    WdState s;
    wd_start(&s, im, bitpos);
    int nrounds = 0;
    for (int j = 0; j < WD_LANES; j++) wd_cache_clear(m, j);
    while (!s.done) {
        nrounds++;
        for (int j = 0; j < WD_LANES; j++) wd_stage(m, im, s.bitpos, j);
        WdBits b;
        wd_bits_begin(&b, m->in, WD_IN_WORDS, (s.bitpos >> 5) << 5, s.bitpos);
        WdRound r;
        wd_round_begin(&r, s);
        for (;;) {
            if (r.want != s.group) {
                for (int j = 0; j < WD_LANES; j++) wd_group_load(m, im, r.want, j);
                s.group = r.want;
            }
            wd_decode(m, im, &s, &b, &r, 0);
            if (r.want == s.group) break;
        }
        for (int t = 0; t < r.ntok;) {
            const int t1 = wd_run_end(m, t, r.ntok);
            for (int j = 0; j < WD_LANES; j++) wd_emit_run(m, im, t, t1, j);
            t = t1;
            if (t < r.ntok) {
                for (int j = 0; j < WD_LANES; j++) wd_emit_copy(m, im, t, j);
                if (im.cache_bits) {
                    for (int j = 0; j < WD_LANES; j++) wd_cache_stamp(m, im, t, j);
                    for (int j = 0; j < WD_LANES; j++) wd_cache_put(m, im, t, j);
                }
                t++;
            }
        }
        wd_round_end(&s, im, r);
    }
    *feat |= s.feat;
    *endbit = s.bitpos;
    if (rounds) *rounds = nrounds;
    return s.status;
}

}  // namespace imp
