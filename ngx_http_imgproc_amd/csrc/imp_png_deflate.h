// imp_png_deflate.h -- the deflate side of the PNG encoder (csrc/imp_png_enc.hip), written once for the device kernels and
// the host diagnostic impgpu_png_deflate.  What it reproduces is zlib 1.2.11 at strategy Z_RLE, windowBits 15, memLevel 8
// (what OpenCV 2.4.9's PngEncoder asks libpng 1.6 for), over a stream fed in one piece:
//
//   symbols   deflate_rle: at s > 0, when bytes s, s+1, s+2 all equal byte s-1, a match at distance 1 whose length is the
//             bytes from s equal to byte s-1 (at most 258, at most what is left); otherwise a literal.  For a maximal run of
//             L equal bytes that is one literal, then matches of min(m, 258) while m >= 3 (m = L - 1 to start), then m
//             literals: a pure function of the runs, so any segment of the stream can be coded by itself once it knows
//             where the runs that cross its edges begin and end (png_run_symbols).
//   blocks    one block per 16383 symbols (lit_bufsize - 1), and a final block with the rest (possibly none).
//   trees     trees.c: build_tree with the heap ordered by (frequency, depth) and replayed exactly (equal pairs are broken by
//             the heap's own layout), gen_bitlen's 15-bit repair, the bit-length tree (7 bits), send_all_trees' run codes,
//             _tr_flush_block's choice: stored when stored_len + 4 <= min(opt, static) in bytes, fixed when static <= opt.
//             A stored-worthy block is never slid out of the window: it spans at most ~20.5 KB of input (each literal costs
//             at most 9 bits of the static estimate, a match at least 12, stored costs 8 per byte), and a block leaves the
//             window only after spanning more than 32506 bytes -- so `buf` is never NULL where it matters.
#pragma once
#include <cstdint>

#ifndef IMP_HD
#define IMP_HD __host__ __device__
#endif

namespace imp {
namespace png {

constexpr int L_CODES = 286, D_CODES = 30, BL_CODES = 19, HEAP_SIZE = 2 * L_CODES + 1, MAX_BITS = 15, MAX_BL_BITS = 7;
constexpr int END_BLOCK = 256, BLOCK_SYMS = 16383;              // lit_bufsize - 1 at memLevel 8
constexpr int MAX_MATCH = 258;

IMP_HD inline int extra_lbits(int code) { return code < 8 ? 0 : code >= 28 ? 0 : (code - 4) >> 2; }
IMP_HD inline int base_length(int code) {                       // trees.c base_length[], code 28 (length 258) -> 0
    if (code >= 28) return 0;
    if (code < 8) return code;
    return (8 + 2 * ((code - 8) & 3)) << ((code - 8) >> 2);     // 8, 10, 12, 14 | 16, 20, 24, 28 | ... | 224
}
// _length_code[lc] for lc = length - 3 in 0..255
IMP_HD inline int length_code(int lc) {
    if (lc == 255) return 28;
    if (lc < 8) return lc;
    int code = 8;
    while (code < 27 && base_length(code + 1) <= lc) code++;
    return code;
}
IMP_HD inline int extra_blbits(int code) { return code == 16 ? 2 : code == 17 ? 3 : code == 18 ? 7 : 0; }
IMP_HD inline int static_llen(int n) { return n < 144 ? 8 : n < 256 ? 9 : n < 280 ? 7 : 8; }
IMP_HD inline unsigned bi_reverse(unsigned code, int len) {
    unsigned res = 0;
    do { res |= code & 1; code >>= 1; res <<= 1; } while (--len > 0);
    return res >> 1;
}
IMP_HD inline int bl_order(int i) {
    const uint8_t o[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    return o[i];
}

// One symbol as the coder stores it: bits 0-8 = literal / length symbol (0..285), 9-13 = extra value, 14-16 = extra bits.
IMP_HD inline uint32_t sym_literal(int byte) { return (uint32_t)byte; }
IMP_HD inline uint32_t sym_match(int len) {
    const int lc = len - 3, code = length_code(lc), xb = extra_lbits(code);
    return (uint32_t)(257 + code) | (uint32_t)(xb ? lc - base_length(code) : 0) << 9 | (uint32_t)xb << 14;
}

// The symbols of the run [a, b) (all bytes equal to `byte`) that start inside [lo, hi), in stream order: f(pos, sym).
template <class F>
IMP_HD inline void png_run_symbols(uint32_t a, uint32_t b, int byte, uint32_t lo, uint32_t hi, F&& f) {
    if (a >= lo && a < hi) f(a, sym_literal(byte));
    const uint32_t m = b - a - 1, q = m / MAX_MATCH, r = m % MAX_MATCH;
    // full matches at a + 1 + 258 j, j < q
    if (q) {
        uint32_t j = lo > a + 1 ? (lo - a - 1 + MAX_MATCH - 1) / MAX_MATCH : 0;
        for (; j < q; j++) {
            const uint32_t p = a + 1 + MAX_MATCH * j;
            if (p >= hi) return;
            f(p, sym_match(MAX_MATCH));
        }
    }
    const uint32_t t = a + 1 + MAX_MATCH * q;                   // the tail: one match of r >= 3, or r literals
    if (r >= 3) {
        if (t >= lo && t < hi) f(t, sym_match((int)r));
    } else {
        for (uint32_t p = t; p < b; p++)
            if (p >= lo && p < hi) f(p, sym_literal(byte));
    }
}

// Symbols in the run [a, b) that start inside [lo, hi): png_run_symbols without the calls.
IMP_HD inline uint32_t png_run_count(uint32_t a, uint32_t b, uint32_t lo, uint32_t hi) {
    uint32_t n = 0;
    if (a >= lo && a < hi) n++;
    const uint32_t m = b - a - 1, q = m / MAX_MATCH, r = m % MAX_MATCH;
    if (q) {
        // j in [j0, j1) with lo <= a + 1 + 258 j < hi
        const uint32_t j0 = lo > a + 1 ? (lo - a - 1 + MAX_MATCH - 1) / MAX_MATCH : 0;
        const uint32_t j1 = hi > a + 1 ? (hi - a - 1 + MAX_MATCH - 1) / MAX_MATCH : 0;
        const uint32_t e = j1 < q ? j1 : q;
        if (e > j0) n += e - j0;
    }
    const uint32_t t = a + 1 + MAX_MATCH * q;
    if (r >= 3) n += (t >= lo && t < hi);
    else {
        const uint32_t s = t > lo ? t : lo, e = b < hi ? b : hi;
        if (e > s) n += e - s;
    }
    return n;
}

// ---------------------------------------------------------------- trees.c
// A tree as trees.c keeps it: `fc` = Freq (Code after gen_codes is kept apart in `code`), `dl` = Dad, overwritten by Len
// in gen_bitlen -- the two share storage in zlib and gen_bitlen depends on it (a node reads its parent's Len).
struct TreeWork {
    int heap[HEAP_SIZE];
    uint8_t depth[HEAP_SIZE];
    uint16_t bl_count[MAX_BITS + 1];
    int heap_len, heap_max;
};
struct BlockTrees {
    uint32_t lf[HEAP_SIZE]; uint16_t ll[HEAP_SIZE]; uint16_t lcode[L_CODES + 1];
    uint32_t df[2 * D_CODES + 1]; uint16_t dlen[2 * D_CODES + 1]; uint16_t dcode[D_CODES + 1];
    uint32_t bf[2 * BL_CODES + 1]; uint16_t blen[2 * BL_CODES + 1]; uint16_t bcode[BL_CODES + 1];
    uint32_t opt_len, static_len;
    int lmax, dmax, max_blindex;
    TreeWork w;
};

IMP_HD inline bool tw_smaller(const uint32_t* f, int n, int m, const uint8_t* depth) {
    return f[n] < f[m] || (f[n] == f[m] && depth[n] <= depth[m]);
}
IMP_HD inline void pqdownheap(TreeWork& w, const uint32_t* f, int k) {
    const int v = w.heap[k];
    int j = k << 1;
    while (j <= w.heap_len) {
        if (j < w.heap_len && tw_smaller(f, w.heap[j + 1], w.heap[j], w.depth)) j++;
        if (tw_smaller(f, v, w.heap[j], w.depth)) break;
        w.heap[k] = w.heap[j];
        k = j;
        j <<= 1;
    }
    w.heap[k] = v;
}

// which: 0 = literal/length, 1 = distance, 2 = bit length
IMP_HD inline void build_tree(BlockTrees& T, int which) {
    TreeWork& w = T.w;
    uint32_t* f = which == 0 ? T.lf : which == 1 ? T.df : T.bf;
    uint16_t* dl = which == 0 ? T.ll : which == 1 ? T.dlen : T.blen;
    uint16_t* code = which == 0 ? T.lcode : which == 1 ? T.dcode : T.bcode;
    const int elems = which == 0 ? L_CODES : which == 1 ? D_CODES : BL_CODES;
    const int max_length = which == 2 ? MAX_BL_BITS : MAX_BITS;
    int max_code = -1;
    w.heap_len = 0;
    w.heap_max = HEAP_SIZE;
    for (int n = 0; n < elems; n++) {
        if (f[n] != 0) { w.heap[++w.heap_len] = max_code = n; w.depth[n] = 0; }
        else dl[n] = 0;
    }
    while (w.heap_len < 2) {                                    // force at least two codes of non-zero frequency
        const int node = w.heap[++w.heap_len] = (max_code < 2 ? ++max_code : 0);
        f[node] = 1;
        w.depth[node] = 0;
        T.opt_len--;
        if (which == 0) T.static_len -= static_llen(node);
        else if (which == 1) T.static_len -= 5;
    }
    if (which == 0) T.lmax = max_code; else if (which == 1) T.dmax = max_code;
    for (int n = w.heap_len / 2; n >= 1; n--) pqdownheap(w, f, n);
    int node = elems;
    do {
        const int n = w.heap[1];
        w.heap[1] = w.heap[w.heap_len--];
        pqdownheap(w, f, 1);
        const int m = w.heap[1];
        w.heap[--w.heap_max] = n;
        w.heap[--w.heap_max] = m;
        f[node] = f[n] + f[m];
        w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
        dl[n] = dl[m] = (uint16_t)node;
        w.heap[1] = node++;
        pqdownheap(w, f, 1);
    } while (w.heap_len >= 2);
    w.heap[--w.heap_max] = w.heap[1];

    // gen_bitlen
    for (int b = 0; b <= MAX_BITS; b++) w.bl_count[b] = 0;
    dl[w.heap[w.heap_max]] = 0;
    int overflow = 0, h;
    for (h = w.heap_max + 1; h < HEAP_SIZE; h++) {
        const int n = w.heap[h];
        int bits = dl[dl[n]] + 1;
        if (bits > max_length) { bits = max_length; overflow++; }
        dl[n] = (uint16_t)bits;
        if (n > max_code) continue;
        w.bl_count[bits]++;
        int xbits = 0;
        if (which == 0 && n >= 257) xbits = extra_lbits(n - 257);
        else if (which == 2) xbits = extra_blbits(n);
        T.opt_len += f[n] * (uint32_t)(bits + xbits);
        if (which == 0) T.static_len += f[n] * (uint32_t)(static_llen(n) + xbits);
        else if (which == 1) T.static_len += f[n] * (uint32_t)(5 + xbits);
    }
    if (overflow) {
        do {
            int bits = max_length - 1;
            while (w.bl_count[bits] == 0) bits--;
            w.bl_count[bits]--;
            w.bl_count[bits + 1] += 2;
            w.bl_count[max_length]--;
            overflow -= 2;
        } while (overflow > 0);
        for (int bits = max_length; bits != 0; bits--) {
            int n = w.bl_count[bits];
            while (n != 0) {
                const int m = w.heap[--h];
                if (m > max_code) continue;
                if (dl[m] != (unsigned)bits) {
                    T.opt_len += ((uint32_t)bits - dl[m]) * f[m];
                    dl[m] = (uint16_t)bits;
                }
                n--;
            }
        }
    }
    // gen_codes
    uint16_t next_code[MAX_BITS + 1];
    unsigned c = 0;
    for (int bits = 1; bits <= MAX_BITS; bits++) { c = (c + w.bl_count[bits - 1]) << 1; next_code[bits] = (uint16_t)c; }
    for (int n = 0; n <= max_code; n++) {
        const int len = dl[n];
        code[n] = len ? (uint16_t)bi_reverse(next_code[len]++, len) : 0;
    }
}

IMP_HD inline void scan_tree(BlockTrees& T, uint16_t* len, int max_code) {
    int prevlen = -1, nextlen = len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    len[max_code + 1] = 0xffff;                                 // guard
    for (int n = 0; n <= max_code; n++) {
        const int curlen = nextlen;
        nextlen = len[n + 1];
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) T.bf[curlen] += count;
        else if (curlen != 0) {
            if (curlen != prevlen) T.bf[curlen]++;
            T.bf[16]++;
        } else if (count <= 10) T.bf[17]++;
        else T.bf[18]++;
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}

// Block kinds, as the 2-bit BTYPE field.
constexpr int BT_STORED = 0, BT_FIXED = 1, BT_DYN = 2;

// _tr_flush_block's decision for a block of the given literal/length histogram (286 counts, END_BLOCK not included) and
// `stored_len` input bytes.  Leaves the trees in T (dynamic codes) and returns the kind.
IMP_HD inline int plan_block(BlockTrees& T, const uint32_t* hist, uint32_t stored_len) {
    uint32_t matches = 0;
    for (int n = 0; n < L_CODES; n++) T.lf[n] = hist[n];
    for (int n = 257; n < L_CODES; n++) matches += hist[n];
    T.lf[END_BLOCK] = 1;
    for (int n = 0; n < D_CODES; n++) T.df[n] = 0;
    T.df[0] = matches;
    for (int n = 0; n < BL_CODES; n++) T.bf[n] = 0;
    T.opt_len = T.static_len = 0;
    build_tree(T, 0);
    build_tree(T, 1);
    scan_tree(T, T.ll, T.lmax);
    scan_tree(T, T.dlen, T.dmax);
    build_tree(T, 2);
    int mb = BL_CODES - 1;
    for (; mb >= 3; mb--)
        if (T.blen[bl_order(mb)] != 0) break;
    T.max_blindex = mb;
    T.opt_len += 3 * ((uint32_t)mb + 1) + 5 + 5 + 4;
    uint32_t opt_lenb = (T.opt_len + 3 + 7) >> 3;
    const uint32_t static_lenb = (T.static_len + 3 + 7) >> 3;
    if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
    if (stored_len + 4 <= opt_lenb) return BT_STORED;
    return static_lenb == opt_lenb ? BT_FIXED : BT_DYN;
}

// A plain LSB-first bit writer into 32-bit words (zeroed by the caller); `at` = bit position.
struct BitWords {
    uint32_t* w;
    uint64_t at;
    IMP_HD void put(uint32_t v, int n) {
        if (!n) return;
        const uint64_t x = (uint64_t)v << (at & 31);
        w[at >> 5] |= (uint32_t)x;
        if ((at & 31) + n > 32) w[(at >> 5) + 1] |= (uint32_t)(x >> 32);
        at += (uint64_t)n;
    }
};

// send_all_trees after the 3 block-type bits: HLIT, HDIST, HCLEN, the bit-length code lengths, send_tree twice.
IMP_HD inline void send_tree(BitWords& o, const BlockTrees& T, const uint16_t* len, int max_code) {
    int prevlen = -1, nextlen = len[0], count = 0, max_count = 7, min_count = 4;
    if (nextlen == 0) { max_count = 138; min_count = 3; }
    auto code = [&](int c) { o.put(T.bcode[c], T.blen[c]); };
    for (int n = 0; n <= max_code; n++) {
        const int curlen = nextlen;
        nextlen = len[n + 1];
        if (++count < max_count && curlen == nextlen) continue;
        else if (count < min_count) { do { code(curlen); } while (--count != 0); }
        else if (curlen != 0) {
            if (curlen != prevlen) { code(curlen); count--; }
            code(16); o.put((uint32_t)(count - 3), 2);
        } else if (count <= 10) { code(17); o.put((uint32_t)(count - 3), 3); }
        else { code(18); o.put((uint32_t)(count - 11), 7); }
        count = 0;
        prevlen = curlen;
        if (nextlen == 0) { max_count = 138; min_count = 3; }
        else if (curlen == nextlen) { max_count = 6; min_count = 3; }
        else { max_count = 7; min_count = 4; }
    }
}
IMP_HD inline void send_all_trees(BitWords& o, const BlockTrees& T) {
    const int lcodes = T.lmax + 1, dcodes = T.dmax + 1, blcodes = T.max_blindex + 1;
    o.put((uint32_t)(lcodes - 257), 5);
    o.put((uint32_t)(dcodes - 1), 5);
    o.put((uint32_t)(blcodes - 4), 4);
    for (int rank = 0; rank < blcodes; rank++) o.put(T.blen[bl_order(rank)], 3);
    send_tree(o, T, T.ll, lcodes - 1);
    send_tree(o, T, T.dlen, dcodes - 1);
}

// The code table a block's symbols are written with: [n] = code | length << 16 for n < 286, [286] = distance code 0.
IMP_HD inline void code_table(const BlockTrees& T, int kind, uint32_t* tab) {
    if (kind == BT_FIXED) {
        // static_ltree: gen_codes over the fixed lengths (bl_count 8: 144 + 8, 9: 112, 7: 24)
        for (int n = 0; n < L_CODES; n++) {
            const int len = static_llen(n);
            unsigned first = len == 7 ? 0 : len == 8 ? 48 : 400;   // next_code[7] = 0, [8] = 48, [9] = 400
            unsigned idx = n < 144 ? n : n < 256 ? n - 144 : n < 280 ? n - 256 : 144 + (n - 280);
            tab[n] = bi_reverse(first + idx, len) | (uint32_t)len << 16;
        }
        tab[L_CODES] = 0u | 5u << 16;                           // static_dtree[0]: bi_reverse(0, 5)
    } else {
        for (int n = 0; n < L_CODES; n++) tab[n] = n <= T.lmax ? (uint32_t)T.lcode[n] | (uint32_t)T.ll[n] << 16 : 0;
        tab[L_CODES] = (uint32_t)T.dcode[0] | (uint32_t)T.dlen[0] << 16;
    }
}

// A symbol's bits under a code table: value (LSB first) and count.
IMP_HD inline int sym_bits(uint32_t s, const uint32_t* tab, uint64_t* v) {
    const int n = (int)(s & 511);
    const uint32_t c = tab[n];
    int bits = (int)(c >> 16);
    uint64_t x = c & 0xffff;
    if (n > END_BLOCK) {
        const int xb = (int)((s >> 14) & 7);
        x |= (uint64_t)((s >> 9) & 31) << bits;
        bits += xb;
        const uint32_t d = tab[L_CODES];
        x |= (uint64_t)(d & 0xffff) << bits;
        bits += (int)(d >> 16);
    }
    *v = x;
    return bits;
}

// The zlib header libpng writes (pngwutil.c optimize_cmf): 78 01 for Z_RLE, with CINFO lowered to fit `size` bytes of
// filtered data when that is at most 16 KB.
IMP_HD inline void zlib_header(uint64_t size, uint8_t* out) {
    unsigned cmf = 0x78, flg = 0x01;
    if (size <= 16384) {
        unsigned cinfo = cmf >> 4, half = 1u << (cinfo + 7);
        if (size <= half) {
            do { half >>= 1; --cinfo; } while (cinfo > 0 && size <= half);
            cmf = (cmf & 0x0f) | (cinfo << 4);
            unsigned tmp = flg & 0xe0;
            tmp += 0x1f - ((cmf << 8) + tmp) % 0x1f;
            flg = tmp;
        }
    }
    out[0] = (uint8_t)cmf;
    out[1] = (uint8_t)flg;
}

// Adler-32 pieces: a stretch of n bytes x_k contributes A = sum x_k and B = sum (n - k) x_k (mod 65521); two stretches
// combine as (A1 + A2, B1 + B2 + n2 A1) and the stream's checksum is a = 1 + A, b = B + N.
constexpr uint32_t ADLER_MOD = 65521;

// ---------------------------------------------------------------- the whole stream on one thread (impgpu_png_deflate)
// The same pieces the kernels run -- png_run_symbols over the runs, plan_block, send_all_trees, code_table, sym_bits --
// one after the other.  `words` = zeroed room for the stream's bits; returns the zlib stream's length in bytes (header and
// Adler-32 trailer included).  `tw` = one BlockTrees of scratch, `hist` = 286 counts, `syms` = room for BLOCK_SYMS symbols.
inline uint64_t deflate_serial(const uint8_t* d, uint32_t n, uint32_t* words, BlockTrees& T, uint32_t* hist, uint32_t* syms) {
    BitWords o{words, 16};
    uint32_t nsym = 0, block_start = 0, tab[L_CODES + 1];
    uint8_t hdr[2];
    zlib_header(n, hdr);
    words[0] |= (uint32_t)hdr[0] | (uint32_t)hdr[1] << 8;
    for (int k = 0; k < L_CODES; k++) hist[k] = 0;
    auto flush = [&](uint32_t end, bool last) {
        const int kind = plan_block(T, hist, end - block_start);
        if (kind == BT_STORED) {
            o.put((uint32_t)last, 3);
            o.at = (o.at + 7) & ~(uint64_t)7;
            const uint32_t len = end - block_start;
            o.put(len & 0xffff, 16);
            o.put(~len & 0xffff, 16);
            for (uint32_t k = block_start; k < end; k++) o.put(d[k], 8);
        } else {
            o.put((uint32_t)(kind << 1 | (int)last), 3);
            if (kind == BT_DYN) send_all_trees(o, T);
            code_table(T, kind, tab);
            for (uint32_t k = 0; k < nsym; k++) {
                uint64_t v;
                const int b = sym_bits(syms[k], tab, &v);
                o.put((uint32_t)v, b > 32 ? 32 : b);
                if (b > 32) o.put((uint32_t)(v >> 32), b - 32);
            }
            o.put(tab[END_BLOCK] & 0xffff, (int)(tab[END_BLOCK] >> 16));
        }
        for (int k = 0; k < L_CODES; k++) hist[k] = 0;
        nsym = 0;
        block_start = end;
    };
    uint32_t a = 0;
    for (uint32_t i = 1; i <= n; i++) {
        if (i < n && d[i] == d[a]) continue;
        png_run_symbols(a, i, d[a], 0, n, [&](uint32_t pos, uint32_t s) {
            syms[nsym++] = s;
            hist[s & 511]++;
            if (nsym == (uint32_t)BLOCK_SYMS) {
                const uint32_t len = (s & 511) > END_BLOCK ? (uint32_t)(base_length((int)(s & 511) - 257) + ((s >> 9) & 31) + 3) : 1;
                flush(pos + len, false);
            }
        });
        a = i;
    }
    flush(n, true);
    o.at = (o.at + 7) & ~(uint64_t)7;
    uint32_t A = 1, B = 0;
    for (uint32_t k = 0; k < n; k++) { A = (A + d[k]) % ADLER_MOD; B = (B + A) % ADLER_MOD; }
    const uint32_t adler = B << 16 | A;
    for (int k = 3; k >= 0; k--) o.put((adler >> (8 * k)) & 0xff, 8);
    return o.at >> 3;
}

}  // namespace png
}  // namespace imp
