// imp_jpeg_prog.h -- progressive (SOF2) JPEG files: what the host front records about their scans and the four scan
// decoders of ITU T.81 annex G (DC first, DC refinement, AC first, AC refinement), written once for both sides like
// imp_jpeg_core.h: k_jpeg_prog_level (imp_jpeg_prog.hip) runs jpeg_prog_item per lane, jpeg_prog_emulate (imp_jpeg_prog.cpp)
// runs the very same function item by item on the host (impgpu_jpeg_coefficients_ex, how = 1; the sanitizer fuzz).
//
// A progressive file whose scans are complete holds the coefficients of its sequential twin, and libjpeg makes the same
// pixels from them, so the stage fills the MCU-padded planes with absolute DC terms (JpegJob::dcadd == nullptr) and
// k_jpeg_pixels does the rest unchanged.
//
// The unit of work is an ITEM: one restart interval of one scan of one file.  Items of one LEVEL are independent of each
// other; a scan's level is 1 + the highest level of an earlier scan that touches the same component and an overlapping
// band (an AC refinement reads which coefficients of its band are non-zero already: what the earlier levels wrote).
#pragma once
#include <vector>
#include "imp_jpeg_core.h"

namespace imp {

constexpr int JPEG_PROG_MAX_SCANS = 32;      // (include/impgpu.h states it: libjpeg's default script has 10 scans, mozjpeg's 9-12)
constexpr uint32_t JPEG_PROG_GUARD_WORDS = 2;   // all-ones words behind every interval's last word: the reader is a word ahead

enum { JPEG_PROG_DC_FIRST = 0, JPEG_PROG_DC_REFINE = 1, JPEG_PROG_AC_FIRST = 2, JPEG_PROG_AC_REFINE = 3 };

// ---- what the kernels read
struct JpegProgScanDev {                     // one scan
    uint8_t ncomp, ss, se, ah, al, kind;
    uint8_t comp[3];                         // frame component of each scan component
    uint8_t tab[3];                          // its Huffman table: index into the file's JpegProgFileDev::tables
};
struct JpegProgFileDev {                     // one file
    int ncomp, mcux, mcuy;
    int h[3], v[3];                          // sampling factors
    int bw[3];                               // blocks per row of the MCU-padded plane
    int cbw[3], cbh[3];                      // the component's own block grid: what a one-component scan walks
    unsigned coef_off[3];
    int16_t* coef;
    const uint32_t* words;                   // every scan's unstuffed intervals, each on a word boundary
    const JpegHuffDev* tables;
    const JpegProgScanDev* scans;
    uint32_t* header;                        // [1]: status (JPEG_ST_*), as the sequential jobs' -- ORed by every item
    uint32_t* verdict;                       // where k_jpeg_prog_verdict leaves header[0..3] for the host (null: the host copies them)
    unsigned total_slots;
};
struct JpegProgItem {
    uint32_t file, scan;
    uint32_t word0, nbits;                   // where the interval starts in `words`; its payload in bits
    uint32_t unit0, nunits;                  // its first MCU (interleaved scan) / block of the component's grid, and how many
};

// ---- what the host front keeps
struct JpegProgScan {
    int ncomp = 0, comp[3] = {}, td[3] = {}, ta[3] = {};
    int ss = 0, se = 0, ah = 0, al = 0, kind = 0, level = 0;
    int tab[3] = {};                         // index into JpegProg::tables
    int restart_interval = 0;
    size_t data_begin = 0, data_end = 0;     // the entropy-coded bytes in the file (data_end: the marker that ends them)
    uint32_t nunits = 0, nsegs = 0;
};
struct JpegProg {
    std::vector<JpegProgScan> scans;
    std::vector<JpegHuffSpec> tables;        // the distinct tables the scans decode with, as in force at their SOS
    std::vector<uint8_t> table_is_dc;
    int nlevels = 0;
    size_t data_bytes = 0;                   // all scans' entropy-coded bytes
    size_t max_items = 0;                    // an upper bound of the intervals of all scans
};

// jpeg_parse that also takes SOF2 files when `prog` is given: *prog is filled for one (prog->scans is empty for a sequential
// file, which gives what jpeg_parse gives); refusals as include/impgpu.h lists them, with H->why = JPEG_WHY_PROGRESSIVE.
int jpeg_parse_ex(const uint8_t* blob, size_t size, JpegHeader* H, JpegProg* prog);
size_t jpeg_prog_capacity(const JpegProg& P);
// unstuffs every scan into `out` (cap bytes, 4-byte aligned) and lists the items, sorted by (level, kind);
// level_first[l] .. level_first[l + 1] are level l's
int jpeg_prog_prepare(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, uint8_t* out, size_t cap,
                      std::vector<JpegProgItem>* items, std::vector<uint32_t>* level_first);
void jpeg_prog_file_dev(const JpegHeader& H, const JpegFrame& F, JpegProgFileDev* D);
void jpeg_prog_scans_dev(const JpegProg& P, JpegProgScanDev* out);
// the plain sequential decoder (how = 0) and the device's stage item by item on the host (how = 1); planes zeroed by the caller
int jpeg_prog_reference(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, const JpegFrame& F, int16_t* coef);
int jpeg_prog_emulate(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, const JpegFrame& F, int16_t* coef, unsigned* status);

// ---- imp_jpeg_prog.hip
// zeroes the planes of `nfiles` files, then one launch per level (items[level_first[l] .. level_first[l + 1]) of the
// device's item table), then the verdict words.  `marks`: null or two events recorded behind the fill and the last level.
int launch_jpeg_prog(const JpegProgFileDev* files, unsigned nfiles, const JpegProgItem* items, const uint32_t* level_first, int nlevels,
                     hipStream_t s, hipEvent_t* marks, unsigned* launches);

// ---- the lane code
// zig-zag position -> position in the block (T.81 figure A.6), eight positions to a 64-bit word so that a lane reads it
// from registers / constants, not from a table in scratch memory
IMP_HD inline uint32_t jpeg_prog_natural(uint32_t k) {
    const uint32_t i = k >> 3;
    const uint64_t w = i == 0 ? 0x0a03020910080100ull : i == 1 ? 0x05040b1219201811ull : i == 2 ? 0x22293028211a130cull : i == 3 ? 0x1c150e07060d141bull
                     : i == 4 ? 0x242b323938312a23ull : i == 5 ? 0x332c251e170f161dull : i == 6 ? 0x2e271f262d343b3aull : 0x3f3e372f363d3c35ull;
    return (uint32_t)(w >> (8 * (k & 7))) & 63u;
}

template <class WordFn>
struct JpegProgBits {
    JpegBitReader1<WordFn> r;
    uint32_t p, nbits;
    bool bad;                                                       // asked for bits the interval does not have
    IMP_HD JpegProgBits(WordFn f, uint32_t n) : r(f), p(0), nbits(n), bad(false) { r.start(0); }
    IMP_HD uint32_t window() const { return r.window(); }
    IMP_HD void drop(uint32_t n) {
        if (p + n > nbits) { bad = true; return; }                  // (nothing moves: the words behind the guard are never asked for)
        p += n;
        r.take(n);
    }
    IMP_HD uint32_t take(uint32_t n) {                              // n = 0 .. 16
        const uint32_t v = n ? r.window() >> (32 - n) : 0u;
        drop(n);
        return v;
    }
};

// one Huffman symbol: 0..255, or -1 (no code starts with these bits / the interval ran out)
template <class Bits>
IMP_HD inline int jpeg_prog_symbol(Bits& b, const JpegHuffDev& t) {
    const uint32_t win = b.window(), peek = win >> 16;
    uint32_t e = t.lut[peek >> (16 - JPEG_LOOKBITS)];
    uint32_t len, sym;
    if (e & 31) {
        len = e & 31;
        sym = (((e >> 9) & 15) << 4) | ((e >> 5) & 15);             // (run << 4 | size: an EOBn symbol keeps its run)
    } else if ((e & 0x8000u) && t.sub[(((e >> 5) & 127) << 1) + ((win >> (32 - JPEG_LOOKBITS - ((e >> 12) & 7))) & ((1u << ((e >> 12) & 7)) - 1))]) {
        e = t.sub[(((e >> 5) & 127) << 1) + ((win >> (32 - JPEG_LOOKBITS - ((e >> 12) & 7))) & ((1u << ((e >> 12) & 7)) - 1))];
        len = e & 31;
        sym = (((e >> 9) & 15) << 4) | ((e >> 5) & 15);
    } else if (e & 0x8000u) {
        return -1;
    } else {                                                        // the canonical limits (a table with too many long codes)
        len = JPEG_LOOKBITS + 1;
        for (int l = JPEG_LOOKBITS + 1; l < 16; l++) len += peek >= t.limit[l] ? 1u : 0u;
        if (peek >= t.limit[16]) return -1;
        sym = t.vals[(uint32_t)(t.offs[len] + (int)(peek >> (16 - len))) & 255];
    }
    b.drop(len);
    return b.bad ? -1 : (int)sym;
}

IMP_HD inline int jpeg_prog_extend(uint32_t v, uint32_t s) {        // T.81 F.2.2.1: s value bits, negative when the first is 0
    return s == 0 ? 0 : (v < (1u << (s - 1)) ? (int)v - (int)(1u << s) + 1 : (int)v);
}

IMP_HD inline int16_t jpeg_prog_get(const int16_t* coef, uint32_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef const int16_t __attribute__((address_space(1))) * GlobalCoef;
    return ((GlobalCoef)(uintptr_t)coef)[at];
#else
    return coef[at];
#endif
}

// where unit u's blocks are: a one-component scan walks the component's own grid, an interleaved one the MCUs
IMP_HD inline uint32_t jpeg_prog_block_single(const JpegProgFileDev& D, uint32_t ci, uint32_t u) {
    const uint32_t cbw = (uint32_t)(ci == 0 ? D.cbw[0] : ci == 1 ? D.cbw[1] : D.cbw[2]);
    const uint32_t bw = (uint32_t)(ci == 0 ? D.bw[0] : ci == 1 ? D.bw[1] : D.bw[2]);
    const uint32_t off = ci == 0 ? D.coef_off[0] : ci == 1 ? D.coef_off[1] : D.coef_off[2];
    const uint32_t row = u / cbw, col = u - row * cbw;
    return off + (row * bw + col) * 64u;
}

// G.1.2.1, first pass: the difference as in the sequential process, prediction on the unshifted values, the stored term << Al
template <class Bits>
IMP_HD inline uint32_t jpeg_prog_dc_first(const JpegProgFileDev& D, const JpegProgScanDev& S, Bits& b, uint32_t unit0, uint32_t nunits) {
    int pred0 = 0, pred1 = 0, pred2 = 0;
    for (uint32_t u = unit0; u < unit0 + nunits; u++) {
        const uint32_t my = u / (uint32_t)D.mcux, mx = u - my * (uint32_t)D.mcux;
        for (uint32_t i = 0; i < S.ncomp; i++) {
            const uint32_t ci = i == 0 ? S.comp[0] : i == 1 ? S.comp[1] : S.comp[2];
            const uint32_t tb = i == 0 ? S.tab[0] : i == 1 ? S.tab[1] : S.tab[2];
            const uint32_t h = S.ncomp == 1 ? 1u : (uint32_t)(ci == 0 ? D.h[0] : ci == 1 ? D.h[1] : D.h[2]);
            const uint32_t v = S.ncomp == 1 ? 1u : (uint32_t)(ci == 0 ? D.v[0] : ci == 1 ? D.v[1] : D.v[2]);
            const uint32_t bw = (uint32_t)(ci == 0 ? D.bw[0] : ci == 1 ? D.bw[1] : D.bw[2]);
            const uint32_t off = ci == 0 ? D.coef_off[0] : ci == 1 ? D.coef_off[1] : D.coef_off[2];
            for (uint32_t q = 0; q < h * v; q++) {
                const uint32_t by = q / h, bx = q - by * h;
                const uint32_t at = S.ncomp == 1 ? jpeg_prog_block_single(D, ci, u) : off + ((my * v + by) * bw + mx * h + bx) * 64u;
                const int s = jpeg_prog_symbol(b, D.tables[tb]);
                if (s < 0) return JPEG_ST_BAD_CODE;
                if (s > 15) return JPEG_ST_BAD_CODE;
                const int diff = jpeg_prog_extend(b.take((uint32_t)s), (uint32_t)s);
                if (b.bad) return JPEG_ST_BAD_CODE;
                int& pred = i == 0 ? pred0 : i == 1 ? pred1 : pred2;
                pred += diff;
                jpeg_put_coef(D.coef, at, (int16_t)(pred * (1 << S.al)));
            }
        }
    }
    return 0;
}

// G.1.2.1, refinement: one bit per block, the term's bit Al
template <class Bits>
IMP_HD inline uint32_t jpeg_prog_dc_refine(const JpegProgFileDev& D, const JpegProgScanDev& S, Bits& b, uint32_t unit0, uint32_t nunits) {
    for (uint32_t u = unit0; u < unit0 + nunits; u++) {
        const uint32_t my = u / (uint32_t)D.mcux, mx = u - my * (uint32_t)D.mcux;
        for (uint32_t i = 0; i < S.ncomp; i++) {
            const uint32_t ci = i == 0 ? S.comp[0] : i == 1 ? S.comp[1] : S.comp[2];
            const uint32_t h = S.ncomp == 1 ? 1u : (uint32_t)(ci == 0 ? D.h[0] : ci == 1 ? D.h[1] : D.h[2]);
            const uint32_t v = S.ncomp == 1 ? 1u : (uint32_t)(ci == 0 ? D.v[0] : ci == 1 ? D.v[1] : D.v[2]);
            const uint32_t bw = (uint32_t)(ci == 0 ? D.bw[0] : ci == 1 ? D.bw[1] : D.bw[2]);
            const uint32_t off = ci == 0 ? D.coef_off[0] : ci == 1 ? D.coef_off[1] : D.coef_off[2];
            for (uint32_t q = 0; q < h * v; q++) {
                const uint32_t by = q / h, bx = q - by * h;
                const uint32_t at = S.ncomp == 1 ? jpeg_prog_block_single(D, ci, u) : off + ((my * v + by) * bw + mx * h + bx) * 64u;
                const uint32_t bit = b.take(1);
                if (b.bad) return JPEG_ST_BAD_CODE;
                if (bit) jpeg_put_coef(D.coef, at, (int16_t)(jpeg_prog_get(D.coef, at) | (int16_t)(1 << S.al)));
            }
        }
    }
    return 0;
}

// G.1.2.2, first pass of a band: run / size symbols as in the sequential process, values << Al, and EOBn symbols that end
// this block's band and those of the next 2^n + (n more bits) - 1 blocks
template <class Bits>
IMP_HD inline uint32_t jpeg_prog_ac_first(const JpegProgFileDev& D, const JpegProgScanDev& S, Bits& b, uint32_t unit0, uint32_t nunits) {
    const uint32_t ci = S.comp[0];
    const JpegHuffDev& T = D.tables[S.tab[0]];
    uint32_t eobrun = 0;
    for (uint32_t u = unit0; u < unit0 + nunits; u++) {
        if (eobrun) { eobrun--; continue; }
        const uint32_t at = jpeg_prog_block_single(D, ci, u);
        for (uint32_t k = S.ss; k <= S.se; k++) {
            const int rs = jpeg_prog_symbol(b, T);
            if (rs < 0) return JPEG_ST_BAD_CODE;
            const uint32_t r = (uint32_t)rs >> 4, s = (uint32_t)rs & 15;
            if (s) {
                k += r;
                const int val = jpeg_prog_extend(b.take(s), s);
                if (b.bad || k > S.se) return JPEG_ST_BAD_CODE;     // (a run that leaves the band: damaged)
                jpeg_put_coef(D.coef, at + jpeg_prog_natural(k), (int16_t)(val * (1 << S.al)));
            } else if (r == 15) {
                k += 15;
                if (k > S.se) return JPEG_ST_BAD_CODE;
            } else {
                eobrun = (1u << r) + b.take(r) - 1;                 // this block's end is the first of the run
                if (b.bad) return JPEG_ST_BAD_CODE;
                break;
            }
        }
    }
    return eobrun ? JPEG_ST_BAD_COUNT : 0u;                         // an end-of-band run that leaves the interval
}

// G.1.2.3, refinement of a band.  A coefficient that is non-zero already gets one correction bit as the walk passes it; a
// symbol's zero run counts only coefficients that are still zero; a new coefficient is +-1 << Al.
template <class Bits>
IMP_HD inline uint32_t jpeg_prog_ac_refine(const JpegProgFileDev& D, const JpegProgScanDev& S, Bits& b, uint32_t unit0, uint32_t nunits) {
    const uint32_t ci = S.comp[0];
    const JpegHuffDev& T = D.tables[S.tab[0]];
    const int p1 = 1 << S.al;
    uint32_t eobrun = 0;
    for (uint32_t u = unit0; u < unit0 + nunits; u++) {
        const uint32_t at = jpeg_prog_block_single(D, ci, u);
        uint32_t k = S.ss;
        if (eobrun == 0) {
            while (k <= S.se) {
                const int rs = jpeg_prog_symbol(b, T);
                if (rs < 0) return JPEG_ST_BAD_CODE;
                uint32_t r = (uint32_t)rs >> 4;
                const uint32_t s = (uint32_t)rs & 15;
                int val = 0;
                if (s) {
                    if (s != 1) return JPEG_ST_BAD_CODE;            // a refinement brings one new bit
                    val = b.take(1) ? p1 : -p1;
                    if (b.bad) return JPEG_ST_BAD_CODE;
                } else if (r != 15) {
                    eobrun = (1u << r) + b.take(r);                 // (this block included: counted down below)
                    if (b.bad) return JPEG_ST_BAD_CODE;
                    break;
                }
                // over r coefficients that are still zero (and every non-zero one on the way) to the one the symbol means
                bool placed = false;
                while (k <= S.se) {
                    const uint32_t pos = at + jpeg_prog_natural(k);
                    const int c = jpeg_prog_get(D.coef, pos);
                    if (c != 0) {
                        const uint32_t bit = b.take(1);
                        if (b.bad) return JPEG_ST_BAD_CODE;
                        if (bit && (c & p1) == 0) jpeg_put_coef(D.coef, pos, (int16_t)(c + (c > 0 ? p1 : -p1)));
                    } else {
                        if (r == 0) {
                            if (s) jpeg_put_coef(D.coef, pos, (int16_t)val);
                            placed = true;
                            k++;
                            break;
                        }
                        r--;
                    }
                    k++;
                }
                if (!placed) return JPEG_ST_BAD_CODE;               // the run left the band
            }
        }
        if (eobrun) {                                               // the rest of the band: correction bits only
            for (; k <= S.se; k++) {
                const uint32_t pos = at + jpeg_prog_natural(k);
                const int c = jpeg_prog_get(D.coef, pos);
                if (c != 0) {
                    const uint32_t bit = b.take(1);
                    if (b.bad) return JPEG_ST_BAD_CODE;
                    if (bit && (c & p1) == 0) jpeg_put_coef(D.coef, pos, (int16_t)(c + (c > 0 ? p1 : -p1)));
                }
            }
            eobrun--;
        }
    }
    return eobrun ? JPEG_ST_BAD_COUNT : 0u;
}

// One item.  `word(i)` = the i-th word of the interval as loaded.  Returns the status bits it found (0 = the interval
// decoded to exactly its blocks and what is left of it is the encoder's padding: fewer than 8 bits).
template <class WordFn>
IMP_HD inline uint32_t jpeg_prog_item(const JpegProgFileDev& D, const JpegProgScanDev& S, WordFn word, uint32_t nbits, uint32_t unit0, uint32_t nunits) {
    JpegProgBits<WordFn> b(word, nbits);
    uint32_t st;
    if (S.kind == JPEG_PROG_DC_FIRST) st = jpeg_prog_dc_first(D, S, b, unit0, nunits);
    else if (S.kind == JPEG_PROG_DC_REFINE) st = jpeg_prog_dc_refine(D, S, b, unit0, nunits);
    else if (S.kind == JPEG_PROG_AC_FIRST) st = jpeg_prog_ac_first(D, S, b, unit0, nunits);
    else st = jpeg_prog_ac_refine(D, S, b, unit0, nunits);
    if (!st && nbits - b.p >= 8) st = JPEG_ST_BAD_COUNT;            // data behind the last block
    return st;
}

}  // namespace imp
