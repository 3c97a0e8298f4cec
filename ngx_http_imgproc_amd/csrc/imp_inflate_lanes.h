// imp_inflate_lanes.h -- inflate (RFC 1950 container, RFC 1951 blocks) on one wavefront per zlib stream: the lanes' logic,
// shared by k_png_inflate (imp_png_inflate.hip) and the host diagnostic impgpu_png_inflate_lanes, which runs the same
// rounds one lane after the other (and under the sanitizers, tests/c/inflate_lanes_test.cpp).  Depends on nothing but
// <stdint.h>: every function here is __host__ __device__.
//
// A stream is decoded into exactly out_size bytes.  Work goes in ROUNDS:
//   1. the wave stages INF_IN_WORDS words of the compressed bytes, from the word the next bit lies in, into LDS
//      (inf_stage: nothing at or past in_size is kept, nothing at or past in_cap is read);
//   2. outside a block, the block header is read (inf_block_begin); a dynamic block's code-length code is built, its
//      code lengths are read through it (inf_block_lens), and the literal/length and distance codes are built.  A code
//      is built by the whole wave (inf_build_*): lane l counts the symbols of length l; the counts are scanned into first
//      codes, offsets and left-aligned limits and JUDGED by zlib's rules (over-subscribed: refused; incomplete: refused
//      but for no code at all and for a single code of one bit; the code-length code must be complete); lane l then
//      writes the symbols of length l in order; the lanes fill the direct-lookup table.  Nothing is looked up in a
//      refused code, so a lookup ends within 15 compares and always inside the symbol array;
//   3. symbols are decoded (inf_decode; wave-uniform: every lane computes the same, lane 0 writes) into a token list --
//      a literal, or length + distance with their extra bits already added -- with every token's output offset, until
//      the list is full, the staged words run low, the round's output bound is reached, the block ends, out_size is
//      reached, or something is wrong with the token that would come next;
//   4. all lanes emit into the WINDOW RING in LDS (inf_emit_par): a literal at once, a match whose source lies wholly
//      before the round's first byte side by side with them, one lane per token; the other matches -- their source was
//      produced in this round, or overlaps the match itself -- in token order, the whole wave on one match
//      (inf_emit_ord: lane j writes byte j, j + 64, ... reading byte j mod distance of the source, so that no lane
//      reads what the same step writes);
//   5. the round's bytes go from the ring to the destination (inf_flush -> inf_store, the ONE store to the destination:
//      it drops a byte at or past out_size).
// A round consumes at least one symbol (or a stored block's header or bytes) or ends the stream.
//
// The ring holds INF_WINDOW + INF_ROUND_OUT bytes: a round writes at most INF_ROUND_OUT bytes, the farthest source of any
// of them lies INF_WINDOW before the round's first byte, and these two ranges never share a slot -- so what step 4 writes
// side by side cannot overwrite a byte another token of the round still has to read.
//
// The verdict is inflate_exact's (imp_inflate.cpp): the decoder stops the moment out_size bytes exist -- mid-block, and
// with tokens of the round already decoded beyond that point -- and whatever follows is neither read nor judged; a token
// is only judged when the bytes before it do not fill the output, which is why step 3 stops AT a bad token and the
// round's end decides (inf_round_end).  The Adler-32 trailer is not checked.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define IMP_INF_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define IMP_INF_HD inline
#endif

namespace imp {

// a stream's status word (0: out_size bytes were produced); any other value makes the FILE IMP_ERROR_DECODE_FAILED
enum : int {
    INF_OK = 0,
    INF_DAMAGED = 1,           // bad zlib header, block type 3, LEN != ~NLEN, a refused code-length set, a bad repeat, an invalid code, symbol 286 / 287, distance symbol 30 / 31, a distance before the first byte
    INF_SHORT = 2,             // the input, or the final block, ended before out_size bytes
    INF_FILTER = 3,            // (k_png_inflate alone) a row's filter byte above 4
};
constexpr int INF_LANES = 64;
constexpr uint32_t INF_WINDOW = 32768;
constexpr uint32_t INF_ROUND_OUT = 8192;                     // what one round may write
constexpr uint32_t INF_RING = INF_WINDOW + INF_ROUND_OUT;
constexpr int INF_TOKENS = 512;
constexpr int INF_IN_WORDS = 512;                            // staged per round; a dynamic block's header is 141 words at most
constexpr int INF_LL_FAST = 10, INF_D_FAST = 8;              // bits of the direct-lookup tables
constexpr uint32_t INF_MAX_IN = 0xfffff000u;                 // byte offsets are 32-bit words (bit offsets 64-bit)
constexpr uint32_t INF_MAX_OUT = 0xfffff000u;

// one canonical Huffman code: per length the count, the first code, where its symbols start in sorted[], and the
// left-aligned (15-bit) limit below which a 15-bit peek belongs to a code of at most that length
struct InfCode {
    uint16_t count[16], first[16], offs[16], lim[16];
    uint16_t sorted[288];
};

// What one stream's wave works on.  In LDS on the device (52 KB: three workgroups of one wave on a CU's 160 KB), an
// ordinary object on the host.
struct InfMem {
    uint8_t ring[INF_RING];
    uint32_t in[INF_IN_WORDS];
    uint32_t tok[INF_TOKENS];            // literal: byte << 9; match: length | distance << 9
    uint32_t toff[INF_TOKENS];           // the token's first output byte
    uint16_t ord[INF_TOKENS];            // the matches that go in token order
    uint16_t fast_ll[1 << INF_LL_FAST];  // symbol << 4 | length, 0: not a code of at most INF_LL_FAST bits
    uint16_t fast_d[1 << INF_D_FAST];
    InfCode ll, d, cl;
    uint8_t lens[320];                   // HLIT + HDIST code lengths (fixed block: 288 + 32)
    uint8_t cllens[32];
};

// wave-uniform: the decoder between two rounds
struct InfState {
    uint64_t bitpos;                     // of the next bit of the stream
    uint32_t in_size, out_size;
    uint32_t outpos;                     // bytes produced so far
    int block;                           // 0: between blocks, 1: inside a stored block, 2: inside a compressed one
    int last;                            // BFINAL of the block
    uint32_t stored_left;
    int nlen, ndist;                     // of the block whose header is being read
    int status, done;
};

// wave-uniform: the bit reader over the staged words
struct InfBits {
    uint64_t bb;
    int bn, widx;
    uint64_t base;                       // stream bit offset of in[0]
};

// wave-uniform: what a round decoded
struct InfRound {
    uint32_t start;                      // the round's first output byte
    uint32_t out;                        // bytes its tokens (or stored bytes) produce, not yet cut at out_size
    int ntok, nord;
    uint32_t stored, stored_from;        // a stored block's round: bytes to take, from this byte of the input
    int eob, err;                        // the block ended; the verdict on the token that would come next (0: none)
    uint64_t bitpos;                     // behind the last token
};

IMP_INF_HD uint32_t inf_rev15(uint32_t x) {                  // bits 0..14 of x, reversed
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0f0fu) << 4) | ((x >> 4) & 0x0f0fu);
    x = ((x & 0x00ffu) << 8) | ((x >> 8) & 0x00ffu);
    return (x >> 1) & 0x7fffu;
}

// THE store to the destination: nothing at or past out_size
IMP_INF_HD void inf_store(uint8_t* out, uint32_t out_size, uint32_t pos, uint8_t v) {
    if (pos < out_size) out[pos] = v;
}

// RFC 1950 2.2: the two header bytes.  Sets done / status when the stream ends here.
IMP_INF_HD void inf_start(InfState* s, const uint8_t* in, uint32_t in_size, uint32_t out_size) {
    s->bitpos = 16;
    s->in_size = in_size; s->out_size = out_size;
    s->outpos = 0;
    s->block = 0; s->last = 0; s->stored_left = 0; s->nlen = 0; s->ndist = 0;
    s->status = INF_OK; s->done = 0;
    if (in_size < 2) { s->status = INF_SHORT; s->done = 1; return; }
    const uint32_t cmf = in[0], flg = in[1];
    if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 0x20u)) { s->status = INF_DAMAGED; s->done = 1; return; }
    if (out_size == 0) s->done = 1;                          // (nothing wanted: nothing read)
}

// Step 1, lane `lane`'s words: in[] from the word that holds bit `bitpos`.  `in` is 4-byte aligned and in_cap (a multiple
// of 4, >= in_size) bytes of it may be read; a byte at or past in_size reads as zero whatever the memory holds.
IMP_INF_HD void inf_stage(InfMem* m, const uint8_t* in, uint32_t in_cap, const InfState& s, int lane) {
    const uint32_t w0 = (uint32_t)(s.bitpos >> 5);
    for (int k = lane; k < INF_IN_WORDS; k += INF_LANES) {
        const uint64_t off = ((uint64_t)w0 + (uint64_t)k) * 4u;
        uint32_t w = 0;
        if (off + 4u <= (uint64_t)in_cap) {
            w = ((const uint32_t*)in)[w0 + (uint32_t)k];
            if (off + 4u > (uint64_t)s.in_size) {
                const uint32_t keep = off < (uint64_t)s.in_size ? s.in_size - (uint32_t)off : 0u;
                w = keep ? (w & ((1u << (8u * keep)) - 1u)) : 0u;
            }
        }
        m->in[k] = w;
    }
}

IMP_INF_HD void inf_refill(const InfMem* m, InfBits* b) {
    if (b->bn <= 32 && b->widx < INF_IN_WORDS) {
        b->bb |= (uint64_t)m->in[b->widx++] << b->bn;
        b->bn += 32;
    }
}
IMP_INF_HD uint32_t inf_take(InfBits* b, int n) {            // n <= 16
    const uint32_t v = (uint32_t)b->bb & ((1u << n) - 1u);
    b->bb >>= n;
    b->bn -= n;
    return v;
}
IMP_INF_HD uint64_t inf_bits_pos(const InfBits& b) { return b.base + (uint64_t)b.widx * 32u - (uint64_t)b.bn; }
IMP_INF_HD bool inf_overrun(const InfBits& b, const InfState& s) { return inf_bits_pos(b) > (uint64_t)s.in_size * 8u; }
IMP_INF_HD void inf_bits_begin(const InfMem* m, InfBits* b, const InfState& s) {
    b->bb = 0; b->bn = 0; b->widx = 0;
    b->base = (s.bitpos >> 5) << 5;
    inf_refill(m, b);
    (void)inf_take(b, (int)(s.bitpos & 31u) & 15);
    (void)inf_take(b, (int)(s.bitpos & 16u));
}

// One symbol of code `c` from the next 15 bits of the stream (`peek`, the stream's first bit in bit 0; absent bits are
// zero): the symbol and *len, or -1 where no code of the set starts these bits.
IMP_INF_HD int inf_sym(const InfCode* c, const uint16_t* fast, int fbits, uint32_t peek, int* len) {
    if (fbits) {
        const uint32_t e = fast[peek & ((1u << fbits) - 1u)];
        if (e) { *len = (int)(e & 15u); return (int)(e >> 4); }
    }
    const uint32_t v = inf_rev15(peek);
    for (int l = fbits + 1; l <= 15; l++) {
        if (v < c->lim[l]) {
            const uint32_t idx = (uint32_t)c->offs[l] + (v >> (15 - l)) - (uint32_t)c->first[l];
            *len = l;
            return (int)c->sorted[idx < 288u ? idx : 287u];
        }
    }
    return -1;
}

// ---- a code built by the whole wave from n code lengths (n <= 288)
// count: lane l the symbols of length l; the lanes clear the lookup table
IMP_INF_HD void inf_build_count(InfCode* c, const uint8_t* lens, int n, uint16_t* fast, int fbits, int lane) {
    if (lane < 16) {
        int cnt = 0;
        for (int i = 0; i < n; i++) cnt += lens[i] == lane ? 1 : 0;
        c->count[lane] = (uint16_t)cnt;
    }
    if (fbits)
        for (int i = lane; i < (1 << fbits); i += INF_LANES) fast[i] = 0;
}
// scan and verdict (wave-uniform; lane 0 writes): false = refused
IMP_INF_HD bool inf_build_scan(InfCode* c, bool must_be_complete, int lane) {
    int left = 1, used = 0;
    bool ok = true;
    uint32_t code = 0, off = 0;
    for (int l = 1; l <= 15; l++) {
        const int cnt = c->count[l];
        left = (left << 1) - cnt;
        if (left < 0) { ok = false; left = 0; }              // over-subscribed
        used += cnt;
        if (lane == 0) {
            c->first[l] = (uint16_t)code;
            c->offs[l] = (uint16_t)off;
            c->lim[l] = (uint16_t)(ok ? (code + (uint32_t)cnt) << (15 - l) : 0u);
        }
        code = (code + (uint32_t)cnt) << 1;
        off += (uint32_t)cnt;
    }
    // zlib (inftrees.c): an incomplete code is an error, except no code at all and a single code of one bit; the
    // code-length code must be complete
    if (left > 0 && used != 0 && (must_be_complete || !(used == 1 && c->count[1] == 1))) ok = false;
    return ok;
}
// fill 1: lane l the symbols of length l, in symbol order
IMP_INF_HD void inf_build_sort(InfCode* c, const uint8_t* lens, int n, int lane) {
    if (lane < 1 || lane > 15) return;
    uint32_t k = c->offs[lane];
    for (int i = 0; i < n; i++)
        if (lens[i] == lane && k < 288u) c->sorted[k++] = (uint16_t)i;
}
// fill 2: the lookup table, the lanes striding over the sorted symbols
IMP_INF_HD void inf_build_fill(const InfCode* c, uint16_t* fast, int fbits, int lane) {
    if (!fbits) return;
    const int used = (int)c->offs[15] + (int)c->count[15];
    for (int p = lane; p < used && p < 288; p += INF_LANES) {
        int l = 1;
        while (l < 15 && p >= (int)c->offs[l] + (int)c->count[l]) l++;
        if (l > fbits) continue;
        const uint32_t code = (uint32_t)c->first[l] + (uint32_t)(p - (int)c->offs[l]);
        const uint32_t rev = inf_rev15(code << (15 - l));
        const uint16_t e = (uint16_t)(((uint32_t)c->sorted[p] << 4) | (uint32_t)l);
        for (uint32_t i = rev; i < (1u << fbits); i += 1u << l) fast[i] = e;
    }
}

// ---- step 2: a block's header
enum : int { INF_B_STORED = 0, INF_B_FIXED = 1, INF_B_DYNAMIC = 2, INF_B_NONE = -1 };
IMP_INF_HD void inf_fail(InfState* s, int status) { s->status = status; s->done = 1; }

// where the i-th length of the code-length code belongs: 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15
IMP_INF_HD int inf_cl_order(int i) {
    if (i < 8) return (int)((0x0609070800121110ull >> (8 * i)) & 255u);
    if (i < 16) return (int)((0x020d030c040b050aull >> (8 * (i - 8))) & 255u);
    return i == 16 ? 14 : i == 17 ? 1 : 15;
}

// Wave-uniform; lane 0 writes cllens[].  The kind of the block, or INF_B_NONE with the stream ended (status set).
IMP_INF_HD int inf_block_begin(InfMem* m, InfState* s, InfBits* b, int lane) {
    inf_refill(m, b);
    s->last = (int)inf_take(b, 1);
    const int type = (int)inf_take(b, 2);
    if (inf_overrun(*b, *s)) { inf_fail(s, INF_SHORT); return INF_B_NONE; }
    if (type == 0) {
        (void)inf_take(b, (int)((0u - (uint32_t)inf_bits_pos(*b)) & 7u));      // to the byte boundary
        inf_refill(m, b);
        const uint32_t len = inf_take(b, 16);
        inf_refill(m, b);
        const uint32_t nlen = inf_take(b, 16);
        if (inf_overrun(*b, *s)) { inf_fail(s, INF_SHORT); return INF_B_NONE; }
        if ((len ^ 0xffffu) != nlen) { inf_fail(s, INF_DAMAGED); return INF_B_NONE; }
        s->bitpos = inf_bits_pos(*b);
        // (inflate_exact's order: a block that promises more bytes than the input holds fails before any of them is taken)
        if ((uint64_t)s->in_size - (s->bitpos >> 3) < (uint64_t)len) { inf_fail(s, INF_SHORT); return INF_B_NONE; }
        s->stored_left = len;
        s->block = 1;
        return INF_B_STORED;
    }
    if (type == 1) {
        s->nlen = 288; s->ndist = 32;
        s->block = 2;
        return INF_B_FIXED;
    }
    if (type == 3) { inf_fail(s, INF_DAMAGED); return INF_B_NONE; }
    s->nlen = (int)inf_take(b, 5) + 257;
    s->ndist = (int)inf_take(b, 5) + 1;
    const int ncode = (int)inf_take(b, 4) + 4;
    if (inf_overrun(*b, *s)) { inf_fail(s, INF_SHORT); return INF_B_NONE; }
    if (s->nlen > 286 || s->ndist > 30) { inf_fail(s, INF_DAMAGED); return INF_B_NONE; }
    for (int i = 0; i < 19; i++) {
        inf_refill(m, b);
        const uint32_t v = i < ncode ? inf_take(b, 3) : 0u;
        const int at = inf_cl_order(i);
        if (lane == 0) m->cllens[at] = (uint8_t)v;
    }
    if (inf_overrun(*b, *s)) { inf_fail(s, INF_SHORT); return INF_B_NONE; }
    s->block = 2;
    return INF_B_DYNAMIC;
}

// a fixed block's code lengths (RFC 1951 3.2.6), the lanes striding
IMP_INF_HD void inf_fixed_lens(InfMem* m, int lane) {
    for (int i = lane; i < 320; i += INF_LANES)
        m->lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
}

// A dynamic block's HLIT + HDIST code lengths through the code-length code (built and judged before).  Wave-uniform;
// lane 0 writes lens[].  Ends the stream (status set) on a bad repeat, an invalid code, a missing end-of-block code.
IMP_INF_HD void inf_block_lens(InfMem* m, InfState* s, InfBits* b, int lane) {
    const int total = s->nlen + s->ndist;
    int i = 0, prev = 0, l256 = 0;
    while (i < total) {
        inf_refill(m, b);
        int l = 0;
        const int sym = inf_sym(&m->cl, nullptr, 0, (uint32_t)b->bb & 0x7fffu, &l);
        if (sym < 0) { inf_fail(s, inf_bits_pos(*b) + 7u > (uint64_t)s->in_size * 8u ? INF_SHORT : INF_DAMAGED); return; }
        (void)inf_take(b, l);
        int rep = 1, val = sym;
        if (sym == 16) {
            if (i == 0) { inf_fail(s, INF_DAMAGED); return; }
            val = prev;
            rep = 3 + (int)inf_take(b, 2);
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (int)inf_take(b, 3);
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (int)inf_take(b, 7);
        }
        if (inf_overrun(*b, *s)) { inf_fail(s, INF_SHORT); return; }
        if (i + rep > total) { inf_fail(s, INF_DAMAGED); return; }
        if (i <= 256 && 256 < i + rep) l256 = val;
        if (lane == 0)
            for (int k = 0; k < rep; k++) m->lens[i + k] = (uint8_t)val;
        i += rep;
        prev = val;
    }
    if (l256 == 0) inf_fail(s, INF_DAMAGED);                 // no end-of-block code
}

IMP_INF_HD void inf_round_begin(InfRound* r, const InfState& s) {
    r->start = s.outpos;
    r->out = 0;
    r->ntok = 0; r->nord = 0;
    r->stored = 0; r->stored_from = 0;
    r->eob = 0; r->err = 0;
    r->bitpos = s.bitpos;
}

// ---- step 3.  Wave-uniform; lane 0 writes the lists.
IMP_INF_HD void inf_decode(InfMem* m, const InfState& s, InfBits* b, InfRound* r, int lane) {
    uint32_t pos = r->start;
    int ntok = 0, nord = 0;
    const uint64_t in_bits = (uint64_t)s.in_size * 8u;
    for (;;) {
        r->bitpos = inf_bits_pos(*b);
        if (pos >= s.out_size) break;                        // nothing behind this point is read or judged
        if (ntok >= INF_TOKENS || pos - r->start > INF_ROUND_OUT - 258u || b->widx > INF_IN_WORDS - 3) break;
        inf_refill(m, b);
        int l = 0;
        const int sym = inf_sym(&m->ll, m->fast_ll, INF_LL_FAST, (uint32_t)b->bb & 0x7fffu, &l);
        if (sym < 0) { r->err = r->bitpos + 15u > in_bits ? INF_SHORT : INF_DAMAGED; break; }
        (void)inf_take(b, l);
        if (inf_bits_pos(*b) > in_bits) { r->err = INF_SHORT; break; }
        if (sym < 256) {
            if (lane == 0) { m->tok[ntok] = (uint32_t)sym << 9; m->toff[ntok] = pos; }
            ntok++;
            pos++;
            continue;
        }
        if (sym == 256) { r->eob = 1; r->bitpos = inf_bits_pos(*b); break; }
        if (sym > 285) { r->err = INF_DAMAGED; break; }
        const int c = sym - 257;
        const int lx = c < 8 || c == 28 ? 0 : (c >> 2) - 1;
        const uint32_t len = (c < 8 ? 3u + (uint32_t)c : c == 28 ? 258u : 3u + ((4u + ((uint32_t)c & 3u)) << lx)) + inf_take(b, lx);
        inf_refill(m, b);
        const uint64_t dpos = inf_bits_pos(*b);
        const int dsym = inf_sym(&m->d, m->fast_d, INF_D_FAST, (uint32_t)b->bb & 0x7fffu, &l);
        if (dsym < 0) { r->err = dpos + 15u > in_bits ? INF_SHORT : INF_DAMAGED; break; }
        (void)inf_take(b, l);
        if (inf_bits_pos(*b) > in_bits) { r->err = INF_SHORT; break; }
        if (dsym > 29) { r->err = INF_DAMAGED; break; }
        const int dx = dsym < 4 ? 0 : (dsym >> 1) - 1;
        const uint32_t dist = (dsym < 4 ? 1u + (uint32_t)dsym : 1u + ((2u + ((uint32_t)dsym & 1u)) << dx)) + inf_take(b, dx);
        if (inf_bits_pos(*b) > in_bits) { r->err = INF_SHORT; break; }
        if (dist > pos) { r->err = INF_DAMAGED; break; }     // before the first output byte
        if (lane == 0) {
            m->tok[ntok] = len | dist << 9;
            m->toff[ntok] = pos;
            if (pos - dist + len > r->start) m->ord[nord] = (uint16_t)ntok;
        }
        if (pos - dist + len > r->start) nord++;
        ntok++;
        pos += len;
    }
    r->ntok = ntok; r->nord = nord;
    r->out = pos - r->start;
}

// a stored block's round: what to take (wave-uniform) ...
IMP_INF_HD void inf_stored_plan(const InfState& s, InfRound* r) {
    uint32_t n = s.stored_left < INF_ROUND_OUT ? s.stored_left : INF_ROUND_OUT;
    if (n > s.out_size - s.outpos) n = s.out_size - s.outpos;
    r->stored = n;
    r->stored_from = (uint32_t)(s.bitpos >> 3);
    r->out = n;
    r->bitpos = s.bitpos + (uint64_t)n * 8u;
    r->eob = n == s.stored_left;
}
// ... and lane `lane`'s bytes of it, into the ring
IMP_INF_HD void inf_stored_copy(InfMem* m, const InfState& s, const InfRound& r, const uint8_t* in, int lane) {
    for (uint32_t j = (uint32_t)lane; j < r.stored; j += INF_LANES) {
        const uint32_t at = r.stored_from + j;
        m->ring[(r.start + j) % INF_RING] = at < s.in_size ? in[at] : (uint8_t)0;
    }
}

// ---- step 4.  Literals and the matches whose source lies wholly before the round: one lane per token, side by side.
IMP_INF_HD void inf_emit_par(InfMem* m, const InfState& s, const InfRound& r, int lane) {
    for (int t = lane; t < r.ntok; t += INF_LANES) {
        const uint32_t tk = m->tok[t], off = m->toff[t], len = tk & 511u, dist = tk >> 9;
        if (!len) { m->ring[off % INF_RING] = (uint8_t)dist; continue; }
        if (off - dist + len > r.start) continue;
        const uint32_t n = len < s.out_size - off ? len : s.out_size - off;
        for (uint32_t j = 0; j < n; j++) m->ring[(off + j) % INF_RING] = m->ring[(off - dist + j) % INF_RING];
    }
}
// Match ord[k] by the whole wave: lane j writes bytes j, j + 64, ... and reads byte (j mod distance) of the source, which
// lies before the match's first byte -- written by an earlier step, never by this one.
IMP_INF_HD void inf_emit_ord(InfMem* m, const InfState& s, int k, int lane) {
    const int t = m->ord[k] & (INF_TOKENS - 1);
    const uint32_t tk = m->tok[t], off = m->toff[t], len = tk & 511u, dist = tk >> 9;
    if (!len || !dist || off >= s.out_size) return;
    const uint32_t n = len < s.out_size - off ? len : s.out_size - off;
    for (uint32_t j = (uint32_t)lane; j < n; j += INF_LANES) {
        const uint32_t from = dist >= len ? j : j % dist;
        m->ring[(off + j) % INF_RING] = m->ring[(off - dist + from) % INF_RING];
    }
}
// ---- step 5: the round's bytes, from the ring to the destination
IMP_INF_HD void inf_flush(const InfMem* m, const InfState& s, const InfRound& r, uint8_t* out, int lane) {
    const uint32_t room = s.out_size - r.start, n = r.out < room ? r.out : room;
    for (uint32_t j = (uint32_t)lane; j < n; j += INF_LANES) inf_store(out, s.out_size, r.start + j, m->ring[(r.start + j) % INF_RING]);
}

// The state behind a round (wave-uniform).  A full output ends the stream as INF_OK before anything else is looked at.
IMP_INF_HD void inf_round_end(InfState* s, const InfRound& r) {
    const uint32_t room = s->out_size - r.start;
    s->outpos = r.start + (r.out < room ? r.out : room);
    if (s->done) return;                                     // (a block header ended the stream)
    if (s->outpos >= s->out_size) { s->status = INF_OK; s->done = 1; return; }
    if (r.err) { inf_fail(s, r.err); return; }
    s->bitpos = r.bitpos;
    if (s->block == 1) s->stored_left -= r.stored;
    if (r.eob) {
        s->block = 0;
        if (s->last) inf_fail(s, INF_SHORT);                 // the final block ended before out_size bytes
    }
}

// ---------------------------------------------------------------- the host's run of the rounds (impgpu_png_inflate_lanes)
// one lane after the other where the wave runs them side by side.  `in`: 4-byte aligned, in_cap readable bytes (see inf_stage)
inline bool inf_build_host(InfCode* c, const uint8_t* lens, int n, uint16_t* fast, int fbits, bool must_be_complete) {
    for (int j = 0; j < INF_LANES; j++) inf_build_count(c, lens, n, fast, fbits, j);
    const bool ok = inf_build_scan(c, must_be_complete, 0);
    if (!ok) return false;
    for (int j = 0; j < INF_LANES; j++) inf_build_sort(c, lens, n, j);
    for (int j = 0; j < INF_LANES; j++) inf_build_fill(c, fast, fbits, j);
    return true;
}

inline int inf_lanes_host(const uint8_t* in, uint32_t in_cap, uint32_t in_size, uint8_t* out, uint32_t out_size, InfMem* m) {
    InfState s;
    inf_start(&s, in, in_size, out_size);
    while (!s.done) {
        for (int j = 0; j < INF_LANES; j++) inf_stage(m, in, in_cap, s, j);
        InfBits b;
        inf_bits_begin(m, &b, s);
        InfRound r;
        inf_round_begin(&r, s);
        if (s.block == 0) {
            const int kind = inf_block_begin(m, &s, &b, 0);
            if (kind == INF_B_DYNAMIC) {
                if (!inf_build_host(&m->cl, m->cllens, 19, nullptr, 0, true)) inf_fail(&s, INF_DAMAGED);
                else inf_block_lens(m, &s, &b, 0);
            } else if (kind == INF_B_FIXED) {
                for (int j = 0; j < INF_LANES; j++) inf_fixed_lens(m, j);
            }
            if (!s.done && kind >= INF_B_FIXED) {
                if (!inf_build_host(&m->ll, m->lens, s.nlen, m->fast_ll, INF_LL_FAST, false) ||
                    !inf_build_host(&m->d, m->lens + s.nlen, s.ndist, m->fast_d, INF_D_FAST, false))
                    inf_fail(&s, INF_DAMAGED);
            }
        }
        if (!s.done) {
            if (s.block == 1) {
                inf_stored_plan(s, &r);
                for (int j = 0; j < INF_LANES; j++) inf_stored_copy(m, s, r, in, j);
            } else {
                inf_decode(m, s, &b, &r, 0);
                for (int j = 0; j < INF_LANES; j++) inf_emit_par(m, s, r, j);
                for (int k = 0; k < r.nord; k++)
                    for (int j = 0; j < INF_LANES; j++) inf_emit_ord(m, s, k, j);
            }
            for (int j = 0; j < INF_LANES; j++) inf_flush(m, s, r, out, j);
        }
        inf_round_end(&s, r);
    }
    return s.status;
}

}  // namespace imp
