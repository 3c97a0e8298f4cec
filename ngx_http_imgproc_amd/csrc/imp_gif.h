// imp_gif.h -- GIF's LZW on one wavefront per page: the lanes' logic, shared by k_gif_lzw (imp_gif.hip) and the host
// diagnostic impgpu_gif_pages(how = 1), which runs the same rounds one lane after the other (and under the sanitizers,
// tests/c/gif_fuzz.cpp).  Depends on nothing but <stdint.h>: every function here is __host__ __device__.
//
// A ROUND is 64 codes.  GIF's code width is a function of how many codes have passed since the last clear code, so every
// lane finds its code's bit offset in closed form from the round's start state (gif_code_at); the round ends at the first
// clear, end-of-information, invalid or missing code (the caller's ballot over gif_extract's kinds).  The entries the
// round adds are linked by pointer jumping over the lanes (gif_link_*: entry n+j takes its prefix from code j-1, and its
// length and first byte from that prefix, which may itself be an entry of this round), a scan of the string lengths
// gives every code's output offset, and every lane writes its string by walking the prefix chain backwards (gif_emit).
//
// IMPGPU_GIF_SPLIT cuts a page at its clear codes and gives every segment a wavefront of its own: the scan, the length
// pass and the emit pass further down (k_gif_lzw_scan / _len / _emit; on the host impgpu_gif_pages_split and
// tests/c/gif_split_fuzz.cpp).
//
// Safe by construction: a store goes through gif_store, which drops every index at or past width x height; a round
// consumes at least one code or ends the page; every chain walk is bounded by the entry's stored length.
#pragma once
#include <stdint.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif
#include "../../include/impgpu.h"      // IMPGPU_GIF_SPLIT_MIN_BYTES
#include "../../include/impgpu_gif.h"

#if defined(__HIPCC__)
#define IMP_GIF_HD __host__ __device__ __forceinline__
#else
#define IMP_GIF_HD inline
#endif

namespace imp {

// a page's status word (0: the plane is complete); any other value makes the FILE IMP_ERROR_DECODE_FAILED
enum : int {
    GIF_LZW_OK = 0,
    GIF_LZW_INVALID = 1,       // a code above the next free code, or a first-after-clear code that is not a literal
    GIF_LZW_SHORT = 2,         // data exhausted (or end-of-information) before width x height indices
    GIF_LZW_LONG = 3,          // indices beyond width x height
};
enum : int { GIF_K_CODE = 0, GIF_K_CLEAR = 1, GIF_K_EOI = 2, GIF_K_INVALID = 3, GIF_K_NODATA = 4 };
constexpr int GIF_LANES = 64;
constexpr int GIF_TABLE = 4096;

// What one page's wave works on: the table (prefix code, string length, first and last byte per entry: 24 KB) and the
// round's per-lane words.  In LDS on the device, an ordinary object on the host.
struct GifLzwMem {
    uint16_t prefix[GIF_TABLE];
    uint16_t len[GIF_TABLE];
    uint8_t first[GIF_TABLE];
    uint8_t last[GIF_TABLE];
    uint16_t code[GIF_LANES];        // the round's codes
    uint16_t acc[GIF_LANES];         // pointer jumping: length gathered so far ...
    int16_t lnk[GIF_LANES];          // ... the lane whose entry the rest of the chain hangs on (-1: resolved) ...
    uint8_t fst[GIF_LANES];          // ... and, once resolved, the entry's first byte
    uint16_t acc2[GIF_LANES];        // what a jump read, held over the barrier between its read and its write phase
    int16_t lnk2[GIF_LANES];
    uint8_t fst2[GIF_LANES];
};

// wave-uniform: the decoder between two rounds
struct GifLzwState {
    uint32_t bitpos;                 // of the round's first code
    int next;                        // the next free code (4096: the table is full, nothing is added until a clear)
    int prev;                        // the code before the round's first (-1: the first after a clear, or of the page)
    uint32_t outpos;                 // indices produced so far (may pass width x height: GIF_LZW_LONG)
    int status, done;
};

struct GifPlane {
    uint8_t* plane;                  // FreeImage's 8-bit page: bottom-up, pitch = (width + 3) & ~3
    int w, h, pitch, interlaced;
    uint32_t total;                  // w * h
};

// Row y of the stream -> row of the picture: interlaced files send rows 0,8,.. then 4,12,.. then 2,6,.. then 1,3,..
IMP_GIF_HD int gif_stream_row(int y, int h, int interlaced) {
    if (!interlaced) return y;
    const int n0 = (h + 7) >> 3, n1 = (h + 3) >> 3, n2 = (h + 1) >> 2;
    if (y < n0) return y << 3;
    y -= n0;
    if (y < n1) return (y << 3) + 4;
    y -= n1;
    if (y < n2) return (y << 2) + 2;
    y -= n2;
    return (y << 1) + 1;
}

// index `pos` of the stream (x = pos % w, stream row pos / w) into the plane; nothing at or past w * h is stored
IMP_GIF_HD void gif_store(const GifPlane& p, uint32_t pos, uint8_t v) {
    if (pos >= p.total) return;
    const int ys = (int)(pos / (uint32_t)p.w), x = (int)(pos - (uint32_t)ys * (uint32_t)p.w);
    const int y = gif_stream_row(ys, p.h, p.interlaced);
    p.plane[(size_t)(p.h - 1 - y) * (size_t)p.pitch + (size_t)x] = v;
}

// the pad bytes of plane row `row` (FreeImage's are 0)
IMP_GIF_HD void gif_pad_row(const GifPlane& p, int row) {
    for (int x = p.w; x < p.pitch; x++) p.plane[(size_t)row * (size_t)p.pitch + (size_t)x] = 0;
}

IMP_GIF_HD void gif_state_start(GifLzwState* s, int mcs) {
    s->bitpos = 0;
    s->next = (1 << mcs) + 2;
    s->prev = -1;
    s->outpos = 0;
    s->status = GIF_LZW_OK;
    s->done = 0;
}

// the literals of lane `lane`'s share of the table (once per page: a clear code never changes them)
IMP_GIF_HD void gif_table_start(GifLzwMem* m, int lane) {
    for (int c = lane; c < 256; c += GIF_LANES) {
        m->prefix[c] = 0;
        m->len[c] = 1;
        m->first[c] = (uint8_t)c;
        m->last[c] = (uint8_t)c;
    }
}

IMP_GIF_HD int gif_width_of(int next) {               // the width a code is read with when `next` is the next free code
    const int w = 32 - __builtin_clz((unsigned)next | 1u);             // (the smallest w with (1 << w) > next, without a loop)
    return w > 12 ? 12 : w;
}

// Code j of a round: *free_code = the next free code when it is read (the entry it adds, if it adds one), *width its
// width; returns its bit offset.  The first code after a clear adds no entry, so the count lags one behind there.
IMP_GIF_HD uint32_t gif_code_at(const GifLzwState& s, int j, int* free_code, int* width) {
    const int a = s.prev < 0 ? 1 : 0;
    const int w0 = gif_width_of(s.next);
    uint32_t bits = (uint32_t)j * (uint32_t)w0;
    for (int t = 2; t <= 12; t++) {                   // codes from index i_t on are at least t bits wide (t > w0; a fixed
        const int it = a + (1 << (t - 1)) - s.next;   // trip count: the scan wants this free of branches)
        if (t > w0 && j > it) bits += (uint32_t)(j - it);
    }
    int n = s.next + (j > a ? j - a : 0);
    if (n > GIF_TABLE) n = GIF_TABLE;
    *free_code = n;
    *width = gif_width_of(n);
    return s.bitpos + bits;
}

// What code c is, read as code j of a round with n the next free code (gif_code_at): nothing here needs a table.
IMP_GIF_HD int gif_kind_of(const GifLzwState& s, int mcs, int j, int c, int n) {
    const int clear = 1 << mcs;
    if (c == clear) return GIF_K_CLEAR;
    if (c == clear + 1) return GIF_K_EOI;
    if (j == 0 && s.prev < 0) return c < clear ? GIF_K_CODE : GIF_K_INVALID;
    if (c > n || (c == n && n >= GIF_TABLE)) return GIF_K_INVALID;
    return GIF_K_CODE;
}
// Lane j reads its code (into m->code[j]) and says what it is.  `data` holds `nbytes` bytes; nothing outside is read.
IMP_GIF_HD int gif_extract(GifLzwMem* m, const GifLzwState& s, int mcs, const uint8_t* data, uint32_t nbytes, int j) {
    int n, width;
    const uint32_t at = gif_code_at(s, j, &n, &width);
    m->code[j] = 0;
    if ((uint64_t)at + (uint64_t)width > (uint64_t)nbytes * 8u) return GIF_K_NODATA;
    const uint32_t b = at >> 3;
    uint32_t v = data[b];
    if (b + 1 < nbytes) v |= (uint32_t)data[b + 1] << 8;
    if (b + 2 < nbytes) v |= (uint32_t)data[b + 2] << 16;
    const int c = (int)((v >> (at & 7)) & ((1u << width) - 1u));
    m->code[j] = (uint16_t)c;
    return gif_kind_of(s, mcs, j, c, n);
}

// Does code j of a round of `ncodes` codes add an entry, and which?  (-1: none)
IMP_GIF_HD int gif_entry_of(const GifLzwState& s, int j, int ncodes) {
    if (j >= ncodes || (j == 0 && s.prev < 0)) return -1;
    int n, width;
    (void)gif_code_at(s, j, &n, &width);
    return n < GIF_TABLE ? n : -1;
}
// the lane of this round that adds entry `code` (only for code >= s.next)
IMP_GIF_HD int gif_lane_of(const GifLzwState& s, int code) { return code - s.next + (s.prev < 0 ? 1 : 0); }

// Linking, step 1: lane j's entry hangs on its prefix -- resolved at once when that is an older entry.
IMP_GIF_HD void gif_link_start(GifLzwMem* m, const GifLzwState& s, int j, int ncodes) {
    m->lnk[j] = -1;
    m->acc[j] = 0;
    m->fst[j] = 0;
    if (gif_entry_of(s, j, ncodes) < 0) return;
    const int pfx = j == 0 ? s.prev : (int)m->code[j - 1];
    if (pfx < s.next) {
        m->acc[j] = (uint16_t)(m->len[pfx] + 1);
        m->fst[j] = m->first[pfx];
    } else {
        m->acc[j] = 1;
        m->lnk[j] = (int16_t)gif_lane_of(s, pfx);     // an earlier lane: a code never exceeds the free code it was read at
    }
}
// step 2, six times (chains span at most 64 lanes): read what the linked lane holds ...
IMP_GIF_HD void gif_link_read(GifLzwMem* m, int j) {
    const int k = m->lnk[j];
    if (k < 0 || k >= j) { m->lnk2[j] = -1; m->acc2[j] = 0; m->fst2[j] = m->fst[j]; return; }
    m->acc2[j] = m->acc[k];
    m->lnk2[j] = m->lnk[k];
    m->fst2[j] = m->fst[k];
}
// ... and, behind a barrier, take it over
IMP_GIF_HD void gif_link_write(GifLzwMem* m, int j) {
    if (m->lnk[j] < 0) return;
    m->acc[j] = (uint16_t)(m->acc[j] + m->acc2[j]);
    m->lnk[j] = m->lnk2[j];
    if (m->lnk2[j] < 0) m->fst[j] = m->fst2[j];
}
// step 3: the entry itself.  Its last byte is the first byte of the lane's OWN code -- an older entry, an entry of this
// round, or (KwKwK) the very entry being written, whose first byte is its prefix's.
IMP_GIF_HD void gif_link_finish(GifLzwMem* m, const GifLzwState& s, int j, int ncodes) {
    const int e = gif_entry_of(s, j, ncodes);
    if (e < 0) return;
    const int c = m->code[j];
    int k = c < s.next ? -1 : gif_lane_of(s, c);
    if (k > j) k = j;                                 // (cannot be: gif_extract called such a code invalid)
    m->prefix[e] = (uint16_t)(j == 0 ? s.prev : (int)m->code[j - 1]);
    m->len[e] = m->acc[j];
    m->first[e] = m->fst[j];
    m->last[e] = k < 0 ? m->first[c] : m->fst[k];
}

// the length of lane j's string (0 for a lane behind the round's end)
IMP_GIF_HD uint32_t gif_string_len(const GifLzwMem* m, int j, int ncodes) { return j < ncodes ? m->len[m->code[j]] : 0u; }

// Lane j writes its string, last byte first, at stream positions [at, at + len).
IMP_GIF_HD void gif_emit(const GifLzwMem* m, const GifPlane& p, int j, int ncodes, uint32_t at) {
    if (j >= ncodes) return;
    int c = m->code[j];
    const uint32_t len = m->len[c];
    for (uint32_t i = 0; i < len; i++) {              // bounded by the stored length, whatever the table holds
        gif_store(p, at + (len - 1 - i), m->last[c]);
        c = m->prefix[c] & (GIF_TABLE - 1);
    }
}

// The state behind a round of `ncodes` codes that produced `produced` indices and ended on a code of kind `kind`
// (GIF_K_CODE: all 64 lanes held codes); `last` is the round's last code (read only when ncodes > 0).
IMP_GIF_HD void gif_round_advance(GifLzwState* s, int mcs, int ncodes, int kind, int last, uint32_t produced, uint32_t total) {
    int n, width;
    const uint32_t at = gif_code_at(*s, ncodes, &n, &width);    // where the code behind the last one lies
    if (ncodes > 0) {
        const int a = s->prev < 0 ? 1 : 0;
        int nx = s->next + (ncodes - a);
        s->next = nx > GIF_TABLE ? GIF_TABLE : nx;
        s->prev = last;
    }
    s->bitpos = at;
    s->outpos += produced;
    if (kind == GIF_K_CLEAR) {
        s->bitpos = at + (uint32_t)width;
        s->next = (1 << mcs) + 2;
        s->prev = -1;
    }
    if (s->outpos > total) { s->status = GIF_LZW_LONG; s->done = 1; }
    else if (kind == GIF_K_INVALID) { s->status = GIF_LZW_INVALID; s->done = 1; }
    else if (kind == GIF_K_EOI || kind == GIF_K_NODATA) { s->done = 1; }
    if (s->done && s->status == GIF_LZW_OK && s->outpos < total) s->status = GIF_LZW_SHORT;
}
IMP_GIF_HD void gif_round_end(GifLzwState* s, const GifLzwMem* m, int mcs, int ncodes, int kind, uint32_t produced, uint32_t total) {
    gif_round_advance(s, mcs, ncodes, kind, ncodes > 0 ? (int)m->code[ncodes - 1] : 0, produced, total);
}

// ---------------------------------------------------------------- a page cut at its clear codes (IMPGPU_GIF_SPLIT)
// LZW is sequential only between clear codes: behind one the decoder's state is known (an empty table, the first code
// width), so the stretch up to the next clear can be decoded by a wavefront of its own.  Three passes:
//   SCAN    the round loop WITHOUT a table (gif_scan_fetch / gif_scan_kind: gif_extract's rules; gif_round_advance with
//           produced = 0) finds the clears.  Its rounds are GIF_SCAN_CODES codes, 16 per lane: with no table to build a
//           round's length is free, and a round costs one memory latency whatever its length.  It stops
//           where any decoder would stop for a reason that needs no table: end-of-information, no data, a code above the
//           free code, a first-after-clear code that is no literal.  (Indices beyond the page it cannot see.)  Its output
//           is the page's SEGMENTS.  Segment 0 starts at bit 0; a clear is a CUT -- the segment ends just behind it, the
//           next one starts there -- when at least IMPGPU_GIF_SPLIT_MIN_BYTES of stream lie between the segment's start
//           and the bit behind the clear and the page's table (gif_seg_cap entries) has room; any other clear stays
//           inside its segment and is the segment decoder's, as in the one-wave route.  The last segment is open
//           (GIF_SEG_OPEN): the stream ends it.  Which clears are cuts changes no answer.
//   LENGTH  per segment, from the fresh state at its start: the rounds without gif_emit, until bitpos IS the segment's end
//           (the scan walked the same code grid from the same state) or the round ends the stream; how many indices
//           the segment holds (saturating at width x height + 1) and whether it ended on an invalid code.
//   EMIT    per segment: the same rounds with gif_emit, at the sum of the earlier segments' lengths; nothing when that
//           sum is at or past width x height.  gif_split_status folds the records into the one-wave decoder's word.
constexpr uint32_t GIF_SEG_OPEN = 0xFFFFFFFFu;
enum : uint32_t { GIF_SEG_RAN = 0, GIF_SEG_ENDED = 1, GIF_SEG_INVALID = 2 };     // ran to its end / EOI or no data / invalid
struct GifSeg { uint32_t start, end, produced, ended; };     // bit offsets (the scan's), then the length pass's record
// A page's segment block in device memory: GifSeg[0].start holds the COUNT (its other words are free), the segments follow.
IMP_GIF_HD uint32_t gif_seg_cap(uint32_t data_bytes) { return data_bytes / (uint32_t)IMPGPU_GIF_SPLIT_MIN_BYTES + 1u; }

// The scan's rounds: lane l holds codes l, l + 64, ... of GIF_SCAN_CODES.  gif_code_at's closed form holds for any j.
constexpr int GIF_SCAN_PER_LANE = 16;
constexpr int GIF_SCAN_CODES = GIF_LANES * GIF_SCAN_PER_LANE;
struct GifScanCode { uint32_t at, v; int n, width; };
// Code j's three bytes, read WITHOUT a branch, so that the loads of a lane's 16 codes are in flight together: every index
// is clamped into the data, and a clamped byte only ever supplies bits that lie past the data's end -- a code that
// reaches there is GIF_K_NODATA whatever was read.  Nothing outside `data` is read.  nbytes >= 1: an empty stream has
// no round (gif_scan_empty).
IMP_GIF_HD GifScanCode gif_scan_fetch(const GifLzwState& s, const uint8_t* data, uint32_t nbytes, int j) {
    GifScanCode c;
    c.at = gif_code_at(s, j, &c.n, &c.width);
    const uint32_t last = nbytes - 1, b = c.at >> 3;
    const uint32_t b0 = b < last ? b : last, b1 = b + 1 < last ? b + 1 : last, b2 = b + 2 < last ? b + 2 : last;
    c.v = (uint32_t)data[b0] | (uint32_t)data[b1] << 8 | (uint32_t)data[b2] << 16;
    return c;
}
IMP_GIF_HD int gif_scan_kind(const GifLzwState& s, int mcs, uint32_t nbytes, int j, const GifScanCode& c) {
    if ((uint64_t)c.at + (uint64_t)c.width > (uint64_t)nbytes * 8u) return GIF_K_NODATA;
    return gif_kind_of(s, mcs, j, (int)((c.v >> (c.at & 7)) & ((1u << c.width) - 1u)), c.n);
}

// the scan's state between two rounds
struct GifScan { GifLzwState s; uint32_t nseg, seg_start; };
IMP_GIF_HD void gif_scan_start(GifScan* sc, int mcs) {
    gif_state_start(&sc->s, mcs);
    sc->nseg = 0;
    sc->seg_start = 0;
}
// Behind a round of the scan (wave-uniform): the state moves on, and a clear that is a cut closes segs[nseg].  When the
// scan is done the last segment is left open.
IMP_GIF_HD void gif_scan_round_end(GifScan* sc, int mcs, int ncodes, int kind, GifSeg* segs, uint32_t cap, bool writer) {
    gif_round_advance(&sc->s, mcs, ncodes, kind, 0, 0u, 0u);
    if (kind == GIF_K_CLEAR && sc->s.bitpos - sc->seg_start >= (uint32_t)IMPGPU_GIF_SPLIT_MIN_BYTES * 8u && sc->nseg + 1 < cap) {
        if (writer) { segs[sc->nseg].start = sc->seg_start; segs[sc->nseg].end = sc->s.bitpos; }
        sc->nseg++;
        sc->seg_start = sc->s.bitpos;
    }
    if (sc->s.done) {
        if (writer) { segs[sc->nseg].start = sc->seg_start; segs[sc->nseg].end = GIF_SEG_OPEN; }
        sc->nseg++;
    }
}

// the scan of a stream of no bytes: one open segment at bit 0
IMP_GIF_HD uint32_t gif_scan_empty(GifSeg* segs, bool writer) {
    if (writer) { segs[0].start = 0; segs[0].end = GIF_SEG_OPEN; }
    return 1;
}

// a segment's decoder before its first round
IMP_GIF_HD void gif_segment_start(GifLzwState* s, int mcs, uint32_t start) {
    gif_state_start(s, mcs);
    s->bitpos = start;
}
// ... and whether it goes on: not past its end, not once the count has saturated (the length pass may stop there)
IMP_GIF_HD bool gif_segment_goes_on(const GifLzwState& s, uint32_t end) { return !s.done && s.bitpos < end; }
// what the length pass records for a segment whose decoder stopped in state `s` (total = width x height)
IMP_GIF_HD void gif_segment_record(GifSeg* seg, const GifLzwState& s, uint32_t total) {
    seg->produced = s.outpos > total ? total + 1u : s.outpos;
    seg->ended = s.status == GIF_LZW_INVALID ? GIF_SEG_INVALID : s.done ? GIF_SEG_ENDED : GIF_SEG_RAN;
}
// Segment k's base: the indices in front of it (saturating at total + 1); *live = it emits: nothing in front of it went
// past the page or ended invalid.
IMP_GIF_HD uint32_t gif_split_base(const GifSeg* segs, uint32_t k, uint32_t total, bool* live) {
    uint64_t sum = 0;
    *live = true;
    for (uint32_t i = 0; i < k; i++) {
        sum += segs[i].produced;
        if (sum > total) { *live = false; return total + 1u; }
        if (segs[i].ended == GIF_SEG_INVALID) *live = false;
    }
    if (sum >= total) *live = false;
    return (uint32_t)sum;
}
// The page's status word, from the records in stream order: the one-wave decoder's for every stream (it checks LONG
// before INVALID at a round's end, and everything before the first problem is the same).
IMP_GIF_HD int gif_split_status(const GifSeg* segs, uint32_t count, uint32_t total) {
    uint64_t sum = 0;
    for (uint32_t i = 0; i < count; i++) {
        sum += segs[i].produced;
        if (sum > total) return GIF_LZW_LONG;
        if (segs[i].ended == GIF_SEG_INVALID) return GIF_LZW_INVALID;
    }
    return sum < total ? GIF_LZW_SHORT : GIF_LZW_OK;
}

// ---------------------------------------------------------------- the host's two decoders (impgpu_gif_pages)
// how = 1: the rounds above, one lane after the other where the wave runs them side by side
inline int gif_lzw_rounds_host(const uint8_t* data, uint32_t nbytes, int mcs, const GifPlane& p, GifLzwMem* m) {
    GifLzwState s;
    gif_state_start(&s, mcs);
    for (int j = 0; j < GIF_LANES; j++) gif_table_start(m, j);
    for (int row = 0; row < p.h; row++) gif_pad_row(p, row);
    while (!s.done) {
        int ncodes = GIF_LANES, kind = GIF_K_CODE;
        for (int j = GIF_LANES - 1; j >= 0; j--) {                       // (the ballot: the FIRST lane that is not a plain code)
            const int k = gif_extract(m, s, mcs, data, nbytes, j);
            if (k != GIF_K_CODE) { ncodes = j; kind = k; }
        }
        for (int j = 0; j < GIF_LANES; j++) gif_link_start(m, s, j, ncodes);
        for (int it = 0; it < 6; it++) {
            for (int j = 0; j < GIF_LANES; j++) gif_link_read(m, j);
            for (int j = 0; j < GIF_LANES; j++) gif_link_write(m, j);
        }
        for (int j = 0; j < GIF_LANES; j++) gif_link_finish(m, s, j, ncodes);
        uint32_t at = s.outpos;
        for (int j = 0; j < GIF_LANES; j++) {                            // (the scan)
            gif_emit(m, p, j, ncodes, at);
            at += gif_string_len(m, j, ncodes);
        }
        gif_round_end(&s, m, mcs, ncodes, kind, at - s.outpos, p.total);
    }
    return s.status;
}

// how = 0: the plain sequential decoder, the same verdicts
inline int gif_lzw_plain_host(const uint8_t* data, uint32_t nbytes, int mcs, const GifPlane& p) {
    static thread_local uint16_t prefix[GIF_TABLE], len[GIF_TABLE];
    static thread_local uint8_t first[GIF_TABLE], last[GIF_TABLE];
    const int clear = 1 << mcs;
    for (int c = 0; c < 256; c++) { prefix[c] = 0; len[c] = 1; first[c] = last[c] = (uint8_t)c; }
    for (int row = 0; row < p.h; row++) gif_pad_row(p, row);
    int next = clear + 2, width = mcs + 1, prev = -1, status = GIF_LZW_OK;
    uint64_t bit = 0, outpos = 0;
    for (;;) {
        if (bit + (uint64_t)width > (uint64_t)nbytes * 8u) break;
        uint32_t v = 0;
        for (int k = 0; k < 3; k++)
            if ((bit >> 3) + (uint64_t)k < nbytes) v |= (uint32_t)data[(bit >> 3) + k] << (8 * k);
        const int c = (int)((v >> (bit & 7)) & ((1u << width) - 1u));
        bit += (uint64_t)width;
        if (c == clear) { next = clear + 2; width = mcs + 1; prev = -1; continue; }
        if (c == clear + 1) break;
        if (prev < 0) {
            if (c >= clear) { status = GIF_LZW_INVALID; break; }
        } else {
            if (c > next || (c == next && next >= GIF_TABLE)) { status = GIF_LZW_INVALID; break; }
            if (next < GIF_TABLE) {
                prefix[next] = (uint16_t)prev;
                len[next] = (uint16_t)(len[prev] + 1);
                first[next] = first[prev];
                last[next] = c == next ? first[prev] : first[c];
                next++;
                if (next == (1 << width) && width < 12) width++;
            }
        }
        const uint32_t n = len[c];
        int q = c;
        for (uint32_t i = 0; i < n; i++) {
            gif_store(p, (uint32_t)(outpos + (n - 1 - i)), last[q]);
            q = prefix[q];
        }
        outpos += n;
        prev = c;
        if (outpos > p.total) { status = GIF_LZW_LONG; break; }
    }
    if (status == GIF_LZW_OK && outpos < p.total) status = GIF_LZW_SHORT;
    return status;
}

// the three passes of a cut page, one lane after the other: the scan ...
inline uint32_t gif_scan_host(const uint8_t* data, uint32_t nbytes, int mcs, GifSeg* segs, uint32_t cap) {
    if (nbytes == 0) return gif_scan_empty(segs, true);
    GifScan sc;
    gif_scan_start(&sc, mcs);
    while (!sc.s.done) {
        int ncodes = GIF_SCAN_CODES, kind = GIF_K_CODE;
        for (int j = GIF_SCAN_CODES - 1; j >= 0; j--) {
            const int k = gif_scan_kind(sc.s, mcs, nbytes, j, gif_scan_fetch(sc.s, data, nbytes, j));
            if (k != GIF_K_CODE) { ncodes = j; kind = k; }
        }
        gif_scan_round_end(&sc, mcs, ncodes, kind, segs, cap, true);
    }
    return sc.nseg;
}
// ... and a segment's rounds from `base`, with gif_emit (the emit pass) or without (the length pass, base 0); the
// decoder's state where it stopped
inline GifLzwState gif_segment_host(const uint8_t* data, uint32_t nbytes, int mcs, const GifPlane& p, GifLzwMem* m, const GifSeg& seg,
                                    uint32_t base, bool emit) {
    GifLzwState s;
    gif_segment_start(&s, mcs, seg.start);
    s.outpos = base;
    for (int j = 0; j < GIF_LANES; j++) gif_table_start(m, j);
    while (gif_segment_goes_on(s, seg.end)) {
        int ncodes = GIF_LANES, kind = GIF_K_CODE;
        for (int j = GIF_LANES - 1; j >= 0; j--) {
            const int k = gif_extract(m, s, mcs, data, nbytes, j);
            if (k != GIF_K_CODE) { ncodes = j; kind = k; }
        }
        for (int j = 0; j < GIF_LANES; j++) gif_link_start(m, s, j, ncodes);
        for (int it = 0; it < 6; it++) {
            for (int j = 0; j < GIF_LANES; j++) gif_link_read(m, j);
            for (int j = 0; j < GIF_LANES; j++) gif_link_write(m, j);
        }
        for (int j = 0; j < GIF_LANES; j++) gif_link_finish(m, s, j, ncodes);
        uint32_t at = s.outpos;
        for (int j = 0; j < GIF_LANES; j++) {
            if (emit) gif_emit(m, p, j, ncodes, at);
            at += gif_string_len(m, j, ncodes);
        }
        gif_round_end(&s, m, mcs, ncodes, kind, at - s.outpos, p.total);
    }
    return s;
}
// how = 2 (impgpu_gif_pages_split): scan, length pass and emit pass as k_gif_lzw_scan / _len / _emit run them
inline int gif_lzw_split_host(const uint8_t* data, uint32_t nbytes, int mcs, const GifPlane& p, GifLzwMem* m, int* nseg) {
    std::vector<GifSeg> segs(gif_seg_cap(nbytes));
    const uint32_t count = gif_scan_host(data, nbytes, mcs, segs.data(), (uint32_t)segs.size());
    if (nseg) *nseg = (int)count;
    for (int row = 0; row < p.h; row++) gif_pad_row(p, row);
    if (count == 1) return gif_segment_host(data, nbytes, mcs, p, m, segs[0], 0, true).status;     // (no length pass: today's loop)
    for (uint32_t k = 0; k < count; k++) gif_segment_record(&segs[k], gif_segment_host(data, nbytes, mcs, p, m, segs[k], 0, false), p.total);
    for (uint32_t k = 0; k < count; k++) {
        bool live;
        const uint32_t base = gif_split_base(segs.data(), k, p.total, &live);
        if (live) (void)gif_segment_host(data, nbytes, mcs, p, m, segs[k], base, true);
    }
    return gif_split_status(segs.data(), count, p.total);
}

inline int gif_pitch(int w) { return (w + 3) & ~3; }
// a page's bit offsets are 32-bit words: compressed pages of 256 MB and more go back to the host decoder
constexpr size_t GIF_DATA_MAX = size_t(1) << 28;

// impgpu_gif_pages / impgpu_gif_pages_split: every page's plane, one after the other, by one of the decoders above
// (how = 2: the split route's passes; segments[f], when given, = page f's segment count)
inline int gif_pages_any(const unsigned char* blob, size_t size, int how, unsigned char* out, size_t capacity, size_t* length,
                         int* segments, int pages_capacity) {
    if (length) *length = 0;
    std::vector<impgpu_gif_desc> pages(64);
    int count = 0, cw = 0, ch = 0;
    int rc = impgpu_gif_walk(blob, size, pages.data(), (int)pages.size(), &count, &cw, &ch);
    if (rc == IMP_ERROR_MALLOC_FAILED) {
        pages.resize((size_t)count);
        rc = impgpu_gif_walk(blob, size, pages.data(), count, &count, &cw, &ch);
    }
    if (rc) return rc;
    size_t need = 0;
    for (int f = 0; f < count; f++)
        if (pages[f].data_bytes >= GIF_DATA_MAX) return IMP_ERROR_UNSUPPORTED;
    for (int f = 0; f < count; f++) need += (size_t)gif_pitch(pages[f].width) * pages[f].height;
    if (length) *length = need;
    if (!out || capacity < need) return IMP_ERROR_MALLOC_FAILED;
    std::vector<uint8_t> data;
    std::vector<GifLzwMem> mem(how != 0 ? 1 : 0);
    size_t at = 0;
    int bad = 0;
    for (int f = 0; f < count; f++) {
        const impgpu_gif_desc& d = pages[f];
        data.assign(d.data_bytes + 1, 0);
        impgpu_gif_gather(blob, &d, data.data());
        GifPlane p;
        p.plane = out + at;
        p.w = d.width; p.h = d.height; p.pitch = gif_pitch(d.width); p.interlaced = d.interlaced;
        p.total = (uint32_t)d.width * (uint32_t)d.height;
        int nseg = 0;
        const int st = how == 2 ? gif_lzw_split_host(data.data(), (uint32_t)d.data_bytes, d.min_code_size, p, mem.data(), &nseg)
                     : how == 1 ? gif_lzw_rounds_host(data.data(), (uint32_t)d.data_bytes, d.min_code_size, p, mem.data())
                                : gif_lzw_plain_host(data.data(), (uint32_t)d.data_bytes, d.min_code_size, p);
        if (segments && f < pages_capacity) segments[f] = nseg;
        if (st != GIF_LZW_OK) bad = 1;
        at += (size_t)p.pitch * p.h;
    }
    return bad ? IMP_ERROR_DECODE_FAILED : IMP_OK;
}
inline int gif_pages_host(const unsigned char* blob, size_t size, int how, unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (how != 0 && how != 1) return IMP_ERROR_INVALID_ARGS;
    return gif_pages_any(blob, size, how, out, capacity, length, nullptr, 0);
}
inline int gif_pages_split_host(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, size_t* length,
                                int* segments, int pages_capacity) {
    if (segments && pages_capacity < 0) { if (length) *length = 0; return IMP_ERROR_INVALID_ARGS; }
    return gif_pages_any(blob, size, 2, out, capacity, length, segments, pages_capacity);
}

}  // namespace imp
