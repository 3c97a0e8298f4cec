// imp_gif_enc.h -- GIF answers written on the device: the lanes' logic of the five launches of imp_gif_enc.hip, shared with
// impgpu_gif_encode_host (imp_gif_enc.cpp), which runs the same functions one lane after the other (and under the
// sanitizers, tests/c/gif_enc_fuzz.cpp).  Every function here is __host__ __device__ and depends on imp_gif.h alone.
//
//   SETS    every pixel becomes a KEY (gif_enc_key: a colour, or "transparent"); a workgroup dedupes its pixels in an LDS
//           hash set (gif_set_insert: open addressing, compare-and-swap) and adds what is left to the frame's set in
//           device memory (gif_frame_set_add), which raises its overflow flag at the 257th key and takes nothing more.
//   TABLES  per album: every frame's keys sorted by rank (gif_rank) -- colours ascending by R<<16 | G<<8 | B, the
//           transparent key last -- their union, and the verdict: one global table, local tables, or refused.
//   INDEX   the table in LDS, a binary search per pixel (gif_table_find), a tight w x h plane of indices.
//   LZW     a wavefront per SEGMENT of the raster stream.  The greedy walk (gif_enc_step) is sequential and wave-uniform;
//           its dictionary is an LDS hash table of (prefix << 8 | byte) << 12 | code words.  The codes it emits are
//           collected in batches of up to 65 and packed by the lanes: a code's width and bit offset are gif_code_at's
//           closed form of its index in the batch (the decoder's view: the first code after a clear adds no entry), so
//           64 lanes place 64 codes at a time (gif_enc_pack_lane), and whole words leave for the segment's scratch slot
//           (gif_enc_drain_lane).  A clear or end-of-information code always ends its batch.
//   PACK    per frame a prefix sum of the segments' bit lengths; every lane then makes whole bytes of the stream from the
//           segments' bit strings (gif_enc_stream_byte) and stores them at their framed place behind the min_code_size
//           byte, length bytes and terminator included (gif_enc_put_byte).
//
// Safe by construction: a probe loop ends after one trip round its table; gif_enc_drain_lane drops words at or past the
// slot's capacity; gif_enc_put_byte drops bytes at or past the region's.
#pragma once
#include <string.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <algorithm>
#include <vector>
#endif
#include "imp_gif.h"

namespace imp {

#if defined(__HIP_DEVICE_COMPILE__)
#define GIF_ENC_UNI(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))      // a wave-uniform value, said to the compiler
#else
#define GIF_ENC_UNI(x) ((uint32_t)(x))
#endif

// the three read-modify-writes of the lanes; plain on the host, where one lane runs after the other
IMP_GIF_HD uint32_t gif_cas(uint32_t* p, uint32_t expect, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(p, expect, v);
#else
    const uint32_t old = *p;
    if (old == expect) *p = v;
    return old;
#endif
}
IMP_GIF_HD uint32_t gif_add(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, v);
#else
    const uint32_t old = *p;
    *p = old + v;
    return old;
#endif
}
IMP_GIF_HD void gif_or(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(p, v);
#else
    *p |= v;
#endif
}

// ---------------------------------------------------------------- keys and colour sets
constexpr uint32_t GIF_KEY_COLOUR = 0x01000000u;          // | R << 16 | G << 8 | B
constexpr uint32_t GIF_KEY_TRANSPARENT = 0x02000000u;     // sorts behind every colour: the table's "next entry"
constexpr int GIF_SET_SLOTS = 1024;                        // 0 = empty; a quarter full at the 257 keys that matter
constexpr uint32_t GIF_SET_MAX = 256;                      // keys a table holds
struct GifColourSet { uint32_t slot[GIF_SET_SLOTS]; uint32_t count, overflow, pad[2]; };

IMP_GIF_HD uint32_t gif_enc_key_bgra(uint32_t u) { return (u >> 24) == 0 ? GIF_KEY_TRANSPARENT : GIF_KEY_COLOUR | (u & 0xFFFFFFu); }
// the key of the pixel at `px` (B,G,R[,A]); `wide`: a 4-channel pixel at a dword address
IMP_GIF_HD uint32_t gif_enc_key(const uint8_t* px, int channels, bool wide) {
    if (wide) return gif_enc_key_bgra(*(const uint32_t*)px);
    const uint32_t u = (uint32_t)px[0] | (uint32_t)px[1] << 8 | (uint32_t)px[2] << 16;
    return channels == 4 ? gif_enc_key_bgra(u | (uint32_t)px[3] << 24) : GIF_KEY_COLOUR | u;
}
// the key of stream position `pos` of a frame
struct GifEncFrame { const uint8_t* src; int w, h, c, step, wide; };
IMP_GIF_HD uint32_t gif_enc_key_at(const GifEncFrame& f, uint32_t pos) {
    const uint32_t y = pos / (uint32_t)f.w, x = pos - y * (uint32_t)f.w;
    return gif_enc_key(f.src + (size_t)y * (size_t)f.step + (size_t)x * (size_t)f.c, f.c, f.wide != 0);
}

// 1: the key is new, 0: it was there, -1: no room (only a set of GIF_SET_SLOTS other keys says so)
IMP_GIF_HD int gif_set_insert(uint32_t* slot, uint32_t key) {
    uint32_t h = (key * 2654435761u) >> 22;
    for (int i = 0; i < GIF_SET_SLOTS; i++) {
        uint32_t old = *(volatile uint32_t*)&slot[h];
        if (old == 0u) old = gif_cas(&slot[h], 0u, key);
        if (old == 0u) return 1;
        if (old == key) return 0;
        h = (h + 1u) & (uint32_t)(GIF_SET_SLOTS - 1);
    }
    return -1;
}
// a key into the frame's set; past GIF_SET_MAX keys the flag goes up and the set takes no more
IMP_GIF_HD void gif_frame_set_add(GifColourSet* fs, uint32_t key) {
    if (*(volatile uint32_t*)&fs->overflow) return;
    const int r = gif_set_insert(fs->slot, key);
    if (r == 0) return;
    if (r < 0 || gif_add(&fs->count, 1u) + 1u > GIF_SET_MAX) *(volatile uint32_t*)&fs->overflow = 1u;
}

// ---------------------------------------------------------------- tables
// What the TABLES launch leaves per frame (and the host reads back with the stream lengths).
enum : uint32_t { GIF_ENC_REFUSED = 0, GIF_ENC_GLOBAL = 1, GIF_ENC_LOCAL = 2 };
struct GifEncRec {
    uint32_t mode;           // GIF_ENC_*: the album's verdict, the same in all its frames
    uint32_t table_frame;    // the frame (of the call) whose table slot holds this frame's table: the album's first, or itself
    uint32_t nkeys;          // keys in that table, the transparent one included
    uint32_t has_trans;      // t_i: this frame has a transparent pixel
    uint32_t trans_index;    // the table's transparent index (nkeys - 1), or 0xFFFFFFFF when it has none
    uint32_t mcs;
    uint32_t stream_bytes;   // PACK: the LZW stream's length
    uint32_t pad;
};
// the rank of list[i] among `n` distinct keys
IMP_GIF_HD uint32_t gif_rank(const uint32_t* list, uint32_t n, uint32_t i) {
    const uint32_t k = list[i];
    uint32_t r = 0;
    for (uint32_t j = 0; j < n; j++) r += list[j] < k ? 1u : 0u;
    return r;
}
IMP_GIF_HD uint32_t gif_table_size(uint32_t nkeys) {       // the next power of two >= max(2, nkeys)
    uint32_t t = 2;
    while (t < nkeys) t <<= 1;
    return t;
}
IMP_GIF_HD uint32_t gif_table_mcs(uint32_t nkeys) {        // max(2, log2(table size))
    uint32_t b = 1;
    while ((1u << b) < nkeys) b++;
    return b < 2 ? 2u : b;
}
IMP_GIF_HD void gif_rec_fill(GifEncRec* r, uint32_t mode, uint32_t table_frame, uint32_t nkeys, bool table_has_trans) {
    r->mode = mode;
    r->table_frame = table_frame;
    r->nkeys = nkeys;
    r->trans_index = table_has_trans ? nkeys - 1u : 0xFFFFFFFFu;
    r->mcs = gif_table_mcs(nkeys);
}
// the index of `key` in a table of 256 ascending words (the keys, then 0xFFFFFFFF): how many entries lie below it
IMP_GIF_HD uint32_t gif_table_find(const uint32_t* tab, uint32_t key) {
    uint32_t lo = 0;
    for (uint32_t step = 128; step; step >>= 1)
        if (tab[lo + step - 1] < key) lo += step;
    return lo;
}

// ---------------------------------------------------------------- a segment's LZW
constexpr int GIF_ENC_SLOTS = 8192;                        // at most 3838 entries between two clears: under half full
constexpr uint32_t GIF_ENC_EMPTY = 0xFFFFFFFFu;            // (no entry looks like it: code 4095 never has prefix 4095)
constexpr int GIF_ENC_CHUNK = 1024;                        // indices staged per load: 16 bytes a lane
constexpr int GIF_ENC_BATCH = 64;                          // a batch is due at this many codes ...
constexpr int GIF_ENC_CODES = 72;                          // ... and never holds more than 65
constexpr int GIF_ENC_WORDS = 32;                          // 31 carried bits + 65 x 12 = 811 bits
// A wavefront's working set, 33.3 KB: in LDS on the device (four fit a CU's 160 KB), an ordinary object on the host.
struct alignas(16) GifEncMem {
    alignas(16) uint32_t slot[GIF_ENC_SLOTS];
    uint32_t bits[GIF_ENC_WORDS];                          // word 0 is the slot word that holds bit s.bitpos
    uint16_t code[GIF_ENC_CODES];
    alignas(16) uint8_t px[GIF_ENC_CHUNK];
};
// wave-uniform: the encoder between two indices
struct GifEncState {
    GifLzwState s;           // the DECODER's view at the batch's first code: bitpos (in the segment's bit string), next, prev
    int cur;                 // the pending code (-1: none)
    int next;                // the encoder's next entry
    int n;                   // codes in the batch
    int tail;                // the batch ends on 1: a clear code, 2: end-of-information
};
// pixels [k * segment, ...) of a stream of `total`: how many segments, and the words a segment's slot holds: 12 bits for
// every code a segment of `segment` pixels can emit (one per pixel, a clear per 2048 at the most, the closing pair)
IMP_GIF_HD uint32_t gif_enc_segments(uint32_t total, uint32_t segment) { return (total + segment - 1u) / segment; }
IMP_GIF_HD uint32_t gif_enc_slot_words(uint32_t segment) { return (uint32_t)((12ull * ((uint64_t)segment + segment / 2048u + 4u) + 31u) / 32u) + 1u; }

IMP_GIF_HD void gif_enc_start(GifEncState* e, int mcs) {
    gif_state_start(&e->s, mcs);
    e->cur = -1;
    e->next = (1 << mcs) + 2;
    e->n = 0;
    e->tail = 0;
}
IMP_GIF_HD void gif_enc_clear_lane(GifEncMem* m, int lane) {
    for (int i = lane * 4; i < GIF_ENC_SLOTS; i += GIF_LANES * 4) {
        m->slot[i] = GIF_ENC_EMPTY; m->slot[i + 1] = GIF_ENC_EMPTY; m->slot[i + 2] = GIF_ENC_EMPTY; m->slot[i + 3] = GIF_ENC_EMPTY;
    }
}
IMP_GIF_HD void gif_enc_rewind_lane(GifEncMem* m, uint32_t carry, int lane) {
    if (lane < GIF_ENC_WORDS) m->bits[lane] = lane == 0 ? carry : 0u;
}
// every lane says the same: on the device the stores of a uniform value to a uniform address are one LDS write
IMP_GIF_HD void gif_enc_push(GifEncMem* m, GifEncState* e, int code) {
    m->code[e->n] = (uint16_t)code;
    e->n++;
}
IMP_GIF_HD void gif_enc_push_tail(GifEncMem* m, GifEncState* e, int mcs, int tail) {
    gif_enc_push(m, e, (1 << mcs) + (tail == 2 ? 1 : 0));
    e->tail = tail;
}
// One index of the stream.  true: the batch is due -- pack, drain and gif_enc_batch_end before the next index.
IMP_GIF_HD bool gif_enc_step(GifEncMem* m, GifEncState* e, int mcs, uint32_t b) {
    if (e->cur < 0) { e->cur = (int)b; return false; }
    const uint32_t key = ((uint32_t)e->cur << 8) | b;
    uint32_t h = (key * 2654435761u) >> 19;
    uint32_t v = GIF_ENC_UNI(m->slot[h]);
    for (int left = GIF_ENC_SLOTS; v != GIF_ENC_EMPTY && (v >> 12) != key && --left;) {      // (ends at an empty slot long before)
        h = (h + 1u) & (uint32_t)(GIF_ENC_SLOTS - 1);
        v = GIF_ENC_UNI(m->slot[h]);
    }
    if (v != GIF_ENC_EMPTY && (v >> 12) == key) { e->cur = (int)(v & 0xFFFu); return false; }
    gif_enc_push(m, e, e->cur);
    if (e->next < GIF_TABLE) {
        m->slot[h] = (key << 12) | (uint32_t)e->next;
        e->next++;
    } else {
        gif_enc_push_tail(m, e, mcs, 1);                                // the table is full and another entry is due
    }
    e->cur = (int)b;
    return e->n >= GIF_ENC_BATCH || e->tail != 0;
}
// Behind a segment's last index: the pending code, then the clear that opens the next segment (at THIS segment's width)
// or, behind the last one, end-of-information.  The batch is due.
IMP_GIF_HD void gif_enc_finish(GifEncMem* m, GifEncState* e, int mcs, bool last) {
    if (e->cur >= 0) gif_enc_push(m, e, e->cur);
    e->cur = -1;
    gif_enc_push_tail(m, e, mcs, last ? 2 : 1);
}
// the batch: lane `lane` places codes lane and lane + 64
IMP_GIF_HD void gif_enc_pack_lane(GifEncMem* m, const GifEncState& e, int lane) {
    const uint32_t base = e.s.bitpos & ~31u;
    for (int j = lane; j < e.n; j += GIF_LANES) {
        int n, width;
        const uint32_t at = gif_code_at(e.s, j, &n, &width) - base;
        const uint32_t c = m->code[j];
        gif_or(&m->bits[at >> 5], c << (at & 31u));
        if ((at & 31u) + (uint32_t)width > 32u) gif_or(&m->bits[(at >> 5) + 1u], c >> (32u - (at & 31u)));
    }
}
IMP_GIF_HD uint32_t gif_enc_batch_bits(const GifEncState& e) {         // the bit behind the batch
    int n, width;
    return gif_code_at(e.s, e.n, &n, &width);
}
// the batch's finished words into the segment's slot of `cap` words
IMP_GIF_HD void gif_enc_drain_lane(const GifEncMem* m, const GifEncState& e, uint32_t* words, uint32_t cap, int lane) {
    const uint32_t w0 = e.s.bitpos >> 5, full = (gif_enc_batch_bits(e) >> 5) - w0;
    if ((uint32_t)lane < full && w0 + (uint32_t)lane < cap) words[w0 + (uint32_t)lane] = m->bits[lane];
}
IMP_GIF_HD uint32_t gif_enc_carry(const GifEncMem* m, const GifEncState& e) {    // the unfinished word behind them
    return m->bits[(gif_enc_batch_bits(e) >> 5) - (e.s.bitpos >> 5)];
}
IMP_GIF_HD void gif_enc_batch_end(GifEncState* e, int mcs) {
    const uint32_t end = gif_enc_batch_bits(*e);
    if (e->tail) {
        e->s.next = (1 << mcs) + 2;
        e->s.prev = -1;
        e->next = (1 << mcs) + 2;
    } else {
        const int nx = e->s.next + e->n - (e->s.prev < 0 ? 1 : 0);
        e->s.next = nx > GIF_TABLE ? GIF_TABLE : nx;
        e->s.prev = 0;
    }
    e->s.bitpos = end;
    e->n = 0;
    e->tail = 0;
}
// the segment's last, unfinished word (lane 0, behind the last batch)
IMP_GIF_HD void gif_enc_last_word(const GifEncMem* m, const GifEncState& e, uint32_t* words, uint32_t cap) {
    if ((e.s.bitpos & 31u) && (e.s.bitpos >> 5) < cap) words[e.s.bitpos >> 5] = m->bits[0];
}

// ---------------------------------------------------------------- pack
IMP_GIF_HD uint32_t gif_enc_framed_size(uint32_t nbytes) { return nbytes + (nbytes + 254u) / 255u + 1u; }    // sub-blocks + terminator
// bits [pos, pos + count) of a segment's bit string, count <= 8: from two shifted bytes
IMP_GIF_HD uint32_t gif_enc_bits_at(const uint8_t* seg, uint32_t pos, uint32_t count) {
    const uint32_t b = pos >> 3, sh = pos & 7u;
    uint32_t v = seg[b];
    if (sh + count > 8u) v |= (uint32_t)seg[b + 1] << 8;
    return (v >> sh) & ((1u << count) - 1u);
}
struct GifPackCursor { uint32_t seg, start; };             // the segment that holds the next bit, and the stream bit it starts at
// the stream's byte at bit `pos` (c->start <= pos); the cursor moves on with it
IMP_GIF_HD uint32_t gif_enc_stream_byte(const uint32_t* segbits, uint32_t nseg, const uint8_t* scratch, size_t slot_bytes,
                                        GifPackCursor* c, uint32_t pos) {
    uint32_t v = 0, got = 0;
    while (got < 8u && c->seg < nseg) {
        const uint32_t len = segbits[c->seg], avail = c->start + len - pos;
        if (!avail) { c->start += len; c->seg++; continue; }
        const uint32_t take = 8u - got < avail ? 8u - got : avail;
        v |= gif_enc_bits_at(scratch + (size_t)c->seg * slot_bytes, pos - c->start, take) << got;
        got += take;
        pos += take;
    }
    return v;
}
// byte k of a stream of `nbytes` at its framed place in a region of `cap` bytes, with the length byte in front of a
// sub-block's first byte and the terminator behind the stream's last
IMP_GIF_HD void gif_enc_put_byte(uint8_t* out, size_t cap, uint32_t k, uint32_t nbytes, uint32_t v) {
    const size_t at = (size_t)k + k / 255u + 1u;
    if (at < cap) out[at] = (uint8_t)v;
    if (k % 255u == 0u && at - 1 < cap) out[at - 1] = (uint8_t)(nbytes - k < 255u ? nbytes - k : 255u);
    if (k + 1u == nbytes && at + 1 < cap) out[at + 1] = 0;
}

// ---------------------------------------------------------------- the launches' descriptors (imp_gif_enc.hip)
// Everything of a call lies in ONE device block `mem`; offsets count from its start.  A frame's plane, its segments'
// scratch slots (slot_words each) and its output region (out_cap bytes: the framed stream) are its own.
constexpr int GIF_ENC_PX_BLOCK = 4096;                     // pixels a workgroup of SETS / INDEX takes: 16 per lane
constexpr int GIF_ENC_PACK_BLOCK = 4096;                   // stream bytes a workgroup of PACK makes: 16 per lane
struct GifEncFrameDesc {
    const uint8_t* src;
    int w, h, c, step, wide, album;
    uint32_t total, segment, nseg, seg0, slot_words, out_cap;
    long long plane_off, scratch_off, out_off;
};
struct GifEncAlbumDesc { int first, count; };
struct GifEncItem { int frame, k; };                      // workgroup b of a launch works on part k of frame `frame`
struct GifEncDev {
    uint8_t* mem;
    const GifEncFrameDesc* frames;
    const GifEncAlbumDesc* albums;
    const GifEncItem *px_items, *seg_items, *pack_items;
    GifColourSet* sets;
    uint32_t* tabs;                                        // 256 keys per frame
    GifEncRec* recs;
    uint32_t* segbits;                                     // a segment's bit length
};

// ---------------------------------------------------------------- limits, bounds, the container (host)
constexpr int GIF_ENC_MAX_SIDE = 4096, GIF_ENC_MAX_FRAMES = 4096;
// the LZW bytes of a page of `pixels` at the most, whatever the segment: a code per pixel, a clear per 256 pixels (the
// smallest segment) and per 2048 (table-full clears), 12 bits each
inline size_t gif_enc_stream_bound(size_t pixels) { return (12 * (pixels + pixels / 256 + pixels / 2048 + 8) + 7) / 8; }
inline size_t gif_enc_frame_bound(size_t pixels) { return 8 + 10 + 768 + 1 + gif_enc_framed_size((uint32_t)gif_enc_stream_bound(pixels)); }
inline size_t gif_enc_file_bound(int w, int h, int frames) {
    if (w <= 0 || h <= 0 || frames <= 0 || w > GIF_ENC_MAX_SIDE || h > GIF_ENC_MAX_SIDE || frames > GIF_ENC_MAX_FRAMES) return 0;
    return 13 + 768 + 19 + (size_t)frames * gif_enc_frame_bound((size_t)w * h) + 1;
}
// the argument rules shared by every entry point (before a device is looked for)
inline int gif_enc_check_args(int frames, const int* dispose, int loop_count, int segment) {
    if (segment != 0 && (segment < 256 || segment > (1 << 24))) return IMP_ERROR_INVALID_ARGS;
    if (loop_count > 65535) return IMP_ERROR_INVALID_ARGS;
    if (dispose)
        for (int i = 0; i < frames; i++)
            if (dispose[i] < 0 || dispose[i] > 3) return IMP_ERROR_INVALID_ARGS;
    return IMP_OK;
}
inline int gif_enc_check_geometry(int w, int h, int c, int frames) {
    if (w <= 0 || h <= 0 || frames <= 0) return IMP_ERROR_INVALID_ARGS;
    if ((c != 3 && c != 4) || w > GIF_ENC_MAX_SIDE || h > GIF_ENC_MAX_SIDE || frames > GIF_ENC_MAX_FRAMES) return IMP_ERROR_UNSUPPORTED;
    return IMP_OK;
}

// A frame as the container writer takes it: its record, its table's keys, and its framed stream (length bytes and
// terminator in place: gif_enc_framed_size(rec.stream_bytes) bytes).
struct GifEncPage { const GifEncRec* rec; const uint32_t* table; const uint8_t* framed; };
inline size_t gif_enc_table_bytes(uint32_t nkeys) { return 3 * (size_t)gif_table_size(nkeys); }
inline size_t gif_enc_file_size(const GifEncPage* pages, int count, int loop_count) {
    size_t n = 13 + (loop_count >= 0 ? 19 : 0) + 1;
    if (pages[0].rec->mode == GIF_ENC_GLOBAL) n += gif_enc_table_bytes(pages[0].rec->nkeys);
    for (int i = 0; i < count; i++) {
        n += 8 + 10 + 1 + gif_enc_framed_size(pages[i].rec->stream_bytes);
        if (pages[i].rec->mode == GIF_ENC_LOCAL) n += gif_enc_table_bytes(pages[i].rec->nkeys);
    }
    return n;
}
inline uint8_t* gif_enc_put_table(uint8_t* p, const uint32_t* keys, uint32_t nkeys) {
    const uint32_t size = gif_table_size(nkeys);
    for (uint32_t k = 0; k < size; k++, p += 3) {
        const uint32_t key = k < nkeys && !(keys[k] & GIF_KEY_TRANSPARENT) ? keys[k] : 0u;      // transparent and padding: 0,0,0
        p[0] = (uint8_t)(key >> 16); p[1] = (uint8_t)(key >> 8); p[2] = (uint8_t)key;
    }
    return p;
}
inline uint8_t* gif_enc_put16(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); return p + 2; }
// the file of gif_enc_file_size bytes: GIF89a, the screen, NETSCAPE2.0, then per frame a graphic control extension, the
// image descriptor (and local table), min_code_size and the framed stream; the trailer
inline void gif_enc_write_file(uint8_t* p, const GifEncPage* pages, int count, int w, int h, const int* time_ms, const int* dispose,
                               int loop_count) {
    const bool global = pages[0].rec->mode == GIF_ENC_GLOBAL;
    memcpy(p, "GIF89a", 6); p += 6;
    p = gif_enc_put16(p, (uint32_t)w); p = gif_enc_put16(p, (uint32_t)h);
    auto size_bits = [](uint32_t nkeys) { uint32_t b = 0; while ((2u << b) < gif_table_size(nkeys)) b++; return b; };
    *p++ = (uint8_t)(global ? 0xF0u | size_bits(pages[0].rec->nkeys) : 0x70u);
    *p++ = 0; *p++ = 0;
    if (global) p = gif_enc_put_table(p, pages[0].table, pages[0].rec->nkeys);
    if (loop_count >= 0) {
        memcpy(p, "\x21\xff\x0bNETSCAPE2.0\x03\x01", 16); p += 16;
        p = gif_enc_put16(p, (uint32_t)loop_count);
        *p++ = 0;
    }
    for (int i = 0; i < count; i++) {
        const GifEncRec& r = *pages[i].rec;
        const long long t = time_ms ? (long long)time_ms[i] / 10 : 0;
        *p++ = 0x21; *p++ = 0xF9; *p++ = 4;
        *p++ = (uint8_t)(((dispose ? dispose[i] : 0) << 2) | (r.has_trans ? 1 : 0));
        p = gif_enc_put16(p, (uint32_t)(t < 0 ? 0 : t > 65535 ? 65535 : t));
        *p++ = (uint8_t)(r.has_trans ? r.trans_index : 0u);
        *p++ = 0;
        *p++ = 0x2C;
        p = gif_enc_put16(p, 0); p = gif_enc_put16(p, 0); p = gif_enc_put16(p, (uint32_t)w); p = gif_enc_put16(p, (uint32_t)h);
        *p++ = (uint8_t)(global ? 0u : 0x80u | size_bits(r.nkeys));
        if (!global) p = gif_enc_put_table(p, pages[i].table, r.nkeys);
        *p++ = (uint8_t)r.mcs;
        const size_t fs = gif_enc_framed_size(r.stream_bytes);
        memcpy(p, pages[i].framed, fs); p += fs;
    }
    *p = 0x3B;
}

// ---------------------------------------------------------------- the host encoder: the launches, one lane after the other
// SETS + TABLES for one album; false: refused
inline bool host_tables(const unsigned char* const* frames, int count, int w, int h, int c, int step, std::vector<GifEncRec>* recs,
                 std::vector<uint32_t>* tabs) {
    const uint32_t total = (uint32_t)w * (uint32_t)h;
    std::vector<GifColourSet> sets((size_t)count);
    std::vector<uint32_t> lset(GIF_SET_SLOTS);
    for (int f = 0; f < count; f++) {
        memset(&sets[(size_t)f], 0, sizeof(GifColourSet));
        const GifEncFrame fr{frames[f], w, h, c, step, (c == 4 && (((uintptr_t)frames[f] | (uintptr_t)step) & 3) == 0) ? 1 : 0};
        for (uint32_t b0 = 0; b0 < total; b0 += GIF_ENC_PX_BLOCK) {                  // a workgroup of k_gif_enc_sets
            if (sets[(size_t)f].overflow) break;
            std::fill(lset.begin(), lset.end(), 0u);
            bool full = false;
            for (uint32_t tid = 0; tid < 256u; tid++) {
                uint32_t last = 0;
                for (uint32_t j = 0; j < 16u; j++) {
                    const uint32_t pos = b0 + tid * 16u + j;
                    if (pos >= total) break;
                    const uint32_t key = gif_enc_key_at(fr, pos);
                    if (key == last) continue;
                    last = key;
                    if (gif_set_insert(lset.data(), key) < 0) full = true;
                }
            }
            if (full) { sets[(size_t)f].overflow = 1u; break; }
            for (int i = 0; i < GIF_SET_SLOTS; i++)
                if (lset[(size_t)i]) gif_frame_set_add(&sets[(size_t)f], lset[(size_t)i]);
        }
        if (sets[(size_t)f].overflow) return false;
    }
    recs->assign((size_t)count, GifEncRec{});
    tabs->assign((size_t)count * 256, 0u);
    std::vector<uint32_t> list, uset(GIF_SET_SLOTS, 0u);
    uint32_t ucount = 0;
    auto sort_out = [&](uint32_t* tab) {
        for (uint32_t i = 0; i < (uint32_t)list.size(); i++) tab[gif_rank(list.data(), (uint32_t)list.size(), i)] = list[i];
    };
    for (int f = 0; f < count; f++) {                                                // k_gif_enc_tables
        list.clear();
        for (int i = 0; i < GIF_SET_SLOTS; i++)
            if (sets[(size_t)f].slot[i]) list.push_back(sets[(size_t)f].slot[i]);
        sort_out(tabs->data() + (size_t)f * 256);
        const bool ufull = ucount > GIF_SET_MAX;
        for (uint32_t k : list) {
            if (k == GIF_KEY_TRANSPARENT) (*recs)[(size_t)f].has_trans = 1u;
            if (ufull) continue;
            const int r = gif_set_insert(uset.data(), k);
            if (r) ucount += r > 0 ? 1u : (uint32_t)GIF_SET_SLOTS;
        }
        (*recs)[(size_t)f].nkeys = (uint32_t)list.size();
    }
    if (ucount <= GIF_SET_MAX) {
        list.clear();
        bool gtrans = false;
        for (uint32_t k : uset)
            if (k) { list.push_back(k); gtrans = gtrans || k == GIF_KEY_TRANSPARENT; }
        sort_out(tabs->data());
        for (int f = 0; f < count; f++) gif_rec_fill(&(*recs)[(size_t)f], GIF_ENC_GLOBAL, 0u, (uint32_t)list.size(), gtrans);
    } else {
        for (int f = 0; f < count; f++) {
            GifEncRec* r = &(*recs)[(size_t)f];
            gif_rec_fill(r, GIF_ENC_LOCAL, (uint32_t)f, r->nkeys, r->has_trans != 0);
        }
    }
    return true;
}

inline void host_flush(GifEncMem* m, GifEncState* e, int mcs, uint32_t* words, uint32_t cap) {     // gif_enc_flush_wave
    for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_pack_lane(m, *e, lane);
    for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_drain_lane(m, *e, words, cap, lane);
    const uint32_t carry = gif_enc_carry(m, *e);
    for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_rewind_lane(m, carry, lane);
    if (e->tail == 1)
        for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_clear_lane(m, lane);
    gif_enc_batch_end(e, mcs);
}

// INDEX + LZW + PACK for one frame: its framed stream; rec->stream_bytes
inline void host_frame(const unsigned char* frame, int w, int h, int c, int step, uint32_t segment, GifEncRec* rec, const uint32_t* table,
                GifEncMem* m, std::vector<uint8_t>* framed) {
    const uint32_t total = (uint32_t)w * (uint32_t)h;
    const GifEncFrame fr{frame, w, h, c, step, (c == 4 && (((uintptr_t)frame | (uintptr_t)step) & 3) == 0) ? 1 : 0};
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256u; i++) tab[i] = i < rec->nkeys ? table[i] : 0xFFFFFFFFu;
    std::vector<uint8_t> plane(total);
    for (uint32_t pos = 0; pos < total; pos++) plane[pos] = (uint8_t)gif_table_find(tab, gif_enc_key_at(fr, pos));
    const int mcs = (int)rec->mcs;
    const uint32_t nseg = gif_enc_segments(total, segment), cap = gif_enc_slot_words(segment < total ? segment : total);
    std::vector<uint32_t> scratch((size_t)nseg * cap, 0u), segbits(nseg);
    for (uint32_t k = 0; k < nseg; k++) {                                            // k_gif_enc_lzw
        uint32_t* words = scratch.data() + (size_t)k * cap;
        const uint32_t begin = k * segment, end = total - begin < segment ? total : begin + segment;
        GifEncState e;
        gif_enc_start(&e, mcs);
        for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_rewind_lane(m, 0u, lane);
        if (k == 0) {
            gif_enc_push_tail(m, &e, mcs, 1);
            host_flush(m, &e, mcs, words, cap);
        } else {
            for (int lane = 0; lane < GIF_LANES; lane++) gif_enc_clear_lane(m, lane);
        }
        for (uint32_t i = begin; i < end; i++)
            if (gif_enc_step(m, &e, mcs, plane[i])) host_flush(m, &e, mcs, words, cap);
        gif_enc_finish(m, &e, mcs, k + 1u == nseg);
        host_flush(m, &e, mcs, words, cap);
        gif_enc_last_word(m, e, words, cap);
        segbits[k] = e.s.bitpos;
    }
    uint64_t bits = 0;                                                               // k_gif_enc_pack
    for (uint32_t k = 0; k < nseg; k++) bits += segbits[k];
    const uint32_t nbytes = (uint32_t)((bits + 7u) >> 3);
    rec->stream_bytes = nbytes;
    framed->assign(gif_enc_framed_size(nbytes), 0);
    GifPackCursor cur{0, 0};
    for (uint32_t k = 0; k < nbytes; k++) {
        const uint32_t v = gif_enc_stream_byte(segbits.data(), nseg, (const uint8_t*)scratch.data(), (size_t)cap * 4u, &cur, k * 8u);
        gif_enc_put_byte(framed->data(), framed->size(), k, nbytes, v);
    }
}

// impgpu_gif_encode_host
inline int gif_encode_host(const unsigned char* const* frames, int count, int width, int height, int channels, int step, const int* time_ms,
                           const int* dispose, int loop_count, int segment, unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (!frames || !length || count <= 0) return IMP_ERROR_INVALID_ARGS;
    if (int rc = gif_enc_check_args(count <= GIF_ENC_MAX_FRAMES ? count : 0, dispose, loop_count, segment)) return rc;
    if (int rc = gif_enc_check_geometry(width, height, channels, count)) return rc;
    if ((long long)step < (long long)width * channels) return IMP_ERROR_INVALID_ARGS;
    for (int f = 0; f < count; f++)
        if (!frames[f]) return IMP_ERROR_INVALID_ARGS;
    const uint32_t seg = segment ? (uint32_t)segment : (uint32_t)IMPGPU_GIF_ENC_SEGMENT;
    std::vector<GifEncRec> recs;
    std::vector<uint32_t> tabs;
    if (!host_tables(frames, count, width, height, channels, step, &recs, &tabs)) return IMP_ERROR_UNSUPPORTED;
    std::vector<std::vector<uint8_t>> framed((size_t)count);
    std::vector<GifEncMem> mem(1);
    for (int f = 0; f < count; f++)
        host_frame(frames[f], width, height, channels, step, seg, &recs[(size_t)f], tabs.data() + (size_t)recs[(size_t)f].table_frame * 256,
                   mem.data(), &framed[(size_t)f]);
    std::vector<GifEncPage> pages;
    for (int f = 0; f < count; f++)
        pages.push_back(GifEncPage{&recs[(size_t)f], tabs.data() + (size_t)recs[(size_t)f].table_frame * 256, framed[(size_t)f].data()});
    const size_t need = gif_enc_file_size(pages.data(), count, loop_count);
    *length = need;
    if (!out || capacity < need) return IMP_ERROR_MALLOC_FAILED;
    gif_enc_write_file(out, pages.data(), count, width, height, time_ms, dispose, loop_count);
    return IMP_OK;
}

}  // namespace imp
