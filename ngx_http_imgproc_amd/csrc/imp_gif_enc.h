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
// Under IMPGPU_GIF_ENC_DELTA a launch runs ahead of these -- DELTA: held bits and the bounds of what changed, per candidate
// frame (gif_delta_lane, gif_delta_publish) -- and the others read a frame through its window and its held plane; see
// "delta frames" below.
//
// Safe by construction: a probe loop ends after one trip round its table; a window read off the bounds lies inside its frame
// (gif_delta_window); gif_enc_drain_lane drops words at or past the
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
// *p = min / max of *p and the `v` of the lanes that `take`.  EVERY lane of a group of 32 consecutive lanes calls it with
// the same p: on the device the group folds its values with five exchanges and one lane goes to memory.
IMP_GIF_HD void gif_group_min(uint32_t* p, uint32_t v, bool take, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t x = take ? v : 0xFFFFFFFFu;
    for (int d = 16; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)x, d); x = o < x ? o : x; }
    if ((lane & 31) == 0 && x != 0xFFFFFFFFu) atomicMin(p, x);
#else
    (void)lane;
    if (take && v < *p) *p = v;
#endif
}
IMP_GIF_HD void gif_group_max(uint32_t* p, uint32_t v, bool take, int lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t x = take ? v + 1u : 0u;
    for (int d = 16; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)x, d); x = o > x ? o : x; }
    if ((lane & 31) == 0 && x != 0u) atomicMax(p, x - 1u);
#else
    (void)lane;
    if (take && v > *p) *p = v;
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
// a key into a workgroup's set, whose new keys `count` counts; true: the set is full, or holds more keys than a table --
// the workgroup's pixels alone are too many colours, and it need not look at the rest
IMP_GIF_HD bool gif_set_count(uint32_t* slot, uint32_t* count, uint32_t key) {
    const int r = gif_set_insert(slot, key);
    return r < 0 || (r > 0 && gif_add(count, 1u) + 1u > GIF_SET_MAX);
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
    uint32_t quant;          // 1: the table is the quantiser's (k_gif_enc_cut), the indices come through its cell -> index table
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

// ---------------------------------------------------------------- the quantiser (IMPGPU_GIF_ENC_QUANTIZE; include/impgpu.h has the definition)
// A frame whose keys outgrow a table is cut to K = 256 - T colours: a median cut over the 32 x 32 x 32 cells of its 5:5:5
// histogram, all in integers.
//   HIST    4096 pixels a workgroup, 16 a lane: a lane sums a run of pixels of one cell in registers, the workgroup
//           combines equal cells in a direct-mapped LDS table (gif_q_wg_add: a cell whose place another cell holds goes
//           to device memory at once), and what the table holds leaves as one add per sum (gif_q_wg_flush_slot).
//   CUT     one workgroup a frame.  The counts become a summed-volume table (gif_q_svt_line along B, G, R), so the pixels
//           of any cell range are eight reads (gif_q_box_sum).  A cut is five steps with a barrier between them: every lane
//           scores its box (gif_q_score_lane), the best scorers name the lowest of them (gif_q_pick_lane), lanes 0 .. s sum
//           planes 0 .. lane across the longest axis and name the plane t (gif_q_marginal_lane), 192 lanes sum the planes
//           of both halves on every axis and shrink them to their non-empty ones (gif_q_shrink_lane), lane 0 files the two
//           boxes (gif_q_commit).  Then the boxes' cells are named (gif_q_map_lane), their sums added up
//           (gif_q_sums_lane), the colours made and ranked (gif_q_colour_lane, gif_q_rank_lane) and every cell's index
//           written (gif_q_cellmap_lane).
// Every loop's bound is a constant: 255 cuts, 32 planes, 256 boxes, 32768 cells.
constexpr int GIF_Q_CELLS = 32768;
constexpr int GIF_Q_WG_SLOTS = 2048;
constexpr uint32_t GIF_Q_NONE = 0xFFFFFFFFu;
constexpr int GIF_Q_HIST_WORDS = 4 * GIF_Q_CELLS;          // planes n, sum R, sum G, sum B: 512 KB
struct GifQuantWg { uint32_t cell[GIF_Q_WG_SLOTS]; uint32_t sum[4][GIF_Q_WG_SLOTS]; };     // 40 KB
// A box's corners are packed r | g << 8 | b << 16 (axis 0, 1, 2).
struct GifQuantCut {
    uint32_t lo[256], hi[256], n[256];                     // the boxes
    uint32_t key[256], rank[256];
    uint32_t acc[3][256];                                  // a box's sums of R, G, B
    uint32_t m[32];                                        // the picked box's pixels per plane of its longest axis
    uint32_t nb, K, total, best, pick, tcut;               // boxes, their limit, the opaque pixels; a cut's best score, box and plane
    uint32_t tlo[2][3], thi[2][3];                         // the tight bounds of the cut's two halves
};

IMP_GIF_HD uint32_t gif_q_cell(uint32_t key) { return ((key >> 19) & 31u) << 10 | ((key >> 11) & 31u) << 5 | ((key >> 3) & 31u); }
IMP_GIF_HD uint32_t gif_q_get(uint32_t corner, int axis) { return (corner >> (8 * axis)) & 255u; }
IMP_GIF_HD uint32_t gif_q_set(uint32_t corner, int axis, uint32_t v) { return (corner & ~(255u << (8 * axis))) | v << (8 * axis); }
IMP_GIF_HD uint32_t gif_q_cell_of(uint32_t corner) { return gif_q_get(corner, 0) << 10 | gif_q_get(corner, 1) << 5 | gif_q_get(corner, 2); }

IMP_GIF_HD void gif_q_hist_add(uint32_t* hist, uint32_t cell, uint32_t n, uint32_t r, uint32_t g, uint32_t b) {
    gif_add(hist + cell, n);
    gif_add(hist + GIF_Q_CELLS + cell, r);
    gif_add(hist + 2 * GIF_Q_CELLS + cell, g);
    gif_add(hist + 3 * GIF_Q_CELLS + cell, b);
}
IMP_GIF_HD void gif_q_wg_clear_lane(GifQuantWg* t, int lane) {
    for (int i = lane; i < GIF_Q_WG_SLOTS; i += 256) { t->cell[i] = GIF_Q_NONE; t->sum[0][i] = 0; t->sum[1][i] = 0; t->sum[2][i] = 0; t->sum[3][i] = 0; }
}
// `n` pixels of one cell: into the workgroup's table where the cell's place is free or its own, else straight to `hist`
IMP_GIF_HD void gif_q_wg_add(GifQuantWg* t, uint32_t* hist, uint32_t cell, uint32_t n, uint32_t r, uint32_t g, uint32_t b) {
    const uint32_t h = (cell * 2654435761u) >> 21;
    uint32_t old = *(volatile uint32_t*)&t->cell[h];
    if (old == GIF_Q_NONE) old = gif_cas(&t->cell[h], GIF_Q_NONE, cell);
    if (old == GIF_Q_NONE || old == cell) {
        gif_add(&t->sum[0][h], n); gif_add(&t->sum[1][h], r); gif_add(&t->sum[2][h], g); gif_add(&t->sum[3][h], b);
    } else {
        gif_q_hist_add(hist, cell, n, r, g, b);
    }
}
IMP_GIF_HD void gif_q_wg_flush_slot(const GifQuantWg* t, uint32_t* hist, int i) {
    if (t->cell[i] != GIF_Q_NONE) gif_q_hist_add(hist, t->cell[i], t->sum[0][i], t->sum[1][i], t->sum[2][i], t->sum[3][i]);
}
// a lane's 16 pixels from stream position p0; true: one of them is transparent
IMP_GIF_HD bool gif_q_lane_pixels(const GifEncFrame& fr, uint32_t p0, uint32_t total, GifQuantWg* t, uint32_t* hist) {
    uint32_t cur = GIF_Q_NONE, n = 0, r = 0, g = 0, b = 0;
    bool trans = false;
    for (uint32_t j = 0; j < 16u; j++) {
        if (p0 + j >= total) break;
        const uint32_t key = gif_enc_key_at(fr, p0 + j);
        if (key & GIF_KEY_TRANSPARENT) { trans = true; continue; }
        const uint32_t cell = gif_q_cell(key);
        if (cell != cur) {
            if (n) gif_q_wg_add(t, hist, cur, n, r, g, b);
            cur = cell; n = 0; r = 0; g = 0; b = 0;
        }
        n++; r += (key >> 16) & 255u; g += (key >> 8) & 255u; b += key & 255u;
    }
    if (n) gif_q_wg_add(t, hist, cur, n, r, g, b);
    return trans;
}

// the summed-volume table S: S[r][g][b] = the pixels of the cells (<= r, <= g, <= b).  One of 1024 lines along `axis`.
IMP_GIF_HD void gif_q_svt_line(uint32_t* S, int axis, int line) {
    const int base = axis == 2 ? line << 5 : axis == 1 ? (line >> 5) << 10 | (line & 31) : line;
    const int stride = axis == 2 ? 1 : axis == 1 ? 32 : 1024;
    uint32_t run = 0;
    for (int j = 0; j < 32; j++) { run += S[base + j * stride]; S[base + j * stride] = run; }
}
IMP_GIF_HD uint32_t gif_q_svt_at(const uint32_t* S, int r, int g, int b) { return (r | g | b) < 0 ? 0u : S[r << 10 | g << 5 | b]; }
// the pixels of the cells lo .. hi (corners, inclusive)
IMP_GIF_HD uint32_t gif_q_box_sum(const uint32_t* S, uint32_t lo, uint32_t hi) {
    const int r0 = (int)gif_q_get(lo, 0) - 1, g0 = (int)gif_q_get(lo, 1) - 1, b0 = (int)gif_q_get(lo, 2) - 1;
    const int r1 = (int)gif_q_get(hi, 0), g1 = (int)gif_q_get(hi, 1), b1 = (int)gif_q_get(hi, 2);
    return gif_q_svt_at(S, r1, g1, b1) - gif_q_svt_at(S, r0, g1, b1) - gif_q_svt_at(S, r1, g0, b1) - gif_q_svt_at(S, r1, g1, b0)
         + gif_q_svt_at(S, r0, g0, b1) + gif_q_svt_at(S, r0, g1, b0) + gif_q_svt_at(S, r1, g0, b0) - gif_q_svt_at(S, r0, g0, b0);
}
// the pixels of plane `p` (a coordinate) across `axis` of the box lo .. hi
IMP_GIF_HD uint32_t gif_q_plane_sum(const uint32_t* S, uint32_t lo, uint32_t hi, int axis, uint32_t p) {
    return gif_q_box_sum(S, gif_q_set(lo, axis, p), gif_q_set(hi, axis, p));
}
// a box's longest side and its axis (ties: R, then G, then B)
IMP_GIF_HD uint32_t gif_q_side(uint32_t lo, uint32_t hi, int* axis) {
    const uint32_t sr = gif_q_get(hi, 0) - gif_q_get(lo, 0), sg = gif_q_get(hi, 1) - gif_q_get(lo, 1), sb = gif_q_get(hi, 2) - gif_q_get(lo, 2);
    *axis = sr >= sg && sr >= sb ? 0 : sg >= sb ? 1 : 2;
    return *axis == 0 ? sr : *axis == 1 ? sg : sb;
}
IMP_GIF_HD uint32_t gif_q_score(const GifQuantCut* Q, uint32_t box) {      // n * s: below 2^24 * 32
    int axis;
    return Q->n[box] * gif_q_side(Q->lo[box], Q->hi[box], &axis);
}
// lane 0: the words a cut's steps meet in, as the next cut wants to find them
IMP_GIF_HD void gif_q_reset(GifQuantCut* Q) {
    Q->best = 0; Q->pick = GIF_Q_NONE; Q->tcut = GIF_Q_NONE;
    for (int c = 0; c < 2; c++)
        for (int a = 0; a < 3; a++) { Q->tlo[c][a] = 31u; Q->thi[c][a] = 0u; }
}
// lane 0: no box yet
IMP_GIF_HD void gif_q_start(GifQuantCut* Q, const uint32_t* S, uint32_t K) {
    Q->nb = 0; Q->K = K; Q->total = S[GIF_Q_CELLS - 1];
    gif_q_reset(Q);
}
IMP_GIF_HD void gif_q_score_lane(GifQuantCut* Q, int lane) {
    const bool take = (uint32_t)lane < Q->nb;
    gif_group_max(&Q->best, take ? gif_q_score(Q, (uint32_t)lane) : 0u, take, lane);
}
IMP_GIF_HD void gif_q_pick_lane(GifQuantCut* Q, int lane) {
    const bool take = (uint32_t)lane < Q->nb && Q->best != 0u && gif_q_score(Q, (uint32_t)lane) == Q->best;
    gif_group_min(&Q->pick, (uint32_t)lane, take, lane);
}
// lanes 0 .. s: the picked box's pixels in planes 0 .. lane of its longest axis (one box sum); the lanes at which that
// reaches ceil(n / 2) name the first of them
IMP_GIF_HD void gif_q_marginal_lane(GifQuantCut* Q, const uint32_t* S, int lane) {
    if (lane >= 32) return;
    int axis;
    const uint32_t box = Q->pick & 255u, lo = Q->lo[box], hi = Q->hi[box], n = Q->n[box], s = gif_q_side(lo, hi, &axis);
    const uint32_t run = (uint32_t)lane <= s ? gif_q_box_sum(S, lo, gif_q_set(hi, axis, gif_q_get(lo, axis) + (uint32_t)lane)) : 0u;
    Q->m[lane] = run;
    gif_group_min(&Q->tcut, (uint32_t)lane, (uint32_t)lane <= s && run >= (n + 1u) / 2u, lane);
}
// the halves [0] and [1] of the cut before the shrink: planes 0 .. t and t + 1 .. s of the picked box, t = the plane the
// marginal named, s - 1 at the most.  Before there is a box: the whole cube, and nothing (corners out of order: no plane
// lies in it).  Every lane works this out for itself from the same words.
struct GifQuantHalves { uint32_t lo[2], hi[2], n[2]; };
IMP_GIF_HD GifQuantHalves gif_q_halves(const GifQuantCut* Q) {
    GifQuantHalves H;
    if (Q->nb == 0u) {
        H.lo[0] = 0u; H.hi[0] = 31u | 31u << 8 | 31u << 16; H.n[0] = Q->total;
        H.lo[1] = 1u | 1u << 8 | 1u << 16; H.hi[1] = 0u; H.n[1] = 0u;
        return H;
    }
    int axis;
    const uint32_t box = Q->pick & 255u, lo = Q->lo[box], hi = Q->hi[box], s = gif_q_side(lo, hi, &axis);
    const uint32_t t = (Q->tcut < s ? Q->tcut : s - 1u) & 31u, a0 = gif_q_get(lo, axis);
    H.lo[0] = lo; H.hi[0] = gif_q_set(hi, axis, a0 + t); H.n[0] = Q->m[t];
    H.lo[1] = gif_q_set(lo, axis, a0 + t + 1u); H.hi[1] = hi; H.n[1] = Q->n[box] - Q->m[t];
    return H;
}
// lanes 0 .. 191: plane (lane & 31) across axis (lane / 32 % 3) of half (lane / 96), where it lies in that half
IMP_GIF_HD void gif_q_shrink_lane(GifQuantCut* Q, const uint32_t* S, int lane) {
    if (lane >= 192) return;
    const GifQuantHalves H = gif_q_halves(Q);
    const int c = lane / 96, axis = (lane % 96) / 32;
    const uint32_t p = (uint32_t)lane & 31u, lo = H.lo[c], hi = H.hi[c];
    bool hit = p >= gif_q_get(lo, axis) && p <= gif_q_get(hi, axis);
    for (int a = 0; a < 3; a++) hit = hit && gif_q_get(lo, a) <= gif_q_get(hi, a) && gif_q_get(hi, a) <= 31u;
    hit = hit && gif_q_plane_sum(S, lo, hi, axis, p) != 0u;
    gif_group_min(&Q->tlo[c][axis], p, hit, lane);
    gif_group_max(&Q->thi[c][axis], p, hit, lane);
}
IMP_GIF_HD void gif_q_file(GifQuantCut* Q, uint32_t box, int c, uint32_t n) {
    Q->lo[box] = Q->tlo[c][0] | Q->tlo[c][1] << 8 | Q->tlo[c][2] << 16;
    Q->hi[box] = Q->thi[c][0] | Q->thi[c][1] << 8 | Q->thi[c][2] << 16;
    Q->n[box] = n;
}
// lane 0, behind the first shrink: the first box (none when the frame has no opaque pixel)
IMP_GIF_HD void gif_q_commit_first(GifQuantCut* Q) {
    if (Q->total != 0u) {
        gif_q_file(Q, 0u, 0, Q->total);
        Q->nb = 1u;
    }
    gif_q_reset(Q);
}
// lane 0, behind a cut's shrink: planes 0 .. t keep the box's number, the rest is the next box
IMP_GIF_HD void gif_q_commit(GifQuantCut* Q) {
    const GifQuantHalves H = gif_q_halves(Q);
    gif_q_file(Q, Q->pick & 255u, 0, H.n[0]);
    gif_q_file(Q, Q->nb & 255u, 1, H.n[1]);
    Q->nb++;
    gif_q_reset(Q);
}
// every cell of every box gets the box's number (`map`: 32768 bytes)
IMP_GIF_HD void gif_q_map_lane(GifQuantCut* Q, uint8_t* map, int lane) {
    for (int a = 0; a < 3; a++) Q->acc[a][lane] = 0u;
    for (uint32_t box = 0; box < 256u && box < Q->nb; box++) {
        const uint32_t lo = Q->lo[box], hi = Q->hi[box];
        const uint32_t dg = gif_q_get(hi, 1) - gif_q_get(lo, 1) + 1u, db = gif_q_get(hi, 2) - gif_q_get(lo, 2) + 1u;
        const uint32_t vol = (gif_q_get(hi, 0) - gif_q_get(lo, 0) + 1u) * dg * db;
        for (uint32_t i = (uint32_t)lane; i < vol && i < (uint32_t)GIF_Q_CELLS; i += 256u) {
            const uint32_t r = i / (dg * db), g = i / db % dg, b = i % db;
            map[(gif_q_cell_of(lo) + (r << 10 | g << 5 | b)) & (uint32_t)(GIF_Q_CELLS - 1)] = (uint8_t)box;
        }
    }
}
IMP_GIF_HD void gif_q_sums_lane(GifQuantCut* Q, const uint8_t* map, const uint32_t* hist, int lane) {
    for (int cell = lane; cell < GIF_Q_CELLS; cell += 256) {
        if (hist[cell] == 0u) continue;
        const uint32_t box = map[cell];
        gif_add(&Q->acc[0][box], hist[GIF_Q_CELLS + cell]);
        gif_add(&Q->acc[1][box], hist[2 * GIF_Q_CELLS + cell]);
        gif_add(&Q->acc[2][box], hist[3 * GIF_Q_CELLS + cell]);
    }
}
// (2 * sum + n) / (2 * n) without the overflow: the quotient, and one more when twice the remainder reaches n
IMP_GIF_HD uint32_t gif_q_mean(uint32_t sum, uint32_t n) {
    if (n == 0u) return 0u;
    const uint32_t q = sum / n, rem = sum - q * n;
    return q + (rem >= n - rem ? 1u : 0u);
}
IMP_GIF_HD void gif_q_colour_lane(GifQuantCut* Q, int lane) {
    if ((uint32_t)lane >= Q->nb) return;
    const uint32_t n = Q->n[lane];
    Q->key[lane] = GIF_KEY_COLOUR | (gif_q_mean(Q->acc[0][lane], n) & 255u) << 16 | (gif_q_mean(Q->acc[1][lane], n) & 255u) << 8 | (gif_q_mean(Q->acc[2][lane], n) & 255u);
}
// the table: the boxes' colours ascending, then the transparent key when T
IMP_GIF_HD void gif_q_rank_lane(GifQuantCut* Q, uint32_t* tab, uint32_t T, int lane) {
    if ((uint32_t)lane < Q->nb) {
        const uint32_t rk = gif_rank(Q->key, Q->nb, (uint32_t)lane);
        Q->rank[lane] = rk;
        tab[rk] = Q->key[lane];
    }
    if (lane == 0 && T && Q->nb < GIF_SET_MAX) tab[Q->nb] = GIF_KEY_TRANSPARENT;
}
// the cell -> index table: 4 cells a lane at a time
IMP_GIF_HD void gif_q_cellmap_lane(const GifQuantCut* Q, const uint8_t* map, uint8_t* out, int lane) {
    for (int i = lane * 4; i < GIF_Q_CELLS; i += 1024) {
        uint32_t v = 0;
        for (int q = 0; q < 4; q++) {
            const uint32_t box = map[i + q];                           // (a cell outside every box holds no pixel: any index will do)
            v |= (box < Q->nb ? Q->rank[box] & 255u : 0u) << (8 * q);
        }
        *(uint32_t*)(out + i) = v;
    }
}
IMP_GIF_HD void gif_q_rec(const GifQuantCut* Q, uint32_t T, GifEncRec* rec) {
    rec->nkeys = Q->nb + T;
    rec->has_trans = T;
    rec->quant = 1u;
}
// a pixel's index in a quantised frame
IMP_GIF_HD uint32_t gif_q_index(const uint8_t* cmap, uint32_t nkeys, uint32_t key) {
    return (key & GIF_KEY_TRANSPARENT) ? nkeys - 1u : cmap[gif_q_cell(key)];
}

// ---------------------------------------------------------------- delta frames (IMPGPU_GIF_ENC_DELTA; include/impgpu.h has the definition)
// A CANDIDATE frame (its own disposal and its predecessor's are 0 or 1) is compared with the frame before it:
//   DELTA   SETS' items, ahead of them: a lane compares its 16 keys with the previous frame's (gif_delta_lane), leaves the
//           16 held bits as one word of the frame's held plane and grows the bounds of its pixels that are NOT held; a
//           workgroup folds the bounds and one lane publishes them with four atomicMax (gif_delta_publish).  The bounds are
//           kept as w - x, h - y, x + 1, y + 1, so that a zeroed record says "no such pixel" and every fold is a maximum.
// The later launches read the window off the bounds (gif_delta_window) and a pixel's WRITTEN key through the held plane
// (gif_delta_key_at): they never read the previous frame again.  SETS fills a second set per candidate, that of the written
// keys (set A); the frame's own keys (set B) stay where they were.  TABLES makes the choice (gif_delta_needs_quant,
// gif_delta_is_delta) and leaves the window every later launch and the container use (gif_delta_rec_fill).
struct GifWindow { uint32_t x0, y0, ww, wh; };
struct GifDeltaDesc { int prev; uint32_t held_off; };     // uploaded, per frame: the frame before it when it is a candidate, else -1; its held plane, in words
struct GifDeltaRec {
    uint32_t raw[4];                                       // DELTA: the maxima of w - x, h - y, x + 1, y + 1 over the pixels not held; 0: there is none
    uint32_t x0, y0, ww, wh;                               // TABLES: the window written (the whole frame unless `delta`)
    uint32_t delta;                                        // 1: a delta frame
    uint32_t total;                                        // ww * wh: the pixels of the frame's stream
    uint32_t pad[2];
};
IMP_GIF_HD void gif_max(uint32_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(p, v);
#else
    if (v > *p) *p = v;
#endif
}
// the smallest rectangle round the pixels not held; 1 x 1 at 0,0 when every pixel is held
IMP_GIF_HD GifWindow gif_delta_window(const uint32_t* raw, uint32_t w, uint32_t h) {
    GifWindow W{0u, 0u, 1u, 1u};
    if (raw[2] == 0u || raw[3] == 0u || raw[0] == 0u || raw[1] == 0u || raw[0] > w || raw[1] > h) return W;
    const uint32_t x0 = w - raw[0], y0 = h - raw[1];
    if (raw[2] <= x0 || raw[3] <= y0 || raw[2] > w || raw[3] > h) return W;
    W.x0 = x0; W.y0 = y0; W.ww = raw[2] - x0; W.wh = raw[3] - y0;
    return W;
}
IMP_GIF_HD bool gif_window_has(const GifWindow& W, uint32_t x, uint32_t y) { return x - W.x0 < W.ww && y - W.y0 < W.wh; }
IMP_GIF_HD uint32_t gif_held_at(const uint16_t* held, uint32_t pos) { return ((uint32_t)held[pos >> 4] >> (pos & 15u)) & 1u; }
// held: the key is a colour and the pixel under it in the previous frame has the same key
IMP_GIF_HD bool gif_delta_held(uint32_t key, uint32_t prev) { return key == prev && !(key & GIF_KEY_TRANSPARENT); }
// A lane's 16 pixels from frame position p0 (a multiple of 16) of `fr` over `pv`, a frame of the same geometry: the held
// bits, bit j for pixel p0 + j; b[0 .. 3] grow by the pixels that are not held.
IMP_GIF_HD uint32_t gif_delta_lane(const GifEncFrame& fr, const GifEncFrame& pv, uint32_t p0, uint32_t total, uint32_t* b) {
    uint32_t mask = 0;
    if (p0 >= total) return mask;
    uint32_t y = p0 / (uint32_t)fr.w, x = p0 - y * (uint32_t)fr.w;
    for (uint32_t j = 0; j < 16u && p0 + j < total; j++) {
        const size_t at = (size_t)y * (size_t)fr.step + (size_t)x * (size_t)fr.c, pat = (size_t)y * (size_t)pv.step + (size_t)x * (size_t)pv.c;
        if (gif_delta_held(gif_enc_key(fr.src + at, fr.c, fr.wide != 0), gif_enc_key(pv.src + pat, pv.c, pv.wide != 0))) {
            mask |= 1u << j;
        } else {
            const uint32_t nx = (uint32_t)fr.w - x, ny = (uint32_t)fr.h - y;
            b[0] = nx > b[0] ? nx : b[0]; b[1] = ny > b[1] ? ny : b[1];
            b[2] = x + 1u > b[2] ? x + 1u : b[2]; b[3] = y + 1u > b[3] ? y + 1u : b[3];
        }
        if (++x == (uint32_t)fr.w) { x = 0; y++; }
    }
    return mask;
}
IMP_GIF_HD void gif_delta_publish(GifDeltaRec* r, const uint32_t* b) {
    if (b[2] == 0u) return;
    for (int i = 0; i < 4; i++) gif_max(&r->raw[i], b[i]);
}
// the key frame position `pos` (= y * w + x) adds to the set of WRITTEN keys: its own when it is not held, "transparent"
// when it is held inside the window, nothing (0) outside it
IMP_GIF_HD uint32_t gif_delta_set_key(const GifEncFrame& fr, const GifWindow& W, const uint16_t* held, uint32_t pos) {
    const uint32_t y = pos / (uint32_t)fr.w, x = pos - y * (uint32_t)fr.w;
    if (!gif_held_at(held, pos)) return gif_enc_key(fr.src + (size_t)y * (size_t)fr.step + (size_t)x * (size_t)fr.c, fr.c, fr.wide != 0);
    return gif_window_has(W, x, y) ? GIF_KEY_TRANSPARENT : 0u;
}
// the written key of WINDOW position `wpos` (raster order inside W)
IMP_GIF_HD uint32_t gif_delta_key_at(const GifEncFrame& fr, const GifWindow& W, const uint16_t* held, uint32_t wpos) {
    const uint32_t wy = wpos / W.ww, y = W.y0 + wy, x = W.x0 + (wpos - wy * W.ww);
    if (held && gif_held_at(held, y * (uint32_t)fr.w + x)) return GIF_KEY_TRANSPARENT;
    return gif_enc_key(fr.src + (size_t)y * (size_t)fr.step + (size_t)x * (size_t)fr.c, fr.c, fr.wide != 0);
}
// the choice, from "the written keys outgrew a table" and "the frame's own keys did"
IMP_GIF_HD bool gif_delta_needs_quant(bool cand, bool a_over, bool b_over) { return cand ? a_over && b_over : b_over; }
IMP_GIF_HD bool gif_delta_is_delta(bool cand, bool a_over, bool b_over) { return cand && (!a_over || b_over); }
IMP_GIF_HD void gif_delta_rec_fill(GifDeltaRec* r, bool delta, uint32_t w, uint32_t h) {
    const GifWindow W = delta ? gif_delta_window(r->raw, w, h) : GifWindow{0u, 0u, w, h};
    r->x0 = W.x0; r->y0 = W.y0; r->ww = W.ww; r->wh = W.wh;
    r->delta = delta ? 1u : 0u;
    r->total = W.ww * W.wh;
}
IMP_GIF_HD GifWindow gif_delta_rec_window(const GifDeltaRec& r) { return GifWindow{r.x0, r.y0, r.ww, r.wh}; }
// gif_q_lane_pixels for a delta frame: the lane's 16 FRAME positions from p0; the pixels that are neither held nor
// transparent are summed; true: one of them is transparent, or held inside the window
IMP_GIF_HD bool gif_q_lane_pixels_delta(const GifEncFrame& fr, const GifWindow& W, const uint16_t* held, uint32_t p0, uint32_t total,
                                        GifQuantWg* t, uint32_t* hist) {
    uint32_t cur = GIF_Q_NONE, n = 0, r = 0, g = 0, b = 0;
    bool trans = false;
    for (uint32_t j = 0; j < 16u; j++) {
        if (p0 + j >= total) break;
        const uint32_t key = gif_delta_set_key(fr, W, held, p0 + j);
        if (key == 0u) continue;
        if (key & GIF_KEY_TRANSPARENT) { trans = true; continue; }
        const uint32_t cell = gif_q_cell(key);
        if (cell != cur) {
            if (n) gif_q_wg_add(t, hist, cur, n, r, g, b);
            cur = cell; n = 0; r = 0; g = 0; b = 0;
        }
        n++; r += (key >> 16) & 255u; g += (key >> 8) & 255u; b += key & 255u;
    }
    if (n) gif_q_wg_add(t, hist, cur, n, r, g, b);
    return trans;
}

// ---------------------------------------------------------------- a segment's LZW
constexpr int GIF_ENC_SLOTS = 8192;                      // at most 3838 entries between two clears: under half full
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
    // the quantiser (flags & IMPGPU_GIF_ENC_QUANTIZE; null and 0 otherwise): a pool of `nslots` slots -- a histogram
    // (GIF_Q_HIST_WORDS), a cell -> index table (GIF_Q_CELLS bytes) and the words "has a transparent pixel" and "frame + 1"
    // each -- which k_gif_enc_claim hands to the frames that overflowed, a whole album or none of it
    int flags, nslots;
    int* slot_of;                                          // per frame: its slot, or -1
    uint32_t* slot_frame;                                  // per slot: frame + 1, or 0
    uint32_t* slot_trans;
    uint32_t* hist;
    uint8_t* cmaps;
    uint32_t* album_need;                                  // per album: 0, or the slots it needed and did not get (it is deferred)
    // delta frames (flags & IMPGPU_GIF_ENC_DELTA; null otherwise): per frame its candidate word and held plane, its window
    // record (behind the records, zeroed with them) and the set of its written keys
    const GifDeltaDesc* ddesc;
    GifDeltaRec* wins;
    uint16_t* held;
    GifColourSet* sets_a;
};
constexpr size_t GIF_Q_SLOT_BYTES = (size_t)GIF_Q_HIST_WORDS * 4 + GIF_Q_CELLS + 8;

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
// (wins: the frames' windows under IMPGPU_GIF_ENC_DELTA; null: every frame is w x h at 0,0)
inline void gif_enc_write_file(uint8_t* p, const GifEncPage* pages, int count, int w, int h, const int* time_ms, const int* dispose,
                               int loop_count, const GifDeltaRec* wins = nullptr) {
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
        if (wins) { p = gif_enc_put16(p, wins[i].x0); p = gif_enc_put16(p, wins[i].y0); p = gif_enc_put16(p, wins[i].ww); p = gif_enc_put16(p, wins[i].wh); }
        else { p = gif_enc_put16(p, 0); p = gif_enc_put16(p, 0); p = gif_enc_put16(p, (uint32_t)w); p = gif_enc_put16(p, (uint32_t)h); }
        *p++ = (uint8_t)(global ? 0u : 0x80u | size_bits(r.nkeys));
        if (!global) p = gif_enc_put_table(p, pages[i].table, r.nkeys);
        *p++ = (uint8_t)r.mcs;
        const size_t fs = gif_enc_framed_size(r.stream_bytes);
        memcpy(p, pages[i].framed, fs); p += fs;
    }
    *p = 0x3B;
}

// ---------------------------------------------------------------- the host encoder: the launches, one lane after the other
// HIST + CUT for one frame: its table (256 words), the record's nkeys / has_trans / quant, its cell -> index table
// (held and W: a delta frame -- the pixels that are neither held nor transparent, T from the window)
inline void host_quantize(const GifEncFrame& fr, uint32_t total, GifEncRec* rec, uint32_t* tab, uint8_t* cmap, const uint16_t* held = nullptr,
                          const GifWindow* W = nullptr) {
    std::vector<uint32_t> hist((size_t)GIF_Q_HIST_WORDS, 0u), S((size_t)GIF_Q_CELLS);
    std::vector<GifQuantWg> wg(1);
    std::vector<GifQuantCut> cut(1);
    GifQuantCut* Q = cut.data();
    uint32_t T = 0;
    for (uint32_t b0 = 0; b0 < total; b0 += GIF_ENC_PX_BLOCK) {                      // a workgroup of k_gif_enc_hist
        for (int lane = 0; lane < 256; lane++) gif_q_wg_clear_lane(wg.data(), lane);
        for (uint32_t tid = 0; tid < 256u; tid++)
            if (held ? gif_q_lane_pixels_delta(fr, *W, held, b0 + tid * 16u, total, wg.data(), hist.data())
                     : gif_q_lane_pixels(fr, b0 + tid * 16u, total, wg.data(), hist.data())) T = 1u;
        for (int i = 0; i < GIF_Q_WG_SLOTS; i++) gif_q_wg_flush_slot(wg.data(), hist.data(), i);
    }
    std::copy(hist.begin(), hist.begin() + GIF_Q_CELLS, S.begin());                  // k_gif_enc_cut
    for (int axis = 2; axis >= 0; axis--)
        for (int line = 0; line < 1024; line++) gif_q_svt_line(S.data(), axis, line);
    gif_q_start(Q, S.data(), GIF_SET_MAX - T);
    for (int lane = 0; lane < 256; lane++) gif_q_shrink_lane(Q, S.data(), lane);
    gif_q_commit_first(Q);
    for (int k = 0; k < 255 && Q->nb != 0u && Q->nb < Q->K; k++) {
        for (int lane = 0; lane < 256; lane++) gif_q_score_lane(Q, lane);
        for (int lane = 0; lane < 256; lane++) gif_q_pick_lane(Q, lane);
        if (Q->best == 0u) break;
        for (int lane = 0; lane < 256; lane++) gif_q_marginal_lane(Q, S.data(), lane);
        for (int lane = 0; lane < 256; lane++) gif_q_shrink_lane(Q, S.data(), lane);
        gif_q_commit(Q);
    }
    uint8_t* map = (uint8_t*)S.data();                                               // (the table has done its work)
    for (int lane = 0; lane < 256; lane++) gif_q_map_lane(Q, map, lane);
    for (int lane = 0; lane < 256; lane++) gif_q_sums_lane(Q, map, hist.data(), lane);
    for (int lane = 0; lane < 256; lane++) gif_q_colour_lane(Q, lane);
    for (int lane = 0; lane < 256; lane++) gif_q_rank_lane(Q, tab, T, lane);
    for (int lane = 0; lane < 256; lane++) gif_q_cellmap_lane(Q, map, cmap, lane);
    gif_q_rec(Q, T, rec);
}

inline int gif_frame_wide(const unsigned char* frame, int c, int step) { return (c == 4 && (((uintptr_t)frame | (uintptr_t)step) & 3) == 0) ? 1 : 0; }

// a frame's walk through k_gif_enc_sets: its own keys into `fs`, or (held) its written keys
inline void host_set(const GifEncFrame& fr, uint32_t total, GifColourSet* fs, const uint16_t* held, const GifWindow* W) {
    std::vector<uint32_t> lset(GIF_SET_SLOTS);
    memset(fs, 0, sizeof(GifColourSet));
    for (uint32_t b0 = 0; b0 < total; b0 += GIF_ENC_PX_BLOCK) {                      // a workgroup of k_gif_enc_sets
        if (fs->overflow) break;
        std::fill(lset.begin(), lset.end(), 0u);
        bool full = false;
        uint32_t lcount = 0;
        for (uint32_t tid = 0; tid < 256u; tid++) {
            uint32_t last = 0;
            for (uint32_t j = 0; j < 16u; j++) {
                const uint32_t pos = b0 + tid * 16u + j;
                if (pos >= total || full) break;
                const uint32_t key = held ? gif_delta_set_key(fr, *W, held, pos) : gif_enc_key_at(fr, pos);
                if (key == last || key == 0u) continue;
                last = key;
                if (gif_set_count(lset.data(), &lcount, key)) full = true;
            }
        }
        if (full) { fs->overflow = 1u; break; }
        for (int i = 0; i < GIF_SET_SLOTS; i++)
            if (lset[(size_t)i]) gif_frame_set_add(fs, lset[(size_t)i]);
    }
}

// k_gif_enc_delta for one candidate frame: its held plane and the bounds in its record
inline void host_delta(const GifEncFrame& fr, const GifEncFrame& pv, uint32_t total, std::vector<uint16_t>* held, GifDeltaRec* rec) {
    held->assign(((size_t)total + 15) / 16, 0);
    for (uint32_t b0 = 0; b0 < total; b0 += GIF_ENC_PX_BLOCK) {
        uint32_t b[4] = {0u, 0u, 0u, 0u};
        for (uint32_t tid = 0; tid < 256u; tid++) {
            const uint32_t p0 = b0 + tid * 16u;
            if (p0 < total) (*held)[p0 >> 4] = (uint16_t)gif_delta_lane(fr, pv, p0, total, b);
        }
        gif_delta_publish(rec, b);
    }
}

// DELTA + SETS + TABLES (+ HIST + CUT under IMPGPU_GIF_ENC_QUANTIZE) for one album; false: refused.  cmaps: GIF_Q_CELLS bytes a
// frame.  Under IMPGPU_GIF_ENC_DELTA (`dispose` counts then, null = all 0): wins and held, per frame
inline bool host_tables(const unsigned char* const* frames, int count, int w, int h, int c, int step, int flags, const int* dispose,
                        std::vector<GifEncRec>* recs, std::vector<uint32_t>* tabs, std::vector<uint8_t>* cmaps, std::vector<GifDeltaRec>* wins,
                        std::vector<std::vector<uint16_t>>* held) {
    const uint32_t total = (uint32_t)w * (uint32_t)h;
    const bool delta = (flags & IMPGPU_GIF_ENC_DELTA) != 0;
    bool quant = false;
    std::vector<GifColourSet> sets((size_t)count), sets_a(delta ? (size_t)count : 0);
    std::vector<char> needs((size_t)count, 0), isd((size_t)count, 0);
    if (delta) { wins->assign((size_t)count, GifDeltaRec{}); held->assign((size_t)count, std::vector<uint16_t>()); }
    auto frame_of = [&](int f) { return GifEncFrame{frames[f], w, h, c, step, gif_frame_wide(frames[f], c, step)}; };
    auto keeps = [&](int f) { const int d = dispose ? dispose[f] : 0; return d == 0 || d == 1; };
    for (int f = 0; f < count; f++) {
        const GifEncFrame fr = frame_of(f);
        const bool cand = delta && f >= 1 && keeps(f - 1) && keeps(f);
        host_set(fr, total, &sets[(size_t)f], nullptr, nullptr);
        bool a_over = false;
        if (cand) {
            host_delta(fr, frame_of(f - 1), total, &(*held)[(size_t)f], &(*wins)[(size_t)f]);
            const GifWindow W = gif_delta_window((*wins)[(size_t)f].raw, (uint32_t)w, (uint32_t)h);
            host_set(fr, total, &sets_a[(size_t)f], (*held)[(size_t)f].data(), &W);
            a_over = sets_a[(size_t)f].overflow != 0u;
        }
        needs[(size_t)f] = gif_delta_needs_quant(cand, a_over, sets[(size_t)f].overflow != 0u) ? 1 : 0;
        isd[(size_t)f] = gif_delta_is_delta(cand, a_over, sets[(size_t)f].overflow != 0u) ? 1 : 0;
        if (needs[(size_t)f] && !(flags & IMPGPU_GIF_ENC_QUANTIZE)) return false;
        quant = quant || needs[(size_t)f];
    }
    recs->assign((size_t)count, GifEncRec{});
    tabs->assign((size_t)count * 256, 0u);
    if (quant) cmaps->assign((size_t)count * GIF_Q_CELLS, 0);
    std::vector<uint32_t> list, uset(GIF_SET_SLOTS, 0u);
    uint32_t ucount = 0;
    auto sort_out = [&](uint32_t* tab) {
        for (uint32_t i = 0; i < (uint32_t)list.size(); i++) tab[gif_rank(list.data(), (uint32_t)list.size(), i)] = list[i];
    };
    for (int f = 0; f < count; f++) {                                                // k_gif_enc_tables
        if (delta) gif_delta_rec_fill(&(*wins)[(size_t)f], isd[(size_t)f] != 0, (uint32_t)w, (uint32_t)h);
        if (needs[(size_t)f]) {
            const GifWindow W = delta ? gif_delta_rec_window((*wins)[(size_t)f]) : GifWindow{};
            host_quantize(frame_of(f), total, &(*recs)[(size_t)f], tabs->data() + (size_t)f * 256, cmaps->data() + (size_t)f * GIF_Q_CELLS,
                          isd[(size_t)f] ? (*held)[(size_t)f].data() : nullptr, &W);
            continue;
        }
        const GifColourSet& fs = isd[(size_t)f] ? sets_a[(size_t)f] : sets[(size_t)f];
        list.clear();
        for (int i = 0; i < GIF_SET_SLOTS; i++)
            if (fs.slot[i]) list.push_back(fs.slot[i]);
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
    if (!quant && ucount <= GIF_SET_MAX) {
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
// (win: the frame's window under IMPGPU_GIF_ENC_DELTA, held: a delta frame's held plane; the segments are planned for the whole
// frame, as the device's are, and those behind the window's last pixel stay empty)
inline void host_frame(const unsigned char* frame, int w, int h, int c, int step, uint32_t segment, GifEncRec* rec, const uint32_t* table,
                const uint8_t* cmap, GifEncMem* m, std::vector<uint8_t>* framed, const GifDeltaRec* win = nullptr, const uint16_t* held = nullptr) {
    const uint32_t whole = (uint32_t)w * (uint32_t)h, total = win ? win->total : whole;
    const GifWindow W = win ? gif_delta_rec_window(*win) : GifWindow{0u, 0u, (uint32_t)w, (uint32_t)h};
    const GifEncFrame fr{frame, w, h, c, step, (c == 4 && (((uintptr_t)frame | (uintptr_t)step) & 3) == 0) ? 1 : 0};
    uint32_t tab[256];
    for (uint32_t i = 0; i < 256u; i++) tab[i] = i < rec->nkeys ? table[i] : 0xFFFFFFFFu;
    std::vector<uint8_t> plane(total);
    for (uint32_t pos = 0; pos < total; pos++) {
        const uint32_t key = win ? gif_delta_key_at(fr, W, win->delta ? held : nullptr, pos) : gif_enc_key_at(fr, pos);
        plane[pos] = (uint8_t)(rec->quant ? gif_q_index(cmap, rec->nkeys, key) : gif_table_find(tab, key));
    }
    const int mcs = (int)rec->mcs;
    const uint32_t nseg = gif_enc_segments(whole, segment), cap = gif_enc_slot_words(segment < whole ? segment : whole);
    std::vector<uint32_t> scratch((size_t)nseg * cap, 0u), segbits(nseg);
    for (uint32_t k = 0; k < nseg; k++) {                                            // k_gif_enc_lzw
        uint32_t* words = scratch.data() + (size_t)k * cap;
        const uint32_t begin = k * segment;
        if (begin >= total) { segbits[k] = 0u; continue; }
        const uint32_t end = total - begin <= segment ? total : begin + segment;
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
        gif_enc_finish(m, &e, mcs, end == total);
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

// impgpu_gif_encode_host_ex2
inline int gif_encode_host_ex2(const unsigned char* const* frames, int count, int width, int height, int channels, int step, const int* time_ms,
                               const int* dispose, int loop_count, int segment, int flags, unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (flags & ~(IMPGPU_GIF_ENC_QUANTIZE | IMPGPU_GIF_ENC_DELTA)) return IMP_ERROR_INVALID_ARGS;
    if (!frames || !length || count <= 0) return IMP_ERROR_INVALID_ARGS;
    if (int rc = gif_enc_check_args(count <= GIF_ENC_MAX_FRAMES ? count : 0, dispose, loop_count, segment)) return rc;
    if (int rc = gif_enc_check_geometry(width, height, channels, count)) return rc;
    if ((long long)step < (long long)width * channels) return IMP_ERROR_INVALID_ARGS;
    for (int f = 0; f < count; f++)
        if (!frames[f]) return IMP_ERROR_INVALID_ARGS;
    const uint32_t seg = segment ? (uint32_t)segment : (uint32_t)IMPGPU_GIF_ENC_SEGMENT;
    std::vector<GifEncRec> recs;
    std::vector<uint32_t> tabs;
    std::vector<uint8_t> cmaps;
    const bool delta = (flags & IMPGPU_GIF_ENC_DELTA) != 0;
    std::vector<GifDeltaRec> wins;
    std::vector<std::vector<uint16_t>> held;
    if (!host_tables(frames, count, width, height, channels, step, flags, dispose, &recs, &tabs, &cmaps, &wins, &held)) return IMP_ERROR_UNSUPPORTED;
    std::vector<std::vector<uint8_t>> framed((size_t)count);
    std::vector<GifEncMem> mem(1);
    for (int f = 0; f < count; f++)
        host_frame(frames[f], width, height, channels, step, seg, &recs[(size_t)f], tabs.data() + (size_t)recs[(size_t)f].table_frame * 256,
                   recs[(size_t)f].quant ? cmaps.data() + (size_t)f * GIF_Q_CELLS : nullptr, mem.data(), &framed[(size_t)f],
                   delta ? &wins[(size_t)f] : nullptr, delta ? held[(size_t)f].data() : nullptr);
    std::vector<GifEncPage> pages;
    for (int f = 0; f < count; f++)
        pages.push_back(GifEncPage{&recs[(size_t)f], tabs.data() + (size_t)recs[(size_t)f].table_frame * 256, framed[(size_t)f].data()});
    const size_t need = gif_enc_file_size(pages.data(), count, loop_count);
    *length = need;
    if (!out || capacity < need) return IMP_ERROR_MALLOC_FAILED;
    gif_enc_write_file(out, pages.data(), count, width, height, time_ms, dispose, loop_count, delta ? wins.data() : nullptr);
    return IMP_OK;
}
// impgpu_gif_encode_host_ex: no bit but IMPGPU_GIF_ENC_QUANTIZE
inline int gif_encode_host_ex(const unsigned char* const* frames, int count, int width, int height, int channels, int step, const int* time_ms,
                              const int* dispose, int loop_count, int segment, int flags, unsigned char* out, size_t capacity, size_t* length) {
    if (length) *length = 0;
    if (flags & ~IMPGPU_GIF_ENC_QUANTIZE) return IMP_ERROR_INVALID_ARGS;
    return gif_encode_host_ex2(frames, count, width, height, channels, step, time_ms, dispose, loop_count, segment, flags, out, capacity, length);
}
// impgpu_gif_encode_host
inline int gif_encode_host(const unsigned char* const* frames, int count, int width, int height, int channels, int step, const int* time_ms,
                           const int* dispose, int loop_count, int segment, unsigned char* out, size_t capacity, size_t* length) {
    return gif_encode_host_ex(frames, count, width, height, channels, step, time_ms, dispose, loop_count, segment, 0, out, capacity, length);
}

// impgpu_gif_quantize_host: steps 1-5 on one frame, whatever its colour count
inline int gif_quantize_host(const unsigned char* frame, int width, int height, int channels, int step, unsigned char* table, int* entries,
                             int* transparent_index, unsigned char* indices) {
    if (!frame || !table || !entries || !transparent_index || !indices) return IMP_ERROR_INVALID_ARGS;
    if (int rc = gif_enc_check_geometry(width, height, channels, 1)) return rc;
    if ((long long)step < (long long)width * channels) return IMP_ERROR_INVALID_ARGS;
    const GifEncFrame fr{frame, width, height, channels, step, gif_frame_wide(frame, channels, step)};
    const uint32_t total = (uint32_t)width * (uint32_t)height;
    GifEncRec rec{};
    std::vector<uint32_t> tab(256, 0u);
    std::vector<uint8_t> cmap((size_t)GIF_Q_CELLS);
    host_quantize(fr, total, &rec, tab.data(), cmap.data());
    for (uint32_t k = 0; k < rec.nkeys; k++) {
        const uint32_t key = (tab[k] & GIF_KEY_TRANSPARENT) ? 0u : tab[k];
        table[3 * k] = (uint8_t)(key >> 16); table[3 * k + 1] = (uint8_t)(key >> 8); table[3 * k + 2] = (uint8_t)key;
    }
    *entries = (int)rec.nkeys;
    *transparent_index = rec.has_trans ? (int)rec.nkeys - 1 : -1;
    for (uint32_t pos = 0; pos < total; pos++) indices[pos] = (uint8_t)gif_q_index(cmap.data(), rec.nkeys, gif_enc_key_at(fr, pos));
    return IMP_OK;
}

}  // namespace imp
