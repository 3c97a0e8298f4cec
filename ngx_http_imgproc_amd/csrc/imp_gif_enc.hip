// imp_gif_enc.hip -- the launches that turn the albums of a call into GIF streams (impgpu_batch_encode_gif):
// k_gif_enc_sets, _tables, _index, _lzw and _pack.  The lanes' logic is imp_gif_enc.h's, which the host encoder
// (impgpu_gif_encode_host) runs too.  Each launch reads what the one before wrote across the kernel boundary of one
// stream; no wavefront waits for another workgroup.  Workgroup b of a launch finds its work in an item table
// (GifEncItem: a frame of the call and the part of it), so the launches do not depend on how many albums there are.
// Under IMPGPU_GIF_ENC_QUANTIZE three launches more run between the sets and the tables -- k_gif_enc_claim, _hist and _cut:
// the frames past 256 colours get a median-cut table -- and k_gif_enc_index reads such a frame's cell -> index table.
// Under IMPGPU_GIF_ENC_DELTA one launch more runs ahead of the sets -- k_gif_enc_delta: the held planes and the bounds of what
// changed -- and the later launches are their DELTA instantiations; without the bit they are the ones they were.
#include "imp_internal.h"
#include "imp_gif_enc.h"

namespace imp {

__device__ __forceinline__ GifEncFrame gif_enc_frame_of(const GifEncFrameDesc& f) { return GifEncFrame{f.src, f.w, f.h, f.c, f.step, f.wide}; }

// DELTA (under IMPGPU_GIF_ENC_DELTA, ahead of SETS, on its items): a candidate frame against the frame before it.  A lane
// leaves the held bits of its 16 pixels as one word of the frame's held plane; the bounds of the pixels that are not held
// are folded across the wave with six exchanges, across the workgroup's four waves in LDS, and lane 0 publishes them.
__global__ __launch_bounds__(256) void k_gif_enc_delta(GifEncDev D) {
    __shared__ uint32_t wb[4][4];
    const GifEncItem it = D.px_items[blockIdx.x];
    const GifDeltaDesc dd = D.ddesc[it.frame];
    if (dd.prev < 0) return;
    const GifEncFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    const GifEncFrame fr = gif_enc_frame_of(f), pv = gif_enc_frame_of(D.frames[dd.prev]);
    const uint32_t p0 = (uint32_t)it.k * GIF_ENC_PX_BLOCK + (uint32_t)tid * 16u;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    const uint32_t mask = gif_delta_lane(fr, pv, p0, f.total, b);
    if (p0 < f.total) D.held[(size_t)dd.held_off + (p0 >> 4)] = (uint16_t)mask;
    for (int i = 0; i < 4; i++) {
        uint32_t x = b[i];
        for (int d = 32; d; d >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)x, d); x = o > x ? o : x; }
        if ((tid & 63) == 0) wb[tid >> 6][i] = x;
    }
    __syncthreads();
    if (tid == 0) {
        for (int i = 0; i < 4; i++) {
            uint32_t x = wb[0][i];
            for (int w = 1; w < 4; w++) x = wb[w][i] > x ? wb[w][i] : x;
            b[i] = x;
        }
        gif_delta_publish(&D.wins[it.frame], b);
    }
}

// what TABLES, CLAIM and HIST ask of a frame under IMPGPU_GIF_ENC_DELTA: a candidate?  did its written keys (set A), did
// its own keys (set B) outgrow a table?
struct GifDeltaState { bool cand, a_over, b_over; };
__device__ __forceinline__ GifDeltaState gif_delta_state(const GifEncDev& D, int f) {
    const bool cand = D.ddesc[f].prev >= 0;
    return GifDeltaState{cand, cand && D.sets_a[f].overflow != 0u, D.sets[f].overflow != 0u};
}
template <bool DELTA>
__device__ __forceinline__ bool gif_enc_needs_quant(const GifEncDev& D, int f) {
    if (!DELTA) return D.sets[f].overflow != 0u;
    const GifDeltaState st = gif_delta_state(D, f);
    return gif_delta_needs_quant(st.cand, st.a_over, st.b_over);
}

// SETS: 4096 pixels a workgroup, 16 consecutive ones a lane (a lane skips a key equal to its last one).  The LDS set
// holds 1024 keys: a workgroup that fills it has seen four times what any table takes, and says so in the frame's flag.
// WRITTEN: a candidate's written keys (through the held plane and the window) into its set A, not its own into set B.
template <bool WRITTEN>
__device__ __forceinline__ void gif_enc_sets_pass(const GifEncDev& D, const GifEncItem it, uint32_t* lset, uint32_t* flag) {
    const GifEncFrameDesc& f = D.frames[it.frame];
    GifColourSet* fs = WRITTEN ? &D.sets_a[it.frame] : &D.sets[it.frame];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < GIF_SET_SLOTS; i += 256) lset[i] = 0;
    if (tid == 0) { flag[0] = *(volatile uint32_t*)&fs->overflow; flag[1] = 0; flag[2] = 0; }
    __syncthreads();
    if (flag[0]) return;                                               // the frame is lost already
    const GifEncFrame fr = gif_enc_frame_of(f);
    const GifWindow W = WRITTEN ? gif_delta_window(D.wins[it.frame].raw, (uint32_t)f.w, (uint32_t)f.h) : GifWindow{};
    const uint16_t* held = WRITTEN ? D.held + D.ddesc[it.frame].held_off : nullptr;
    const uint32_t p0 = (uint32_t)it.k * GIF_ENC_PX_BLOCK + (uint32_t)tid * 16u;
    uint32_t last = 0;
    for (uint32_t j = 0; j < 16u; j++) {
        if (p0 + j >= f.total || *(volatile uint32_t*)&flag[1]) break;
        const uint32_t key = WRITTEN ? gif_delta_set_key(fr, W, held, p0 + j) : gif_enc_key_at(fr, p0 + j);
        if (key == last || (WRITTEN && key == 0u)) continue;
        last = key;
        if (gif_set_count(lset, &flag[2], key)) flag[1] = 1;           // (a photo stops here, long before its keys crowd the set)
    }
    __syncthreads();
    if (flag[1]) {
        if (tid == 0) *(volatile uint32_t*)&fs->overflow = 1u;
        return;
    }
    for (int i = tid; i < GIF_SET_SLOTS; i += 256)
        if (lset[i]) gif_frame_set_add(fs, lset[i]);
}
// DELTA: the launch under IMPGPU_GIF_ENC_DELTA, in which a candidate's workgroup goes on to the frame's written keys
template <bool DELTA>
__global__ __launch_bounds__(256) void k_gif_enc_sets(GifEncDev D) {
    __shared__ uint32_t lset[GIF_SET_SLOTS];
    __shared__ uint32_t flag[3];
    const GifEncItem it = D.px_items[blockIdx.x];
    gif_enc_sets_pass<false>(D, it, lset, flag);
    if (DELTA && D.ddesc[it.frame].prev >= 0) {
        __syncthreads();
        gif_enc_sets_pass<true>(D, it, lset, flag);
    }
}

// `n` keys (<= 256) of `list` into tabs[0 .. n), ascending: every lane ranks its own
__device__ __forceinline__ void gif_enc_sort_out(const uint32_t* list, uint32_t n, uint32_t* tab, int tid) {
    if ((uint32_t)tid < n) tab[gif_rank(list, n, (uint32_t)tid)] = list[tid];
}

// TABLES: a workgroup per album walks its frames: the frame's keys out of its set, sorted into the frame's table slot,
// and into the album's union (an LDS set; past 256 keys it is of no more use and takes no more).  Then the verdict.
// DELTA: the launch under IMPGPU_GIF_ENC_DELTA: the choice per candidate, its window, and set A where it is a delta frame.
template <bool DELTA>
__global__ __launch_bounds__(256) void k_gif_enc_tables(GifEncDev D) {
    __shared__ uint32_t list[GIF_SET_MAX];
    __shared__ uint32_t uset[GIF_SET_SLOTS];
    __shared__ uint32_t n, ucount, gtrans;
    const GifEncAlbumDesc a = D.albums[blockIdx.x];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < GIF_SET_SLOTS; i += 256) uset[i] = 0;
    if (tid == 0) { n = 0; ucount = 0; gtrans = 0; }
    __syncthreads();
    bool quant = false;
    for (int q = 0; q < a.count; q++) {                                // (the sets are final: every lane reads the same)
        if (!gif_enc_needs_quant<DELTA>(D, a.first + q)) continue;
        if (!D.slot_of || D.slot_of[a.first + q] < 0) return;          // a frame fits no table, or got no slot: every record stays REFUSED
        quant = true;                                                  // k_gif_enc_cut has made its table: local tables
    }
    for (int q = 0; q < a.count; q++) {
        const int f = a.first + q;
        bool isd = false;
        if (DELTA) {
            const GifDeltaState st = gif_delta_state(D, f);
            isd = gif_delta_is_delta(st.cand, st.a_over, st.b_over);
            if (tid == 0) gif_delta_rec_fill(&D.wins[f], isd, (uint32_t)D.frames[f].w, (uint32_t)D.frames[f].h);
        }
        if (gif_enc_needs_quant<DELTA>(D, f)) continue;
        const GifColourSet* fs = DELTA && isd ? &D.sets_a[f] : &D.sets[f];
        const bool ufull = ucount > GIF_SET_MAX;
        for (int i = tid; i < GIF_SET_SLOTS; i += 256) {
            const uint32_t k = fs->slot[i];
            if (!k) continue;
            const uint32_t at = atomicAdd(&n, 1u);
            if (at < GIF_SET_MAX) list[at] = k;
        }
        __syncthreads();
        const uint32_t cnt = n < GIF_SET_MAX ? n : GIF_SET_MAX;
        gif_enc_sort_out(list, cnt, D.tabs + (size_t)f * 256, tid);
        if ((uint32_t)tid < cnt) {
            if (list[tid] == GIF_KEY_TRANSPARENT) D.recs[f].has_trans = 1u;
            if (!ufull) {
                const int r = gif_set_insert(uset, list[tid]);
                if (r) atomicAdd(&ucount, r > 0 ? 1u : (uint32_t)GIF_SET_SLOTS);
            }
        }
        if (tid == 0) D.recs[f].nkeys = cnt;
        __syncthreads();
        if (tid == 0) n = 0;
        __syncthreads();
    }
    if (!quant && ucount <= GIF_SET_MAX) {                             // one global table: the union, sorted, in the first frame's slot
        for (int i = tid; i < GIF_SET_SLOTS; i += 256) {
            const uint32_t k = uset[i];
            if (!k) continue;
            const uint32_t at = atomicAdd(&n, 1u);
            if (at < GIF_SET_MAX) list[at] = k;
            if (k == GIF_KEY_TRANSPARENT) gtrans = 1u;
        }
        __syncthreads();
        const uint32_t cnt = n < GIF_SET_MAX ? n : GIF_SET_MAX;
        gif_enc_sort_out(list, cnt, D.tabs + (size_t)a.first * 256, tid);
        for (int q = tid; q < a.count; q += 256) gif_rec_fill(&D.recs[a.first + q], GIF_ENC_GLOBAL, (uint32_t)a.first, cnt, gtrans != 0);
    } else {
        for (int q = tid; q < a.count; q += 256) {
            GifEncRec* r = &D.recs[a.first + q];
            gif_rec_fill(r, GIF_ENC_LOCAL, (uint32_t)(a.first + q), r->nkeys, r->has_trans != 0);
        }
    }
}

// CLAIM (under IMPGPU_GIF_ENC_QUANTIZE): one workgroup walks the albums in their order and hands the pool's slots to the
// frames that overflowed -- to all of an album's or to none, so an album is either finished by this group or deferred
// whole (album_need says how many slots it wants).  Every frame's slot_of is written.
template <bool DELTA>
__global__ __launch_bounds__(256) void k_gif_enc_claim(GifEncDev D, int nalbums) {
    __shared__ uint32_t need, taken;
    const int tid = (int)threadIdx.x;
    if (tid == 0) taken = 0;
    uint32_t next = 0;                                                 // (= taken at every album's start; the same in all lanes)
    for (int ai = 0; ai < nalbums; ai++) {
        const GifEncAlbumDesc a = D.albums[ai];
        if (tid == 0) need = 0;
        __syncthreads();
        for (int q = tid; q < a.count; q += 256)
            if (gif_enc_needs_quant<DELTA>(D, a.first + q)) atomicAdd(&need, 1u);
        __syncthreads();
        const uint32_t nd = need;
        const bool fits = nd <= (uint32_t)D.nslots - next;
        if (tid == 0) D.album_need[ai] = fits ? 0u : nd;
        for (int q = tid; q < a.count; q += 256) {
            const int f = a.first + q;
            int slot = -1;
            if (fits && gif_enc_needs_quant<DELTA>(D, f)) {
                const uint32_t s = atomicAdd(&taken, 1u);
                if (s < (uint32_t)D.nslots) { slot = (int)s; D.slot_frame[s] = (uint32_t)f + 1u; }
            }
            D.slot_of[f] = slot;
        }
        if (fits) next += nd;
        __syncthreads();
    }
}

// HIST: SETS' items again, for the frames that hold a slot.  A lane sums a run of pixels of one cell in registers, the
// workgroup combines equal cells in its LDS table, and a cell's four sums leave for device memory once a workgroup (a
// cell that finds its place in the table taken goes there at once: that is the frame of many colours, whose adds spread).
// DELTA: a delta frame's pixels that are neither held nor transparent
template <bool DELTA>
__global__ __launch_bounds__(256) void k_gif_enc_hist(GifEncDev D) {
    __shared__ GifQuantWg wg;
    const GifEncItem it = D.px_items[blockIdx.x];
    const int slot = D.slot_of[it.frame];
    if (slot < 0) return;
    const GifEncFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    uint32_t* hist = D.hist + (size_t)slot * GIF_Q_HIST_WORDS;
    gif_q_wg_clear_lane(&wg, tid);
    __syncthreads();
    const GifEncFrame fr = gif_enc_frame_of(f);
    const uint32_t p0 = (uint32_t)it.k * GIF_ENC_PX_BLOCK + (uint32_t)tid * 16u;
    bool trans;
    if (DELTA && D.ddesc[it.frame].prev >= 0)                          // (a candidate that is quantised is a delta frame)
        trans = gif_q_lane_pixels_delta(fr, gif_delta_window(D.wins[it.frame].raw, (uint32_t)f.w, (uint32_t)f.h), D.held + D.ddesc[it.frame].held_off, p0,
                                        f.total, &wg, hist);
    else
        trans = gif_q_lane_pixels(fr, p0, f.total, &wg, hist);
    if (trans) *(volatile uint32_t*)&D.slot_trans[slot] = 1u;
    __syncthreads();
    for (int i = tid; i < GIF_Q_WG_SLOTS; i += 256) gif_q_wg_flush_slot(&wg, hist, i);
}

// CUT: a workgroup per slot.  The counts go into LDS and become the summed-volume table; up to 255 cuts of five steps
// each; then the table, the record and the cell -> index table.  The box numbers of the cells overlay the summed-volume
// table once the cuts are done.
__global__ __launch_bounds__(256) void k_gif_enc_cut(GifEncDev D) {
    __shared__ alignas(16) uint32_t S[GIF_Q_CELLS];                                // 128 KB of the CU's 160
    __shared__ GifQuantCut Q;
    const int slot = (int)blockIdx.x;
    if (D.slot_frame[slot] == 0u) return;
    const int frame = (int)(D.slot_frame[slot] - 1u);
    const int tid = (int)threadIdx.x;
    const uint32_t* hist = D.hist + (size_t)slot * GIF_Q_HIST_WORDS;
    const uint32_t T = D.slot_trans[slot] ? 1u : 0u;
    for (int i = tid * 4; i < GIF_Q_CELLS; i += 1024) *(uint4*)&S[i] = *(const uint4*)&hist[i];
    __syncthreads();
    for (int axis = 2; axis >= 0; axis--) {
        for (int line = tid; line < 1024; line += 256) gif_q_svt_line(S, axis, line);
        __syncthreads();
    }
    if (tid == 0) gif_q_start(&Q, S, GIF_SET_MAX - T);
    __syncthreads();
    gif_q_shrink_lane(&Q, S, tid);
    __syncthreads();
    if (tid == 0) gif_q_commit_first(&Q);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < 255; k++) {
        if (Q.nb == 0u || Q.nb >= Q.K) break;                          // (LDS words behind a barrier: the same in every lane)
        gif_q_score_lane(&Q, tid);
        __syncthreads();
        gif_q_pick_lane(&Q, tid);
        __syncthreads();
        if (Q.best == 0u) break;
        gif_q_marginal_lane(&Q, S, tid);
        __syncthreads();
        gif_q_shrink_lane(&Q, S, tid);
        __syncthreads();
        if (tid == 0) gif_q_commit(&Q);
        __syncthreads();
    }
    uint8_t* map = (uint8_t*)S;
    gif_q_map_lane(&Q, map, tid);
    __syncthreads();
    gif_q_sums_lane(&Q, map, hist, tid);
    __syncthreads();
    gif_q_colour_lane(&Q, tid);
    __syncthreads();
    gif_q_rank_lane(&Q, D.tabs + (size_t)frame * 256, T, tid);
    __syncthreads();
    gif_q_cellmap_lane(&Q, map, D.cmaps + (size_t)slot * GIF_Q_CELLS, tid);
    if (tid == 0) gif_q_rec(&Q, T, &D.recs[frame]);
}

// INDEX: the frame's table in LDS, four pixels a lane at a time, a dword of indices out.  QUANT: the launch under
// IMPGPU_GIF_ENC_QUANTIZE, in which a quantised frame's workgroup stages the frame's cell -> index table instead.
// DELTA: the launch under IMPGPU_GIF_ENC_DELTA: the items count WINDOW positions, the plane is the window's, and a held
// pixel gets the transparent index.
template <bool QUANT, bool DELTA>
__global__ __launch_bounds__(256) void k_gif_enc_index(GifEncDev D) {
    __shared__ uint32_t tab[256];
    __shared__ alignas(16) uint32_t cmap[QUANT ? GIF_Q_CELLS / 4 : 4];
    const GifEncItem it = D.px_items[blockIdx.x];
    const GifEncFrameDesc& f = D.frames[it.frame];
    const GifEncRec& rec = D.recs[it.frame];
    if (rec.mode == GIF_ENC_REFUSED) return;
    const int tid = (int)threadIdx.x;
    const bool quant = QUANT && rec.quant != 0u;
    if (QUANT && quant) {
        const uint32_t* src = (const uint32_t*)(D.cmaps + (size_t)D.slot_of[it.frame] * GIF_Q_CELLS);
        for (int i = tid * 4; i < GIF_Q_CELLS / 4; i += 1024) *(uint4*)&cmap[i] = *(const uint4*)&src[i];
    } else {
        tab[tid] = (uint32_t)tid < rec.nkeys ? D.tabs[(size_t)rec.table_frame * 256 + tid] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const GifEncFrame fr = gif_enc_frame_of(f);
    uint8_t* plane = D.mem + f.plane_off;
    const GifWindow W = DELTA ? gif_delta_rec_window(D.wins[it.frame]) : GifWindow{};
    const uint16_t* held = DELTA && D.wins[it.frame].delta ? D.held + D.ddesc[it.frame].held_off : nullptr;
    const uint32_t total = DELTA ? W.ww * W.wh : f.total;
#pragma unroll 1
    for (int j = 0; j < GIF_ENC_PX_BLOCK / 1024; j++) {
        const uint32_t pos = (uint32_t)it.k * GIF_ENC_PX_BLOCK + 4u * (uint32_t)(tid + 256 * j);
        if (pos >= total) break;
        const uint32_t cnt = total - pos < 4u ? total - pos : 4u;
        uint32_t v = 0;
        for (uint32_t q = 0; q < cnt; q++) {
            const uint32_t key = DELTA ? gif_delta_key_at(fr, W, held, pos + q) : gif_enc_key_at(fr, pos + q);
            v |= (QUANT && quant ? gif_q_index((const uint8_t*)cmap, rec.nkeys, key) : gif_table_find(tab, key)) << (8u * q);
        }
        if (cnt == 4u) *(uint32_t*)(plane + pos) = v;
        else for (uint32_t q = 0; q < cnt; q++) plane[pos + q] = (uint8_t)(v >> (8u * q));
    }
}

// a due batch: packed by the lanes, its whole words out, the rest carried
__device__ __forceinline__ void gif_enc_flush_wave(GifEncMem& m, GifEncState& e, int mcs, uint32_t* words, uint32_t cap, int lane) {
    __syncthreads();
    gif_enc_pack_lane(&m, e, lane);
    __syncthreads();
    gif_enc_drain_lane(&m, e, words, cap, lane);
    const uint32_t carry = gif_enc_carry(&m, e);
    __syncthreads();
    gif_enc_rewind_lane(&m, carry, lane);
    if (e.tail == 1) gif_enc_clear_lane(&m, lane);
    gif_enc_batch_end(&e, mcs);
    __syncthreads();
}

// LZW: a workgroup IS one wavefront and owns one segment; its barriers are that wave's own.  DELTA: the launch under
// IMPGPU_GIF_ENC_DELTA: the stream is the window's; a segment planned behind its last pixel is empty.
template <bool DELTA>
__global__ __launch_bounds__(GIF_LANES) void k_gif_enc_lzw(GifEncDev D) {
    __shared__ GifEncMem m;
    const GifEncItem it = D.seg_items[blockIdx.x];
    const GifEncFrameDesc& f = D.frames[it.frame];
    const GifEncRec& rec = D.recs[it.frame];
    if (rec.mode == GIF_ENC_REFUSED) return;
    const int lane = (int)threadIdx.x;
    const int mcs = (int)rec.mcs;
    const uint32_t k = (uint32_t)it.k;
    if (k >= f.nseg) return;
    const uint32_t total = DELTA ? D.wins[it.frame].total : f.total;
    const uint32_t begin = k * f.segment;
    if (DELTA && (begin >= total || total > f.total)) {
        if (lane == 0) D.segbits[f.seg0 + k] = 0u;
        return;
    }
    const uint32_t end = total - begin < f.segment ? total : begin + f.segment;
    const uint8_t* px = D.mem + f.plane_off;
    const uint32_t cap = f.slot_words;
    uint32_t* words = (uint32_t*)(D.mem + f.scratch_off) + (size_t)k * cap;
    GifEncState e;
    gif_enc_start(&e, mcs);
    gif_enc_rewind_lane(&m, 0u, lane);
    if (k == 0) {
        gif_enc_push_tail(&m, &e, mcs, 1);                             // the stream's opening clear (the flush empties the table)
        gif_enc_flush_wave(m, e, mcs, words, cap, lane);
    } else {
        gif_enc_clear_lane(&m, lane);
        __syncthreads();
    }
    for (uint32_t c0 = begin; c0 < end; c0 += GIF_ENC_CHUNK) {
        const uint32_t cn = end - c0 < (uint32_t)GIF_ENC_CHUNK ? end - c0 : (uint32_t)GIF_ENC_CHUNK;
        const uint32_t o = (uint32_t)lane * 16u;
        if (o + 16u <= cn && ((c0 + o) & 15u) == 0u) *(uint4*)&m.px[o] = *(const uint4*)(px + c0 + o);
        else for (uint32_t b = o; b < o + 16u && b < cn; b++) m.px[b] = px[c0 + b];
        __syncthreads();
        for (uint32_t i = 0; i < cn; i += 4u) {                         // four indices per LDS read: the walk waits for one load less
            const uint32_t quad = GIF_ENC_UNI(*(const uint32_t*)&m.px[i]);
#pragma unroll 1
            for (uint32_t q = 0; q < 4u && i + q < cn; q++)
                if (gif_enc_step(&m, &e, mcs, (quad >> (8u * q)) & 255u)) gif_enc_flush_wave(m, e, mcs, words, cap, lane);
        }
        __syncthreads();
    }
    gif_enc_finish(&m, &e, mcs, DELTA ? end == total : k + 1u == f.nseg);
    gif_enc_flush_wave(m, e, mcs, words, cap, lane);
    if (lane == 0) {
        gif_enc_last_word(&m, e, words, cap);
        D.segbits[f.seg0 + k] = e.s.bitpos;
    }
}

// PACK: 4096 bytes of a frame's stream a workgroup, 16 a lane.  The segments' bit lengths are summed 256 at a time
// (every workgroup of a frame does that again: the lengths are a few words); a lane whose first bit falls into the chunk
// finds its segment there by bisection.
__global__ __launch_bounds__(256) void k_gif_enc_pack(GifEncDev D) {
    __shared__ uint32_t pre[256];
    const GifEncItem it = D.pack_items[blockIdx.x];
    const GifEncFrameDesc& f = D.frames[it.frame];
    GifEncRec* rec = &D.recs[it.frame];
    if (rec->mode == GIF_ENC_REFUSED) return;
    const int tid = (int)threadIdx.x;
    const uint32_t* segbits = D.segbits + f.seg0;
    const uint32_t k0 = (uint32_t)it.k * GIF_ENC_PACK_BLOCK + (uint32_t)tid * 16u;
    const uint64_t first_bit = (uint64_t)k0 * 8u;
    uint32_t run = 0;
    GifPackCursor c{f.nseg, 0};
    bool found = false;
    for (uint32_t c0 = 0; c0 < f.nseg; c0 += 256u) {
        pre[tid] = c0 + (uint32_t)tid < f.nseg ? segbits[c0 + tid] : 0u;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint32_t t = tid >= d ? pre[tid - d] : 0u;
            __syncthreads();
            pre[tid] += t;
            __syncthreads();
        }
        const uint32_t tot = pre[255];
        if (!found && first_bit < (uint64_t)run + tot) {
            const uint32_t rel = (uint32_t)first_bit - run;
            uint32_t lo = 0;
            for (uint32_t step = 128; step; step >>= 1)
                if (pre[lo + step - 1] <= rel) lo += step;
            c.seg = c0 + lo;
            c.start = run + (lo ? pre[lo - 1] : 0u);
            found = true;
        }
        run += tot;
        __syncthreads();
    }
    const uint32_t nbytes = (run + 7u) >> 3;
    if (it.k == 0 && tid == 0) rec->stream_bytes = nbytes;
    if (!found) return;
    uint8_t* out = D.mem + f.out_off;
    const uint8_t* scratch = D.mem + f.scratch_off;
    for (uint32_t j = 0; j < 16u && k0 + j < nbytes; j++) {
        const uint32_t v = gif_enc_stream_byte(segbits, f.nseg, scratch, (size_t)f.slot_words * 4u, &c, (k0 + j) * 8u);
        gif_enc_put_byte(out, f.out_cap, k0 + j, nbytes, v);
    }
}

int launch_gif_encode(const GifEncDev& D, long long npx, long long nseg, long long npack, int nalbums, hipStream_t s) {
    if (!D.mem || npx <= 0 || nseg <= 0 || npack <= 0 || nalbums <= 0 || npx > 0x7fffffffLL || nseg > 0x7fffffffLL || npack > 0x7fffffffLL)
        return IMP_ERROR_INVALID_ARGS;
    const bool quant = (D.flags & IMPGPU_GIF_ENC_QUANTIZE) != 0;
    if (quant && (D.nslots <= 0 || !D.slot_of || !D.slot_frame || !D.slot_trans || !D.hist || !D.cmaps || !D.album_need)) return IMP_ERROR_INVALID_ARGS;
    const bool delta = (D.flags & IMPGPU_GIF_ENC_DELTA) != 0;
    if (delta && (!D.ddesc || !D.wins || !D.held || !D.sets_a)) return IMP_ERROR_INVALID_ARGS;
    if (delta) {                                                       // one launch more: the held planes and the windows' bounds
        hipLaunchKernelGGL(k_gif_enc_delta, dim3((unsigned)npx), dim3(256), 0, s, D);
        IMP_HIP(hipGetLastError());
    }
    if (delta) hipLaunchKernelGGL(k_gif_enc_sets<true>, dim3((unsigned)npx), dim3(256), 0, s, D);
    else hipLaunchKernelGGL(k_gif_enc_sets<false>, dim3((unsigned)npx), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    if (quant) {                                                       // three launches more, whatever overflowed
        if (delta) hipLaunchKernelGGL(k_gif_enc_claim<true>, dim3(1), dim3(256), 0, s, D, nalbums);
        else hipLaunchKernelGGL(k_gif_enc_claim<false>, dim3(1), dim3(256), 0, s, D, nalbums);
        IMP_HIP(hipGetLastError());
        if (delta) hipLaunchKernelGGL(k_gif_enc_hist<true>, dim3((unsigned)npx), dim3(256), 0, s, D);
        else hipLaunchKernelGGL(k_gif_enc_hist<false>, dim3((unsigned)npx), dim3(256), 0, s, D);
        IMP_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_gif_enc_cut, dim3((unsigned)D.nslots), dim3(256), 0, s, D);
        IMP_HIP(hipGetLastError());
    }
    if (delta) hipLaunchKernelGGL(k_gif_enc_tables<true>, dim3((unsigned)nalbums), dim3(256), 0, s, D);
    else hipLaunchKernelGGL(k_gif_enc_tables<false>, dim3((unsigned)nalbums), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    if (delta && quant) hipLaunchKernelGGL((k_gif_enc_index<true, true>), dim3((unsigned)npx), dim3(256), 0, s, D);
    else if (delta) hipLaunchKernelGGL((k_gif_enc_index<false, true>), dim3((unsigned)npx), dim3(256), 0, s, D);
    else if (quant) hipLaunchKernelGGL((k_gif_enc_index<true, false>), dim3((unsigned)npx), dim3(256), 0, s, D);
    else hipLaunchKernelGGL((k_gif_enc_index<false, false>), dim3((unsigned)npx), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    if (delta) hipLaunchKernelGGL(k_gif_enc_lzw<true>, dim3((unsigned)nseg), dim3(GIF_LANES), 0, s, D);
    else hipLaunchKernelGGL(k_gif_enc_lzw<false>, dim3((unsigned)nseg), dim3(GIF_LANES), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gif_enc_pack, dim3((unsigned)npack), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
