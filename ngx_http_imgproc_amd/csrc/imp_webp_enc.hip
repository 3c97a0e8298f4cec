// imp_webp_enc.hip -- the six launches that turn the frames of a call into lossless WebP files (impgpu_batch_encode_webp):
// k_webp_modes, _resid, _codes, _measure, _scan and _emit; with IMPGPU_WEBP_ENC_BACKREFS (D.lz) a seventh, k_webp_parse,
// between _resid and _codes, and the others take their token form, chosen per launch by a uniform branch.  The lanes' logic is imp_webp_enc.h's, which the host encoder
// (impgpu_webp_encode_host) runs too.  Each launch reads what the one before wrote across the kernel boundary of one
// stream; no wavefront waits for another workgroup.  Workgroup b of a launch finds its work in an item table (a frame of
// the call and the part of it), so the launches do not depend on how many frames there are.  No kernel walks a frame's
// pixels one after the other: the only sequential work is k_webp_codes' five small trees per frame, a lane each.
#include "imp_internal.h"
#include "imp_webp_enc.h"

namespace imp {

__device__ __forceinline__ WebpFrame webp_frame_of(const WebpFrameDesc& f) { return WebpFrame{f.src, f.w, f.h, f.c, f.step}; }

// MODES: four tiles a workgroup, a wavefront each.  The 14 sums cross the wave by exchanges; lane 0 writes the mode and
// counts it in the mode image's histogram.
__global__ __launch_bounds__(256) void k_webp_modes(WebpDev D) {
    const WebpTileItem it = D.tile_items[blockIdx.x];
    const WebpFrameDesc& f = D.frames[it.frame];
    const int lane = (int)threadIdx.x & 63;
    const uint32_t tile = it.k * 4u + (threadIdx.x >> 6);
    if (tile >= f.ntiles) return;                                      // (wave-uniform)
    uint32_t cost[WEBP_MODES];
#pragma unroll
    for (int m = 0; m < WEBP_MODES; m++) cost[m] = 0;
    const bool alpha = webp_tile_costs_lane(webp_frame_of(f), D.tile_bits, (int)(tile % (uint32_t)f.tiles_x), (int)(tile / (uint32_t)f.tiles_x), lane, 64, cost);
#pragma unroll
    for (int m = 0; m < WEBP_MODES; m++)
        for (int d = 32; d; d >>= 1) cost[m] += __shfl_xor(cost[m], d, 64);
    const bool any_alpha = __ballot(alpha) != 0ull;
    if (lane != 0) return;
    WebpWork* W = &D.works[it.frame];
    const int mode = f.has_forced ? (int)(D.mem + f.forced_off)[tile] : webp_pick_mode(cost);
    (D.mem + f.modes_off)[tile] = (uint8_t)mode;
    atomicAdd(&W->hist[WEBP_CODE_MODES][mode], 1u);
    if (any_alpha) atomicOr(&W->alpha_seen, 1u);
}

// RESID: 1024 pixels a workgroup, four consecutive ones a lane.  The four histograms are kept in LDS and reach the frame's
// once a workgroup; the sums do not depend on the order, so every run counts the same.
__global__ __launch_bounds__(256) void k_webp_resid(WebpDev D) {
    __shared__ uint32_t lh[4 * 256];
    const WebpItem it = D.items[blockIdx.x];
    if (it.kind != WEBP_IT_PIXELS) return;
    const WebpFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    for (int i = tid; i < 1024; i += 256) lh[i] = 0;
    __syncthreads();
    const WebpFrame fr = webp_frame_of(f);
    const uint8_t* modes = D.mem + f.modes_off;
    uint32_t* resid = (uint32_t*)(D.mem + f.resid_off);
    const uint32_t p0 = it.k * WEBP_ITEM + (uint32_t)tid * 4u;
    if (D.lz) {                                                         // (uniform) the plane alone: k_webp_parse counts the tokens
        for (uint32_t j = 0; j < 4u && p0 + j < f.npix; j++) resid[p0 + j] = webp_residual_at(fr, modes, D.tile_bits, f.tiles_x, p0 + j);
        return;
    }
    for (uint32_t j = 0; j < 4u && p0 + j < f.npix; j++) {
        const uint32_t r = webp_residual_at(fr, modes, D.tile_bits, f.tiles_x, p0 + j);
        resid[p0 + j] = r;
        webp_count(lh, r);
    }
    __syncthreads();
    uint32_t* hist = &D.works[it.frame].hist[0][0];
    for (int i = tid; i < 1024; i += 256)
        if (lh[i]) atomicAdd(&hist[i], lh[i]);
}

// PARSE (IMPGPU_WEBP_ENC_BACKREFS): a workgroup per pixel item, lane t holding positions t, t + 256, t + 512 and t + 768 of
// it, so that a wave's ballot is 64 consecutive equality bits.  (1) per candidate the item's 1024 equality bits go to LDS as
// 32 words; a lane per candidate notes where the words with a zero bit are.  (2) a position's match under a candidate is the
// distance to the next zero bit; the longest of at least 3 makes its token and its jump (position + length, or + 1).
// (3) the token starts are the positions reached from position 0: ten jump tables by doubling, then marks from the highest
// power down -- after the table of 2^t every position a multiple of 2^t jumps from position 0 is marked.  (4) the marked
// positions' tokens go to the token plane (0 elsewhere) and into LDS histograms, which reach the frame's once a workgroup;
// the sums do not depend on the order.  Every read resid[p - d] has d <= p (webp_lz_equal); every LDS index is a position
// below 1024 or a jump checked against the item's length; nothing waits for another workgroup.
__global__ __launch_bounds__(256) void k_webp_parse(WebpDev D) {
    __shared__ uint32_t eq[WEBP_LZ_CANDS][32];
    __shared__ uint8_t skip[WEBP_LZ_CANDS][36];
    __shared__ uint32_t tokv[WEBP_ITEM];
    __shared__ uint16_t jump[10][WEBP_ITEM];
    __shared__ uint8_t mark[WEBP_ITEM];
    __shared__ uint32_t lh[WEBP_LZ_SYMS + 3 * 256 + 1];                 // WebpLz::hist, then red, blue, alpha, then the extra bits
    const WebpItem it = D.items[blockIdx.x];
    if (it.kind != WEBP_IT_PIXELS) return;
    const WebpFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    const uint32_t s = it.k * WEBP_ITEM, n = f.npix - s < WEBP_ITEM ? f.npix - s : WEBP_ITEM, e = s + n;
    const uint32_t* resid = (const uint32_t*)(D.mem + f.resid_off);
    for (int i = tid; i < WEBP_LZ_SYMS + 3 * 256 + 1; i += 256) lh[i] = 0;
    uint32_t mine[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t i = (uint32_t)(j * 256 + tid);
        mine[j] = i < n ? resid[s + i] : 0u;
    }
#pragma unroll 1
    for (int c = 0; c < WEBP_LZ_CANDS; c++) {                            // (1)
        const int d = webp_lz_distance(c + 1, f.w);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t p = s + (uint32_t)(j * 256 + tid);
            const bool same = p < e && d >= 1 && (uint32_t)d <= p && mine[j] == resid[p - (uint32_t)d];   // (webp_lz_equal)
            const unsigned long long b = __ballot(same);
            if ((tid & 63) == 0) {
                eq[c][j * 8 + (tid >> 6) * 2] = (uint32_t)b;
                eq[c][j * 8 + (tid >> 6) * 2 + 1] = (uint32_t)(b >> 32);
            }
        }
    }
    __syncthreads();
    if (tid < WEBP_LZ_CANDS) webp_lz_skips(eq[tid], skip[tid]);
    __syncthreads();
#pragma unroll 1
    for (int j = 0; j < 4; j++) {                                       // (2)
        const uint32_t i = (uint32_t)(j * 256 + tid);
        uint32_t t = 0u, to = WEBP_ITEM;
        if (i < n) {
            uint32_t best = 0, bk = 0;
#pragma unroll 1
            for (int c = 0; c < WEBP_LZ_CANDS; c++) {
                const uint32_t len = webp_lz_length(eq[c], skip[c], i);
                if (len > best) { best = len; bk = (uint32_t)c + 1u; }  // a tie stays with the lowest k
            }
            t = webp_lz_token(best, bk);
            to = i + webp_lz_step(t);
            if (to >= n) to = WEBP_ITEM;                                // the item's end
        }
        tokv[i] = t;
        jump[0][i] = (uint16_t)to;
        mark[i] = i == 0u;
    }
    __syncthreads();
#pragma unroll 1
    for (int t = 1; t < 10; t++) {                                      // (3) 2^t jumps are two times 2^(t-1)
        for (int i = tid; i < (int)WEBP_ITEM; i += 256) {
            const uint32_t a = jump[t - 1][i];
            jump[t][i] = a < WEBP_ITEM ? jump[t - 1][a] : (uint16_t)WEBP_ITEM;
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int t = 9; t >= 0; t--) {
        uint32_t to[4];
#pragma unroll
        for (int j = 0; j < 4; j++) to[j] = mark[j * 256 + tid] ? jump[t][j * 256 + tid] : WEBP_ITEM;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (to[j] < WEBP_ITEM) mark[to[j]] = 1;
        __syncthreads();
    }
    uint32_t* tok = (uint32_t*)(D.mem + f.tok_off);                     // (4)
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const uint32_t i = (uint32_t)(j * 256 + tid);
        if (i >= n) break;
        const uint32_t t = mark[i] ? tokv[i] : 0u;
        tok[s + i] = t;
        if (t) webp_lz_count(t, mine[j], lh, lh + WEBP_LZ_SYMS, lh + WEBP_LZ_SYMS + 3 * 256);
    }
    __syncthreads();
    WebpLz* L = &D.lz[it.frame];
    uint32_t* rba = &D.works[it.frame].hist[1][0];
    for (int i = tid; i < WEBP_LZ_SYMS; i += 256)
        if (lh[i]) atomicAdd(&L->hist[i], lh[i]);
    for (int i = tid; i < 3 * 256; i += 256)
        if (lh[WEBP_LZ_SYMS + i]) atomicAdd(&rba[i], lh[WEBP_LZ_SYMS + i]);
    if (tid == 0 && lh[WEBP_LZ_SYMS + 3 * 256]) atomicAdd(&L->extra_bits, (unsigned long long)lh[WEBP_LZ_SYMS + 3 * 256]);
}

// CODES: a workgroup (one wavefront) per frame; lanes 0..4 build a prefix code each, then lane 0 writes the header pieces,
// the record and the container's first 20 bytes.
__global__ __launch_bounds__(64) void k_webp_codes(WebpDev D) {
    const int frame = (int)blockIdx.x, lane = (int)threadIdx.x;
    const WebpFrameDesc& f = D.frames[frame];
    WebpWork* W = &D.works[frame];
    if (D.lz) {                                                         // (uniform) a sixth lane: the distance code
        WebpLz* L = &D.lz[frame];
        if (lane <= WEBP_CODES) webp_code_lane_lz(W, L, lane);
        __syncthreads();
        if (lane == 0) webp_headers(W, f.w, f.h, f.c, D.tile_bits, &D.recs[frame], (uint32_t*)(D.mem + f.out_off), L);
        return;
    }
    if (lane < WEBP_CODES) webp_code_lane(W, lane);
    __syncthreads();
    if (lane == 0) webp_headers(W, f.w, f.h, f.c, D.tile_bits, &D.recs[frame], (uint32_t*)(D.mem + f.out_off));
}

// symbol i of the item, in whichever form the call has (LZ: tab's last WEBP_LZ_SYMS entries are WebpLz::tab)
template <bool LZ>
__device__ __forceinline__ uint32_t webp_symbol_of(const WebpItem& it, const WebpFrameDesc& f, const WebpDev& D, const WebpWork* W, const uint32_t* tab, uint32_t i,
                                                   uint32_t* code, uint32_t* len) {
    if (LZ)
        return webp_symbol_lz(it.kind, it.k, i, W, tab, tab + WEBP_CODES * 256, D.mem + f.modes_off, (const uint32_t*)(D.mem + f.resid_off),
                              (const uint32_t*)(D.mem + f.tok_off), code, len);
    return webp_symbol(it.kind, it.k, i, W, tab, D.mem + f.modes_off, (const uint32_t*)(D.mem + f.resid_off), code, len);
}
// the bits of the item's symbols 4 tid .. 4 tid + 3
template <bool LZ>
__device__ __forceinline__ uint32_t webp_lane_bits(const WebpItem& it, const WebpFrameDesc& f, const WebpDev& D, const uint32_t* tab, int tid) {
    const WebpWork* W = &D.works[it.frame];
    const uint32_t ns = webp_item_symbols(it.kind, it.k, W, f.ntiles, f.npix);
    uint32_t total = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t i = (uint32_t)tid * 4u + j;
        if (i >= ns) break;
        uint32_t code[4], len[4];
        total += webp_symbol_of<LZ>(it, f, D, W, tab, i, code, len);
    }
    return total;
}
__device__ __forceinline__ void webp_stage_tab(const WebpDev& D, int frame, uint32_t* tab, int tid) {
    const uint32_t* src = &D.works[frame].tab[0][0];
    for (int i = tid; i < WEBP_CODES * 256; i += 256) tab[i] = src[i];
    if (D.lz)
        for (int i = tid; i < WEBP_LZ_SYMS; i += 256) tab[WEBP_CODES * 256 + i] = D.lz[frame].tab[i];
    __syncthreads();
}

// MEASURE: an item's bits
__global__ __launch_bounds__(256) void k_webp_measure(WebpDev D) {
    __shared__ uint32_t tab[WEBP_CODES * 256 + WEBP_LZ_SYMS];
    __shared__ uint32_t sum;
    const WebpItem it = D.items[blockIdx.x];
    const WebpFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    if (tid == 0) sum = 0;
    webp_stage_tab(D, it.frame, tab, tid);
    const uint32_t mine = D.lz ? webp_lane_bits<true>(it, f, D, tab, tid) : webp_lane_bits<false>(it, f, D, tab, tid);
    if (mine) atomicAdd(&sum, mine);
    __syncthreads();
    if (tid == 0) D.item_bits[blockIdx.x] = sum;
}

// SCAN: a workgroup per frame over its items' bits, 256 at a time: the items' bit offsets into the payload, in 64 bits
__global__ __launch_bounds__(256) void k_webp_scan(WebpDev D) {
    __shared__ uint64_t pre[256];
    const WebpFrameDesc& f = D.frames[blockIdx.x];
    const int tid = (int)threadIdx.x;
    uint64_t run = 0;
    for (uint32_t c0 = 0; c0 < f.nitems; c0 += 256u) {
        const uint32_t i = c0 + (uint32_t)tid;
        const uint64_t mine = i < f.nitems ? D.item_bits[f.item0 + i] : 0u;
        pre[tid] = mine;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const uint64_t t = tid >= d ? pre[tid - d] : 0u;
            __syncthreads();
            pre[tid] += t;
            __syncthreads();
        }
        if (i < f.nitems) D.item_off[f.item0 + i] = run + pre[tid] - mine;
        run += pre[255];
        __syncthreads();
    }
}

// EMIT: an item's symbols again; the lanes' bit positions are a scan of their totals, the bits are ORed together in LDS
// at the item's phase inside its first dword, and whole dwords leave: plain stores for the dwords the item owns, an OR
// into the zeroed file for its first and last, which a neighbour may share.
__global__ __launch_bounds__(256) void k_webp_emit(WebpDev D) {
    __shared__ uint32_t tab[WEBP_CODES * 256 + WEBP_LZ_SYMS];
    __shared__ uint32_t words[WEBP_EMIT_WORDS];
    __shared__ uint32_t pre[256];
    const WebpItem it = D.items[blockIdx.x];
    const WebpFrameDesc& f = D.frames[it.frame];
    const int tid = (int)threadIdx.x;
    const uint32_t bits = D.item_bits[blockIdx.x];
    if (bits == 0u || bits > WEBP_ITEM * (uint32_t)WEBP_SYMBOL_BITS) return;       // (uniform; the second never holds)
    const uint64_t off = D.item_off[blockIdx.x];
    for (int i = tid; i < WEBP_EMIT_WORDS; i += 256) words[i] = 0;
    webp_stage_tab(D, it.frame, tab, tid);
    const bool lz = D.lz != nullptr;                                    // (uniform)
    const uint32_t mine = lz ? webp_lane_bits<true>(it, f, D, tab, tid) : webp_lane_bits<false>(it, f, D, tab, tid);
    pre[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const uint32_t t = tid >= d ? pre[tid - d] : 0u;
        __syncthreads();
        pre[tid] += t;
        __syncthreads();
    }
    uint32_t pos = (uint32_t)(off & 31u) + pre[tid] - mine;
    const WebpWork* W = &D.works[it.frame];
    const uint32_t ns = webp_item_symbols(it.kind, it.k, W, f.ntiles, f.npix);
#pragma unroll 1
    for (uint32_t j = 0; j < 4u; j++) {                                 // the lane's symbols again, part by part into their places
        const uint32_t i = (uint32_t)tid * 4u + j;
        if (i >= ns) break;
        uint32_t code[4], len[4];
        if (lz) webp_symbol_of<true>(it, f, D, W, tab, i, code, len);
        else webp_symbol_of<false>(it, f, D, W, tab, i, code, len);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            if (pos + len[q] <= (uint32_t)WEBP_EMIT_WORDS * 32u) webp_emit_put(words, pos, code[q], len[q]);
            pos += len[q];
        }
    }
    __syncthreads();
    const uint32_t nw = webp_emit_words(off, bits);
    uint32_t* out32 = (uint32_t*)(D.mem + f.out_off);
    for (uint32_t j = (uint32_t)tid; j < nw && j < (uint32_t)WEBP_EMIT_WORDS; j += 256u) webp_emit_store(out32, f.out_words, off, j, nw, words[j]);
}

int launch_webp_encode(const WebpDev& D, long long ntile_items, long long nitems, int nframes, hipStream_t s) {
    if (!D.mem || ntile_items <= 0 || nitems <= 0 || nframes <= 0 || ntile_items > 0x7fffffffLL || nitems > 0x7fffffffLL) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_webp_modes, dim3((unsigned)ntile_items), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_resid, dim3((unsigned)nitems), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    if (D.lz) {
        hipLaunchKernelGGL(k_webp_parse, dim3((unsigned)nitems), dim3(256), 0, s, D);
        IMP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_webp_codes, dim3((unsigned)nframes), dim3(64), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_measure, dim3((unsigned)nitems), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_scan, dim3((unsigned)nframes), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_emit, dim3((unsigned)nitems), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
