// imp_gif.hip -- k_gif_lzw (and, for IMPGPU_GIF_SPLIT, k_gif_lzw_scan / _len / _emit below): the LZW pages of every GIF file of a call, decoded on the device straight into the index
// planes gif_walk (imp_geom.hip) reads.  One wavefront per page, dealt over the launch by the mix index like every
// descriptor launch; the lanes' logic is imp_gif.h's, which the host diagnostic (impgpu_gif_pages, how = 1) runs too.
//
// A workgroup IS one wavefront: the page's table and the round's words (GifLzwMem, 25 KB) are the workgroup's LDS, six
// of them fit a CU's 160 KB, and the barriers between a round's steps are barriers of that one wave -- the rounds of
// different pages never wait for each other.
#include "imp_internal.h"
#include "imp_gif.h"

namespace imp {

__global__ __launch_bounds__(GIF_LANES) void k_gif_lzw(uint8_t* blob, const GifLzwDesc* __restrict__ d, MixIndex ix,
                                                       uint32_t* __restrict__ status) {
    __shared__ GifLzwMem m;
    int blk;
    const int i = mix_pick(d, ix, &blk);
    if (i < 0) return;
    const int lane = (int)threadIdx.x;
    const int mcs = d[i].mcs;
    const uint8_t* data = blob + d[i].data_off;
    const uint32_t nbytes = d[i].data_bytes;
    GifPlane p;
    p.plane = blob + d[i].plane_off;
    p.w = d[i].w; p.h = d[i].h; p.pitch = d[i].pitch; p.interlaced = d[i].interlaced;
    p.total = (uint32_t)p.w * (uint32_t)p.h;
    GifLzwState s;
    gif_state_start(&s, mcs);
    gif_table_start(&m, lane);
    for (int row = lane; row < p.h; row += GIF_LANES) gif_pad_row(p, row);
    __syncthreads();
    while (!s.done) {
        // 1. every lane its code; the round ends at the first that is not a plain code
        const int mine = gif_extract(&m, s, mcs, data, nbytes, lane);
        const unsigned long long stop = __ballot(mine != GIF_K_CODE);
        const int ncodes = __builtin_amdgcn_readfirstlane(stop ? __ffsll((long long)stop) - 1 : GIF_LANES);
        const int kind = __builtin_amdgcn_readfirstlane(stop ? __shfl(mine, ncodes & (GIF_LANES - 1)) : (int)GIF_K_CODE);
        __syncthreads();
        // 2. the round's entries, linked across the lanes
        gif_link_start(&m, s, lane, ncodes);
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < 6; it++) {
            gif_link_read(&m, lane);
            __syncthreads();
            gif_link_write(&m, lane);
            __syncthreads();
        }
        gif_link_finish(&m, s, lane, ncodes);
        __syncthreads();
        // 3. a scan of the string lengths: where every lane's string goes
        const uint32_t len = gif_string_len(&m, lane, ncodes);
        uint32_t upto = len;
#pragma unroll
        for (int k = 1; k < GIF_LANES; k <<= 1) {
            const uint32_t t = __shfl_up(upto, k);
            if (lane >= k) upto += t;
        }
        const uint32_t produced = __builtin_amdgcn_readfirstlane(__shfl(upto, GIF_LANES - 1));
        // 4. every lane its string
        gif_emit(&m, p, lane, ncodes, s.outpos + upto - len);
        gif_round_end(&s, &m, mcs, ncodes, kind, produced, p.total);
        __syncthreads();
    }
    if (lane == 0) status[d[i].slot] = (uint32_t)s.status;
}

int launch_gif_lzw(uint8_t* blob, size_t table_off, const MixIndex& ix, int most, uint32_t* status, hipStream_t s) {
    if (most <= 0) return IMP_OK;
    if (!blob || !status || (table_off & 7)) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_gif_lzw, dim3((unsigned)most * 8), dim3(GIF_LANES), 0, s, blob, (const GifLzwDesc*)(blob + table_off), ix, status);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

// ---------------------------------------------------------------- IMPGPU_GIF_SPLIT: a page cut at its clear codes
// Three launches where k_gif_lzw is one (imp_gif.h says what the passes compute); each reads what the one before wrote
// across the kernel boundary, and no wavefront waits for another workgroup.  A page's segment block is GifSeg[cap + 1]
// behind the planes: entry 0 holds the count, the segments follow.

// the scan: one wavefront per page, dealt like k_gif_lzw's; no table, no LDS, every word of its state wave-uniform.  It is
// the one sequential walk of a cut page, and each of its rounds waits for memory once: hence rounds of 1024 codes.
__global__ __launch_bounds__(GIF_LANES) void k_gif_lzw_scan(uint8_t* blob, const GifLzwDesc* __restrict__ d,
                                                            const GifSplitPage* __restrict__ sp, MixIndex ix) {
    int blk;
    const int i = mix_pick(d, ix, &blk);
    if (i < 0) return;
    const int lane = (int)threadIdx.x;
    const int mcs = d[i].mcs;
    const uint8_t* data = blob + d[i].data_off;
    const uint32_t nbytes = d[i].data_bytes;
    GifSeg* segs = (GifSeg*)(blob + sp[i].seg_off);
    const uint32_t cap = sp[i].cap;
    if (nbytes == 0) {
        const uint32_t one = gif_scan_empty(segs + 1, lane == 0);
        if (lane == 0) segs[0].start = one;
        return;
    }
    GifScan sc;
    gif_scan_start(&sc, mcs);
    while (!sc.s.done) {
        // a round of 16 x 64 codes: all of a lane's loads first, then the ballots in code order up to the round's end
        GifScanCode c[GIF_SCAN_PER_LANE];
#pragma unroll
        for (int i = 0; i < GIF_SCAN_PER_LANE; i++) c[i] = gif_scan_fetch(sc.s, data, nbytes, lane + GIF_LANES * i);
        int ncodes = GIF_SCAN_CODES, kind = GIF_K_CODE;
#pragma unroll
        for (int i = 0; i < GIF_SCAN_PER_LANE; i++) {
            if (ncodes != GIF_SCAN_CODES) continue;            // (wave-uniform: the round has ended)
            const int mine = gif_scan_kind(sc.s, mcs, nbytes, lane + GIF_LANES * i, c[i]);
            const unsigned long long stop = __ballot(mine != GIF_K_CODE);
            if (stop) {
                const int first = __ffsll((long long)stop) - 1;
                ncodes = GIF_LANES * i + first;
                kind = __builtin_amdgcn_readfirstlane(__shfl(mine, first));
            }
        }
        gif_scan_round_end(&sc, mcs, ncodes, kind, segs + 1, cap, lane == 0);
    }
    if (lane == 0) segs[0].start = sc.nseg;
}

// a segment's rounds (k_gif_lzw's), with or without the stores, until the segment's end or the stream's
template <bool EMIT>
__device__ __forceinline__ void gif_segment_wave(GifLzwMem& m, GifLzwState& s, const uint8_t* data, uint32_t nbytes, int mcs,
                                                 const GifPlane& p, uint32_t end, int lane) {
    while (gif_segment_goes_on(s, end)) {
        const int mine = gif_extract(&m, s, mcs, data, nbytes, lane);
        const unsigned long long stop = __ballot(mine != GIF_K_CODE);
        const int ncodes = __builtin_amdgcn_readfirstlane(stop ? __ffsll((long long)stop) - 1 : GIF_LANES);
        const int kind = __builtin_amdgcn_readfirstlane(stop ? __shfl(mine, ncodes & (GIF_LANES - 1)) : (int)GIF_K_CODE);
        __syncthreads();
        gif_link_start(&m, s, lane, ncodes);
        __syncthreads();
#pragma unroll 1
        for (int it = 0; it < 6; it++) {
            gif_link_read(&m, lane);
            __syncthreads();
            gif_link_write(&m, lane);
            __syncthreads();
        }
        gif_link_finish(&m, s, lane, ncodes);
        __syncthreads();
        const uint32_t len = gif_string_len(&m, lane, ncodes);
        uint32_t upto = len;
#pragma unroll
        for (int k = 1; k < GIF_LANES; k <<= 1) {
            const uint32_t t = __shfl_up(upto, k);
            if (lane >= k) upto += t;
        }
        const uint32_t produced = __builtin_amdgcn_readfirstlane(__shfl(upto, GIF_LANES - 1));
        if (EMIT) gif_emit(&m, p, lane, ncodes, s.outpos + upto - len);
        gif_round_end(&s, &m, mcs, ncodes, kind, produced, p.total);
        __syncthreads();
    }
}

__device__ __forceinline__ GifPlane gif_plane_of(uint8_t* blob, const GifLzwDesc& z) {
    GifPlane p;
    p.plane = blob + z.plane_off;
    p.w = z.w; p.h = z.h; p.pitch = z.pitch; p.interlaced = z.interlaced;
    p.total = (uint32_t)p.w * (uint32_t)p.h;
    return p;
}

// the length pass: one wavefront per segment slot (slots[blockIdx.x] = page, k); a page of one segment has none
__global__ __launch_bounds__(GIF_LANES) void k_gif_lzw_len(uint8_t* blob, const GifLzwDesc* __restrict__ d,
                                                           const GifSplitPage* __restrict__ sp, const GifSegSlot* __restrict__ slots) {
    __shared__ GifLzwMem m;
    const int i = slots[blockIdx.x].page;
    const uint32_t k = (uint32_t)slots[blockIdx.x].k;
    GifSeg* segs = (GifSeg*)(blob + sp[i].seg_off);
    const uint32_t count = segs[0].start;
    if (count == 1 || k >= count || k >= sp[i].cap) return;
    const int lane = (int)threadIdx.x;
    const int mcs = d[i].mcs;
    const GifPlane p = gif_plane_of(blob, d[i]);
    GifLzwState s;
    gif_segment_start(&s, mcs, segs[1 + k].start);
    const uint32_t end = segs[1 + k].end;
    gif_table_start(&m, lane);
    __syncthreads();
    gif_segment_wave<false>(m, s, blob + d[i].data_off, d[i].data_bytes, mcs, p, end, lane);
    if (lane == 0) gif_segment_record(&segs[1 + k], s, p.total);
}

// the emit pass: one wavefront per slot; segment 0's writes the pad bytes and the page's status word
__global__ __launch_bounds__(GIF_LANES) void k_gif_lzw_emit(uint8_t* blob, const GifLzwDesc* __restrict__ d,
                                                            const GifSplitPage* __restrict__ sp, const GifSegSlot* __restrict__ slots,
                                                            uint32_t* __restrict__ status) {
    __shared__ GifLzwMem m;
    const int i = slots[blockIdx.x].page;
    const uint32_t k = (uint32_t)slots[blockIdx.x].k;
    const GifSeg* segs = (const GifSeg*)(blob + sp[i].seg_off);
    const uint32_t count = segs[0].start;
    if (k >= count || k >= sp[i].cap) return;
    const int lane = (int)threadIdx.x;
    const int mcs = d[i].mcs;
    const GifPlane p = gif_plane_of(blob, d[i]);
    if (k == 0)
        for (int row = lane; row < p.h; row += GIF_LANES) gif_pad_row(p, row);
    bool live = true;
    const uint32_t base = count == 1 ? 0u : gif_split_base(segs + 1, k, p.total, &live);
    GifLzwState s;
    gif_segment_start(&s, mcs, segs[1 + k].start);
    s.outpos = base;
    if (live) {
        gif_table_start(&m, lane);
        __syncthreads();
        gif_segment_wave<true>(m, s, blob + d[i].data_off, d[i].data_bytes, mcs, p, segs[1 + k].end, lane);
    }
    if (k == 0 && lane == 0) status[d[i].slot] = (uint32_t)(count == 1 ? s.status : gif_split_status(segs + 1, count, p.total));
}

int launch_gif_lzw_split(uint8_t* blob, size_t table_off, size_t split_off, size_t slots_off, const MixIndex& ix, int most, long long nslots,
                         uint32_t* status, hipStream_t s) {
    if (most <= 0) return IMP_OK;
    if (!blob || !status || ((table_off | split_off | slots_off) & 7) || nslots <= 0 || nslots > 0x7fffffffLL) return IMP_ERROR_INVALID_ARGS;
    const GifLzwDesc* d = (const GifLzwDesc*)(blob + table_off);
    const GifSplitPage* sp = (const GifSplitPage*)(blob + split_off);
    const GifSegSlot* slots = (const GifSegSlot*)(blob + slots_off);
    hipLaunchKernelGGL(k_gif_lzw_scan, dim3((unsigned)most * 8), dim3(GIF_LANES), 0, s, blob, d, sp, ix);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gif_lzw_len, dim3((unsigned)nslots), dim3(GIF_LANES), 0, s, blob, d, sp, slots);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_gif_lzw_emit, dim3((unsigned)nslots), dim3(GIF_LANES), 0, s, blob, d, sp, slots, status);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
