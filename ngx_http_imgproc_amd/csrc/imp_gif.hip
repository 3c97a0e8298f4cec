// imp_gif.hip -- k_gif_lzw: the LZW pages of every GIF file of a call, decoded on the device straight into the index
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

}  // namespace imp
