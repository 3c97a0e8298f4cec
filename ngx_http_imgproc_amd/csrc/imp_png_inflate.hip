// imp_png_inflate.hip -- k_png_inflate: the zlib streams of every PNG file of a call (impgpu_batch_decode_png_ex with
// IMPGPU_PNG_DEVICE_INFLATE), inflated on the device straight into the scanline regions k_png_unfilter_batch and k_png_place
// read.  One workgroup of ONE wavefront per stream; the lanes' logic is imp_inflate_lanes.h's, which the host diagnostic
// (impgpu_png_inflate_lanes) runs too.
//
// The stream's tables, token list and window ring (InfMem, 52 KB) are the workgroup's LDS: three workgroups fit a CU's
// 160 KB, so a CU runs three streams and the device 768 -- three times the most a call can hold.  The barriers between a
// round's steps are barriers of that one wave; the rounds of different streams never wait for each other.  Back-references
// are read from the LDS ring, never from the destination.  Behind the inflate the same wave reads the rows' filter bytes
// back from the destination: those are loads of bytes that other lanes of the workgroup stored, and what makes the stores
// visible to them is the __syncthreads() in between -- a workgroup-scope release and acquire around the barrier, for which
// the compiler waits for every outstanding store (s_waitcnt vmcnt(0) / vscnt) before s_barrier; the waves of a workgroup
// share one CU and its write-through vector L1 (the kernel is not built for threadgroup-split mode).
//
// Every store is plain C++ (vector stores): no inline assembly.
#include "imp_internal.h"
#include "imp_inflate_lanes.h"
#include "imp_png.h"

namespace imp {

// a code by the whole wave: count | scan and verdict | symbols by length | lookup table
__device__ __forceinline__ bool png_inf_build(InfCode* c, const uint8_t* lens, int n, uint16_t* fast, int fbits, bool must_be_complete, int lane) {
    inf_build_count(c, lens, n, fast, fbits, lane);
    __syncthreads();
    const bool ok = inf_build_scan(c, must_be_complete, lane);
    __syncthreads();
    inf_build_sort(c, lens, n, lane);
    __syncthreads();
    inf_build_fill(c, fast, fbits, lane);
    __syncthreads();
    return __builtin_amdgcn_readfirstlane((int)ok) != 0;
}

__global__ __launch_bounds__(INF_LANES) void k_png_inflate(const PngInflateDesc* __restrict__ descs) {
    __shared__ InfMem m;
    const PngInflateDesc& d = descs[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint8_t* in = d.in;
    uint8_t* out = d.out;
    // the region behind the scanlines: the slack the unfilter kernels' word loads may touch, the palette of a palette file
    for (uint32_t i = (uint32_t)lane; i < d.slack; i += INF_LANES) out[(size_t)d.out_size + i] = 0;
    if (d.pal)
        for (int i = lane; i < 256; i += INF_LANES) d.pal_dst[i] = d.pal[i];
    InfState s;
    inf_start(&s, in, d.in_size, d.out_size);
    while (!__builtin_amdgcn_readfirstlane(s.done)) {
        inf_stage(&m, in, d.in_cap, s, lane);
        __syncthreads();
        InfBits b;
        inf_bits_begin(&m, &b, s);
        InfRound r;
        inf_round_begin(&r, s);
        if (__builtin_amdgcn_readfirstlane(s.block) == 0) {
            const int kind = __builtin_amdgcn_readfirstlane(inf_block_begin(&m, &s, &b, lane));
            __syncthreads();
            if (kind == INF_B_DYNAMIC) {
                if (!png_inf_build(&m.cl, m.cllens, 19, nullptr, 0, true, lane)) inf_fail(&s, INF_DAMAGED);
                else inf_block_lens(&m, &s, &b, lane);
                __syncthreads();
            } else if (kind == INF_B_FIXED) {
                inf_fixed_lens(&m, lane);
                __syncthreads();
            }
            if (!__builtin_amdgcn_readfirstlane(s.done) && kind >= INF_B_FIXED) {
                const int nlen = __builtin_amdgcn_readfirstlane(s.nlen), ndist = __builtin_amdgcn_readfirstlane(s.ndist);
                const bool ll_ok = png_inf_build(&m.ll, m.lens, nlen, m.fast_ll, INF_LL_FAST, false, lane);
                const bool d_ok = png_inf_build(&m.d, m.lens + nlen, ndist, m.fast_d, INF_D_FAST, false, lane);
                if (!ll_ok || !d_ok) inf_fail(&s, INF_DAMAGED);
            }
        }
        if (!__builtin_amdgcn_readfirstlane(s.done)) {
            if (__builtin_amdgcn_readfirstlane(s.block) == 1) {
                inf_stored_plan(s, &r);
                inf_stored_copy(&m, s, r, in, lane);
            } else {
                inf_decode(&m, s, &b, &r, lane);
                __syncthreads();
                inf_emit_par(&m, s, r, lane);
                const int nord = __builtin_amdgcn_readfirstlane(r.nord);
#pragma unroll 1
                for (int k = 0; k < nord; k++) {
                    __syncthreads();
                    inf_emit_ord(&m, s, k, lane);
                }
            }
            __syncthreads();
            inf_flush(&m, s, r, out, lane);
        }
        inf_round_end(&s, r);
        __syncthreads();
    }
    // every row's filter byte: above 4 is damage (PNG specification 9.2); cleared, so the unfilter kernels never meet one
    __syncthreads();
    int bad = 0;
    uint32_t off = 0;
    for (int k = 0; k < d.nitems && k < 7; k++) {
        for (uint32_t row = (uint32_t)lane; row < d.rows[k]; row += INF_LANES) {
            const uint64_t at = (uint64_t)off + (uint64_t)row * d.stride[k];
            if (at >= (uint64_t)d.out_size) break;
            if (out[at] > 4) {
                bad = 1;
                inf_store(out, d.out_size, (uint32_t)at, 0);
            }
        }
        off += d.rows[k] * d.stride[k];
    }
    const bool any_bad = __ballot(bad) != 0ull;
    if (lane == 0) *d.status = (uint32_t)(s.status != INF_OK ? s.status : any_bad ? INF_FILTER : INF_OK);
}

int launch_png_inflate(const PngInflateDesc* descs, int count, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    hipLaunchKernelGGL(k_png_inflate, dim3((unsigned)count), dim3(INF_LANES), 0, s, descs);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
