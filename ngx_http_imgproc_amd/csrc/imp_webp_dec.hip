// imp_webp_dec.hip -- lossless WebP uploads decoded on the device (impgpu_batch_decode_webp): the three launches a group
// of files takes, whatever it holds.  The lanes' logic is imp_webp_dec.h's, which the host model runs too.
//   k_webp_dec_tables   a wavefront per prefix code (every group of every file, side by side): count, scan and verdict,
//                       symbols by length, the lookup table -- into global memory (a file may have thousands of groups);
//                       a refused code makes the FILE's status word WD_DAMAGED
//   k_webp_dec_pixels   a wavefront per file, in rounds (imp_webp_dec.h): the compressed words are staged into LDS, the
//                       token list, the colour cache and the loaded group's five codes live there (WdMem, about 34 KB:
//                       four workgroups of one wave on a CU's 160 KB); the residual plane is in global memory
//   k_webp_dec_inverse  a workgroup of 256 per file undoes the transforms last to first and writes B,G,R,A
// A file whose status word is not zero is left alone by the launches behind the one that set it.
//
// ORDER OF STORES AND LOADS.  A match may reach back to the first pixel, so a wave reads sources from the plane it stored
// in earlier rounds and earlier in this round, and the predictor's inverse reads the pixels the lane above stored a step
// before: loads of words that OTHER lanes of the same workgroup stored.  What makes those stores visible is the
// __syncthreads() between the two steps -- a workgroup-scope release and acquire around the barrier, for which the
// compiler waits for every outstanding store (s_waitcnt vmcnt(0) / vscnt) before s_barrier; the waves of a workgroup
// share one CU and its write-through vector L1 (the kernels are not built for threadgroup-split mode).  Nothing here is
// read by another workgroup of the same launch.
//
// Every store is plain C++ (vector stores); the status words are set with atomicMax: no inline assembly.
#include "imp_internal.h"
#include "imp_webp_dec.h"

namespace imp {

__global__ __launch_bounds__(WD_LANES) void k_webp_dec_tables(uint8_t* __restrict__ mem, const WdFileDesc* __restrict__ files,
                                                               const WdCodeItem* __restrict__ items, uint32_t* __restrict__ status) {
    const WdCodeItem it = items[blockIdx.x];
    const WdFileDesc& d = files[it.file];
    const int lane = (int)threadIdx.x;
    const uint32_t stride = wd_sorted_stride(d.cache_bits);
    const size_t at = (size_t)it.group * stride + wd_sorted_at(it.k, d.cache_bits);
    const uint8_t* lens = mem + d.lens_off + at;
    uint16_t* sorted = (uint16_t*)(mem + d.sorted_off) + at;
    WdCode* c = (WdCode*)(mem + d.codes_off) + (size_t)it.group * WD_CODES + it.k;
    const int n = (int)wd_alphabet(it.k, d.cache_bits);
    wd_build_count(c, lens, n, lane);
    __syncthreads();
    const bool ok = __builtin_amdgcn_readfirstlane((int)wd_build_scan(c, n, lane)) != 0;
    __syncthreads();
    if (!ok) {
        if (lane == 0) atomicMax(&status[it.file], (uint32_t)WD_DAMAGED);
        return;
    }
    wd_build_sort(c, lens, n, sorted, lane);
    __syncthreads();
    wd_build_fill(c, sorted, lane);
}

__global__ __launch_bounds__(WD_LANES) void k_webp_dec_pixels(uint8_t* __restrict__ mem, const WdFileDesc* __restrict__ files,
                                                               uint32_t* __restrict__ status) {
    __shared__ WdMem m;
    const int f = (int)blockIdx.x;
    const WdFileDesc& d = files[f];
    const int lane = (int)threadIdx.x;
    if (status[f] != 0u) return;                                // a refused code: nothing is looked up in it
    WdImage im;
    im.in = mem + d.in_off; im.in_size = d.in_size; im.in_cap = d.in_cap;
    im.w = d.cw; im.h = d.h; im.npix = (uint32_t)d.cw * (uint32_t)d.h;
    im.cache_bits = d.cache_bits;
    im.meta_bits = d.meta_bits; im.meta_w = d.meta_w; im.meta = (const uint32_t*)(mem + d.meta_off);
    im.codes = (const WdCode*)(mem + d.codes_off); im.sorted = (const uint16_t*)(mem + d.sorted_off);
    im.sorted_stride = wd_sorted_stride(d.cache_bits); im.green_n = wd_green_n(d.cache_bits); im.ngroups = d.ngroups;
    im.out = (uint32_t*)(mem + d.plane_off);
    WdState s;
    wd_start(&s, im, d.bitpos);
    wd_cache_clear(&m, lane);
    __syncthreads();
    while (!__builtin_amdgcn_readfirstlane(s.done)) {
        wd_stage(&m, im, s.bitpos, lane);
        __syncthreads();
        WdBits b;
        wd_bits_begin(&b, m.in, WD_IN_WORDS, (s.bitpos >> 5) << 5, s.bitpos);
        WdRound r;
        wd_round_begin(&r, s);
        for (;;) {
            const int want = __builtin_amdgcn_readfirstlane(r.want);
            if (want != __builtin_amdgcn_readfirstlane(s.group)) {
                __syncthreads();
                wd_group_load(&m, im, want, lane);
                s.group = want;
                __syncthreads();
            }
            wd_decode(&m, im, &s, &b, &r, lane);
            if (__builtin_amdgcn_readfirstlane(r.want) == __builtin_amdgcn_readfirstlane(s.group)) break;
        }
        __syncthreads();
        const int ntok = __builtin_amdgcn_readfirstlane(r.ntok);
#pragma unroll 1
        for (int t = 0; t < ntok;) {
            const int t1 = __builtin_amdgcn_readfirstlane(wd_run_end(&m, t, ntok));
            wd_emit_run(&m, im, t, t1, lane);
            __syncthreads();
            t = t1;
            if (t < ntok) {
                wd_emit_copy(&m, im, t, lane);
                __syncthreads();
                if (im.cache_bits) {
                    wd_cache_stamp(&m, im, t, lane);
                    __syncthreads();
                    wd_cache_put(&m, im, t, lane);
                    __syncthreads();
                }
                t++;
            }
        }
        wd_round_end(&s, im, r);
        __syncthreads();
    }
    if (lane == 0 && s.status != WD_OK) atomicMax(&status[f], (uint32_t)s.status);
}

constexpr int WD_INV_THREADS = WD_INV_LANES;

__global__ __launch_bounds__(WD_INV_THREADS) void k_webp_dec_inverse(uint8_t* __restrict__ mem, const WdFileDesc* __restrict__ files,
                                                                      const uint32_t* __restrict__ status) {
    const int f = (int)blockIdx.x;
    const WdFileDesc& d = files[f];
    if (status[f] != 0u) return;
    const uint32_t lane = threadIdx.x, nl = WD_INV_THREADS;
    uint32_t* cur = (uint32_t*)(mem + d.plane_off);
    uint32_t* other = (uint32_t*)d.img;
    const int ntrans = d.ntrans < 4 ? d.ntrans : 4;
#pragma unroll 1
    for (int i = ntrans - 1; i >= 0; i--) {
        const WdTransform t = d.tr[i];
        const uint32_t* data = (const uint32_t*)(mem + t.data_off);
        const int w = t.xsize;
        const uint32_t npix = (uint32_t)w * (uint32_t)d.h;
        if (t.type == WD_TR_SUB_GREEN) {
            wd_inv_add_green(cur, npix, lane, nl);
        } else if (t.type == WD_TR_COLOR) {
            wd_inv_color(cur, w, d.h, t.bits, data, lane, nl);
        } else if (t.type == WD_TR_INDEXING) {
            wd_inv_index(cur, other, w, d.h, t.bits, data, t.ncolors, lane, nl);
            uint32_t* x = cur; cur = other; other = x;
        } else {
            const int band = d.h < WD_INV_THREADS ? d.h : WD_INV_THREADS;     // rows side by side
            const int steps = wd_pred_steps(w, band);
#pragma unroll 1
            for (int row0 = 0; row0 < d.h; row0 += band) {
#pragma unroll 1
                for (int s = 0; s < steps; s++) {
                    if ((int)lane < band) wd_inv_pred_step(cur, w, d.h, t.bits, data, row0, s, (int)lane);
                    __syncthreads();
                }
            }
        }
        __syncthreads();
    }
    wd_finish(cur, (uint32_t*)d.img, (uint32_t)d.w * (uint32_t)d.h, d.alpha_used, lane, nl);
}

int launch_webp_decode(uint8_t* mem, const WdFileDesc* files, const WdCodeItem* items, long long nitems, uint32_t* status, int nfiles, hipStream_t s) {
    if (nfiles <= 0 || nitems <= 0 || nitems > 0x7fffffffLL) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_webp_dec_tables, dim3((unsigned)nitems), dim3(WD_LANES), 0, s, mem, files, items, status);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_dec_pixels, dim3((unsigned)nfiles), dim3(WD_LANES), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_webp_dec_inverse, dim3((unsigned)nfiles), dim3(WD_INV_THREADS), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
