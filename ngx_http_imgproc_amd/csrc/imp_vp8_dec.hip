// imp_vp8_dec.hip -- lossy WebP uploads (VP8 key frames) decoded on the device (impgpu_batch_decode_webp_ex with
// IMPGPU_WEBP_ACCEPT_LOSSY): the three launches a group's lossy files take, whatever they hold.  The lanes' logic is
// imp_vp8_dec.h's, which the host model runs too.
//   k_vp8_dec_recon    a workgroup per file, files side by side.  One lane walks the file's macroblocks in raster order:
//                      modes out of the first partition, tokens out of the row's partition, prediction plus inverse
//                      transforms into the padded planes.  Everything a macroblock needs (the contexts of the row above,
//                      the samples above, above-right and left) is that lane's own earlier work: nothing is waited for,
//                      and the walk ends after mbw x mbh macroblocks whatever the bytes say.  The macroblock in work and
//                      the nine boolean decoders live in LDS.
//   k_vp8_dec_filter   a workgroup (one wave) per file: the loop filter, macroblocks in raster order as libwebp runs them
//                      (the result depends on the order); within a macroblock eight steps, the 16 + 8 + 8 lines of an edge
//                      side by side, a barrier between steps.
//   k_vp8_dec_frame    fully parallel: fancy upsampling, YUV -> B,G,R,A, the crop.
// A file whose status word is not zero is left alone by the launches behind the one that set it.
//
// ORDER OF STORES AND LOADS.  k_vp8_dec_filter's lanes read samples that other lanes of the same wave stored a step
// before; the __syncthreads() between steps is the workgroup-scope release and acquire that makes them visible.  Nothing
// is read by another workgroup of the same launch.  Every store is plain C++; the status words are set with atomicMax.
#include "imp_internal.h"
#include "imp_vp8_dec.h"

namespace imp {

constexpr int VD_THREADS = 64, VD_FRAME_THREADS = 256, VD_FRAME_BLOCKS = 64;

__device__ __forceinline__ VdPlanes vd_planes(uint8_t* mem, const VdFileDesc& d) {
    return VdPlanes{mem + d.y_off, mem + d.u_off, mem + d.v_off, d.hdr.mbw * 16, d.hdr.mbw * 8};
}

__global__ __launch_bounds__(VD_THREADS) void k_vp8_dec_recon(uint8_t* __restrict__ mem, const VdFileDesc* __restrict__ files, uint32_t* __restrict__ status) {
    __shared__ VdWalk walk;
    __shared__ VdMb mb;
    const int f = (int)blockIdx.x;
    const VdFileDesc& d = files[f];
    if (threadIdx.x != 0) return;
    uint8_t* ctx = mem + d.ctx_off;
    walk.top_nz = ctx; walk.top_dc = ctx + d.hdr.mbw; walk.top_modes = ctx + 2 * (size_t)d.hdr.mbw;
    const int st = vd_decode_mbs(d.hdr, mem + d.chunk_off, walk, mb, vd_planes(mem, d), (uint32_t*)(mem + d.finfo_off));
    if (st != VD_OK) atomicMax(&status[f], (uint32_t)st);
}

__global__ __launch_bounds__(VD_THREADS) void k_vp8_dec_filter(uint8_t* __restrict__ mem, const VdFileDesc* __restrict__ files, const uint32_t* __restrict__ status) {
    const int f = (int)blockIdx.x;
    const VdFileDesc& d = files[f];
    if (status[f] != 0u || d.hdr.filter_type == 0) return;
    const VdPlanes P = vd_planes(mem, d);
    const uint32_t* finfo = (const uint32_t*)(mem + d.finfo_off);
    const int lane = (int)threadIdx.x, nmb = d.hdr.mbw * d.hdr.mbh;
#pragma unroll 1
    for (int i = 0; i < nmb; i++) {
        const uint32_t info = finfo[i];
        const int mx = i % d.hdr.mbw, my = i / d.hdr.mbw;
#pragma unroll 1
        for (int step = 0; step < VD_FILTER_STEPS; step++) {
            vd_filter_step(d.hdr, P, info, mx, my, step, lane);
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(VD_FRAME_THREADS) void k_vp8_dec_frame(uint8_t* __restrict__ mem, const VdFileDesc* __restrict__ files, const uint32_t* __restrict__ status) {
    const int f = (int)blockIdx.x;
    const VdFileDesc& d = files[f];
    if (status[f] != 0u) return;
    const VdPlanes P = vd_planes(mem, d);
    const int w = d.hdr.w, h = d.hdr.h;
    const long long npix = (long long)w * h;
    uint32_t* out = (uint32_t*)d.img;
    for (long long i = (long long)blockIdx.y * VD_FRAME_THREADS + threadIdx.x; i < npix; i += (long long)VD_FRAME_BLOCKS * VD_FRAME_THREADS)
        out[i] = vd_frame_pixel(P, w, h, (int)(i % w), (int)(i / w));
}

int launch_vp8_decode(uint8_t* mem, const VdFileDesc* files, uint32_t* status, int nfiles, hipStream_t s) {
    if (nfiles <= 0) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_vp8_dec_recon, dim3((unsigned)nfiles), dim3(VD_THREADS), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vp8_dec_filter, dim3((unsigned)nfiles), dim3(VD_THREADS), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vp8_dec_frame, dim3((unsigned)nfiles, VD_FRAME_BLOCKS), dim3(VD_FRAME_THREADS), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
