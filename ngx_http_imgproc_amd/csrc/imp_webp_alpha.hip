// imp_webp_alpha.hip -- the alpha plane of lossy WebP uploads (impgpu_batch_decode_webp_ex with IMPGPU_WEBP_ACCEPT_LOSSY |
// IMPGPU_WEBP_ACCEPT_ALPHA): the one launch a group takes for its files that have an ALPH chunk, behind k_vp8_dec_frame
// (which wrote the frame with A = 255) and, for a VP8L plane, behind k_webp_dec_inverse (which wrote the scratch plane).
// The lanes' logic and the filter rule are imp_webp_alpha.h's, which the host model runs too.
//   k_webp_alpha   a workgroup (WA_THREADS lanes, four waves) per file.  It reads the residuals -- raw bytes, or byte 1 of
//                  each scratch word -- undoes the filter and stores byte 3 of every pixel; nothing else is written.  A
//                  file with a status word set is left alone.  None: a copy.  Horizontal: wave 0 sums column 0 downwards
//                  into LDS, 64 rows a step; then a wave a row, 64 columns a step, a wave scan plus the carry.  Vertical:
//                  wave 0 sums row 0 into LDS; then a lane a column downwards.  Gradient: wave 0 alone, a band of 64 rows
//                  skewed a column apart, one band after the other (imp_webp_alpha.h).
//
// ORDER OF STORES AND LOADS.  The LDS line is written by wave 0 and read by every wave behind one __syncthreads()
// (horizontal, vertical).  In the gradient it is written and read by lanes of wave 0 only: the last lane of a band stores
// column x at step x + 63, lane 0 of the next band loads it no sooner than w steps later, and a wavefront-scope fence
// between bands keeps the compiler from moving one across the other; a wave's LDS operations run in order.  The cross-lane
// moves are __shfl_up (ds_bpermute), executed by all 64 lanes outside divergent code.  Every store is plain C++.
#include "imp_internal.h"
#include "imp_webp_alpha.h"

namespace imp {

// inclusive prefix sum over the wave's 64 lanes
__device__ __forceinline__ uint32_t wa_wave_scan(uint32_t v, int lane) {
#pragma unroll
    for (int d = 1; d < WA_WAVE; d <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, d, WA_WAVE);
        if (lane >= d) v += u;
    }
    return v;
}

// a line of n residuals, the first at index `first`, the next `stride` further: their running sums (plus `carry`) into the
// frame and, if `keep`, into LDS -- one wave, 64 a step
__device__ __forceinline__ void wa_line(const WaSrc& src, uint8_t* img, size_t first, size_t stride, int n, uint32_t carry, uint8_t* keep, int lane) {
#pragma unroll 1
    for (int k0 = 0; k0 < n; k0 += WA_WAVE) {
        const int k = k0 + lane;
        const size_t i = first + (size_t)k * stride;
        const uint32_t a = (carry + wa_wave_scan(k < n ? wa_res(src, i) : 0u, lane)) & 255u;
        if (k < n) {
            wa_put(img, i, a);
            if (keep) keep[k] = (uint8_t)a;
        }
        carry = (uint32_t)__shfl((int)a, WA_WAVE - 1, WA_WAVE);
    }
}

__global__ __launch_bounds__(WA_THREADS) void k_webp_alpha(uint8_t* __restrict__ mem, const WaFileDesc* __restrict__ files, const uint32_t* __restrict__ status) {
    __shared__ uint8_t line[WA_MAX_SIDE + 1];                            // column 0, row 0, or the last row of the gradient's band
    const WaFileDesc& d = files[blockIdx.x];
    if (status[d.status_frame] != 0u || status[d.status_stream] != 0u) return;
    const int w = d.w, h = d.h;
    if (w < 1 || h < 1 || w > WA_MAX_SIDE || h > WA_MAX_SIDE) return;    // (the host front lets no such file through)
    const WaSrc src{mem + d.src_off, d.method ? 4 : 1, d.method ? 1 : 0};
    uint8_t* img = d.img;
    const int t = (int)threadIdx.x, lane = t & (WA_WAVE - 1), wave = t / WA_WAVE;
    if (d.filter == WA_NONE) {
        wa_copy(src, img, (size_t)w * (size_t)h, (uint32_t)t, (uint32_t)WA_THREADS);
    } else if (d.filter == WA_HORIZONTAL) {
        if (wave == 0) wa_line(src, img, 0, (size_t)w, h, 0u, line, lane);
        __syncthreads();
#pragma unroll 1
        for (int y = wave; y < h; y += WA_THREADS / WA_WAVE) wa_line(src, img, (size_t)y * (size_t)w + 1u, 1, w - 1, line[y], nullptr, lane);
    } else if (d.filter == WA_VERTICAL) {
        if (wave == 0) wa_line(src, img, 0, 1, w, 0u, line, lane);
        __syncthreads();
#pragma unroll 1
        for (int x = t; x < w; x += WA_THREADS) wa_column(src, img, w, h, x, line[x]);
    } else if (wave == 0) {
#pragma unroll 1
        for (int row0 = 0; row0 < h; row0 += WA_WAVE) {
            const int rows = h - row0 < WA_WAVE ? h - row0 : WA_WAVE, steps = wa_band_steps(w, rows);
            WaLane L{0u, 0u};
#pragma unroll 1
            for (int step = 0; step < steps; step++) {
                uint32_t top = (uint32_t)__shfl_up((int)L.mine, 1, WA_WAVE);
                if (lane == 0) top = row0 && step < w ? line[step] : 0u;
                if (wa_gradient_step(src, img, w, h, row0, step, lane, top, L) && lane == rows - 1) line[step - lane] = (uint8_t)L.mine;
            }
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        }
    }
}

int launch_webp_alpha(uint8_t* mem, const WaFileDesc* files, const uint32_t* status, int nfiles, hipStream_t s) {
    if (nfiles <= 0) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_webp_alpha, dim3((unsigned)nfiles), dim3(WA_THREADS), 0, s, mem, files, status);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
