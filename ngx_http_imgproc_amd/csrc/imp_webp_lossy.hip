// imp_webp_lossy.hip -- the five launches that turn the frames of a call into lossy WebP files
// (impgpu_batch_encode_webp_lossy): k_vp8_planes, _recon, _tokens, _bool and _pack.  The lanes' logic is imp_webp_lossy.h's,
// which the host encoder (impgpu_webp_lossy_encode_host) runs too.  Each launch reads what the one before wrote across the
// kernel boundary of one stream.  Only k_vp8_recon has wavefronts that wait, and only for wavefronts of their own workgroup:
// a macroblock row waits for the row above, which an earlier wavefront (or an earlier turn of the same one) holds, so the
// first unfinished row can always move.
#include "imp_internal.h"
#include "imp_webp_lossy.h"

namespace imp {

__device__ __forceinline__ Vp8Frame vp8_frame_of(const Vp8FrameDesc& f) { return Vp8Frame{f.src, f.w, f.h, f.c, f.step}; }

// PLANES: a workgroup per macroblock row of a frame of the call
__global__ __launch_bounds__(256) void k_vp8_planes(Vp8Dev D) {
    const Vp8RowItem it = D.rows[blockIdx.x];
    const Vp8FrameDesc& f = D.frames[it.frame];
    const bool seen = vp8_planes_lane(vp8_frame_of(f), f.mbw, it.row, D.mem + f.y_off, D.mem + f.u_off, D.mem + f.v_off,
                                      f.c == 4 ? D.mem + f.alpha_off : nullptr, (int)threadIdx.x, 256);
    if (seen) atomicOr(&D.works[it.frame].alpha_seen, 1u);
}

// the lanes of a wavefront meet: what they wrote to LDS is there for the others
// (a wavefront's LDS instructions execute in order: a fence of wavefront scope keeps the compiler from moving them, and
// needs no wait -- the next macroblock's samples, fetched ahead, stay in flight across it)
__device__ __forceinline__ void vp8_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int vp8_progress(int* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP); }

// RECON: a workgroup per frame, W wavefronts of it at work, wavefront k taking macroblock rows k, k + W, ...  A row's
// macroblock x starts when the row above has finished x (s_prog, a counter a row); the reconstruction's last row of a
// macroblock row (Y, U, V: 2 wpad bytes) lives in slot row % W of the dynamic LDS, and a row takes its slot only when the
// row that read it (row - W + 1) is finished.  W is VP8_WAVES, or as many slots as the dynamic LDS (D.border_lds) holds
// of this frame's width (3 at 16383 pixels).  A lane fetches its share of the next macroblock's samples while this one is
// worked on.
__global__ __launch_bounds__(VP8_WAVES * 64) void k_vp8_recon(Vp8Dev D) {
    extern __shared__ uint8_t s_border[];
    __shared__ Vp8Mb s_mb[VP8_WAVES];
    __shared__ int s_prog[1024];
    const Vp8FrameDesc& f = D.frames[blockIdx.x];
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < f.mbh; i += VP8_WAVES * 64) s_prog[i] = 0;
    __syncthreads();
    const int wpad = f.mbw * 16;
    const int slots = D.border_lds / (2 * wpad), W = slots < VP8_WAVES ? slots : VP8_WAVES;
    if (wave >= W) return;                                              // (no barrier follows)
    Vp8Row R;
    R.ysrc = D.mem + f.y_off; R.usrc = D.mem + f.u_off; R.vsrc = D.mem + f.v_off;
    R.mbw = f.mbw;
    vp8_steps(f.qi, R.q);
    vp8_recips(R.q, R.rq);
    R.levels = (int16_t*)(D.mem + f.lev_off);
    R.info = (uint32_t*)(D.mem + f.info_off);
    R.yrec = R.urec = R.vrec = nullptr;
    Vp8Mb& S = s_mb[wave];
    for (int my = wave; my < f.mbh; my += W) {
        R.my = my;
        Vp8Fetch next = vp8_mb_fetch(R, 0, lane);
        if (my >= W)
            while (vp8_progress(&s_prog[my - W + 1]) < f.mbw) __builtin_amdgcn_s_sleep(8);
        R.above = my ? s_border + (size_t)((my - 1) % W) * 2u * (size_t)wpad : nullptr;
        R.border = s_border + (size_t)(my % W) * 2u * (size_t)wpad;
        int known = 0;                                                  // macroblocks of the row above known to be finished
        for (int mx = 0; mx < f.mbw; mx++) {
            if (my > 0)
                while (known <= mx) {
                    known = vp8_progress(&s_prog[my - 1]);
                    if (known <= mx) __builtin_amdgcn_s_sleep(1);
                }
            const Vp8Fetch cur = next;
            vp8_mb_phase(0, S, R, mx, lane, cur);
            vp8_wave_sync();
            if (mx + 1 < f.mbw) next = vp8_mb_fetch(R, mx + 1, lane);
#pragma unroll 1
            for (int ph = 1; ph < VP8_PHASES; ph++) {
                vp8_mb_phase(ph, S, R, mx, lane, cur);
                vp8_wave_sync();
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");      // every lane's share of the border row is written
            if (lane == 0) __hip_atomic_store(&s_prog[my], mx + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
}

// TOKENS: a lane per macroblock writes its records into the macroblock's own slot
__global__ __launch_bounds__(64) void k_vp8_tokens(Vp8Dev D) {
    const Vp8FrameDesc& f = D.frames[blockIdx.y];
    const uint32_t mb = blockIdx.x * 64u + threadIdx.x;
    if (mb >= f.nmb) return;
    const uint32_t* info = (const uint32_t*)(D.mem + f.info_off);
    const uint32_t mx = mb % (uint32_t)f.mbw;
    ((uint32_t*)(D.mem + f.nrec_off))[mb] = vp8_mb_tokens((const int16_t*)(D.mem + f.lev_off) + (size_t)mb * 400u, info[mb], mx ? info[mb - 1u] : 0u,
                                                           mb >= (uint32_t)f.mbw ? info[mb - (uint32_t)f.mbw] : 0u,
                                                           (uint16_t*)(D.mem + f.rec_off) + (size_t)mb * VP8_MB_RECORDS);
}

// BOOL: a wavefront per (frame, partition): blockIdx.x 0..7 the token partitions, 8 the first one.  The first lane codes;
// for a token partition the 64 lanes stage its records in LDS, 64 at a time, so that the coding lane reads no device
// memory between two of its own stores.
__global__ __launch_bounds__(64) void k_vp8_bool(Vp8Dev D) {
    __shared__ uint16_t s_rec[64];
    const Vp8FrameDesc& f = D.frames[blockIdx.y];
    Vp8Work* W = &D.works[blockIdx.y];
    const int p = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (p == 8) {
        if (lane == 0)
            W->first_len = vp8_len32(vp8_code_first((const uint32_t*)(D.mem + f.info_off), f.nmb, f.qi, f.nparts, D.mem + f.first_off, vp8_first_bound(f.nmb)));
        return;
    }
    if (p >= f.nparts) return;                                          // (uniform)
    const uint16_t* rec = (const uint16_t*)(D.mem + f.rec_off);
    const uint32_t* nrec = (const uint32_t*)(D.mem + f.nrec_off);
    Vp8Bool e = vp8_bool_begin(D.mem + f.part_off[p], vp8_partition_bound(f.mbw, f.mbh, f.nparts, p));
    for (int my = p; my < f.mbh; my += f.nparts)
        for (int mx = 0; mx < f.mbw; mx++) {
            const size_t mb = (size_t)my * (size_t)f.mbw + (size_t)mx;
            const uint16_t* r = rec + mb * VP8_MB_RECORDS;
            const uint32_t n = nrec[mb] < VP8_MB_RECORDS ? nrec[mb] : VP8_MB_RECORDS;
            for (uint32_t at = 0; at < n; at += 64u) {
                __syncthreads();                                        // the chunk before is coded
                if (at + (uint32_t)lane < n) s_rec[lane] = r[at + (uint32_t)lane];
                __syncthreads();
                if (lane == 0) {
                    const uint32_t m = n - at < 64u ? n - at : 64u;
                    for (uint32_t i = 0; i < m; i++) vp8_bool_put(e, s_rec[i] & 255, s_rec[i] >> 8);
                }
            }
        }
    if (lane == 0) W->part_len[p] = vp8_len32(vp8_bool_finish(e));
}

// PACK: VP8_PACK_BLOCKS workgroups a frame copy the pieces to their places; the first writes the bytes between them and
// the record
constexpr int VP8_PACK_BLOCKS = 16;
__device__ __forceinline__ void vp8_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += VP8_PACK_BLOCKS * 256u) dst[i] = src[i];
}
__global__ __launch_bounds__(256) void k_vp8_pack(Vp8Dev D) {
    const Vp8FrameDesc& f = D.frames[blockIdx.y];
    const Vp8Work* W = &D.works[blockIdx.y];
    uint32_t part_len[8];
    bool fits = W->first_len <= vp8_first_bound(f.nmb);
    for (int p = 0; p < 8; p++) {
        part_len[p] = p < f.nparts ? W->part_len[p] : 0u;
        fits = fits && (p >= f.nparts || part_len[p] <= vp8_partition_bound(f.mbw, f.mbh, f.nparts, p));
    }
    const bool alpha = f.c == 4 && W->alpha_seen != 0u;
    const Vp8Layout L = vp8_layout(f.w, f.h, alpha, W->first_len, part_len, f.nparts);
    fits = fits && L.file_len <= f.out_bytes;                           // (always: the regions are the worst case)
    if (blockIdx.x == 0 && threadIdx.x == 0) D.recs[blockIdx.y].file_len = fits ? L.file_len : ~0ull;   // 0: the format cannot hold it
    if (!fits || !L.file_len) return;
    uint8_t* out = D.mem + f.out_off;
    if (blockIdx.x == 0 && threadIdx.x == 0) vp8_write_headers(out, L, f.w, f.h, W->first_len, part_len, f.nparts);
    if (alpha) vp8_copy(out + L.alph_at + 9u, D.mem + f.alpha_off, (uint32_t)f.w * (uint32_t)f.h);
    vp8_copy(out + L.first_at, D.mem + f.first_off, W->first_len);
    for (int p = 0; p < f.nparts; p++) vp8_copy(out + L.part_at[p], D.mem + f.part_off[p], part_len[p]);
}

int launch_vp8_encode(Vp8Dev D, long long nrows, int max_wpad, uint32_t max_nmb, hipStream_t s) {
    if (!D.mem || nrows <= 0 || D.nframes <= 0 || nrows > 0x7fffffffLL || max_wpad <= 0 || max_wpad > 16384 || max_nmb == 0u) return IMP_ERROR_INVALID_ARGS;
    hipLaunchKernelGGL(k_vp8_planes, dim3((unsigned)nrows), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    const hipError_t e = lds_limit_once<k_vp8_recon>();
    if (e != hipSuccess) { set_error("k_vp8_recon", e); return IMP_ERROR_DEVICE; }
    D.border_lds = std::min(VP8_BORDER_LDS, VP8_WAVES * 2 * max_wpad);
    hipLaunchKernelGGL(k_vp8_recon, dim3((unsigned)D.nframes), dim3(VP8_WAVES * 64), (size_t)D.border_lds, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vp8_tokens, dim3((max_nmb + 63u) / 64u, (unsigned)D.nframes), dim3(64), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vp8_bool, dim3(9, (unsigned)D.nframes), dim3(64), 0, s, D);
    IMP_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_vp8_pack, dim3(VP8_PACK_BLOCKS, (unsigned)D.nframes), dim3(256), 0, s, D);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
