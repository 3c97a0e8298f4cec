// imp_jpeg_prog.hip -- the device's entropy stage for progressive JPEG files (imp_jpeg_prog.h): the planes of the call's
// progressive files are zeroed by one launch, then every LEVEL of scans is one launch for all files, a lane per item
// (file, scan, restart interval), running the host-and-device decoders of imp_jpeg_prog.h.  Stream order between the
// launches is what an AC refinement needs: the coefficients the earlier levels wrote.
//
// Shape: an item per lane, items sorted by decoder kind so that a wave runs one decoder, 64 lanes (one wave) per
// workgroup.  An item is a long serial walk and a call has few of them -- a 640 x 480 file without restart intervals has
// ten -- so the workgroups are as small as the hardware makes them: every wave gets a compute unit's scheduler, scalar
// cache and L1 to itself before any unit holds two.  Nothing is staged through LDS: a lane reads its own stream word by
// word (the reader keeps the next word in a register; a lane comes back to its 128-byte line 32 times), the tables
// (3 KB each) are read through the L1/L2 caches, and with one wave per workgroup LDS would buy no sharing.
#include <hip/hip_runtime.h>
#include "imp_jpeg_prog.h"

namespace imp {

namespace {

constexpr int PROG_BLOCK = 64;                      // lanes per workgroup of k_jpeg_prog_level: one wave
constexpr int ZERO_BLOCK = 256, ZERO_GRID_X = 64;   // k_jpeg_prog_zero: 64 workgroups per file, 16 bytes per lane and step

// the planes start out as zeros (libjpeg's coefficient arrays do): blocks no scan reaches -- the MCU padding of a
// one-component scan -- and the coefficients no symbol names stay that way
__global__ __launch_bounds__(ZERO_BLOCK) void k_jpeg_prog_zero(const JpegProgFileDev* __restrict__ files) {
    const JpegProgFileDev& D = files[blockIdx.y];
    typedef int __attribute__((ext_vector_type(4))) v4i;
    v4i* q = (v4i*)D.coef;                                           // (256-byte aligned; total_slots is a multiple of 64 shorts)
    const uint32_t n = D.total_slots / 8;
    const v4i zero = {0, 0, 0, 0};
    for (uint32_t i = blockIdx.x * ZERO_BLOCK + threadIdx.x; i < n; i += ZERO_GRID_X * ZERO_BLOCK) q[i] = zero;
}

__global__ __launch_bounds__(PROG_BLOCK) void k_jpeg_prog_level(const JpegProgFileDev* __restrict__ files, const JpegProgItem* __restrict__ items, uint32_t nitems) {
    const uint32_t i = blockIdx.x * PROG_BLOCK + threadIdx.x;
    if (i >= nitems) return;
    const JpegProgItem it = items[i];
    const JpegProgFileDev& D = files[it.file];
    const JpegProgScanDev S = D.scans[it.scan];
    const uint32_t* __restrict__ w = D.words + it.word0;
    const uint32_t st = jpeg_prog_item(D, S, [w](uint32_t k) { return w[k]; }, it.nbits, it.unit0, it.nunits);
    if (st) atomicOr(D.header + 1, st);
}

__global__ __launch_bounds__(64) void k_jpeg_prog_verdict(const JpegProgFileDev* __restrict__ files, uint32_t nfiles) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= nfiles || !files[i].verdict) return;
    for (int k = 0; k < 4; k++) files[i].verdict[k] = files[i].header[k];
}

}  // namespace

int launch_jpeg_prog(const JpegProgFileDev* files, unsigned nfiles, const JpegProgItem* items, const uint32_t* level_first, int nlevels,
                     hipStream_t s, hipEvent_t* marks, unsigned* launches) {
    if (launches) *launches = 0;
    if (nfiles == 0) return IMP_OK;
    hipLaunchKernelGGL(k_jpeg_prog_zero, dim3(ZERO_GRID_X, nfiles), dim3(ZERO_BLOCK), 0, s, files);
    if (marks) (void)hipEventRecord(marks[0], s);
    for (int l = 0; l < nlevels; l++) {
        const uint32_t n = level_first[l + 1] - level_first[l];
        if (n == 0) continue;
        hipLaunchKernelGGL(k_jpeg_prog_level, dim3((n + PROG_BLOCK - 1) / PROG_BLOCK), dim3(PROG_BLOCK), 0, s, files, items + level_first[l], n);
        if (launches) ++*launches;
    }
    hipLaunchKernelGGL(k_jpeg_prog_verdict, dim3((nfiles + 63) / 64), dim3(64), 0, s, files, nfiles);
    if (marks) (void)hipEventRecord(marks[1], s);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
