// imp_internal.h -- shared declarations of libimpgpu.so (not installed; the public ABI is include/impgpu.h).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/impgpu.h"

namespace imp {

// ---------------------------------------------------------------- images
}  // namespace imp

struct impgpu_image {
    uint8_t* d = nullptr;   // device pointer
    int w = 0, h = 0, c = 0, step = 0;
    size_t cap = 0;         // bytes owned (0 for borrowed views)
    bool owned = false;
    // an album (the frames of one animation, bridge.c:554-572): `frames` frames of this geometry in ONE block, frame i at
    // d + i * fstride, so that every operator of the request is one launch for the whole album.  1 / 0 for a single image.
    int frames = 1;
    size_t fstride = 0;
};

namespace imp {

// A read-only window into device memory: how Crop is folded into the next operator.
struct View {
    const uint8_t* d;
    int w, h, c, step;
};
inline View view_of(const impgpu_image* im) { return View{im->d, im->w, im->h, im->c, im->step}; }
inline View view_sub(const View& v, int x, int y, int w, int h) {
    return View{v.d + (size_t)y * v.step + (size_t)x * v.c, w, h, v.c, v.step};
}
inline int aligned_step(int w, int c) { return (w * c + 3) & ~3; }
// what the kernels' 32-bit pixel / byte indexing can address (see image_new)
inline bool frame_fits(int w, int h, int c) {
    const long long step = ((long long)w * c + 3) & ~3LL;
    return (long long)w * h <= (1LL << 30) && step * h <= 0xffffffffLL && step <= 0x7fffffffLL;
}
// A caller-described frame (batch entry points, impgpu_image_wrap): positive size, a pitch that holds a row, and everything
// the kernels compute in 32 bits -- pixel count, row offsets, byte offsets inside a frame -- in range.  64-bit arithmetic:
// `step < w * c` in int wraps for the sizes this is meant to refuse.
inline bool view_fits(long long w, long long h, int c, long long step) {
    return w > 0 && h > 0 && w <= 0x7fffffffLL && h <= 0x7fffffffLL && step >= w * c && step <= 0x7fffffffLL &&
           w * h <= (1LL << 30) && step * h <= 0xffffffffLL;
}

// The measurement sessions' environment switches, and the kernel variants and tuning values that only they selected, were
// removed once those variants lost their comparisons: each dispatch keeps the branch that won.  The numbers stay in
// profiles/ and in DESIGN.md section 5.

// ---------------------------------------------------------------- runtime (imp_runtime.hip)
void set_error(const char* what, hipError_t e);
void set_error_text(const char* what);             // impgpu_last_error() text for failures that are not HIP errors
bool env_ready();
int  need_env();                                   // IMP_OK, or IMP_ERROR_DEVICE and the error text of a call made before impgpu_env_start
hipStream_t env_stream();
int  dev_alloc(size_t bytes, void** out);          // stream-ordered pool; IMP_* code
void dev_free(void* p);
int  image_new(int w, int h, int c, impgpu_image** out);
int  image_new_album(int w, int h, int c, int frames, impgpu_image** out);
void image_delete(impgpu_image* im);
// Copy a small host blob (tables, taps) into pool memory through the pinned ring, ordered on `s`.
int  upload_small(const void* host, size_t bytes, void** dev, hipStream_t s);
int  upload_to(void* dev, const void* host, size_t bytes, hipStream_t s);   // the same copy into memory the caller holds
// Larger host-built blobs: fill the pinned buffer stage_begin returns, then stage_upload copies it to `dev` on the lane stream.
int  stage_begin(size_t bytes, void** host, void** token);
int  stage_upload(void* token, void* dev, size_t bytes);
void stage_hold(void* token, bool held);                   // a download enqueued into the buffer is read by a later call: keep it out of circulation until then
size_t stage_cap();                                       // $IMPGPU_STAGE_CAP_MB in bytes (0: none)
size_t stage_capacity(void* token);                     // bytes the buffer behind `token` really holds (>= what stage_begin was asked for)
int  stage_upload_part(void* token, size_t offset, void* dev, size_t bytes, bool last);   // pieces of the same buffer; `last` fences it
// Pool memory and caller-supplied ("foreign") streams -- the batch entry points.  The pool recycles blocks in the order
// of the lane's own stream; these keep that sound without a host wait:
void dev_free_on(void* p, hipStream_t s);                  // free once the work enqueued on `s` so far is done
int  dev_alloc_on(size_t bytes, void** out, hipStream_t s); // dev_alloc + make `s` wait for the lane stream's tail
int  stream_join(hipStream_t s);                           // `s` waits for everything the lane stream holds now
int  stream_join_back(hipStream_t s);                      // the lane stream waits for everything `s` holds now
bool lane_stream_idle();
uint32_t* lane_mailbox();                                  // pinned words of the calling thread's lane: [0, 1024) for any caller, then 1024 per JPEG group in flight
int  lane_mark(void** mark);                               // a point of the lane's stream ...
int  lane_mark_on(hipStream_t s, void** mark);             // ... or of another stream of the thread (nullptr: the lane's)
hipStream_t lane_side_stream();                            // the lane's second stream (made on first use; nullptr if it cannot be)
int  lane_wait_mark(void* mark);                           // ... to sleep until (nullptr: the whole stream)
int  lane_wait();                                          // wait for the lane's stream (sleeping, unless IMPGPU_SYNC=spin)
bool on_lane_stream(hipStream_t s);
// Per-lane caches (resize tables): owned by the lane, dropped with it (impgpu_env_destroy), no lock.
struct LaneCache { virtual ~LaneCache() {} };
constexpr int LANE_CACHE_SLOTS = 2;
LaneCache** lane_cache_slot(int which);
// rocTX ranges named after the reference's step codes (required.h:46-54) around each stage of a request, so a
// `rocprofv3 --marker-trace` timeline reads like JobResult.Step.  Resolved with dlopen at impgpu_env_start: no link-time
// dependency, nothing emitted unless a profiler's rocTX library is already in the process or IMPGPU_ROCTX=1.
void trace_push(const char* name);
void trace_pop();
struct TraceRange {
    explicit TraceRange(const char* name) { trace_push(name); }
    ~TraceRange() { trace_pop(); }
    TraceRange(const TraceRange&) = delete;
    TraceRange& operator=(const TraceRange&) = delete;
};
// Fault injection: impgpu_fault_arm(step, n) makes the n-th entry into that IMP_STEP_* behave as if its first
// HIP call had failed: IMP_ERROR_DEVICE, impgpu_last_error() says so, the failing step is reported like any other -- the
// path a lost device takes, testable without losing one.  Never armed from the environment.
bool fault_hit(int step);
#define IMP_FAULT_POINT(step)                                     \
    do {                                                          \
        if (imp::fault_hit(step)) return IMP_ERROR_DEVICE;        \
    } while (0)
// Kernels the calling thread has enqueued since it started (impgpu_batch_run_ops reports the difference): every launch
// site of the library goes through hipLaunchKernelGGL, which counts here before it launches.
extern thread_local unsigned long long t_launches;
#ifdef hipLaunchKernelGGL
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, ...)                              \
    do {                                                                  \
        ++imp::t_launches;                                                \
        hipLaunchKernelGGLInternal((kernelName), __VA_ARGS__);            \
    } while (0)
#endif
#define IMP_HIP(call)                                             \
    do {                                                          \
        hipError_t _e = (call);                                   \
        if (_e != hipSuccess) { imp::set_error(#call, _e); return IMP_ERROR_DEVICE; } \
    } while (0)

// ---------------------------------------------------------------- AlphaBlendOver on one BGRA pixel pair (filters.c:633-659)
// Shared by k_blend_over (imp_pixel.hip) and the fused resize + rotate + watermark kernel (imp_resize.hip): the float
// sequence of the reference, one operation per rounding (`alpha` = 1 - opacity, filters.c:620).
#ifdef __HIPCC__          // device code: the host-only builds of the grammar files (sanitizer tests) skip it
__device__ __forceinline__ uint32_t blend_over_bgra(uint32_t d, uint32_t s, float alpha) {
    const int dB = d & 0xff, dG = (d >> 8) & 0xff, dR = (d >> 16) & 0xff;
    const float dA = (float)((double)(d >> 24) / 255.0);
    const int sB = s & 0xff, sG = (s >> 8) & 0xff, sR = (s >> 16) & 0xff;
    float sA = (float)((double)(s >> 24) / 255.0);
    sA = (float)fmax((double)__fsub_rn(sA, alpha), 0.0);
    const float inv = __fsub_rn(1.f, sA);
    const float tA = __fadd_rn(sA, __fmul_rn(dA, inv));
    int tB = 0, tG = 0, tR = 0;
    if (tA != 0.f) {
        tB = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sB, sA), __fmul_rn(__fmul_rn((float)dB, dA), inv)), tA);
        tG = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sG, sA), __fmul_rn(__fmul_rn((float)dG, dA), inv)), tA);
        tR = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sR, sA), __fmul_rn(__fmul_rn((float)dR, dA), inv)), tA);
    }
    const float a255 = __fmul_rn(tA, 255.f);
    const int tAi = (a255 > -2147483904.f && a255 < 2147483648.f) ? (int)a255 : (int)0x80000000;
    return (uint32_t)(tB & 0xff) | ((uint32_t)(tG & 0xff) << 8) | ((uint32_t)(tR & 0xff) << 16) | ((uint32_t)(tAi & 0xff) << 24);
}
// The same on a 3-channel destination pixel (packed B | G << 8 | R << 16): its alpha is 1 (filters.c:636) and none is written.
__device__ __forceinline__ uint32_t blend_over_bgr(uint32_t d, uint32_t s, float alpha) {
    const int dB = d & 0xff, dG = (d >> 8) & 0xff, dR = (d >> 16) & 0xff;
    const float dA = 1.f;
    const int sB = s & 0xff, sG = (s >> 8) & 0xff, sR = (s >> 16) & 0xff;
    float sA = (float)((double)(s >> 24) / 255.0);
    sA = (float)fmax((double)__fsub_rn(sA, alpha), 0.0);
    const float inv = __fsub_rn(1.f, sA);
    const float tA = __fadd_rn(sA, __fmul_rn(dA, inv));
    int tB = 0, tG = 0, tR = 0;
    if (tA != 0.f) {
        tB = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sB, sA), __fmul_rn(__fmul_rn((float)dB, dA), inv)), tA);
        tG = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sG, sA), __fmul_rn(__fmul_rn((float)dG, dA), inv)), tA);
        tR = (int)__fdiv_rn(__fadd_rn(__fmul_rn((float)sR, sA), __fmul_rn(__fmul_rn((float)dR, dA), inv)), tA);
    }
    return (uint32_t)(tB & 0xff) | ((uint32_t)(tG & 0xff) << 8) | ((uint32_t)(tR & 0xff) << 16);
}
// BlendWithPaper on one BGRA pixel (filters.c:666-687): the colour over white by its alpha, alpha 255.  Shared by
// k_blend_paper (imp_pixel.hip) and the tail of the mixed resize launch (imp_resize.hip), so the two stay bit-identical.
__device__ __forceinline__ uint32_t blend_paper_bgra(uint32_t u) {
    const int a = u >> 24;
    const int diff = 255 - a;
    const float prod = (float)((double)a / 255.0);
    const int tb = (int)__fadd_rn((float)diff, __fmul_rn((float)(u & 0xff), prod));
    const int tg = (int)__fadd_rn((float)diff, __fmul_rn((float)((u >> 8) & 0xff), prod));
    const int tr = (int)__fadd_rn((float)diff, __fmul_rn((float)((u >> 16) & 0xff), prod));
    return (uint32_t)(tb & 0xff) | ((uint32_t)(tg & 0xff) << 8) | ((uint32_t)(tr & 0xff) << 16) | 0xff000000u;
}

// ---------------------------------------------------------------- a window row as a run of bytes (Crop's copy, bridge.c:130-135)
// Shared by k_copy_run (imp_geom.hip) and the bare items of k_window_mix (imp_pixel.hip).  Lane `k` of a row moves bytes
// [16k, 16k + 16) of the row's `n` (= w * channels; nothing here knows the channel count): four dwords out in one store, the
// source as the aligned dwords around them, shifted into place by (source & 3) with v_alignbyte.  A row's ragged end moves as
// dwords while four bytes are left, then bytewise.
// The aligned dword at `p`, reading no byte outside [lo, hi): a window of a BGR frame starts and ends at any byte, and what
// lies around it may be another row, pitch padding -- or, in a caller's wrapped buffer, nothing at all.
__device__ __forceinline__ uint32_t row_dword(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    if (p >= lo && p + 4 <= hi) return *(const uint32_t*)p;
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (p + b >= lo && p + b < hi) v |= (uint32_t)p[b] << (8 * b);
    return v;
}
typedef uint32_t row_u32x4 __attribute__((ext_vector_type(4), aligned(4)));   // four dwords at a dword-aligned address
__device__ __forceinline__ void copy_run16(const uint8_t* __restrict__ s, uint8_t* __restrict__ d, int n, int k) {
    const int o = 16 * k, left = n - o;
    if (left <= 0) return;
    const uint8_t* sa = s + o;
    uint8_t* da = d + o;
    if ((uintptr_t)d & 3) {                                 // a destination row off the dword grid: bytes.  Kept for safety only:
                                                            // both callers hand over dword-aligned destination rows (launch_copy
                                                            // sends the others to k_copy<1>, launch_window_mixed writes pool frames)
        const int m = left < 16 ? left : 16;
        for (int b = 0; b < m; b++) da[b] = sa[b];
        return;
    }
    const unsigned a = (unsigned)((uintptr_t)sa & 3);
    const uint8_t* base = sa - a;                           // (base + 4 .. base + 16 of a whole chunk lie inside the row)
    const uint8_t* hi = s + n;
    if (left >= 16) {
        row_u32x4 q;
        if (base >= s) q = *(const row_u32x4*)base;
        else {
            q.x = row_dword(base, s, hi);
            q.y = *(const uint32_t*)(base + 4); q.z = *(const uint32_t*)(base + 8); q.w = *(const uint32_t*)(base + 12);
        }
        if (a) {
            const uint32_t q4 = row_dword(base + 16, s, hi);
            q.x = __builtin_amdgcn_alignbyte(q.y, q.x, a);
            q.y = __builtin_amdgcn_alignbyte(q.z, q.y, a);
            q.z = __builtin_amdgcn_alignbyte(q.w, q.z, a);
            q.w = __builtin_amdgcn_alignbyte(q4, q.w, a);
        }
        *(row_u32x4*)da = q;
        return;
    }
    int b = 0;
    for (; b + 4 <= left; b += 4) {
        const uint32_t lo = row_dword(base + b, s, hi);
        *(uint32_t*)(da + b) = a ? __builtin_amdgcn_alignbyte(row_dword(base + b + 4, s, hi), lo, a) : lo;
    }
    for (; b < left; b++) da[b] = sa[b];
}
#endif

// ---------------------------------------------------------------- host grammar (imp_args.cpp)
int crop_geometry(int col, int row, const char* args, const char* gravity, int* x, int* y, int* w, int* h);
int resize_geometry(int col, int row, const char* args, unsigned max_w, unsigned max_h, int simple,
                    int* w, int* h, int* interp);

// One stage of the fused pointwise program (imp_pixel.hip runs them per pixel, in order,
// keeping the reference's per-stage 8-bit truncation).
enum StageKind : int {
    ST_LUT4 = 0,      // per-channel 256-entry tables, channels 0..3 (identity rows where unused)
    ST_RGB2HSV,       // helpers.c:70-107
    ST_HSV2RGB,       // helpers.c:109-176
    ST_GRADMAP,       // filters.c:264-276: 768-byte RGB table indexed by ((R+G+B)/3)*3
    ST_VIGNETTE,      // filters.c:312-317 on HSV value; params cx, cy, maxrad, power
    ST_RAINBOW,       // filters.c:368-398; param sat
    ST_SCANLINE,      // filters.c:434-451; params freq, width, s_byte, v_byte
};
struct Stage {
    int kind;
    int lut_off;      // byte offset into the program's table blob (LUT4: 1024 B, GRADMAP: 768 B)
    int i0, i1, i2, i3;
    float f0, f1;
};
struct PixelProgram {
    std::vector<Stage> stages;
    std::vector<uint8_t> tables;
    void clear() { stages.clear(); tables.clear(); }
    bool empty() const { return stages.empty(); }
};

// What one filter-* request turns into.
enum FilterClass : int { FC_POINTWISE = 0, FC_FLIP, FC_ROTATE, FC_BLUR, FC_NOOP };
struct FilterPlan {
    int cls = FC_NOOP;
    int flip_mode = 0;       // cvFlip mode: 0 vertical, 1 horizontal, -1 both
    int rotate = 0;          // 90 / 180 / 270
    float sigma = 0;         // blur
    // pointwise stages are appended to the caller's PixelProgram
};
// Parses "name=args" (filters.c:43-70 + the callback's own checks). For pointwise filters
// appends stages for an image of `channels` channels and w x h pixels to `prog`.
int filter_plan(const char* request, int allow_experiments, int channels, int w, int h,
                FilterPlan* plan, PixelProgram* prog);
int check_destructive(const char* request);

// ---------------------------------------------------------------- coefficient tables (imp_tables.cpp)
struct TapAxis {            // LINEAR / CUBIC / LANCZOS4: one axis of cv::resize's generic branch
    int ksize;
    std::vector<int> ofs;       // dsize entries: source index of the tap-window centre
    std::vector<short> coef;    // dsize * ksize fixed-point (11-bit) weights
};
void build_tap_axis(int ssize, int dsize, double scale, int interp, bool is_x, TapAxis* out);
struct AreaAxis {           // general INTER_AREA: per destination index a run of source indices
    std::vector<int> start;     // first source index of the run
    std::vector<int> count;     // run length
    std::vector<int> aoff;      // offset of the run's first weight in alpha
    std::vector<float> alpha;
    int max_count = 0;
};
void build_area_axis(int ssize, int dsize, double scale, AreaAxis* out);
int  area_max_count(int ssize, int dsize, double scale);          // AreaAxis::max_count alone
int  gaussian_ksize(double sigma);
void gaussian_kernel_fixed(int n, double sigma, std::vector<int>* ik);

// ---------------------------------------------------------------- launchers
struct Frames {             // `count` frames of one geometry
    const uint8_t* src; long long src_stride; View v;   // v.d == src (frame 0)
    uint8_t* dst; long long dst_stride; int dw, dh, dstep;
    int count;
};
// imp_resize.hip
int launch_cv_resize(const Frames& f, int interp, hipStream_t s);
// `count` frames of different geometry, each Resize()d by the reference's rule (BASELINE configs[4], device-resident)
struct MixFrame { const uint8_t* src; int sw, sh, sstep; uint8_t* dst; int dw, dh, dstep; };
int launch_resize_mixed(const MixFrame* frames, int count, int channels, int simple, hipStream_t s);
// exact-2x AREA + rotate 90/270 of BGRA in one pass; IMP_ERROR_UNSUPPORTED when the geometry does not qualify.
// With a 4-channel overlay the Watermark step (bridge.c:629-640) rides on the store phase of the same kernel.
struct OverlayArgs { const uint8_t* ov; int ostep, rx, ry, maxcol, maxrow; float alpha; };
int launch_area2x2_rotate(const Frames& f, int amount, const OverlayArgs* overlay, hipStream_t s);
// general INTER_AREA of BGRA frames + rotate 0/90/180/270 + watermark in one pass (f.dw x f.dh = the resized geometry,
// f.dst = the final frames); IMP_ERROR_UNSUPPORTED when the geometry takes another resize kernel.
int launch_area_rotate(const Frames& f, int amount, const OverlayArgs* overlay, hipStream_t s);
// Does launch_area_rotate take this resize (f.v -> f.dw x f.dh, f.count frames into f.dst)?  *w / *bh: its window and band
// height.  The one acceptance test of the fused resize tail, for the lone launch and the mixed one alike.
bool area_tail_plan(const Frames& f, int* w, int* bh);
// The mixed launch with a tail per frame: resize (general INTER_AREA) -> rotate 0/90/180/270 -> watermark -> flatten, frames
// of different geometry and one channel count in ONE launch.  Every item must pass area_tail_plan (IMP_ERROR_INVALID_ARGS
// otherwise, nothing launched).  `dw` x `dh` of an item is the resized geometry, `dst` the final (turned) frame.
struct TailItem { View v; uint8_t* dst; int dw, dh, dstep; int rot; bool has_wm; OverlayArgs wm; bool flatten; };
int launch_area_tail_mixed(const TailItem* items, int count, int channels, hipStream_t s);
// imp_geom.hip
int launch_copy(const Frames& f, hipStream_t s);                       // crop copy / clone (dw,dh = v.w,v.h)
int launch_flip(const Frames& f, int mode, hipStream_t s);             // cvFlip
int launch_rotate(const Frames& f, int amount, hipStream_t s);         // 90 / 270 (dw,dh = v.h,v.w), 180
int launch_gray2bgr(const Frames& f, hipStream_t s);
int launch_pack_fi(const View& v, int bpp, uint8_t* dst, int dpitch, hipStream_t s);   // IplToFI32/24: flip + repack
// The same for frames of different geometry, one source channel count and one bpp, in ONE launch (impgpu_batch_download_fi):
// frame `src` (w x h, rows sstep apart) into the bitmap `dst` of row pitch `dpitch`.
struct PackFiItem { const uint8_t* src; int w, h, sstep; uint8_t* dst; int dpitch; };
int launch_pack_fi_mixed(const PackFiItem* items, int count, int channels, int bpp, hipStream_t s);
struct GifPageDev { long long idx_off, pal_off; int w, h, pitch, left, top, dispose, key, pad; };   // offsets into one device blob
int launch_gif_compose(const uint8_t* blob, const GifPageDev* pages, uint8_t* const* outs, int npages, int cw, int ch,
                       int ostep, int destructive, int only, hipStream_t s);                 // LoadGIF's compositing loop
// The same for many files in ONE launch (impgpu_batch_gif_compose).  The upload is `bytes` of a pinned staging buffer
// (MixStaged, below): gif_mix_table_bytes(count) bytes left free in front for the descriptor table, then every item's
// GifPageDev[npages] at pages_off, its output pointers (one when only >= 0, else npages) at outs_off, and the palettes and
// index planes the pages' pal_off / idx_off name -- all offsets from the buffer's start.  Everything behind the table is on
// its way to staged.dev when this is called; the table goes last.  staged.dev is freed here whatever happens.
struct GifMixItem { size_t pages_off, outs_off; int npages, cw, ch, ostep, destructive, only; };
struct MixStaged;
size_t gif_mix_table_bytes(int count);
int launch_gif_compose_mixed(const GifMixItem* items, int count, const MixStaged& staged, size_t bytes, hipStream_t s);
// imp_pixel.hip
int launch_pixel_program(uint8_t* d, long long stride, int w, int h, int c, int step, int count,
                         const PixelProgram& prog, hipStream_t s);
int launch_blend_over(uint8_t* d, long long stride, int w, int h, int c, int step, int count,
                      const impgpu_image* overlay, int rx, int ry, int maxcol, int maxrow,
                      float alpha, hipStream_t s);
int launch_blend_paper(uint8_t* d, long long stride, int w, int h, int step, int count, hipStream_t s);
int launch_brightness(const View& v, float* host_result, hipStream_t s);
int launch_ascii(uint8_t* d, int w, int h, int c, int step, const uint8_t* table, int tablelen,
                 float factor, uint8_t* dev_out, hipStream_t s);
// the two of many frames at once (impgpu_batch_calc_perceived_brightness, impgpu_batch_ascii): launches per channel count,
// one wait, a verdict per frame in codes[]; the return value is IMP_OK unless the arguments are unusable
int launch_brightness_mixed(const View* views, int count, float* results, int* codes, hipStream_t s);
struct AsciiItem { uint8_t* d; int w, h, c, step; bool wide; unsigned char* out; };     // out: (w + 1) * h - 1 bytes of host memory
int launch_ascii_mixed(const AsciiItem* items, int count, int* codes, hipStream_t s);
// imp_blur.hip
int launch_gaussian(uint8_t* d, long long stride, int w, int h, int c, int step, int count,
                    double sigma, hipStream_t s);

// fused single-pass BGRA Gaussian, out of place; IMP_ERROR_UNSUPPORTED when it does not apply
int launch_gaussian_fused(const Frames& f, double sigma, hipStream_t s);

// ---------------------------------------------------------------- launches over frames of different geometry
// The descriptor tables of the mixed launches (k_resize_area_mix and the chain kernels of impgpu_batch_run_ops): every
// descriptor owns `nblk` consecutive workgroups of ONE frame (a workgroup never spans two), and the descriptors are dealt
// to the eight XCD lists (workgroup id mod 8 = XCD), heaviest first to the lightest list.  List g is [off[g], off[g + 1]).
struct MixIndex { int off[9]; };
// `desc(d)` names the part of a descriptor holding `first` and `nblk`, `cost(d)` its weight; `v` is consumed, *sorted_out
// holds the lists back to back, *most_out the workgroups of the longest list (the grid is 8 * most).
template <class D, class M, class C>
void mix_deal(std::vector<D>& v, M desc, C cost, std::vector<D>* sorted_out, MixIndex* ix_out, int* most_out) {
    std::vector<int> order(v.size());
    for (size_t i = 0; i < v.size(); i++) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cost(v[x]) > cost(v[y]); });
    std::vector<int> list[8];
    long long load[8] = {0};
    for (int i : order) {
        int g = 0;
        for (int k = 1; k < 8; k++)
            if (load[k] < load[g]) g = k;
        list[g].push_back(i);
        load[g] += cost(v[i]) + 4096;
    }
    std::vector<D>& sorted = *sorted_out;
    sorted.clear();
    sorted.reserve(v.size());
    MixIndex& ix = *ix_out;
    ix = MixIndex{};
    int most = 0;
    for (int g = 0; g < 8; g++) {
        ix.off[g] = (int)sorted.size();
        int first = 0;
        for (int i : list[g]) {
            D d = v[i];
            desc(d).first = first;
            first += desc(d).nblk;
            sorted.push_back(d);
        }
        most = first > most ? first : most;
    }
    ix.off[8] = (int)sorted.size();
    v.clear();
    *most_out = most;
}
// Where a blob that travels behind a table of `n` descriptors starts (mix_launch's `blob`).
template <class D>
constexpr size_t mix_blob_offset(size_t n) { return (n * sizeof(D) + 15) & ~size_t(15); }
#ifdef __HIPCC__
// One launch over the descriptors `v` (consumed; none: no launch): deal them (mix_deal), upload the table -- with `blob`
// behind it in the same allocation, at mix_blob_offset, when one is given -- let `launch(grid, table, ix)` issue the
// kernel on `s` over the grid of 8 * most workgroups, and free the table behind the launch.  The table is freed even
// when the launch failed, and the launch's error is the one reported: the rule every mixed launch shares, said here once.
// `whole`, for blobs of megabytes (the enlargements' tables): the blob with mix_blob_offset<D>(v.size()) bytes left free
// in front of it -- the table is written there and `whole` is what is uploaded, with no second host copy of the blob.
// `staged`, for blobs the caller builds in a pinned staging buffer (stage_begin) and sends piece by piece while it builds
// them (stage_upload_part into `dev`, its own pool block of the whole size): `host` is the buffer, with
// mix_blob_offset<D>(v.size()) bytes left free in front for the table, which is written there and sent as the LAST piece --
// the one that fences the buffer.  `dev` is freed behind the launch like any table, also when something failed.
struct MixStaged { void* host; void* token; void* dev; };
template <class D, class M, class C, class L>
int mix_launch(std::vector<D>& v, M desc, C cost, hipStream_t s, L launch, const std::vector<uint8_t>* blob = nullptr,
               std::vector<uint8_t>* whole = nullptr, const MixStaged* staged = nullptr) {
    if (v.empty()) return IMP_OK;
    std::vector<D> sorted;
    MixIndex ix{};
    int most = 0;
    mix_deal(v, desc, cost, &sorted, &ix, &most);
    void* table = nullptr;
    if (staged) {
        std::memcpy(staged->host, sorted.data(), sorted.size() * sizeof(D));
        int rc = stage_upload_part(staged->token, 0, staged->dev, sorted.size() * sizeof(D), true);
        if (!rc && !on_lane_stream(s)) rc = stream_join(s);
        if (rc) { dev_free(staged->dev); return rc; }
        table = staged->dev;
    } else if (whole) {
        if (whole->size() < mix_blob_offset<D>(sorted.size())) return IMP_ERROR_INVALID_ARGS;
        std::memcpy(whole->data(), sorted.data(), sorted.size() * sizeof(D));
        if (int rc = upload_small(whole->data(), whole->size(), &table, s)) return rc;
    } else if (blob) {
        const size_t dbytes = mix_blob_offset<D>(sorted.size());
        std::vector<uint8_t> both(dbytes + blob->size(), 0);
        std::memcpy(both.data(), sorted.data(), sorted.size() * sizeof(D));
        std::memcpy(both.data() + dbytes, blob->data(), blob->size());
        if (int rc = upload_small(both.data(), both.size(), &table, s)) return rc;
    } else if (int rc = upload_small(sorted.data(), sorted.size() * sizeof(D), &table, s)) {
        return rc;
    }
    launch(dim3((unsigned)most * 8), (const D*)table, ix);
    const hipError_t e = hipGetLastError();
    dev_free_on(table, s);
    IMP_HIP(e);
    return IMP_OK;
}
// the same for descriptors that hold `first` and `nblk` themselves
template <class D, class C, class L>
int mix_launch(std::vector<D>& v, C cost, hipStream_t s, L launch, const std::vector<uint8_t>* blob = nullptr,
               std::vector<uint8_t>* whole = nullptr, const MixStaged* staged = nullptr) {
    return mix_launch(v, [](D& d) -> D& { return d; }, cost, s, launch, blob, whole, staged);
}
// The descriptor of this workgroup (its index; -1: none, the workgroup returns) and the workgroup's index inside it;
// `desc(d)` names the part of a descriptor holding `first` and `nblk`, as in mix_deal.  An index rather than a pointer: the
// callers read the descriptor as d[i], which keeps its fields in scalar registers.
template <class D, class M>
__device__ __forceinline__ int mix_pick(const D* __restrict__ d, const MixIndex& ix, int* blk, M desc) {
    const int g = blockIdx.x & 7, q = blockIdx.x >> 3;
    int lo = ix.off[g], hi = ix.off[g + 1];
    if (lo == hi || q >= desc(d[hi - 1]).first + desc(d[hi - 1]).nblk) return -1;
    while (hi - lo > 1) {                              // last descriptor whose first block is <= q
        const int mid = (lo + hi) >> 1;
        if (desc(d[mid]).first <= q) lo = mid; else hi = mid;
    }
    *blk = q - desc(d[lo]).first;
    return lo;
}
template <class D>
__device__ __forceinline__ int mix_pick(const D* __restrict__ d, const MixIndex& ix, int* blk) {
    return mix_pick(d, ix, blk, [](const D& x) -> const D& { return x; });
}
#endif

// imp_gif.hip: the LZW pages of a call's GIF files, one wavefront per page (impgpu_batch_decode_gif).  A descriptor per
// page, dealt like every mixed launch's (mix_deal; nblk is 1); the table lies INSIDE the call's device block at `table_off`,
// and data_off / plane_off count from that block's start: the compressed bytes (the sub-block payloads, concatenated) and
// the page's index plane, which the kernel writes whole, pad bytes included.  status[slot] gets the page's verdict
// (imp_gif.h: GIF_LZW_*).
struct GifLzwDesc {
    long long data_off, plane_off;
    uint32_t data_bytes;
    int w, h, pitch, mcs, interlaced, slot;
    int first, nblk;
};
int launch_gif_lzw(uint8_t* blob, size_t table_off, const MixIndex& ix, int most, uint32_t* status, hipStream_t s);
// IMPGPU_GIF_SPLIT: the same pages cut at their clear codes, three launches (k_gif_lzw_scan, one wavefront per page over
// the same dealt table; k_gif_lzw_len and k_gif_lzw_emit, one wavefront per segment SLOT).  Beside the table, in the same
// block: GifSplitPage[pages] at `split_off`, entry i belonging to descriptor i of the dealt table -- where the page's
// segment block lies (GifSeg[cap + 1], imp_gif.h; device-written, behind the planes) -- and GifSegSlot[nslots] at
// `slots_off`: workgroup b of the slot launches works on segment k of page `page` (an index into the dealt table), every
// page owning cap consecutive slots, of which those at or past the count the scan found return at once.
struct GifSplitPage { long long seg_off; uint32_t cap, pad; };
struct GifSegSlot { int page, k; };
int launch_gif_lzw_split(uint8_t* blob, size_t table_off, size_t split_off, size_t slots_off, const MixIndex& ix, int most, long long nslots,
                         uint32_t* status, hipStream_t s);

// imp_gif_enc.hip: the albums of a call into GIF streams (impgpu_batch_encode_gif): k_gif_enc_sets and k_gif_enc_index over
// `npx` pixel items, k_gif_enc_tables over the albums, k_gif_enc_lzw over `nseg` segment items, k_gif_enc_pack over `npack`
// items; the descriptors (imp_gif_enc.h) lie in the call's device block.  With D.flags & IMPGPU_GIF_ENC_QUANTIZE three more run
// behind the sets (k_gif_enc_claim, k_gif_enc_hist over `npx`, k_gif_enc_cut over D.nslots): eight launches instead of five.
struct GifEncDev;
int launch_gif_encode(const GifEncDev& D, long long npx, long long nseg, long long npack, int nalbums, hipStream_t s);

// imp_webp_enc.hip: the frames of a call into lossless WebP files (impgpu_batch_encode_webp): k_webp_modes over `ntile_items`
// groups of four tiles, k_webp_codes and k_webp_scan over the frames, k_webp_resid, _measure and _emit over `nitems` stream
// items; the descriptors (imp_webp_enc.h) lie in the call's device block.  Six launches; seven with D.lz (k_webp_parse).
struct WebpDev;
int launch_webp_encode(const WebpDev& D, long long ntile_items, long long nitems, int nframes, hipStream_t s);

// imp_png_inflate.hip: the zlib streams of a call's PNG files, one workgroup of one wavefront per stream (impgpu_batch_decode_png_ex
// with IMPGPU_PNG_DEVICE_INFLATE).  `descs` (imp_png.h) lie in device memory; descriptor k is workgroup k's.
struct PngInflateDesc;
int launch_png_inflate(const PngInflateDesc* descs, int count, hipStream_t s);

// The chain kernels of impgpu_batch_run_ops: one launch per channel count over frames of different geometry.
// imp_pixel.hip: a run of pointwise stages [-> watermark] [-> flatten] on a frame in place.  `prog` must fit one
// k_pixel_program launch (split_program); an overlay of 3 or 4 channels.
struct PixelTailItem {
    uint8_t* d; int w, h, step;
    const PixelProgram* prog;            // may be empty
    bool has_wm; const impgpu_image* ov; int rx, ry, maxcol, maxrow; float alpha;
    bool flatten;
};
int launch_pixel_tail_mixed(const PixelTailItem* items, int count, int channels, hipStream_t s);
// imp_pixel.hip: the same pass out of place, from a window of a larger frame (a View after view_sub: any byte address for
// BGR; BGRA windows are dword aligned) into a fresh frame of the window's size -- how a request WITHOUT a resize leaves its
// crop.  `t.d`, `t.step` name the destination, `t.w` x `t.h` both.  An item with no program, no overlay and no flatten is
// the bare crop: its rows move as runs of bytes (copy_run16).  One launch per channel count and vignette group, as above.
struct WindowItem { const uint8_t* src; int sstep; PixelTailItem t; };
int launch_window_mixed(const WindowItem* items, int count, int channels, hipStream_t s);
// A program past one launch's stage / table limits, cut where launch_pixel_program cuts it (exact anywhere: every stage
// already rounds to 8 bits per channel).  One part when it fits.
void split_program(const PixelProgram& prog, std::vector<PixelProgram>* parts);
// imp_geom.hip: cvFlip (kind 0, mode = flip mode) or a quarter / half turn (kind 1, mode = 90 / 180 / 270) into a fresh frame
struct GeomItem { const uint8_t* src; int sw, sh, sstep; uint8_t* dst; int dw, dh, dstep; int kind, mode; };
int launch_geom_mixed(const GeomItem* items, int count, int channels, hipStream_t s);
// imp_geom.hip: cvCvtColor(GRAY2BGR) of many gray frames into fresh 3-channel frames of the same size, ONE launch
struct Gray2BgrItem { const uint8_t* src; uint8_t* dst; int w, h, sstep, dstep; };
int launch_gray2bgr_mixed(const Gray2BgrItem* items, int count, hipStream_t s);
// imp_blur.hip: which form launch_gaussian_fused gives a frame of this geometry and sigma -- BLUR_MIXABLE when it is one of
// the one-pass forms k_blur_mix takes (k_blur_fused4, k_blur_mfma_fused), BLUR_MIXABLE_PAIR for the two-pass matrix-unit form
// (k_blur_mfma_rows + k_blur_mfma_cols), which k_blur_rows_mix + k_blur_cols_mix take, BLUR_LONE for the others.  `aligned`:
// the dword alignment launch_gaussian_fused asks of BGRA pointers and steps holds.  *planes (may be NULL): the byte planes of
// a matrix-unit form's row sums, 2 or 3 (0 for the other forms) -- frames of different plane counts never share a launch.
// *kernel (may be NULL): impgpu_blur_form's code.
enum { BLUR_LONE = 0, BLUR_MIXABLE = 1, BLUR_MIXABLE_PAIR = 2 };
int blur_form(int w, int h, int c, bool aligned, double sigma, int* planes = nullptr, int* kernel = nullptr);
struct BlurItem { const uint8_t* src; uint8_t* dst; int w, h, sstep, dstep; double sigma; };   // out of place, same geometry
// every item must be BLUR_MIXABLE or BLUR_MIXABLE_PAIR (IMP_ERROR_INVALID_ARGS otherwise, nothing launched): one launch per
// one-pass form and plane count, one launch pair per plane count of the two-pass form
int launch_blur_mixed(const BlurItem* items, int count, int channels, hipStream_t s);

// Watermark placement (bridge.c:254-274 + cvSetImageROI clipping). Returns IMP_* code.
int watermark_rect(int basew, int baseh, int overw, int overh, const impgpu_config* cfg,
                   int* rx, int* ry, int* maxcol, int* maxrow);


// The dynamic-LDS limit of a kernel is a per-function, process-wide attribute: raised ONCE per kernel instantiation (a
// thread-safe static) to everything the device allows beside the kernel's static LDS -- not before every launch with that
// launch's own size, where two request threads with different sizes could interleave set(small) between another thread's
// set(large) and its launch, and every request paid a runtime call for a value that never changes (round 4's review).
#if defined(__HIPCC__)
template <auto Kernel>
inline hipError_t lds_limit_once() {
    static const hipError_t err = [] {
        int dev = 0, cap = 0;
        hipFuncAttributes fa;
        hipError_t e = hipGetDevice(&dev);
        if (e == hipSuccess) e = hipDeviceGetAttribute(&cap, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
        if (e == hipSuccess) e = hipFuncGetAttributes(&fa, (const void*)Kernel);
        if (e != hipSuccess) return e;
        const int room = cap - (int)fa.sharedSizeBytes;
        return hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, room > 0 ? room : 0);
    }();
    return err;
}
#endif
}  // namespace imp
