// imp_resize.hip -- cvResize (reference call site bridge.c:189-191) as gfx950 kernels.
//
// OpenCV 2.4.9 semantics for CV_8U, 1/3/4 interleaved channels (imgwarp.cpp), x86-64 build:
//   NN        nearest source index  min(floor(d * scale), size-1)
//   LINEAR    2 taps,  11-bit fixed-point weights, VResizeLinear's >>4 / >>16 / +2 >>2
//   CUBIC     4 taps,  11-bit weights; vertical pass in float (VResizeCubicVec_32s8u) for the
//             first (dw*cn & ~7) elements of a row, (v + 2^21) >> 22 for the rest
//   LANCZOS4  8 taps,  (v + 2^21) >> 22
//   AREA      integer scales: box sum ((a+b+c+d+2)>>2 for 2x2, else round(sum * 1.f/area));
//             otherwise float accumulation over per-axis (source run, weight) tables
//
// All of these are HBM-bound byte shuffles (no contraction, no MFMA).  Layout: one thread
// per destination pixel, 256-thread blocks over the flattened (dy, dx) index so a wave's 64
// lanes walk 64 neighbouring dx of one destination row: their tap windows fall in the same
// few source rows and every 64-byte sector a wave touches is consumed by neighbouring lanes
// of the same instruction.  blockIdx.y is the frame of the batch.  For BGRA the KS taps of a
// row are one (4-byte aligned) 8/16/32-byte vector load per lane.  The per-geometry weight
// tables (a few KB, built on the host in imp_tables.cpp) stay L1/L2 resident.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <map>
#include <set>
#include <mutex>
#include <tuple>
#include <type_traits>
#include "imp_internal.h"

namespace imp {

struct RArgs {
    const uint8_t* src; long long src_stride; int sstep, sw, sh;
    uint8_t* dst; long long dst_stride; int dstep, dw, dh;
};

template <int N, int I = 0, typename F>
__device__ __forceinline__ void static_for(F&& f) {           // f(integral_constant<int, I>) for I = 0..N-1
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<N, I + 1>(f);
    }
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int sat_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// clamp(v >> sh) for the fixed-point casts.  The empty asm keeps the shift and the clamp apart:
// hipcc 7.2 otherwise fuses two of them plus the byte packing into v_ashr_pk_u8_i32, and on
// MI355X that instruction leaves bits 31:16 of its destination unchanged while the compiler
// assumes they are zero (seen as garbage OR-ed into channels 2 and 3 of the Lanczos output).
__device__ __forceinline__ int shr_sat_u8(int v, int sh) {
    int t = v >> sh;
    asm volatile("" : "+v"(t));
    return sat_u8(t);
}

typedef short short2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ short2_t as_short2(uint32_t v) {
    short2_t r;
    __builtin_memcpy(&r, &v, 4);
    return r;
}

// Source frames are read once per launch and are far larger than L2 / Infinity Cache: load them
// with the non-temporal hint so they do not displace the tables and the neighbours' lines
// (measured +5.7 % on the cubic headline).  The hardware takes any 4-byte aligned address.
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4), aligned(4)));
typedef unsigned int u32x2_t __attribute__((ext_vector_type(2), aligned(4)));
template <int N>
__device__ __forceinline__ void load_stream(uint32_t* dst, const uint8_t* p) {
    static_assert(N % 2 == 0, "even dword counts only");
#pragma unroll
    for (int i = 0; i + 4 <= N; i += 4) {
        const u32x4_t q = __builtin_nontemporal_load((const u32x4_t*)(p + i * 4));
        dst[i] = q.x; dst[i + 1] = q.y; dst[i + 2] = q.z; dst[i + 3] = q.w;
    }
    if (N % 4) {
        const u32x2_t q = __builtin_nontemporal_load((const u32x2_t*)(p + (N - 2) * 4));
        dst[N - 2] = q.x; dst[N - 1] = q.y;
    }
}

// ------------------------------------------------------------------ LINEAR / CUBIC / LANCZOS4
enum { M_LINEAR = 0, M_CUBIC = 1, M_LANCZOS = 2 };

// N dwords starting at an arbitrary byte address, as 4-byte ALIGNED vector loads plus v_alignbyte_b32: a byte-
// misaligned dwordx3/x4 is split by the texture addresser and measured 34 % slower in the BGR AREA kernel.  The one
// extra dword is fetched only when it shares an aligned word with wanted bytes (shift != 0), so the read never
// leaves the word -- and therefore the page -- the last wanted byte lives in.
template <int N>
__device__ __forceinline__ void load_bytes_aligned(uint32_t* w, const uint8_t* p) {
    const unsigned sh = (unsigned)(uintptr_t)p & 3u;
    const uint32_t* a = (const uint32_t*)(p - sh);
    uint32_t t[N + 1];
    __builtin_memcpy(t, __builtin_assume_aligned(a, 4), N * 4);
    t[N] = a[sh ? N : N - 1];
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], sh);
}

template <int KS, int CN, int MODE>
__global__ __launch_bounds__(256) void k_resize_taps(RArgs a, const int* __restrict__ xofs,
                                                     const short* __restrict__ xco,
                                                     const int* __restrict__ yofs,
                                                     const short* __restrict__ yco, int vec_end) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (64-bit: a 2^30-pixel frame times a block size)
    if (idx >= (long long)a.dw * a.dh) return;
    const int dy = (int)(idx / a.dw), dx = (int)(idx - (long long)dy * a.dw);
    const uint8_t* S = a.src + (long long)blockIdx.y * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)dy * a.dstep + (size_t)dx * CN;

    const int sx0 = xofs[dx] - (KS / 2 - 1);
    const int sy0 = yofs[dy] - (KS / 2 - 1);
    int ax[KS], by[KS];
#pragma unroll
    for (int k = 0; k < KS; k++) { ax[k] = xco[dx * KS + k]; by[k] = yco[dy * KS + k]; }

    int hs[KS][CN];     // horizontal pass, one int32 per tap row and channel
    const bool interior = sx0 >= 0 && sx0 + KS <= a.sw;
    if (CN == 4 && interior) {
        uint32_t px[KS][KS];
#pragma unroll
        for (int r = 0; r < KS; r++) {
            const int sy = clampi(sy0 + r, 0, a.sh - 1);
            const uint8_t* row = S + (size_t)sy * a.sstep + (size_t)sx0 * 4;
            load_stream<KS>(px[r], row);
        }
#pragma unroll
        for (int r = 0; r < KS; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) {
                int v = 0;
#pragma unroll
                for (int k = 0; k < KS; k++) v += (int)((px[r][k] >> (8 * c)) & 0xff) * ax[k];
                hs[r][c] = v;
            }
    } else if (CN == 3 && interior && (KS * 3) % 4 == 0) {
        // BGR (every JPEG): the KS taps of a row are KS*3 contiguous bytes at a byte-aligned address -- one unaligned
        // dwordx3 (cubic) or two (lanczos) instead of KS*3 byte loads; tap k, channel c sits at the fixed byte 3k + c
        uint32_t w[KS][KS * 3 / 4];
#pragma unroll
        for (int r = 0; r < KS; r++) {
            const int sy = clampi(sy0 + r, 0, a.sh - 1);
            __builtin_memcpy(w[r], S + (size_t)sy * a.sstep + (size_t)sx0 * 3, KS * 3);   // (aligned + v_alignbyte measured 15 % slower here: one more dword of traffic)
        }
#pragma unroll
        for (int r = 0; r < KS; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                int v = 0;
#pragma unroll
                for (int k = 0; k < KS; k++) {
                    const int o = 3 * k + c;
                    v += (int)((w[r][o >> 2] >> (8 * (o & 3))) & 0xff) * ax[k];
                }
                hs[r][c < CN ? c : 0] = v;
            }
    } else {
        int sxk[KS];
#pragma unroll
        for (int k = 0; k < KS; k++) sxk[k] = clampi(sx0 + k, 0, a.sw - 1) * CN;
#pragma unroll
        for (int r = 0; r < KS; r++) {
            const int sy = clampi(sy0 + r, 0, a.sh - 1);
            const uint8_t* row = S + (size_t)sy * a.sstep;
#pragma unroll
            for (int c = 0; c < CN; c++) {
                int v = 0;
#pragma unroll
                for (int k = 0; k < KS; k++) v += (int)row[sxk[k] + c] * ax[k];
                hs[r][c] = v;
            }
        }
    }

    int out[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) {
        if constexpr (MODE == M_LINEAR) {
            out[c] = (uint8_t)((((by[0] * (hs[0][c] >> 4)) >> 16) + ((by[1] * (hs[1][c] >> 4)) >> 16) + 2) >> 2);
        } else if constexpr (MODE == M_CUBIC) {
            if (dx * CN + c < vec_end) {
                const float sc = 1.f / (2048.f * 2048.f);
                float s = __fmul_rn(__int2float_rn(hs[0][c]), __fmul_rn((float)by[0], sc));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hs[1][c]), __fmul_rn((float)by[1], sc)));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hs[2][c]), __fmul_rn((float)by[2], sc)));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hs[3][c]), __fmul_rn((float)by[3], sc)));
                out[c] = sat_u8(__float2int_rn(s));
            } else {
                int v = __mul24(hs[0][c], by[0]) + __mul24(hs[1][c], by[1]) + __mul24(hs[2][c], by[2]) + __mul24(hs[3][c], by[3]);
                out[c] = shr_sat_u8(v + (1 << 21), 22);
            }
        } else {
            uint32_t v = 0;     // int32 wrap-around like the CPU build
#pragma unroll
            for (int k = 0; k < KS; k++) v += (uint32_t)__mul24(hs[k][c], by[k]);   // |hs| < 2^23 (weights <= 2048 each)
            out[c] = shr_sat_u8((int)(v + (1u << 21)), 22);
        }
    }
    if (CN == 4) {
        *(uint32_t*)D = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    } else {
#pragma unroll
        for (int c = 0; c < CN; c++) D[c] = (uint8_t)out[c];
    }
}

// Frame-per-XCD block order for kernels whose neighbouring blocks re-read the same source rows
// (AREA: consecutive destination rows share their boundary source row).  Blocks are dealt to the
// 8 XCDs round-robin, so linear id mod 8 labels an XCD group; here a group works through whole
// frames, so the shared rows are found in that XCD's L2 instead of being pulled from HBM twice.
// Speed only.  Returns false for the padding blocks of an incomplete last group of 8 frames.
__device__ __forceinline__ bool frame_block(int bpf, int count, int* frame, int* blk) {
    const long long lin = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const int g = (int)(lin & 7);
    const long long q = lin >> 3;
    const int f = (int)(q / bpf) * 8 + g;
    *frame = f;
    *blk = (int)(q % bpf);
    return f < count;
}

// ------------------------------------------------------------------ exact 2x decimation, register-rolling
// When both scale factors are exactly 2 (4K -> 1080p, cfg4) the tap window of consecutive destination
// rows advances by exactly two source rows.  A lane then owns one destination column and walks down a
// strip of rows keeping the horizontal-pass results of its last KS source rows in a register ring: each
// new destination row costs two horizontal passes (two wide loads each in this form) and one vertical
// pass -- no LDS, no barriers, no halo recomputation except KS-2 rows at the top of a strip.  The ring
// advances by two slots per row, so unrolling KS/2 rows makes every ring index a compile-time constant.
// Weights still come from the per-geometry tables (nothing about their values is assumed); the host
// only checks that the tap offsets are the arithmetic progressions 2*d + const.
#define ROLL_STRIP 60      // destination rows per wave strip (a multiple of the ring period KS/2 = 1, 2, 4)

// History (cfg4, 64 frames): this register form ran 0.96 ms; double-buffered and 4-deep register prefetch of the
// windows measured the same (fewer waves), and copying each row segment through VGPRs into a wave-private LDS row was
// slower (1.04-1.07 ms).  What it lacked was bytes in flight, which the asynchronous LDS-DMA ring of
// k_resize_2x_dma below supplies without registers (0.62-0.69 ms); this form remains for pitches the DMA cannot take.
// Instruction rates (tools/valu_rate2.hip): v_perm_b32 and v_dot2c_i32_i16 issue at half the rate of v_mul_f32, like
// every other integer-multiply form, so the perm + dot2 pair is the cheapest exact H pass gfx950 offers.
template <int KS>
__device__ __forceinline__ void hpass_row(const uint8_t* row, int sxv, const int* sxk, bool interior,
                                          const short2_t* axp, int* h) {
    uint32_t p[KS];
    // temporal loads: the two 16-byte halves of a window, the neighbouring lanes' windows and the next wave's
    // share these lines, so they must stay cached (with the non-temporal hint PMC showed every line fetched 1.5x)
    __builtin_memcpy(p, __builtin_assume_aligned(row + sxv, 4), KS * 4);
#pragma unroll
    for (int k = 0; k < KS; k++) asm volatile("" : "+v"(p[k]));     // opaque: keeps the wide load (a guarded wide load next to a per-tap fallback is otherwise folded into dword loads)
    if (!interior) {
#pragma unroll
        for (int k = 0; k < KS; k++) p[k] = *(const uint32_t*)(row + sxk[k]);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int acc = 0;
#pragma unroll
        for (int j = 0; j < KS / 2; j++) {
            const uint32_t pr = __builtin_amdgcn_perm(p[2 * j + 1], p[2 * j], 0x0c040c00u + (c << 16) + c);
            acc = __builtin_amdgcn_sdot2(as_short2(pr), axp[j], acc, false);
        }
        h[c] = acc;
    }
}

// horizontal pass of one window held in registers: v_perm_b32 gathers channel c of two taps, v_dot2c multiplies
template <int KS>
__device__ __forceinline__ void hpass_px(const uint32_t* p, const short2_t* axp, int* h) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int acc;
#pragma unroll
        for (int j = 0; j < KS / 2; j++) {
            const uint32_t pr = __builtin_amdgcn_perm(p[2 * j + 1], p[2 * j], 0x0c040c00u + (c << 16) + c);
            // the chain starts from a literal 0 in the three-operand form: the two-operand v_dot2c the compiler picks
            // needs its accumulator zeroed by a v_mov first
            if (j == 0) asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(acc) : "v"(pr), "v"(axp[0]));
            else acc = __builtin_amdgcn_sdot2(as_short2(pr), axp[j], acc, false);
        }
        h[c] = acc;
    }
}

// ------------------------------------------------------------------ CUBIC enlargement (the reference's only CUBIC dispatch)
// Resize() asks for CV_INTER_CUBIC exactly when an axis grows (bridge.c:190).  Enlarging, the destination is the big side:
// 1920x1080 from 480x270 writes 16 bytes for every byte it reads, every source row feeds ~4 / scale destination rows, and
// instructions per destination pixel -- then the store stream -- set the pace, not the reads.
//
// A WAVE owns 64 destination columns and walks a chunk of rows down the frame, alone: no LDS, no barriers, nothing
// shared with the other waves of its block (an earlier block-wide form with the H sums in an LDS ring stalled every tile
// on its global loads -- table rows, source rows -- behind two barriers: 0.25 of the roofline).  All lanes of a wave
// work on the same destination row, so the row's four footprint rows are wave-uniform and the horizontal sums of the
// current footprint live in REGISTERS (four rows x four channels, already converted to float: exact, |sum| < 2^24, and
// VResizeCubicVec_32s8u's vertical pass is float).  When the footprint advances -- every 1/scale_y rows -- the ring
// shifts by one row and ONE new source row is reduced (one 16-byte window per lane, perm + dot2), its pixels having
// been requested one advance earlier.  The vertical pass is then four packed multiplies and three packed adds per
// channel pair with the row's weights in scalar registers: a row's constants (first footprint row, the four weights as
// the floats b * 2^-22, tabulated on the host) are wave-uniform, so they come by scalar loads, the next row's in flight;
// v_cvt_pk_u8_f32 rounds to nearest even, saturates and packs in one instruction per channel.
typedef float float2v_t __attribute__((ext_vector_type(2)));
#define UP_ROWS 128        // destination rows per wave chunk, at most
#define UP_CAP_PX 1536     // source pixels a wave stages in LDS (6 KB per wave, 28 KB per block with the store patch)

__device__ __forceinline__ uint32_t cvt_pk_u8(float x, uint32_t acc, int byte) {
    // v_cvt_pk_u8_f32: byte `byte` of acc <- saturate_u8(round-half-even(x)) -- exactly saturate_cast<uchar>(cvRound(x))
    // (checked on hardware over ties, negatives and > 255: tools/cvt_probe.hip)
    uint32_t r;
    asm("v_cvt_pk_u8_f32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(byte), "v"(acc));
    return r;
}

// per destination row, 32 bytes: how far the footprint moves before this row, then the four weights b * 2^-22
struct UpRow { int adv; float bf[4]; int first; int pad[2]; };      // first = first footprint row (yofs - 1); adv = first - previous row's first

// The body of one workgroup, shared by the lone kernel (k_resize_up_cubic4: launch arguments) and the mixed launch
// (k_resize_up_cubic_mix<4>: a descriptor per frame).  `frame` = the frame of a uniform batch (a descriptor: 0, strides 0),
// `blk` = the workgroup's index inside its frame; GLOBAL: the frame's pointers were read from memory (a descriptor), where
// the compiler takes them for generic ones -- said to be global, the body's loads and stores are global_* as in the lone
// kernels (a flat_store counts against the LDS counter too: the row loop would wait for its stores at every LDS read).
// The LDS patches are declared HERE, not handed in: indexed through a pointer parameter the reads lose
// their address space (see `fetch`); a kernel that calls the body owns one copy of each.
template <bool GLOBAL, class T>
__device__ __forceinline__ auto up_mem(T* p) {
    if constexpr (GLOBAL) return (__attribute__((address_space(1))) T*)p;
    else return p;
}

template <int PS, bool GLOBAL>     // PS = 2, 3, 4: scale_y is exactly 1/PS (host-checked: every PS-th row advances the footprint); 0: anything
__device__ __forceinline__ void up_cubic4_body(const RArgs& a, unsigned frame, unsigned blk,
                                               const int* __restrict__ xofs, const short* __restrict__ xco,
                                               const short* __restrict__ yco, const UpRow* __restrict__ rows,
                                               int vec_end, int nbx, int rows_per_wave) {
    // a wave's own 4 rows x 64 pixels, used only to turn four row-wise dword results per lane into one 16-byte store per lane
    __shared__ __attribute__((aligned(16))) uint32_t s_tr[4][4][64];
    __shared__ __attribute__((aligned(16))) uint32_t s_src[4][UP_CAP_PX];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cy = blk / nbx, bx = blk - cy * nbx;
    const int tx0 = (bx * 4 + wv) * 64;
    if (tx0 >= a.dw) return;                                   // waves are independent: no barrier follows
    const int txn = min(64, a.dw - tx0);
    const bool live = lane < txn;
    const int dx = tx0 + min(lane, txn - 1);                   // idle lanes of a partial strip shadow its last column
    const int row0 = cy * rows_per_wave, row_end = min(a.dh, row0 + rows_per_wave);
    const auto* S = up_mem<GLOBAL>(a.src) + (long long)frame * a.src_stride;
    auto* D = up_mem<GLOBAL>(a.dst) + (long long)frame * a.dst_stride;        // wave-uniform base; lanes add a 32-bit offset

    short2_t axp[2];
    axp[0].x = xco[dx * 4]; axp[0].y = xco[dx * 4 + 1]; axp[1].x = xco[dx * 4 + 2]; axp[1].y = xco[dx * 4 + 3];

    // The source pixels this wave will ever touch -- its strip's columns x its chunk's footprint rows, a few KB because an
    // enlargement re-reads every source pixel many times -- are copied into the wave's own LDS patch ONCE, already
    // replicated at the image borders (clamped row and column indices), before the row loop starts.  The steady state
    // then holds no global load at all.  That matters more than the bytes: loads and stores share one counter (vmcnt),
    // so a wave that waits for a prefetched window also waits for every store it has issued since, i.e. for the full
    // HBM write latency once per footprint advance.
    const int sxmin = __builtin_amdgcn_readfirstlane(xofs[tx0]) - 1;
    const int W = __builtin_amdgcn_readfirstlane(xofs[tx0 + txn - 1]) + 2 - sxmin + 1;        // strip's source columns
    const int f0 = rows[row0].first;
    const int NR = rows[row_end - 1].first + 3 - f0 + 1;                                         // chunk's footprint rows
    if (NR * W > UP_CAP_PX) return;        // cannot happen: the launcher sizes chunks from the same bounds; keeps LDS sound
    for (int i = lane; i < NR * W; i += 64) {
        const int r = i / W, c = i - r * W;
        s_src[wv][i] = *(const uint32_t*)(S + (size_t)clampi(f0 + r, 0, a.sh - 1) * a.sstep + (size_t)clampi(sxmin + c, 0, a.sw - 1) * 4);
    }
    const int lx = xofs[dx] - 1 - sxmin;                       // this lane's window start inside a patch row
    const int last = f0 + NR - 1;
    // (indexed through s_src itself: a pointer variable here loses its LDS address space and the reads become flat_load)
    auto fetch = [&](int vy, uint32_t* p) {                    // the 4-pixel window of footprint row vy
        const int o = (min(vy, last) - f0) * W + lx;
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = s_src[wv][o + k];
    };

    float2v_t hxy[4], hzw[4];                                  // H sums of footprint rows cur .. cur + 3, channel pairs (B,G) (R,A)
    uint32_t pn[4];                                            // pixels of footprint row cur + 4, requested one advance early
    int cur = f0 - 4;
    fetch(cur + 4, pn);
#pragma unroll
    for (int k = 0; k < 4; k++) { hxy[k] = float2v_t{0.f, 0.f}; hzw[k] = float2v_t{0.f, 0.f}; }

    auto advance = [&]() {                                     // the footprint moves down one source row
        int h[4];
        // perm + dot2 like hpass_px, written with the builtin only: with hpass_px's inline-asm first dot2 hipcc 7.2
        // allocated a perm's destination on top of its own source pixel inside this kernel's unrolled row loop
        // (v_perm_b32 v2, v3, v2, ... followed by a second perm reading v2), i.e. wrong sums for every tap but one
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const uint32_t sel = 0x0c040c00u + ((uint32_t)c << 16) + (uint32_t)c;
            int acc = __builtin_amdgcn_sdot2(as_short2(__builtin_amdgcn_perm(pn[1], pn[0], sel)), axp[0], 0, false);
            h[c] = __builtin_amdgcn_sdot2(as_short2(__builtin_amdgcn_perm(pn[3], pn[2], sel)), axp[1], acc, false);
        }
        cur++;
        fetch(cur + 4, pn);                                    // needed at the NEXT advance
        hxy[0] = hxy[1]; hxy[1] = hxy[2]; hxy[2] = hxy[3];
        hzw[0] = hzw[1]; hzw[1] = hzw[2]; hzw[2] = hzw[3];
        hxy[3] = float2v_t{__int2float_rn(h[0]), __int2float_rn(h[1])};
        hzw[3] = float2v_t{__int2float_rn(h[2]), __int2float_rn(h[3])};
    };
    // channels ride in pairs (v_pk_mul_f32 / v_pk_add_f32 round each half like the scalar ops; contraction is off): the
    // SSE2 sequence s = x0*b0; s += x1*b1; s += x2*b2; s += x3*b3, then v_cvt_pk_u8_f32 = round to nearest even + saturate
    auto vpass = [&](const float* bf) -> uint32_t {
        float2v_t sxy = hxy[0] * bf[0], szw = hzw[0] * bf[0];
#pragma unroll
        for (int k = 1; k < 4; k++) {
            sxy = sxy + hxy[k] * bf[k];
            szw = szw + hzw[k] * bf[k];
        }
        uint32_t px = cvt_pk_u8(sxy.x, 0u, 0);
        px = cvt_pk_u8(sxy.y, px, 1);
        px = cvt_pk_u8(szw.x, px, 2);
        return cvt_pk_u8(szw.y, px, 3);
    };
    for (int k = 0; k < 4; k++) advance();                     // the first row's footprint
    int dy = row0;
    const bool tail = dx * 4 + 3 >= vec_end;                   // this pixel holds bytes of the row's scalar tail
    const unsigned lane_off = (unsigned)dx * 4u;
    auto slow_row = [&](int y) {                               // any row, any strip: a dword per lane
        const UpRow rc = rows[y];
        while (cur < rc.first) advance();
        uint32_t px = vpass(rc.bf);
        if (tail) {
            const float hc[4][4] = {{hxy[0].x, hxy[1].x, hxy[2].x, hxy[3].x}, {hxy[0].y, hxy[1].y, hxy[2].y, hxy[3].y},
                                    {hzw[0].x, hzw[1].x, hzw[2].x, hzw[3].x}, {hzw[0].y, hzw[1].y, hzw[2].y, hzw[3].y}};
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (dx * 4 + c >= vec_end) {
                    int v = 1 << 21;
#pragma unroll
                    for (int k = 0; k < 4; k++) v += __mul24((int)hc[c][k], (int)yco[y * 4 + k]);
                    px = (px & ~(0xffu << (8 * c))) | ((uint32_t)shr_sat_u8(v, 22) << (8 * c));
                }
        }
        if (live) *(uint32_t*)(D + ((unsigned)y * (unsigned)a.dstep + lane_off)) = px;
    };

    // Fast path (wave-uniform): a full 64-column strip, 16-byte aligned destination, whole groups of four rows.  A full
    // strip never holds the row's scalar-tail pixel (that is the last pixel of an odd-width row, and a strip is full
    // only left of it).  Four rows are parked in the wave's LDS patch and leave as ONE 16-byte store per lane
    // (4 rows x 256 B per instruction).  Per row the scalar side does one pointer bump, one 32-byte constant row (the
    // table carries a sentinel row past the last one, so the look-ahead needs no bound) and one compare-and-branch for
    // the footprint advance (0 or 1: scale_y <= 1).
    const bool fast = txn == 64 && !(((uintptr_t)a.dst | (uintptr_t)a.dstep | (uintptr_t)a.dst_stride) & 15);
    if constexpr (PS > 0) {
        // Integer factors: the footprint advances on every PS-th row, so 4 PS rows -- four advances, after which the register
        // ring is back where it started -- unroll into straight code whose ring shifts are renames, not the 12 register
        // moves per advance the generic loop pays (8 % of this VALU-bound kernel's instructions at 4x, 16 % at 2x).
        if (fast) {
            slow_row(dy++);                                    // the chunk's first row: its footprint is in place
            while (dy < row_end && rows[dy].adv == 0) slow_row(dy++);      // up to the next advancing row
            const unsigned voff = (unsigned)(lane >> 4) * (unsigned)a.dstep + (unsigned)(tx0 + (lane & 15) * 4) * 4u;
            uint32_t* park = &s_tr[wv][0][lane];
            const u32x4_t* pick = (const u32x4_t*)&s_tr[wv][lane >> 4][(lane & 15) * 4];
            const size_t group_bytes = (size_t)a.dstep * 4;
            for (; dy + 4 * PS <= row_end; dy += 4 * PS) {
                const UpRow* rq = rows + dy;
                auto* Dg = D + (size_t)dy * a.dstep;
#pragma unroll
                for (int r = 0; r < 4 * PS; r++) {
                    const UpRow rc = rq[r];
                    if (r % PS == 0) advance();                // (static)
                    park[(r & 3) * 64] = vpass(rc.bf);
                    if ((r & 3) == 3) {
                        asm volatile("" ::: "memory");
                        const u32x4_t q = *pick;
                        asm volatile("" ::: "memory");
                        *(u32x4_t*)(Dg + (size_t)(r >> 2) * group_bytes + voff) = q;
                    }
                }
            }
        }
    } else
    if (fast) {
        const unsigned voff = (unsigned)(lane >> 4) * (unsigned)a.dstep + (unsigned)(tx0 + (lane & 15) * 4) * 4u;
        uint32_t* park = &s_tr[wv][0][lane];
        const u32x4_t* pick = (const u32x4_t*)&s_tr[wv][lane >> 4][(lane & 15) * 4];
        const UpRow* rq = rows + row0;
        UpRow rc = *rq;
        rc.adv = 0;                                            // the first row's footprint is already in place
        auto* Dg = D + (size_t)dy * a.dstep;
        const size_t group_bytes = (size_t)a.dstep * 4;
        for (; dy + 4 <= row_end; dy += 4, Dg += group_bytes) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const UpRow rn = *++rq;                        // next row's constants, in flight
                if (rc.adv) advance();
                park[r * 64] = vpass(rc.bf);
                rc = rn;
            }
            // the same wave wrote the patch and LDS serves a wave in order; the compiler must not move the 16-byte read
            // across the four dword writes either
            asm volatile("" ::: "memory");
            const u32x4_t q = *pick;
            asm volatile("" ::: "memory");
            *(u32x4_t*)(Dg + voff) = q;
        }
    }

    // Generic path: partial strips, unaligned destinations, the last (rows % 4) rows of a chunk
    for (; dy < row_end; dy++) slow_row(dy);
}

template <int PS>     // see up_cubic4_body
__global__ __launch_bounds__(256) void k_resize_up_cubic4(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                          const short* __restrict__ yco, const UpRow* __restrict__ rows,
                                                          int vec_end, int nbx, int rows_per_wave) {
    up_cubic4_body<PS, false>(a, blockIdx.y, blockIdx.x, xofs, xco, yco, rows, vec_end, nbx, rows_per_wave);
}

// The same for 3-channel frames -- what cvDecodeImage hands Resize() for every JPEG, so every JPEG enlargement
// (k_resize_taps<4,3> re-did the whole 4 x 4 footprint per output pixel: 0.056 of the roofline).  Differences from the
// BGRA kernel: the LDS patch holds the strip's source bytes (3 per pixel, rows padded to dwords); a lane's window is the
// 12 bytes at byte 3 * (first tap), taken as four aligned dwords + v_alignbyte_b32 and reduced by hpass_bgr's fixed-byte
// perm + dot2; the ring keeps (B,G) as a packed pair and R alone; four finished rows (4 x 192 bytes) leave the patch as
// three dword stores per lane.  The scalar tail of a row ((3 dw) % 8 bytes, up to the last three pixels) again lies only
// in the last, partial strip, which takes the generic path.
template <int KS>
__device__ __forceinline__ void hpass_bgr(const uint32_t* w, const short2_t* axp, int* h);

#define UP_CAP3_BYTES 6144   // bytes of source a wave stages in LDS

template <int PS, bool GLOBAL>     // see up_cubic4_body, also for the parameters
__device__ __forceinline__ void up_cubic3_body(const RArgs& a, unsigned frame, unsigned blk,
                                               const int* __restrict__ xofs, const short* __restrict__ xco,
                                               const short* __restrict__ yco, const UpRow* __restrict__ rows,
                                               int vec_end, int nbx, int rows_per_wave) {
    __shared__ __attribute__((aligned(16))) uint8_t s_tr[4][4 * 192];
    __shared__ __attribute__((aligned(16))) uint8_t s_src[4][UP_CAP3_BYTES];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int cy = blk / nbx, bx = blk - cy * nbx;
    const int tx0 = (bx * 4 + wv) * 64;
    if (tx0 >= a.dw) return;                                   // waves are independent: no barrier follows
    const int txn = min(64, a.dw - tx0);
    const bool live = lane < txn;
    const int dx = tx0 + min(lane, txn - 1);                   // idle lanes of a partial strip shadow its last column
    const int row0 = cy * rows_per_wave, row_end = min(a.dh, row0 + rows_per_wave);
    const auto* S = up_mem<GLOBAL>(a.src) + (long long)frame * a.src_stride;
    auto* D = up_mem<GLOBAL>(a.dst) + (long long)frame * a.dst_stride;

    short2_t axp[2];
    axp[0].x = xco[dx * 4]; axp[0].y = xco[dx * 4 + 1]; axp[1].x = xco[dx * 4 + 2]; axp[1].y = xco[dx * 4 + 3];

    const int sxmin = __builtin_amdgcn_readfirstlane(xofs[tx0]) - 1;
    const int W = __builtin_amdgcn_readfirstlane(xofs[tx0 + txn - 1]) + 2 - sxmin + 1;        // strip's source columns
    const int WB = ((W * 3 + 3) & ~3) + 4;                     // patch row pitch: dword-aligned, + the extra dword a window may touch
    const int f0 = rows[row0].first;
    const int NR = rows[row_end - 1].first + 3 - f0 + 1;       // chunk's footprint rows
    if (NR * WB > UP_CAP3_BYTES) return;   // cannot happen: the launcher sizes chunks from the same bounds; keeps LDS sound
    for (int i = lane; i < NR * W; i += 64) {                  // border replication happens here, once: clamped row / column
        const int r = i / W, c = i - r * W;
        const auto* q = S + (size_t)clampi(f0 + r, 0, a.sh - 1) * a.sstep + (size_t)clampi(sxmin + c, 0, a.sw - 1) * 3;
        uint8_t* o = &s_src[wv][r * WB + c * 3];
        o[0] = q[0]; o[1] = q[1]; o[2] = q[2];
    }
    const int lb = (xofs[dx] - 1 - sxmin) * 3;                 // this lane's first tap byte inside a patch row
    const int last = f0 + NR - 1;
    auto fetch = [&](int vy, uint32_t* t) {                    // the four aligned dwords around the 12-byte window of row vy
        const int o = ((min(vy, last) - f0) * WB + lb) >> 2;
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = ((const uint32_t*)&s_src[wv][0])[o + k];
    };

    float2v_t hxy[4];                                          // H sums of footprint rows cur .. cur + 3: (B,G) pairs ...
    float hz[4];                                               // ... and R
    uint32_t tn[4];                                            // dwords of footprint row cur + 4, requested one advance early
    int cur = f0 - 4;
    fetch(cur + 4, tn);
#pragma unroll
    for (int k = 0; k < 4; k++) { hxy[k] = float2v_t{0.f, 0.f}; hz[k] = 0.f; }
    const unsigned sh8 = (unsigned)lb & 3u;

    auto advance = [&]() {
        uint32_t w[3];
#pragma unroll
        for (int i = 0; i < 3; i++) w[i] = __builtin_amdgcn_alignbyte(tn[i + 1], tn[i], sh8);
        int h[3];
        hpass_bgr<4>(w, axp, h);
        cur++;
        fetch(cur + 4, tn);
        hxy[0] = hxy[1]; hxy[1] = hxy[2]; hxy[2] = hxy[3];
        hz[0] = hz[1]; hz[1] = hz[2]; hz[2] = hz[3];
        hxy[3] = float2v_t{__int2float_rn(h[0]), __int2float_rn(h[1])};
        hz[3] = __int2float_rn(h[2]);
    };
    auto vpass = [&](const float* bf) -> uint32_t {            // B | G << 8 | R << 16
        float2v_t sxy = hxy[0] * bf[0];
        float sz = __fmul_rn(hz[0], bf[0]);
#pragma unroll
        for (int k = 1; k < 4; k++) {
            sxy = sxy + hxy[k] * bf[k];
            sz = __fadd_rn(sz, __fmul_rn(hz[k], bf[k]));
        }
        uint32_t px = cvt_pk_u8(sxy.x, 0u, 0);
        px = cvt_pk_u8(sxy.y, px, 1);
        return cvt_pk_u8(sz, px, 2);
    };
    for (int k = 0; k < 4; k++) advance();
    int dy = row0;
    const bool tail = dx * 3 + 2 >= vec_end;
    auto slow_row = [&](int y) {                               // any row, any strip: three bytes per lane
        const UpRow rc = rows[y];
        while (cur < rc.first) advance();
        uint32_t px = vpass(rc.bf);
        if (tail) {
            const float hc[3][4] = {{hxy[0].x, hxy[1].x, hxy[2].x, hxy[3].x}, {hxy[0].y, hxy[1].y, hxy[2].y, hxy[3].y}, {hz[0], hz[1], hz[2], hz[3]}};
#pragma unroll
            for (int c = 0; c < 3; c++)
                if (dx * 3 + c >= vec_end) {
                    int v = 1 << 21;
#pragma unroll
                    for (int k = 0; k < 4; k++) v += __mul24((int)hc[c][k], (int)yco[y * 4 + k]);
                    px = (px & ~(0xffu << (8 * c))) | ((uint32_t)shr_sat_u8(v, 22) << (8 * c));
                }
        }
        if (live) {
            auto* o = D + (size_t)y * a.dstep + (size_t)dx * 3;
            o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16);
        }
    };

    const bool fast = txn == 64 && !(((uintptr_t)a.dst | (uintptr_t)a.dstep | (uintptr_t)a.dst_stride) & 3);
    if constexpr (PS > 0) {
        if (fast) {                                            // integer factors: the advance schedule is static (k_resize_up_cubic4)
            slow_row(dy++);
            while (dy < row_end && rows[dy].adv == 0) slow_row(dy++);
            uint8_t* park = &s_tr[wv][lane * 3];
            const size_t group_bytes = (size_t)a.dstep * 4;
            unsigned voff[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int n = lane + 64 * j;
                voff[j] = (unsigned)(n / 48) * (unsigned)a.dstep + (unsigned)(n % 48) * 4u;
            }
            for (; dy + 4 * PS <= row_end; dy += 4 * PS) {
                const UpRow* rq = rows + dy;
                auto* Dg = D + (size_t)dy * a.dstep + (size_t)tx0 * 3;
#pragma unroll
                for (int r = 0; r < 4 * PS; r++) {
                    const UpRow rc = rq[r];
                    if (r % PS == 0) advance();
                    const uint32_t px = vpass(rc.bf);
                    park[(r & 3) * 192] = (uint8_t)px; park[(r & 3) * 192 + 1] = (uint8_t)(px >> 8); park[(r & 3) * 192 + 2] = (uint8_t)(px >> 16);
                    if ((r & 3) == 3) {
                        asm volatile("" ::: "memory");
                        uint32_t q[3];
#pragma unroll
                        for (int j = 0; j < 3; j++) q[j] = ((const uint32_t*)&s_tr[wv][0])[lane + 64 * j];
                        asm volatile("" ::: "memory");
#pragma unroll
                        for (int j = 0; j < 3; j++) *(uint32_t*)(Dg + (size_t)(r >> 2) * group_bytes + voff[j]) = q[j];
                    }
                }
            }
        }
    } else
    if (fast) {
        uint8_t* park = &s_tr[wv][lane * 3];
        const UpRow* rq = rows + row0;
        UpRow rc = *rq;
        rc.adv = 0;
        auto* Dg = D + (size_t)dy * a.dstep + (size_t)tx0 * 3;
        const size_t group_bytes = (size_t)a.dstep * 4;
        // the 4 x 48 dwords of a group go out as three dword stores per lane: dword n = lane + 64 j -> row n / 48, column n % 48
        unsigned voff[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const int n = lane + 64 * j;
            voff[j] = (unsigned)(n / 48) * (unsigned)a.dstep + (unsigned)(n % 48) * 4u;
        }
        for (; dy + 4 <= row_end; dy += 4, Dg += group_bytes) {
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const UpRow rn = *++rq;
                if (rc.adv) advance();
                const uint32_t px = vpass(rc.bf);
                park[r * 192] = (uint8_t)px; park[r * 192 + 1] = (uint8_t)(px >> 8); park[r * 192 + 2] = (uint8_t)(px >> 16);
                rc = rn;
            }
            asm volatile("" ::: "memory");                     // the compiler must not move the dword reads across the byte writes
            uint32_t q[3];
#pragma unroll
            for (int j = 0; j < 3; j++) q[j] = ((const uint32_t*)&s_tr[wv][0])[lane + 64 * j];
            asm volatile("" ::: "memory");
#pragma unroll
            for (int j = 0; j < 3; j++) *(uint32_t*)(Dg + voff[j]) = q[j];
        }
    }

    for (; dy < row_end; dy++) slow_row(dy);                   // partial strips, unaligned destinations, a chunk's last rows
}

template <int PS>     // see up_cubic4_body
__global__ __launch_bounds__(256) void k_resize_up_cubic3(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                          const short* __restrict__ yco, const UpRow* __restrict__ rows,
                                                          int vec_end, int nbx, int rows_per_wave) {
    up_cubic3_body<PS, false>(a, blockIdx.y, blockIdx.x, xofs, xco, yco, rows, vec_end, nbx, rows_per_wave);
}

// Enlargements of DIFFERENT geometry in one launch (launch_resize_mixed's MIX_UP class): the descriptor scheme of
// k_resize_area_mix around the two bodies above, so the bytes are the lone launch's.  A descriptor is one frame: its views,
// where its four tables lie in the blob that travels behind the descriptor table (byte offsets from `blob`; `rows` -- the
// UpRow array with its sentinel -- at a 32-byte multiple of the allocation, read as 32-byte scalar rows), and the lone
// kernels' three launch arguments.  The workgroup's index inside its descriptor is the lone kernels' blockIdx.x:
// nblk = nbx * (chunks of rows_per_wave rows).  Only the generic footprint advance is carried (PS = 0): a frame with a
// whole factor, which alone runs the unrolled PS form, pays the ring's register moves here -- 8 % of the instructions at
// 4x, 16 % at 2x -- for one kernel instead of four in the launch.  Same registers and LDS as the lone <0> kernels; the
// descriptor's fields arrive by scalar loads (d[di]: block-uniform) where the lone kernels read launch arguments.
struct alignas(32) UpMixDesc { RArgs a; unsigned xofs, xco, yco, rows; int vec_end, nbx, rows_per_wave, first, nblk; };
static_assert(sizeof(UpMixDesc) % 32 == 0, "the blob behind n descriptors starts at a 32-byte multiple (UpRow rows)");

template <int CN>
__global__ __launch_bounds__(256) void k_resize_up_cubic_mix(const UpMixDesc* __restrict__ d, MixIndex ix, const uint8_t* __restrict__ blob) {
    static_assert(CN == 3 || CN == 4, "BGR and BGRA");
    int blk;
    const int di = mix_pick(d, ix, &blk);
    if (di < 0) return;
    const UpMixDesc& m = d[di];
    RArgs a = m.a;
    a.src_stride = a.dst_stride = 0;                   // a descriptor is one frame: the fast path's alignment test is its pointer and pitch
    const int* xofs = (const int*)(blob + m.xofs);
    const short* xco = (const short*)(blob + m.xco);
    const short* yco = (const short*)(blob + m.yco);
    const UpRow* rows = (const UpRow*)(blob + m.rows);
    if constexpr (CN == 4) up_cubic4_body<0, true>(a, 0u, (unsigned)blk, xofs, xco, yco, rows, m.vec_end, m.nbx, m.rows_per_wave);
    else up_cubic3_body<0, true>(a, 0u, (unsigned)blk, xofs, xco, yco, rows, m.vec_end, m.nbx, m.rows_per_wave);
}

// vertical pass over the register ring at phase U of its period; returns the packed BGRA destination pixel
// {sat_u8(v0 >> sh), sat_u8(v1 >> sh), sat_u8(v2 >> sh), sat_u8(v3 >> sh)} as bytes 0..3 in two instructions.
// v_ashr_pk_u8_i32 writes ONE 16-bit half of its destination ({sat(S1 >> S2), sat(S0 >> S2)}) and leaves the other
// half alone; op_sel:[0,0,0,1] selects the upper half.  Checked on hardware by tools/pk_probe.hip -- this is the
// instruction hipcc itself mis-used (it assumes the other half is cleared; see shr_sat_u8).
__device__ __forceinline__ uint32_t shr_sat_pack4(int v0, int v1, int v2, int v3, int sh) {
    uint32_t r;
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3" : "=v"(r) : "v"(v0), "v"(v1), "v"(sh));
    asm("v_ashr_pk_u8_i32 %0, %1, %2, %3 op_sel:[0,0,0,1]" : "+v"(r) : "v"(v2), "v"(v3), "v"(sh));
    return r;
}

// a * b + c on the 24-bit multiplier as ONE instruction (hipcc otherwise splits it into v_mul_i32_i24 + v_add3_u32,
// and every integer multiply form issues at half rate on gfx950: profiles/r01_valu_rates.txt)
__device__ __forceinline__ int mad24(int a, int b, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// the same with the weight in a scalar register (wave-uniform row weights): no v_mov of it into a VGPR
__device__ __forceinline__ int mad24s(int a, int b_uniform, int c) {
    int r;
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(b_uniform), "v"(c));
    return r;
}

// VSYM: the KS row weights are mirror-symmetric (host-checked; true at the half-pixel phase of an exact 2x scale),
// so mirrored ring rows are added first (full-rate v_add_u32, exact) and the multiplies halve.
template <int KS, int MODE, int U, bool VSYM = false>
__device__ __forceinline__ uint32_t vpass_px(const int (*ring)[4], const int* b, int dx, int vec_end) {
    int out[4];
    if constexpr (MODE == M_LANCZOS) {
        int v[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            int hc[KS];
#pragma unroll
            for (int k = 0; k < KS; k++) hc[k] = ring[(k + 2 * U) % KS][c];
            v[c] = 1 << 21;                                    // |hc| < 2^23: the 24-bit multiplier is exact
            if constexpr (VSYM) {
#pragma unroll
                for (int k = 0; k < KS / 2; k++) v[c] = mad24s(hc[k] + hc[KS - 1 - k], b[k], v[c]);   // VSYM callers pass uniform weights
            } else {
#pragma unroll
                for (int k = 0; k < KS; k++) v[c] = mad24(hc[k], b[k], v[c]);
            }
        }
        return shr_sat_pack4(v[0], v[1], v[2], v[3], 22);
    }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int hc[KS];
#pragma unroll
        for (int k = 0; k < KS; k++) hc[k] = ring[(k + 2 * U) % KS][c];
        if constexpr (MODE == M_LINEAR) {
            out[c] = (uint8_t)(((__mul24(b[0], hc[0] >> 4) >> 16) + (__mul24(b[1], hc[1] >> 4) >> 16) + 2) >> 2);   // (|hc >> 4| < 2^15, b <= 2^11: the 24-bit multiplier is exact)
        } else if constexpr (MODE == M_CUBIC) {
            if (dx * 4 + c < vec_end) {
                const float sc = 1.f / (2048.f * 2048.f);
                float s = __fmul_rn(__int2float_rn(hc[0]), __fmul_rn((float)b[0], sc));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[1]), __fmul_rn((float)b[1], sc)));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[2]), __fmul_rn((float)b[2], sc)));
                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[3]), __fmul_rn((float)b[3], sc)));
                out[c] = sat_u8(__float2int_rn(s));
            } else {
                int v = __mul24(hc[0], b[0]) + __mul24(hc[1], b[1]) + __mul24(hc[2], b[2]) + __mul24(hc[3], b[3]);
                out[c] = shr_sat_u8(v + (1 << 21), 22);
            }
        } else {
            int v = 1 << 21;                                   // |hc| < 2^23: the 24-bit multiplier is exact
            if constexpr (VSYM) {
#pragma unroll
                for (int k = 0; k < KS / 2; k++) v = mad24s(hc[k] + hc[KS - 1 - k], b[k], v);   // VSYM callers pass uniform weights
            } else {
#pragma unroll
                for (int k = 0; k < KS; k++) v = mad24(hc[k], b[k], v);
            }
            out[c] = shr_sat_u8(v, 22);
        }
    }
    return (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
}

// one wave's strip with the windows loaded straight into registers (any column range, clamped taps at the borders)
template <int KS, int MODE>
__device__ __forceinline__ void roll_strip(const RArgs& a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                           const int* __restrict__ yofs, const short* __restrict__ yco, int vec_end,
                                           int strip, int lane) {
    const int dx = strip * 64 + lane;
    const int dy0 = blockIdx.y * ROLL_STRIP;
    const int dyn = min(ROLL_STRIP, a.dh - dy0);
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;                       // idle lanes shadow the last column (no stores)
    const uint8_t* S = a.src + (long long)blockIdx.z * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride;

    short2_t axp[KS / 2];
#pragma unroll
    for (int j = 0; j < KS / 2; j++) { axp[j].x = xco[dxc * KS + 2 * j]; axp[j].y = xco[dxc * KS + 2 * j + 1]; }
    const int sx0 = xofs[dxc] - (KS / 2 - 1);
    const bool interior = sx0 >= 0 && sx0 + KS <= a.sw;
    const int sxv = clampi(sx0, 0, a.sw - KS) * 4;
    int sxk[KS];
#pragma unroll
    for (int k = 0; k < KS; k++) sxk[k] = clampi(sx0 + k, 0, a.sw - 1) * 4;
    int by[KS];                                                 // identical for every destination row (host-checked)
#pragma unroll
    for (int k = 0; k < KS; k++) by[k] = yco[dy0 * KS + k];

    // ring[(k + 2*i) % KS] holds the horizontal pass of source row (first tap row of destination row dy0+i) + k
    int ring[KS][4];
    const int sy_first = yofs[dy0] - (KS / 2 - 1);              // yofs[dy] = yofs[dy0] + 2*(dy - dy0), checked on the host
#pragma unroll
    for (int k = 0; k < KS - 2; k++)
        hpass_row<KS>(S + (size_t)clampi(sy_first + k, 0, a.sh - 1) * a.sstep, sxv, sxk, interior, axp, ring[k]);

    constexpr int UN = KS / 2;                                  // ring period: every ring index below is a constant
    for (int i0 = 0; i0 < dyn; i0 += UN) {
        static_for<UN>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            const int i = i0 + u;
            if (i < dyn) {
                const int dy = dy0 + i;
                const int sy = sy_first + 2 * i;
                hpass_row<KS>(S + (size_t)clampi(sy + KS - 2, 0, a.sh - 1) * a.sstep, sxv, sxk, interior, axp, ring[(KS - 2 + 2 * u) % KS]);
                hpass_row<KS>(S + (size_t)clampi(sy + KS - 1, 0, a.sh - 1) * a.sstep, sxv, sxk, interior, axp, ring[(KS - 1 + 2 * u) % KS]);
                const uint32_t px = vpass_px<KS, MODE, u>(ring, by, dx, vec_end);
                if (live) *(uint32_t*)(D + (size_t)dy * a.dstep + (size_t)dx * 4) = px;
            }
        });
    }
}

template <int KS, int MODE>
__global__ __launch_bounds__(256) void k_resize_2x_roll(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                        const int* __restrict__ yofs, const short* __restrict__ yco, int vec_end) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the four waves of a block take four neighbouring 64-column strips of the SAME rows: together they read
    // 2 KB contiguous runs of each source row (DRAM page locality) and share the overlapping window columns in L1
    const int strip = blockIdx.x * 4 + wv;
    if (strip * 64 >= a.dw) return;
    roll_strip<KS, MODE>(a, xofs, xco, yofs, yco, vec_end, strip, lane);
}

// ------------------------------------------------------------------ exact 2x decimation, 3-channel strips
// The register-rolling strip for BGR frames (every JPEG; 4K photo -> 1080p is this case).  A window is KS pixels =
// 3*KS bytes at a byte address: one unaligned dwordx3 (cubic) or two (lanczos); tap k, channel c is the fixed byte
// 3k + c, so v_perm_b32 still pairs two taps of a channel for v_dot2 -- the selector just names other bytes, possibly
// of the next dword.  Ring of KS x 3 row sums, 3 byte stores per output.  (The per-pixel k_resize_taps did the whole
// KS x KS footprint for every output: 18.8 k img/s for 4K lanczos; this form shares each row sum between KS/2 outputs.)
template <int KS>
__device__ __forceinline__ void hpass_bgr(const uint32_t* w, const short2_t* axp, int* h) {
    constexpr int NDW = (KS * 3 + 3) / 4;                       // (KS = 2: six bytes in two dwords)
#pragma unroll
    for (int c = 0; c < 3; c++) {
        int acc = 0;
#pragma unroll
        for (int j = 0; j < KS / 2; j++) {
            const int b0 = 6 * j + c, d0 = b0 >> 2, i0 = b0 - 4 * d0, i1 = i0 + 3;      // bytes of taps 2j and 2j+1
            const uint32_t lo = w[d0], hi = w[d0 + 1 < NDW ? d0 + 1 : d0];
            const uint32_t pr = __builtin_amdgcn_perm(hi, lo, 0x0c000c00u | (uint32_t)i0 | ((uint32_t)i1 << 16));
            acc = __builtin_amdgcn_sdot2(as_short2(pr), axp[j], acc, false);
        }
        h[c] = acc;
    }
}

template <int KS, int MODE, bool VSYM>
__global__ __launch_bounds__(256) void k_resize_2x_roll3(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                         const int* __restrict__ yofs, const short* __restrict__ yco, int vec_end) {
    static_assert((KS * 3) % 4 == 0 && MODE != M_LINEAR, "cubic and lanczos only");
    constexpr int NDW = KS * 3 / 4;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = blockIdx.x * 4 + wv;
    if (strip * 64 >= a.dw) return;
    const int dx = strip * 64 + lane;
    const int dy0 = blockIdx.y * ROLL_STRIP;
    const int dyn = min(ROLL_STRIP, a.dh - dy0);
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;
    const uint8_t* S = a.src + (long long)blockIdx.z * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride + (size_t)dx * 3;

    short2_t axp[KS / 2];
#pragma unroll
    for (int j = 0; j < KS / 2; j++) { axp[j].x = xco[dxc * KS + 2 * j]; axp[j].y = xco[dxc * KS + 2 * j + 1]; }
    const int sx0 = xofs[dxc] - (KS / 2 - 1);
    const bool interior = sx0 >= 0 && sx0 + KS <= a.sw;
    const int sxv = clampi(sx0, 0, a.sw - KS) * 3;
    int by[KS];
#pragma unroll
    for (int k = 0; k < KS; k++) by[k] = __builtin_amdgcn_readfirstlane((int)yco[dy0 * KS + k]);
    const int sy_first = yofs[dy0] - (KS / 2 - 1);

    auto hrow = [&](int sy, int* h) {
        const uint8_t* row = S + (size_t)clampi(sy, 0, a.sh - 1) * a.sstep;
        uint32_t w[NDW];
        load_bytes_aligned<NDW>(w, row + sxv);                              // aligned dwords + v_alignbyte (the window starts at any byte)
#pragma unroll
        for (int i = 0; i < NDW; i++) asm volatile("" : "+v"(w[i]));          // opaque: keeps the wide load next to the fallback
        if (!interior) {                                                      // border columns: clamped taps, byte by byte
#pragma unroll
            for (int i = 0; i < NDW; i++) w[i] = 0;
#pragma unroll
            for (int k = 0; k < KS; k++) {
                const uint8_t* q = row + clampi(sx0 + k, 0, a.sw - 1) * 3;
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int o = 3 * k + c;
                    w[o >> 2] |= (uint32_t)q[c] << (8 * (o & 3));
                }
            }
        }
        hpass_bgr<KS>(w, axp, h);
    };

    int ring[KS][3];
#pragma unroll
    for (int k = 0; k < KS - 2; k++) hrow(sy_first + k, ring[k]);

    constexpr int UN = KS / 2;
    for (int i0 = 0; i0 < dyn; i0 += UN) {
        static_for<UN>([&](auto uc) {
            constexpr int u = decltype(uc)::value;
            const int i = i0 + u;
            if (i < dyn) {
                const int sy = sy_first + 2 * i;
                hrow(sy + KS - 2, ring[(KS - 2 + 2 * u) % KS]);
                hrow(sy + KS - 1, ring[(KS - 1 + 2 * u) % KS]);
                int out[3];
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    int hc[KS];
#pragma unroll
                    for (int k = 0; k < KS; k++) hc[k] = ring[(k + 2 * u) % KS][c];
                    if constexpr (MODE == M_CUBIC) {
                        if (dx * 3 + c < vec_end) {
                            const float sc = 1.f / (2048.f * 2048.f);
                            float s = __fmul_rn(__int2float_rn(hc[0]), __fmul_rn((float)by[0], sc));
                            s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[1]), __fmul_rn((float)by[1], sc)));
                            s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[2]), __fmul_rn((float)by[2], sc)));
                            s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[3]), __fmul_rn((float)by[3], sc)));
                            out[c] = sat_u8(__float2int_rn(s));
                        } else {
                            int v = __mul24(hc[0], by[0]) + __mul24(hc[1], by[1]) + __mul24(hc[2], by[2]) + __mul24(hc[3], by[3]);
                            out[c] = shr_sat_u8(v + (1 << 21), 22);
                        }
                    } else {
                        int v = 1 << 21;
                        if constexpr (VSYM) {
#pragma unroll
                            for (int k = 0; k < KS / 2; k++) v = mad24s(hc[k] + hc[KS - 1 - k], by[k], v);
                        } else {
#pragma unroll
                            for (int k = 0; k < KS; k++) v = mad24s(hc[k], by[k], v);
                        }
                        out[c] = v;
                    }
                }
                if constexpr (MODE != M_CUBIC) {
                    const uint32_t pk = shr_sat_pack4(out[0], out[1], out[2], 0, 22);
                    out[0] = pk & 0xff; out[1] = (pk >> 8) & 0xff; out[2] = (pk >> 16) & 0xff;
                }
                if (live) {
                    uint8_t* q = D + (size_t)(dy0 + i) * a.dstep;
                    q[0] = (uint8_t)out[0]; q[1] = (uint8_t)out[1]; q[2] = (uint8_t)out[2];
                }
            }
        });
    }
}

// ------------------------------------------------------------------ any scale up to 2, any enlargement: rolling strips
// LINEAR and LANCZOS4 at every scale that is not exactly 2 (those have the static schedules above), CUBIC when y shrinks
// while x grows (Resize() asks for CUBIC as soon as ONE axis grows, bridge.c:190), BGRA and BGR.  Replaces the LDS-tiled
// kernel of rounds 1-2 (0.13 of the roofline: ~250 VALU operations per output, a block-wide barrier pair per tile) and
// the per-pixel gather that 3-channel frames used to fall to.
// The exact-2x strips generalised: a lane owns one destination column, a wave walks a strip of rows down and keeps the
// horizontal sums of the CURRENT footprint -- rows first .. first + KS - 1, in order -- in registers.  The footprint moves
// by yofs[dy] - yofs[dy - 1] rows per destination row (0 or 1 when enlarging, 1 or 2 when shrinking by up to 2): every
// step reduces one new source row into the ring slot of the row that leaves (the windows come straight from memory:
// neighbouring lanes overlap, so a wave's request is a few contiguous lines).  The row's weights are wave-uniform
// (scalar loads).  Nothing is shared between waves: no LDS, no barrier.
constexpr int strip_row_ints(int ks) { return ks <= 2 ? 4 : 16; }   // per destination row: {first footprint row, KS weights, padding; CUBIC: the weights as floats at [8..11]}

// The vertical pass of the strip kernels: footprint row k is ring[(k + P) & (KS - 1)] (P = 0 where the ring is shifted, the
// footprint's position in the slots where it is not).
//   LINEAR: the ring holds S >> 4, the only form VResizeLinear reads a horizontal sum in (shifted once per SOURCE row, not
//     once per use); the result cannot exceed 255, so the bytes are packed without masks.
//   CUBIC: VResizeCubicVec_32s8u's four float products, added in footprint order, two channels per packed instruction, from
//     a ring of floats; the weights come as the floats b * 2^-22 the host tabulated (one IEEE multiply each, the same one
//     the kernel used to do per lane and row).
template <int KS, int MODE, int CN, int P>
__device__ __forceinline__ uint32_t strip_vpass(const int (*ring)[CN], const int* by, const float* bf, int dx, int vec_end) {
    if constexpr (MODE == M_LINEAR) {
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) {                          // (T < 2^15, b <= 2^11: the 24-bit multiplier is exact)
            const uint32_t o = ((((uint32_t)__mul24(by[0], ring[P & 1][c])) >> 16) + (((uint32_t)__mul24(by[1], ring[(P + 1) & 1][c])) >> 16) + 2u) >> 2;
            px |= o << (8 * c);
        }
        return px;
    } else if constexpr (MODE == M_LANCZOS) {
        int v[4] = {0, 0, 0, 0};
#pragma unroll
        for (int c = 0; c < CN; c++) {
            v[c] = 1 << 21;                                     // |h| < 2^23: the 24-bit multiplier is exact
#pragma unroll
            for (int k = 0; k < KS; k++) v[c] = mad24s(ring[(k + P) & (KS - 1)][c], by[k], v[c]);
        }
        return shr_sat_pack4(v[0], v[1], v[2], v[3], 22) & (CN == 4 ? 0xffffffffu : 0xffffffu);
    } else {
        // the ring holds the sums as floats (exact: |sum| < 2^24; converted once per source row); channels ride in pairs
        // (v_pk_mul_f32 / v_pk_add_f32 round each half like the scalar operations, contraction is off), v_cvt_pk_u8_f32 is
        // saturate_cast<uchar>(cvRound(x)) -- k_resize_up_cubic4's vertical pass
        float f[KS][4];
#pragma unroll
        for (int k = 0; k < KS; k++)
#pragma unroll
            for (int c = 0; c < 4; c++) f[k][c] = c < CN ? __int_as_float(ring[(k + P) & (KS - 1)][c < CN ? c : 0]) : 0.f;
        float2v_t sxy = float2v_t{f[0][0], f[0][1]} * bf[0];
#pragma unroll
        for (int k = 1; k < KS; k++) sxy = sxy + float2v_t{f[k][0], f[k][1]} * bf[k];
        uint32_t px = cvt_pk_u8(sxy.x, 0u, 0);
        px = cvt_pk_u8(sxy.y, px, 1);
        if constexpr (CN == 4) {
            float2v_t szw = float2v_t{f[0][2], f[0][3]} * bf[0];
#pragma unroll
            for (int k = 1; k < KS; k++) szw = szw + float2v_t{f[k][2], f[k][3]} * bf[k];
            px = cvt_pk_u8(szw.x, px, 2);
            px = cvt_pk_u8(szw.y, px, 3);
        } else {
            float sz = __fmul_rn(f[0][2], bf[0]);
#pragma unroll
            for (int k = 1; k < KS; k++) sz = __fadd_rn(sz, __fmul_rn(f[k][2], bf[k]));
            px = cvt_pk_u8(sz, px, 2);
        }
        if (dx * CN + CN > vec_end) {                           // the row's scalar tail (its last 0..7 bytes): the integer form
#pragma unroll
            for (int c = 0; c < CN; c++)
                if (dx * CN + c >= vec_end) {
                    int v = 1 << 21;
#pragma unroll
                    for (int k = 0; k < KS; k++) v += __mul24(__float2int_rn(f[k][c]), by[k]);
                    px = (px & ~(0xffu << (8 * c))) | ((uint32_t)shr_sat_u8(v, 22) << (8 * c));
                }
        }
        return px;
    }
}

// What a lane of a strip kernel knows about its destination column: the horizontal weights, where its window starts, and
// how to fetch and reduce one source row's window.
template <int KS, int MODE, int CN>
struct StripLane {
    static constexpr int NDW = (KS * 3 + 3) / 4;               // dwords holding a BGR window
    static constexpr int NW = CN == 4 ? KS : NDW + 1;          // registers of one window in flight (BGR: before the byte alignment)
    const uint8_t* S;
    int sstep, sh;
    short2_t axp[KS / 2];
    bool interior;
    int sxv;
    unsigned bsh;                                              // BGR: where the window starts inside its first aligned dword
    int sxk[KS];

    __device__ __forceinline__ void init(const RArgs& a, const uint8_t* src, int dxc, const int* __restrict__ xofs, const short* __restrict__ xco) {
        S = src; sstep = a.sstep; sh = a.sh;
#pragma unroll
        for (int j = 0; j < KS / 2; j++) { axp[j].x = xco[dxc * KS + 2 * j]; axp[j].y = xco[dxc * KS + 2 * j + 1]; }
        const int sx0 = xofs[dxc] - (KS / 2 - 1);
        interior = sx0 >= 0 && sx0 + KS <= a.sw;
        sxv = clampi(sx0, 0, a.sw - KS) * CN;
        bsh = (unsigned)(uintptr_t)(S + sxv) & 3u;
#pragma unroll
        for (int k = 0; k < KS; k++) sxk[k] = clampi(sx0 + k, 0, a.sw - 1) * CN;
    }
    // A source row's window is REQUESTED two footprint steps before it is reduced (no wait at the request: loads and stores
    // share vmcnt, and a wave that waited for every window where it asks for it spent its time in that wait) ...
    __device__ __forceinline__ void request(int sy, uint32_t* w) const {
        const uint8_t* row = S + (size_t)clampi(sy, 0, sh - 1) * sstep;
        if constexpr (CN == 4) __builtin_memcpy(w, __builtin_assume_aligned(row + sxv, 4), KS * 4);
        else {
            const uint32_t* q = (const uint32_t*)(row + sxv - bsh);
            __builtin_memcpy(w, __builtin_assume_aligned(q, 4), NDW * 4);
            w[NDW] = q[(bsh + 3 * KS - 1) >> 2];                // the word the window's last byte lives in: never past it
        }
    }
    // ... and reduced here: horizontal sums of that row for this column.  Border columns (the strips at the frame's edges)
    // re-read their taps one by one at clamped positions.
    __device__ __forceinline__ void reduce(int sy, uint32_t* w, int* h) const {
#pragma unroll
        for (int i = 0; i < NW; i++) asm volatile("" : "+v"(w[i]));   // opaque: keeps the wide load apart from the fallback below
        if constexpr (CN == 4) {
            if (!interior) {
                const uint8_t* row = S + (size_t)clampi(sy, 0, sh - 1) * sstep;
#pragma unroll
                for (int k = 0; k < KS; k++) w[k] = *(const uint32_t*)(row + sxk[k]);
            }
            hpass_px<KS>(w, axp, h);
        } else {
            uint32_t v[NDW];
#pragma unroll
            for (int i = 0; i < NDW; i++) v[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], bsh);
            if (!interior) {
                const uint8_t* row = S + (size_t)clampi(sy, 0, sh - 1) * sstep;
#pragma unroll
                for (int i = 0; i < NDW; i++) v[i] = 0;
#pragma unroll
                for (int k = 0; k < KS; k++)
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int o = 3 * k + c;
                        v[o >> 2] |= (uint32_t)row[sxk[k] + c] << (8 * (o & 3));
                    }
            }
            hpass_bgr<KS>(v, axp, h);
        }
        if constexpr (MODE == M_CUBIC) {
#pragma unroll
            for (int c = 0; c < CN; c++) h[c] = __float_as_int(__int2float_rn(h[c]));   // the vertical pass is float (strip_vpass)
        }
        if constexpr (MODE == M_LINEAR) {
#pragma unroll
            for (int c = 0; c < CN; c++) h[c] = (h[c] >> 4) & 0xffff;   // VResizeLinear reads S >> 4 and nothing else of S (0 <= S < 2^20: one v_bfe_u32, and the multiplier's operand is known to fit)
        }
    }
};

template <int CN>
__device__ __forceinline__ void strip_store(uint8_t* q, uint32_t px) {
    if constexpr (CN == 4) *(uint32_t*)q = px;
    else { q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); }
}

// any advance pattern: the ring is shifted by one row per footprint step
template <int KS, int MODE, int CN>
__global__ __launch_bounds__(256) void k_resize_strip(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                      const int* __restrict__ srows, int vec_end, int rows_per_strip) {
    static_assert(CN == 3 || CN == 4, "interleaved BGR / BGRA");
    using Lane = StripLane<KS, MODE, CN>;
    constexpr int NW = Lane::NW;
    constexpr int SR = strip_row_ints(KS);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = blockIdx.x * 4 + wv;                      // the four waves of a block: neighbouring strips of the same rows
    if (strip * 64 >= a.dw) return;
    const int dx = strip * 64 + lane;
    const int dy0 = blockIdx.y * rows_per_strip, dy1 = min(a.dh, dy0 + rows_per_strip);
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;                       // idle lanes shadow the last column (no stores)
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride + (size_t)dx * CN;
    Lane L;
    L.init(a, a.src + (long long)blockIdx.z * a.src_stride, dxc, xofs, xco);

    int ring[KS][CN];
    int first = srows[(size_t)dy0 * SR];
    {
        uint32_t w[NW];
#pragma unroll
        for (int k = 0; k < KS; k++) { L.request(first + k, w); L.reduce(first + k, w, ring[k]); }
    }
    uint32_t p0[NW], p1[NW];                                    // windows of rows first + KS and first + KS + 1, in flight
    L.request(first + KS, p0);
    L.request(first + KS + 1, p1);
    for (int dy = dy0; dy < dy1; dy++) {
        const int* __restrict__ rw = srows + (size_t)dy * SR;   // (wave-uniform: scalar loads)
        const int want = rw[0];
        while (first < want) {                                  // one source row further: shift, reduce the row that enters
#pragma unroll
            for (int k = 0; k + 1 < KS; k++)
#pragma unroll
                for (int c = 0; c < CN; c++) ring[k][c] = ring[k + 1][c];
            L.reduce(first + KS, p0, ring[KS - 1]);
            first++;
#pragma unroll
            for (int i = 0; i < NW; i++) p0[i] = p1[i];
            L.request(first + KS + 1, p1);
        }
        int by[KS];
        float bf[KS];
#pragma unroll
        for (int k = 0; k < KS; k++) { by[k] = rw[1 + k]; bf[k] = MODE == M_CUBIC ? __int_as_float(rw[(SR > 8 ? 8 : 0) + k]) : 0.f; }
        const uint32_t px = strip_vpass<KS, MODE, CN, 0>(ring, by, bf, dx, vec_end);
        if (live) strip_store<CN>(D + (size_t)dy * a.dstep, px);
    }
}

// The same walk for the geometries whose footprint advance is periodic with period two -- A0 rows after every even
// destination row, A1 after every odd one: (1, 0) / (0, 1) is the exact 2x enlargement, (1, 2) / (2, 1) the 1.5x
// reduction -- which are the common ones (bridge.c:183-193 reaches LINEAR / LANCZOS4 only through a `resize` with explicit
// interpolation, and callers ask for round factors).  The schedule is then static: a block of 2 * NP destination rows is
// unrolled until the footprint is back in the ring slot it started from, so nothing is ever shifted -- source row j of the
// block lives in ring[j & (KS - 1)], the vertical pass names its rows by its position P in the block -- and the window
// registers alternate by the row's parity.  (The shifts were 28 of LANCZOS4's ~70 instructions per footprint step.  The
// same walk with DYNAMIC slots -- scalar branches on first & (KS - 1) -- was built and is slower than shifting: the
// branches cost what the moves did and hipcc's s_waitcnt placement at the joins waits for the windows in flight.)
// Strips start on multiples of the block, so every strip sees the pattern at the same phase; the last block of a frame
// computes past the last row (clamped table row, clamped source rows) and stores nothing there.
template <int KS, int MODE, int CN, int A0, int A1>
__global__ __launch_bounds__(256) void k_resize_strip2(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                       const int* __restrict__ srows, int vec_end, int rows_per_strip, int wide_stores) {
    static_assert(CN == 3 || CN == 4, "interleaved BGR / BGRA");
    static_assert((A0 + A1) % 2 == 1, "an odd advance per pair of rows: the block is 2 * KS rows");
    __shared__ __attribute__((aligned(16))) uint32_t s_patch[4][4][64];   // per wave: four finished rows of its 64 columns
    using Lane = StripLane<KS, MODE, CN>;
    constexpr int NW = Lane::NW;
    constexpr int SR = strip_row_ints(KS);
    constexpr int A = A0 + A1, NP = KS;                         // KS pairs advance KS * A rows: a multiple of KS, and even
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int strip = blockIdx.x * 4 + wv;
    if (strip * 64 >= a.dw) return;
    const int dx = strip * 64 + lane;
    const int dy0 = blockIdx.y * rows_per_strip, dy1 = min(a.dh, dy0 + rows_per_strip);
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride + (size_t)dx * CN;
    uint8_t* Dw = a.dst + (long long)blockIdx.z * a.dst_stride + (size_t)strip * 64 * CN;     // the strip's first byte of row 0
    const bool patch = wide_stores && strip * 64 + 64 <= a.dw;  // (wave-uniform; the frame's last, partial strip stores pixel by pixel)
    Lane L;
    L.init(a, a.src + (long long)blockIdx.z * a.src_stride, dxc, xofs, xco);

    int ring[KS][CN];
    int first = __builtin_amdgcn_readfirstlane(srows[(size_t)dy0 * SR]);
    {
        uint32_t w[NW];
#pragma unroll
        for (int k = 0; k < KS; k++) { L.request(first + k, w); L.reduce(first + k, w, ring[k]); }
    }
    uint32_t pe[NW], po[NW];                                    // windows in flight: block rows KS, KS + 2, ... in pe, the odd ones in po
    L.request(first + KS, pe);
    L.request(first + KS + 1, po);
    for (int dyb = dy0; dyb < dy1; dyb += 2 * NP) {
        static_for<2 * NP>([&](auto mc) {
            constexpr int m = decltype(mc)::value;
            constexpr int rel = (m / 2) * A + ((m & 1) ? A0 : 0);       // the footprint's first row, in block rows
            const int dy = dyb + m;
            const int* __restrict__ rw = srows + (size_t)min(dy, a.dh) * SR;   // (row dh is the table's sentinel)
            int by[KS];
            float bf[KS];
#pragma unroll
            for (int k = 0; k < KS; k++) { by[k] = rw[1 + k]; bf[k] = MODE == M_CUBIC ? __int_as_float(rw[(SR > 8 ? 8 : 0) + k]) : 0.f; }
            const uint32_t px = strip_vpass<KS, MODE, CN, rel & (KS - 1)>(ring, by, bf, dx, vec_end);
            if (patch) {
                // four finished rows of the wave's 64 columns leave as 16-byte (BGR: 4-byte) stores: a pixel per lane and
                // row is a 256-byte (192-byte, in byte stores) write per instruction, and the store stream is what bounds
                // the enlargements once the arithmetic is down
                if constexpr (CN == 4) s_patch[wv][m & 3][lane] = px;
                else {
                    uint8_t* pb = (uint8_t*)s_patch[wv][m & 3] + lane * 3;
                    pb[0] = (uint8_t)px; pb[1] = (uint8_t)(px >> 8); pb[2] = (uint8_t)(px >> 16);
                }
                if constexpr ((m & 3) == 3) {
                    const int dyg = dyb + m - 3;
                    if constexpr (CN == 4) {
                        const int r = lane >> 4, g = lane & 15;
                        const uint4 v = *(const uint4*)&s_patch[wv][r][g * 4];
                        if (dyg + r < dy1) *(uint4*)(Dw + (size_t)(dyg + r) * a.dstep + g * 16) = v;
                    } else {
#pragma unroll
                        for (int t = 0; t < 3; t++) {
                            const int i = lane + 64 * t, r = i / 48, wd = i % 48;
                            const uint32_t v = s_patch[wv][r][wd];
                            if (dyg + r < dy1) *(uint32_t*)(Dw + (size_t)(dyg + r) * a.dstep + wd * 4) = v;
                        }
                    }
                }
            } else if (live && dy < dy1) strip_store<CN>(D + (size_t)dy * a.dstep, px);
            constexpr int adv = (m & 1) ? A1 : A0;
            static_for<adv>([&](auto sc) {
                constexpr int j = rel + decltype(sc)::value + KS;       // the block row that enters
                if constexpr (j & 1) { L.reduce(first + j, po, ring[j & (KS - 1)]); L.request(first + j + 2, po); }
                else                 { L.reduce(first + j, pe, ring[j & (KS - 1)]); L.request(first + j + 2, pe); }
            });
        });
        first += NP * A;
    }
}

// ------------------------------------------------------------------ exact 2x decimation, LDS-DMA row ring
// The register-rolling strip above keeps only ~1 KB of unique source bytes in flight per wave (two 536-byte row
// segments), ~20 KB per CU -- under half of what Little's law asks for at HBM speed, and prefetching further ahead
// into registers costs the occupancy it buys.  Here each wave streams its row segments D iterations ahead with
// global_load_lds_dwordx4 (global -> LDS DMA: no VGPRs, no ds_write) into a private ring of 2D+2 LDS row slots and
// takes its tap windows from there.  Nothing is shared between waves, so there are no barriers: a wave orders its
// own DMA against its own reads with s_waitcnt vmcnt(2D): fetches retire in order among themselves, so a row still
// in flight would have the 2D younger fetches in flight behind it and the count could not be <= 2D -- the destination
// stores in the queue can only make the wait stricter, in whatever order they retire (counting them too, vmcnt(3D),
// assumes loads and stores retire in one order; the 3-channel kernel showed that assumption to be wrong).  In strips that touch the image border the granules outside the row are
// masked off and the taps are read from LDS at clamped indices (a wave-uniform branch).
#define DMA_SLOT 576       // bytes per LDS row slot: (2 * 64 + KS + 3 rounded to 4) pixels = 34 lanes x 16 B, padded

#ifndef DMA_WAVES
#define DMA_WAVES 6
#endif
// MF (round 5): the HORIZONTAL pass on the matrix unit.  The counters (profiles/r05_sq_cfg4.txt) have this kernel bound by vector
// issue -- 71 % busy, 61 % of the wave cycles queueing to issue -- at ~110 vector instructions per output pixel, 64 of them the
// two horizontal passes (perm + dot2 per tap pair and channel).  At an exact 2x scale every column has the same taps, so a source
// row's 64 x 4 horizontal sums are ONE banded product: C[16 x 16] = A[16 x 64] x B[64 x 16] with
//   B[k][n] = byte k of WINDOW n of the row (window n = the 64 bytes from byte 32 n of the row slot: the taps of output pixels
//             4n .. 4n + 3 of the strip lie in its bytes 4 .. 59; a lane's operand is one ds_read_b128, biased to signed by one XOR per dword),
//   A[m][k] = the tap weight of (output o = m >> 2, channel c = m & 3) on byte k: tap j sits at k = 8 o + 4 + 4 j + c (the strip's
//             first tap is dword 1 of the slot: sx00 = 2 dx0 - 3 = 1 mod 4 for interior strips), split into two signed bytes, two MFMAs,
//   C[m][n] -> lane l holds reg r = channel r of output pixel 4 (l & 15) + (l >> 4) of the strip (operand maps of the 16x16x64 i8
//             MFMA as probed on hardware, imp_blur.hip) -- exactly what the vertical pass wants in a lane, under a permuted
//             lane -> pixel map, which only the stores have to know.
// Integer and exact: pixels enter as p - 128 and 128 x (the weights' sum: 2048 give or take the table's rounding) is added back; the sums
// are the same 32-bit integers.
// Per source row a lane issues one LDS read, four XORs, two MFMAs and eight adds/shifts where it issued eight LDS reads and
// thirty-two perm / dot2.  Border strips (clamped taps) keep the vector form.
typedef int rz_v4i __attribute__((ext_vector_type(4)));

template <int KS, int MODE, int DEPTH, bool VSYM, int WPB, bool MF = false>
__global__ __launch_bounds__(64 * WPB, DMA_WAVES) void k_resize_2x_dma(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                       const int* __restrict__ yofs, const short* __restrict__ yco, int vec_end,
                                                       int nbx, int bpf, int count) {
    constexpr int R = 2 * DEPTH + 2;
    __shared__ __attribute__((aligned(16))) uint8_t lds[WPB][R][DMA_SLOT];
    // four finished rows of a wave's 64 columns, parked only to leave as ONE 16-byte store per lane (4 rows x 256 B per
    // instruction) instead of four dword stores: stores sit in the same vmcnt queue as the DMA fetches, so every store
    // still in flight takes one of the 2*DEPTH places the prefetch is allowed to hold -- a store per row and a write
    // latency of several iterations cut the effective prefetch depth to a fraction of DEPTH
    __shared__ __attribute__((aligned(16))) uint32_t s_tr[WPB][4][64];
    // one frame per XCD at a time, its blocks in row-major order: an XCD then streams whole source rows (DRAM page
    // runs of 15 KB instead of one 2 KB column band of every frame) and the strips' shared halo rows meet in its L2
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int bx = blk % nbx, byy = blk / nbx;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dx0 = (bx * WPB + wv) * 64;
    if (dx0 >= a.dw) return;
    const int sx00 = __builtin_amdgcn_readfirstlane(xofs[dx0]) - (KS / 2 - 1);   // first tap of the strip's first column
    const int wstart = sx00 & ~3;                                                // window start, 16-byte aligned (may be < 0)
    const int nl = (sx00 - wstart + 126 + KS + 3) >> 2;                          // lanes (x 16 B) that cover the window
    // border strips: granules outside the row are not fetched and every tap index is clamped like the CPU's
    const bool edge = wstart < 0 || wstart + nl * 4 > a.sw || dx0 + 64 > a.dw;   // wave-uniform
    const int dx = dx0 + lane;
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;                                        // idle lanes shadow the last column
    const int gpx = wstart + 4 * lane;                                           // first pixel of this lane's DMA granule
    const bool fetch = lane < nl && gpx >= 0 && gpx + 4 <= a.sw;                 // sw % 4 == 0 (host-checked): never partial
    const int sx0e = xofs[dxc] - (KS / 2 - 1);
    const int dy0 = byy * ROLL_STRIP;
    const int dyn = min(ROLL_STRIP, a.dh - dy0);
    // wave-uniform bases (scalar registers) + 32-bit lane offsets: the saddr + voffset form of global_load_lds / store
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)wstart * 4;
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dx0 * 4;
    const unsigned lane16 = lane * 16u, lane4 = lane * 4u;

    short2_t axp[KS / 2];
#pragma unroll
    for (int j = 0; j < KS / 2; j++) { axp[j].x = xco[dxc * KS + 2 * j]; axp[j].y = xco[dxc * KS + 2 * j + 1]; }
    int by[KS];                                                 // wave-uniform: scalar registers
#pragma unroll
    for (int k = 0; k < KS; k++) by[k] = __builtin_amdgcn_readfirstlane((int)yco[dy0 * KS + k]);
    const int lane_dw = 2 * lane + (sx00 - wstart);             // this lane's first tap, in dwords from the slot start
    const int sy_first = yofs[dy0] - (KS / 2 - 1);

    // source row sy_first + r (clamped) -> slot r % R
    auto issue = [&](int r) {
        // 32-bit offset from the scalar frame base (saddr + voffset addressing; a frame is < 4 GB, host-checked):
        // the 64-bit form costs a v_mad_i64_i32 per address
        const uint8_t* g = S + ((unsigned)clampi(sy_first + r, 0, a.sh - 1) * (unsigned)a.sstep + lane16);
        if (fetch)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)&lds[wv][r % R][0], 16, 0, 0);
    };
    // the whole strip twice, under one wave-uniform branch: written as a single loop with the branch inside the
    // window read, hipcc if-converts it and every wave pays the border's per-tap clamped addressing
    auto strip = [&](auto edge_c) {
        constexpr bool EDGE = decltype(edge_c)::value;
        auto window = [&](int r, uint32_t* p) {
            const uint32_t* w = (const uint32_t*)&lds[wv][r % R][0];
#pragma unroll
            for (int k = 0; k < KS; k++) p[k] = EDGE ? w[clampi(sx0e + k, 0, a.sw - 1) - wstart] : w[lane_dw + k];
        };
        constexpr bool MFS = MF && !EDGE;                           // this strip's horizontal pass runs on the matrix unit
        // the lane's output pixel within the strip (MFS: the MFMA's accumulator layout decides)
        const int xl = MFS ? 4 * (lane & 15) + (lane >> 4) : lane;
        rz_v4i band_hi = {0, 0, 0, 0}, band_lo = {0, 0, 0, 0};
        int hbias = 0;                                              // 128 x (the weights' sum): what the bias of the pixels took away
        if constexpr (MFS) {
#pragma unroll
            for (int k = 0; k < KS; k++) hbias += 128 * (int)xco[(size_t)dx0 * KS + k];
            // A operand: lane l holds A[m = l & 15][k = 16 (l >> 4) .. + 15]
            const int m = lane & 15, o = m >> 2, c = m & 3;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                uint32_t hi = 0, lo = 0;
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    const int k = 16 * (lane >> 4) + 4 * q + b, t = k - 8 * o - 4 - c;
                    int w = 0;
                    if (t >= 0 && !(t & 3) && (t >> 2) < KS) w = (int)xco[(size_t)dx0 * KS + (t >> 2)];
                    const int wl = (int)(int8_t)(w & 0xff), wh = (w - wl) >> 8;           // w = 256 wh + wl, both signed bytes (|w| < 2^15)
                    lo |= (uint32_t)(wl & 0xff) << (8 * b);
                    hi |= (uint32_t)(wh & 0xff) << (8 * b);
                }
                band_hi[q] = (int)hi;
                band_lo[q] = (int)lo;
            }
        }
        // the horizontal sums of source row r for this lane's output pixel, all four channels
        auto hrow = [&](int r, int* h) {
            if constexpr (MFS) {
                const rz_v4i raw = *(const rz_v4i*)&lds[wv][r % R][32 * (lane & 15) + 16 * (lane >> 4)];
                const rz_v4i d = {raw[0] ^ (int)0x80808080u, raw[1] ^ (int)0x80808080u, raw[2] ^ (int)0x80808080u, raw[3] ^ (int)0x80808080u};
                const rz_v4i zero = {0, 0, 0, 0};
                const rz_v4i ch = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_hi, d, zero, 0, 0, 0);
                const rz_v4i cl = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_lo, d, zero, 0, 0, 0);
#pragma unroll
                for (int c = 0; c < 4; c++) h[c] = (ch[c] << 8) + cl[c] + hbias;
            } else {
                uint32_t p[KS];
                window(r, p);
                hpass_px<KS>(p, axp, h);
            }
        };

        // prologue: fill the ring, take the KS-2 rows above the first destination row, then top the queue up to
        // DEPTH iterations ahead (those rows reuse the slots just consumed)
        static_assert(R >= KS - 2 && R <= KS - 2 + 2 * DEPTH, "ring too small for the prologue");
        int ring[KS][4];
#pragma unroll
        for (int r = 0; r < R; r++) issue(r);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R - (KS - 2)) : "memory");
#pragma unroll
        for (int k = 0; k < KS - 2; k++) hrow(k, ring[k]);
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = R; r < KS - 2 + 2 * DEPTH; r++) issue(r);

        constexpr int UN = KS / 2;
        // whole groups of four rows of a full strip with a 16-byte aligned destination leave through the LDS patch
        const bool wide = !EDGE && UN == 4 && !(((uintptr_t)a.dst | (uintptr_t)a.dstep | (uintptr_t)a.dst_stride) & 15);
        const unsigned voff4 = (unsigned)(lane >> 4) * (unsigned)a.dstep + (unsigned)(lane & 15) * 16u;
        const int dxl = dx0 + xl;                                  // this lane's destination column
        const unsigned xl4 = (unsigned)xl * 4u;
        for (int i0 = 0; i0 < dyn; i0 += UN) {
            const bool park = wide && i0 + UN <= dyn;          // wave-uniform
            static_for<UN>([&](auto uc) {
                constexpr int u = decltype(uc)::value;
                const int i = i0 + u;
                if (i < dyn) {
                    const int r0 = KS - 2 + 2 * i;
                    if (i + DEPTH < dyn) {
                        issue(r0 + 2 * DEPTH);
                        issue(r0 + 2 * DEPTH + 1);
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DEPTH) : "memory");
                    } else {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    if constexpr (MFS) {
                        // both rows' operands and all four MFMAs first, the sums afterwards: a wave does not wait for a product it
                        // has just asked for
                        const rz_v4i ra = *(const rz_v4i*)&lds[wv][r0 % R][32 * (lane & 15) + 16 * (lane >> 4)];
                        const rz_v4i rb = *(const rz_v4i*)&lds[wv][(r0 + 1) % R][32 * (lane & 15) + 16 * (lane >> 4)];
                        const rz_v4i da = {ra[0] ^ (int)0x80808080u, ra[1] ^ (int)0x80808080u, ra[2] ^ (int)0x80808080u, ra[3] ^ (int)0x80808080u};
                        const rz_v4i db = {rb[0] ^ (int)0x80808080u, rb[1] ^ (int)0x80808080u, rb[2] ^ (int)0x80808080u, rb[3] ^ (int)0x80808080u};
                        const rz_v4i zero = {0, 0, 0, 0};
                        const rz_v4i ah = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_hi, da, zero, 0, 0, 0);
                        const rz_v4i al = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_lo, da, zero, 0, 0, 0);
                        const rz_v4i bh = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_hi, db, zero, 0, 0, 0);
                        const rz_v4i bl = __builtin_amdgcn_mfma_i32_16x16x64_i8(band_lo, db, zero, 0, 0, 0);
#pragma unroll
                        for (int c = 0; c < 4; c++) {
                            ring[(KS - 2 + 2 * u) % KS][c] = (ah[c] << 8) + al[c] + hbias;
                            ring[(KS - 1 + 2 * u) % KS][c] = (bh[c] << 8) + bl[c] + hbias;
                        }
                    } else {
                        hrow(r0, ring[(KS - 2 + 2 * u) % KS]);
                        hrow(r0 + 1, ring[(KS - 1 + 2 * u) % KS]);
                    }
                    asm volatile("" ::: "memory");             // the slots just read may be refilled from here on
                    const uint32_t px = vpass_px<KS, MODE, u, VSYM>(ring, by, EDGE ? dx : dxl, vec_end);
                    if (park) s_tr[wv][u & 3][xl] = px;
                    else if (!EDGE || live) *(uint32_t*)(D + ((unsigned)(dy0 + i) * (unsigned)a.dstep + (EDGE ? lane4 : xl4))) = px;
                }
            });
            if (park) {
                asm volatile("" ::: "memory");                 // the compiler must not move the 16-byte read across the dword writes
                const u32x4_t q = *(const u32x4_t*)&s_tr[wv][lane >> 4][(lane & 15) * 4];
                asm volatile("" ::: "memory");
                *(u32x4_t*)(D + ((unsigned)(dy0 + i0) * (unsigned)a.dstep + voff4)) = q;
            }
        }
    };
    if (edge) strip(std::true_type{});
    else strip(std::false_type{});
}

// ------------------------------------------------------------------ exact 2x decimation, LDS-DMA row ring, 3 channels
// k_resize_2x_dma for BGR frames.  Everything is counted in bytes: the strip's window starts at the 16-byte granule
// holding byte 3 * (first tap) and spans (126 + KS) pixels = at most 27 granules; a lane's taps start 6 bytes after
// its neighbour's, so it reads the aligned dwords around them and realigns with v_alignbyte_b32 (shift 0..3), then
// runs the fixed-byte perm + dot2 pass of hpass_bgr.  Each row is three byte stores per lane.
#define DMA3_SLOT 448      // bytes per LDS row slot: 28 granules

template <int KS, int MODE, int DEPTH, bool VSYM>
__global__ __launch_bounds__(256, 5) void k_resize_2x_dma3(RArgs a, const int* __restrict__ xofs, const short* __restrict__ xco,
                                                        const int* __restrict__ yofs, const short* __restrict__ yco, int vec_end,
                                                        int nbx, int bpf, int count) {
    static_assert((KS * 3) % 4 == 0 && MODE != M_LINEAR, "cubic and lanczos only");
    constexpr int R = 2 * DEPTH + 2, NDW = KS * 3 / 4;
    __shared__ __attribute__((aligned(16))) uint8_t lds[4][R][DMA3_SLOT];
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int bx = blk % nbx, byy = blk / nbx;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dx0 = (bx * 4 + wv) * 64;
    if (dx0 >= a.dw) return;
    const int sx00 = __builtin_amdgcn_readfirstlane(xofs[dx0]) - (KS / 2 - 1);   // first tap of the strip's first column
    const int b00 = sx00 * 3;                                                    // ... as a byte offset in the row
    const int wstart = b00 & ~15;                                                // window start byte, 16-byte aligned (may be < 0)
    const int nl = (b00 - wstart + (126 + KS) * 3 + 15) >> 4;                    // granules that cover the window (<= 27)
    const int rowbytes = a.sw * 3;                                               // a multiple of 16 (host-checked): no partial granule
    const bool edge = wstart < 0 || wstart + nl * 16 > rowbytes || dx0 + 64 > a.dw;   // wave-uniform
    const int dx = dx0 + lane;
    const bool live = dx < a.dw;
    const int dxc = live ? dx : a.dw - 1;
    const int gb = wstart + 16 * lane;                                           // first byte of this lane's DMA granule
    const bool fetch = lane < nl && gb >= 0 && gb + 16 <= rowbytes;
    const int sx0e = xofs[dxc] - (KS / 2 - 1);
    const int dy0 = byy * ROLL_STRIP;
    const int dyn = min(ROLL_STRIP, a.dh - dy0);
    const uint8_t* S = a.src + (long long)frame * a.src_stride + wstart;
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dx0 * 3;
    const unsigned lane16 = lane * 16u, lane3 = lane * 3u;

    short2_t axp[KS / 2];
#pragma unroll
    for (int j = 0; j < KS / 2; j++) { axp[j].x = xco[dxc * KS + 2 * j]; axp[j].y = xco[dxc * KS + 2 * j + 1]; }
    int by[KS];
#pragma unroll
    for (int k = 0; k < KS; k++) by[k] = __builtin_amdgcn_readfirstlane((int)yco[dy0 * KS + k]);
    const int lane_b = 6 * lane + (b00 - wstart);               // this lane's first tap byte inside a slot
    const int sy_first = yofs[dy0] - (KS / 2 - 1);

    auto issue = [&](int r) {
        const uint8_t* g = S + ((unsigned)clampi(sy_first + r, 0, a.sh - 1) * (unsigned)a.sstep + lane16);
        if (fetch)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)&lds[wv][r % R][0], 16, 0, 0);
    };
    auto strip = [&](auto edge_c) {
        constexpr bool EDGE = decltype(edge_c)::value;
        auto window = [&](int r, uint32_t* w) {
            const uint8_t* slot = &lds[wv][r % R][0];
            if constexpr (!EDGE) {
                const uint32_t* q = (const uint32_t*)slot + (lane_b >> 2);
                uint32_t t[NDW + 1];
#pragma unroll
                for (int i = 0; i <= NDW; i++) t[i] = q[i];
#pragma unroll
                for (int i = 0; i < NDW; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], (unsigned)lane_b & 3u);
            } else {
#pragma unroll
                for (int i = 0; i < NDW; i++) w[i] = 0;
#pragma unroll
                for (int k = 0; k < KS; k++) {
                    const uint8_t* q = slot + (clampi(sx0e + k, 0, a.sw - 1) * 3 - wstart);
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int o = 3 * k + c;
                        w[o >> 2] |= (uint32_t)q[c] << (8 * (o & 3));
                    }
                }
            }
        };

        static_assert(R >= KS - 2 && R <= KS - 2 + 2 * DEPTH, "ring too small for the prologue");
        int ring[KS][3];
#pragma unroll
        for (int r = 0; r < R; r++) issue(r);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(R - (KS - 2)) : "memory");
#pragma unroll
        for (int k = 0; k < KS - 2; k++) {
            uint32_t w[NDW];
            window(k, w);
            hpass_bgr<KS>(w, axp, ring[k]);
        }
        asm volatile("" ::: "memory");
#pragma unroll
        for (int r = R; r < KS - 2 + 2 * DEPTH; r++) issue(r);

        constexpr int UN = KS / 2;
        for (int i0 = 0; i0 < dyn; i0 += UN) {
            static_for<UN>([&](auto uc) {
                constexpr int u = decltype(uc)::value;
                const int i = i0 + u;
                if (i < dyn) {
                    const int r0 = KS - 2 + 2 * i;
                    if (i + DEPTH < dyn) {
                        issue(r0 + 2 * DEPTH);
                        issue(r0 + 2 * DEPTH + 1);
                        // vmcnt <= 2 DEPTH proves this iteration's rows have landed whatever the stores in the queue do:
                        // fetches retire in order among themselves, so a row still in flight would have all 2 DEPTH younger
                        // fetches in flight behind it.  (Counting the 3 DEPTH stores as well -- vmcnt(5 DEPTH) -- assumes
                        // stores retire in order with loads; it gave intermittent wrong rows here, so they do not.)
                        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * DEPTH) : "memory");
                    } else {
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    }
                    uint32_t p[NDW], q[NDW];
                    window(r0, p);
                    window(r0 + 1, q);
                    hpass_bgr<KS>(p, axp, ring[(KS - 2 + 2 * u) % KS]);
                    hpass_bgr<KS>(q, axp, ring[(KS - 1 + 2 * u) % KS]);
                    asm volatile("" ::: "memory");
                    int out[3];
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        int hc[KS];
#pragma unroll
                        for (int k = 0; k < KS; k++) hc[k] = ring[(k + 2 * u) % KS][c];
                        if constexpr (MODE == M_CUBIC) {
                            if (dx * 3 + c < vec_end) {
                                const float sc = 1.f / (2048.f * 2048.f);
                                float s = __fmul_rn(__int2float_rn(hc[0]), __fmul_rn((float)by[0], sc));
                                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[1]), __fmul_rn((float)by[1], sc)));
                                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[2]), __fmul_rn((float)by[2], sc)));
                                s = __fadd_rn(s, __fmul_rn(__int2float_rn(hc[3]), __fmul_rn((float)by[3], sc)));
                                out[c] = sat_u8(__float2int_rn(s));
                            } else {
                                int v = __mul24(hc[0], by[0]) + __mul24(hc[1], by[1]) + __mul24(hc[2], by[2]) + __mul24(hc[3], by[3]);
                                out[c] = shr_sat_u8(v + (1 << 21), 22);
                            }
                        } else {
                            int v = 1 << 21;
                            if constexpr (VSYM) {
#pragma unroll
                                for (int k = 0; k < KS / 2; k++) v = mad24s(hc[k] + hc[KS - 1 - k], by[k], v);
                            } else {
#pragma unroll
                                for (int k = 0; k < KS; k++) v = mad24s(hc[k], by[k], v);
                            }
                            out[c] = v;
                        }
                    }
                    if constexpr (MODE != M_CUBIC) {
                        const uint32_t pk = shr_sat_pack4(out[0], out[1], out[2], 0, 22);
                        out[0] = pk & 0xff; out[1] = (pk >> 8) & 0xff; out[2] = (pk >> 16) & 0xff;
                    }
                    // always three store instructions per iteration (the wait above counts them): idle lanes of a
                    // partial strip are masked per lane, the instructions still issue
                    uint8_t* o = D + ((unsigned)(dy0 + i) * (unsigned)a.dstep + lane3);
                    if (!EDGE || live) { o[0] = (uint8_t)out[0]; o[1] = (uint8_t)out[1]; o[2] = (uint8_t)out[2]; }
                }
            });
        }
    };
    if (edge) strip(std::true_type{});
    else strip(std::false_type{});
}

// ------------------------------------------------------------------ NN
// (the body is shared with k_resize_nn_mix: `idx` = the destination pixel, `frame` = the frame of a uniform batch)
template <int CN>
__device__ __forceinline__ void resize_nn_body(const RArgs& a, double scale_x, double scale_y, long long idx, unsigned frame) {
    if (idx >= (long long)a.dw * a.dh) return;
    const int dy = (int)(idx / a.dw), dx = (int)(idx - (long long)dy * a.dw);
    int sx = (int)floor(dx * scale_x), sy = (int)floor(dy * scale_y);
    sx = sx > a.sw - 1 ? a.sw - 1 : sx;
    sy = sy > a.sh - 1 ? a.sh - 1 : sy;
    const uint8_t* s = a.src + (long long)frame * a.src_stride + (size_t)sy * a.sstep + (size_t)sx * CN;
    uint8_t* d = a.dst + (long long)frame * a.dst_stride + (size_t)dy * a.dstep + (size_t)dx * CN;
    if (CN == 4) *(uint32_t*)d = *(const uint32_t*)s;
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) d[c] = s[c];
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_resize_nn(RArgs a, double scale_x, double scale_y) {
    resize_nn_body<CN>(a, scale_x, scale_y, (long long)blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------ AREA, integer scales
// (the bodies of this kernel and of the streaming forms below are shared with k_area_int_mix: `idx` / `gw` = the work
// item, `frame` = the frame of a uniform batch)
template <int CN>
__device__ __forceinline__ void area_int_body(const RArgs& a, int isx, int isy, int idx, unsigned frame) {
    if (idx >= a.dw * a.dh) return;
    const int dy = idx / a.dw, dx = idx - dy * a.dw;
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)(dy * isy) * a.sstep + (size_t)(dx * isx) * CN;
    int sum[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) sum[c] = 0;
    for (int ky = 0; ky < isy; ky++) {
        const uint8_t* row = S + (size_t)ky * a.sstep;
        for (int kx = 0; kx < isx; kx++) {
            if (CN == 4) {
                uint32_t p = *(const uint32_t*)(row + kx * 4);
                sum[0] += p & 0xff; sum[1] += (p >> 8) & 0xff; sum[2] += (p >> 16) & 0xff; sum[3] += p >> 24;
            } else {
#pragma unroll
                for (int c = 0; c < CN; c++) sum[c] += row[kx * CN + c];
            }
        }
    }
    uint8_t* d = a.dst + (long long)frame * a.dst_stride + (size_t)dy * a.dstep + (size_t)dx * CN;
    int out[CN];
    if (isx == 2 && isy == 2) {
#pragma unroll
        for (int c = 0; c < CN; c++) out[c] = (sum[c] + 2) >> 2;
    } else {
        const float scale = 1.f / (float)(isx * isy);
#pragma unroll
        for (int c = 0; c < CN; c++) out[c] = sat_u8(__float2int_rn(__fmul_rn((float)sum[c], scale)));
    }
    if (CN == 4) *(uint32_t*)d = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) d[c] = (uint8_t)out[c];
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_resize_area_int(RArgs a, int isx, int isy) {
    area_int_body<CN>(a, isx, isy, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------ AREA, exact 2x2 box, streaming form
// resizeAreaFast_ with both scales 2: (a + b + c + d + 2) >> 2 per channel -- a pure stream (every source byte read
// once, a quarter as many written), so it is written like a copy: a lane owns FOUR neighbouring destination pixels of a
// row = 32 source bytes in each of two rows (two 16-byte non-temporal loads per row, all four in flight before the first
// use) and one 16-byte store; a wave reads two 2 KB runs and writes one 1 KB run.  The four channels of a pixel are
// summed two at a time in 16-bit halves of a dword (1022 fits).  The per-pixel k_resize_area_int it replaces issued
// four dword loads and one dword store per lane and reached 0.49 of the HBM roofline.
__device__ __forceinline__ uint32_t box4_swar(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const uint32_t M = 0x00ff00ffu;
    const uint32_t e = (a & M) + (b & M) + (c & M) + (d & M) + 0x00020002u;
    const uint32_t o = ((a >> 8) & M) + ((b >> 8) & M) + ((c >> 8) & M) + ((d >> 8) & M) + 0x00020002u;
    return ((e >> 2) & M) | (((o >> 2) & M) << 8);
}

__device__ __forceinline__ void area2x2_v4_body(const RArgs& a, int qpr, int idx, unsigned frame) {
    if (idx >= qpr * a.dh) return;
    const int dy = idx / qpr, q = idx - dy * qpr;
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)(2 * dy) * a.sstep + (size_t)q * 32;
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dy * a.dstep + (size_t)q * 16;
    const int n = min(4, a.dw - 4 * q);
    if (n == 4) {
        uint32_t r0[8], r1[8];
        load_stream<8>(r0, S);
        load_stream<8>(r1, S + a.sstep);
        u32x4_t o;
        o.x = box4_swar(r0[0], r0[1], r1[0], r1[1]);
        o.y = box4_swar(r0[2], r0[3], r1[2], r1[3]);
        o.z = box4_swar(r0[4], r0[5], r1[4], r1[5]);
        o.w = box4_swar(r0[6], r0[7], r1[6], r1[7]);
        __builtin_nontemporal_store(o, (u32x4_t*)D);
    } else {
        for (int j = 0; j < n; j++) {
            const uint32_t* p0 = (const uint32_t*)(S + 8 * j);
            const uint32_t* p1 = (const uint32_t*)(S + a.sstep + 8 * j);
            *(uint32_t*)(D + 4 * j) = box4_swar(p0[0], p0[1], p1[0], p1[1]);
        }
    }
}

__global__ __launch_bounds__(256) void k_area2x2_v4(RArgs a, int qpr) {
    area2x2_v4_body(a, qpr, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// The same for 3-channel frames (every JPEG): four destination pixels = 12 bytes out, 24 bytes in from each of two rows
// (dwordx4 + dwordx2, 4-byte aligned because 24 q is); source byte 6 j + c (+3 for the right neighbour) of each row.
__device__ __forceinline__ void area2x2_v3_body(const RArgs& a, int qpr, int idx, unsigned frame) {
    if (idx >= qpr * a.dh) return;
    const int dy = idx / qpr, q = idx - dy * qpr;
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)(2 * dy) * a.sstep + (size_t)q * 24;
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dy * a.dstep + (size_t)q * 12;
    const int n = min(4, a.dw - 4 * q);
    if (n == 4) {
        uint32_t r0[6], r1[6];
        load_stream<6>(r0, S);
        load_stream<6>(r1, S + a.sstep);
        uint32_t o[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const int i0 = 6 * j + c, i1 = i0 + 3, ob = 3 * j + c;
                const uint32_t sum = ((r0[i0 >> 2] >> (8 * (i0 & 3))) & 0xff) + ((r0[i1 >> 2] >> (8 * (i1 & 3))) & 0xff) +
                                     ((r1[i0 >> 2] >> (8 * (i0 & 3))) & 0xff) + ((r1[i1 >> 2] >> (8 * (i1 & 3))) & 0xff) + 2;
                o[ob >> 2] |= (sum >> 2) << (8 * (ob & 3));
            }
        typedef unsigned int u32x3_t __attribute__((ext_vector_type(3), aligned(4)));
        const u32x3_t ov = {o[0], o[1], o[2]};
        *(u32x3_t*)D = ov;
    } else {
        const uint8_t* p0 = S;
        const uint8_t* p1 = S + a.sstep;
        for (int j = 0; j < n; j++)
            for (int c = 0; c < 3; c++)
                D[3 * j + c] = (uint8_t)((p0[6 * j + c] + p0[6 * j + 3 + c] + p1[6 * j + c] + p1[6 * j + 3 + c] + 2) >> 2);
    }
}

__global__ __launch_bounds__(256) void k_area2x2_v3(RArgs a, int qpr) {
    area2x2_v3_body(a, qpr, blockIdx.x * 256 + threadIdx.x, blockIdx.y);
}

// ------------------------------------------------------------------ AREA, other integer scales (3x3, 4x4, 4x3 ...), streaming form
// resizeAreaFast_ for integer scales: the box sum is exact integer work and the mean is saturate(cvRound(sum * (1.f/area))).
// Two channels per add in the 16-bit halves of a dword (ISX * ISY * 255 fits 16 bits up to 257 source pixels per box).
// The per-pixel k_resize_area_int these replace issued one dword load per source pixel: 0.45 (4x4) and 0.27 (8x8) of the
// roofline; a first streaming form that gave each lane ISX adjacent 16-byte granules (64 to 128 bytes between lanes) had
// every 128-byte line fetched by four to eight different instructions: 0.49 / 0.29 (0.57 for ISX = 3).
//
// Power-of-two widths (1/4 and 1/8 thumbnails): here every wave-instruction reads 1 KB CONTIGUOUS (lane l takes the l-th
// 16-byte granule of the j-th 1 KB piece), so a 16-byte granule is one whole box column group (ISX = 4) or half of one
// (ISX = 8, the two halves meet through one DPP exchange at the end).
template <int ISX>
__global__ __launch_bounds__(256) void k_area_boxc(RArgs a, int isy, int gpr, float scale) {
    static_assert(ISX == 4 || ISX == 8, "16-byte granules must tile a box row");
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    // granules (16 bytes = 4 source pixels) are numbered along a band of ISY source rows, then band by band: a wave takes
    // 4 x 64 consecutive ones, so a band's end does not leave lanes idle (gpr = granules per source row)
    const int total = gpr * a.dh;
    int gx[4], dy[4];
    const uint8_t* S = a.src + (long long)blockIdx.y * a.src_stride;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int gid = (gw * 4 + j) * 64 + lane;
        dy[j] = gid / gpr;
        gx[j] = gid - dy[j] * gpr;
        if (gid >= total) dy[j] = -1;
    }
    if (dy[0] < 0) return;                                     // lanes past the end only ever trail a wave (ISX = 8 pairs stay whole: gpr is even)
    const uint32_t M = 0x00ff00ffu;
    uint32_t e[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
    for (int ky = 0; ky < isy; ky++) {
        uint32_t p[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (dy[j] >= 0) load_stream<4>(p[j], S + (size_t)(dy[j] * isy + ky) * a.sstep + (size_t)gx[j] * 16);
            else p[j][0] = p[j][1] = p[j][2] = p[j][3] = 0;
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 4; k++) { e[j] += p[j][k] & M; o[j] += (p[j][k] >> 8) & M; }
    }
    uint8_t* D = a.dst + (long long)blockIdx.y * a.dst_stride;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint32_t ee = e[j], oo = o[j];
        if (ISX == 8) {                                       // the other half of the box sits in the neighbouring lane
            ee += (uint32_t)__shfl_xor((int)ee, 1);
            oo += (uint32_t)__shfl_xor((int)oo, 1);
        }
        uint32_t px = cvt_pk_u8(__fmul_rn((float)(ee & 0xffff), scale), 0u, 0);
        px = cvt_pk_u8(__fmul_rn((float)(oo & 0xffff), scale), px, 1);
        px = cvt_pk_u8(__fmul_rn((float)(ee >> 16), scale), px, 2);
        px = cvt_pk_u8(__fmul_rn((float)(oo >> 16), scale), px, 3);
        if (dy[j] >= 0 && (ISX == 4 || !(lane & 1))) *(uint32_t*)(D + (size_t)dy[j] * a.dstep + (size_t)(gx[j] * 4 / ISX) * 4) = px;
    }
}

// 2x2 in the same contiguous form (even destination widths): a granule is two destination pixels, a wave reads 2 x 1 KB
// runs of each of its two source rows and writes 2 x 512 bytes.
__global__ __launch_bounds__(256) void k_area2x2_c4(RArgs a, int gpr) {
    const int lane = threadIdx.x & 63;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int total = gpr * a.dh;
    const uint8_t* S = a.src + (long long)blockIdx.y * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.y * a.dst_stride;
    uint32_t r0[2][4], r1[2][4];
    int gx[2], dy[2];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int gid = (gw * 2 + j) * 64 + lane;
        dy[j] = gid / gpr;
        gx[j] = gid - dy[j] * gpr;
        if (gid >= total) dy[j] = -1;
        if (dy[j] >= 0) {
            const uint8_t* row = S + (size_t)(2 * dy[j]) * a.sstep + (size_t)gx[j] * 16;
            load_stream<4>(r0[j], row);
            load_stream<4>(r1[j], row + a.sstep);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
        if (dy[j] >= 0) {
            typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));
            const u32x2_t o = {box4_swar(r0[j][0], r0[j][1], r1[j][0], r1[j][1]), box4_swar(r0[j][2], r0[j][3], r1[j][2], r1[j][3])};
            __builtin_nontemporal_store(o, (u32x2_t*)(D + (size_t)dy[j] * a.dstep + (size_t)gx[j] * 8));
        }
}

// The same for 3-channel frames (every JPEG), any ISX in 2..8 -- 2 x 2 keeps k_area2x2_v3's integer rounding -- and for
// the BGRA widths whose box rows no 16-byte granule respects (3, 5, 6, 7).  The work is split the other way round: a wave
// takes a run of P destination pixels of one row (P * CN * ISX <= 4096 source bytes, P a multiple of 4), reads the ISY source
// rows of that run as contiguous 16-byte granules and adds them up BYTE COLUMN by byte column (two columns per 32-bit
// add in 16-bit halves), parks the 16-bit column sums in a wave-private LDS line, and then every lane gathers the
// ISX x CN columns of four destination pixels from that line: box sums are exact integers whatever the order.
#define BOXL_LINE 2048     // dwords of a wave's LDS line: 4096 byte columns x 16 bit
template <int CN, int ISX>     // gw = the wave's run (wave-uniform), cols = the wave's LDS line
__device__ __forceinline__ void area_boxl_body(const RArgs& a, int isy, int P, int cpr, float scale, int gw, unsigned frame, uint32_t* cols) {
    const int lane = threadIdx.x & 63;
    if (gw >= cpr * a.dh) return;
    const int dy = gw / cpr, d0 = (gw - dy * cpr) * P;
    const int np = min(P, a.dw - d0);                            // destination pixels of this run
    const int nbytes = np * CN * ISX;                             // source bytes per row
    const int ndw = (nbytes + 3) >> 2;                           // ... in dwords (rows are 4-byte aligned and padded)
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)(dy * isy) * a.sstep + (size_t)d0 * CN * ISX;
    const uint32_t M = 0x00ff00ffu;
    uint32_t e[4][4], o[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int t = 0; t < 4; t++) e[j][t] = o[j][t] = 0;
    for (int ky = 0; ky < isy; ky++) {
        const uint8_t* row = S + (size_t)ky * a.sstep;
        uint32_t p[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int w0 = (j * 64 + lane) * 4;                  // first dword of this lane's granule
            if (w0 + 4 <= ndw) load_stream<4>(p[j], row + (size_t)w0 * 4);
            else {
#pragma unroll
                for (int t = 0; t < 4; t++) p[j][t] = w0 + t < ndw ? *(const uint32_t*)(row + (size_t)(w0 + t) * 4) : 0u;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int t = 0; t < 4; t++) { e[j][t] += p[j][t] & M; o[j][t] += (p[j][t] >> 8) & M; }
    }
    asm volatile("" ::: "memory");
#pragma unroll
    for (int j = 0; j < 4; j++) {                                // byte column c of the run -> 16-bit slot c of the line
        typedef unsigned int u32x4a_t __attribute__((ext_vector_type(4), aligned(16)));
        const int g = j * 64 + lane;
        const u32x4a_t lo = {(e[j][0] & 0xffffu) | (o[j][0] << 16), (e[j][0] >> 16) | (o[j][0] & 0xffff0000u),
                             (e[j][1] & 0xffffu) | (o[j][1] << 16), (e[j][1] >> 16) | (o[j][1] & 0xffff0000u)};
        const u32x4a_t hi = {(e[j][2] & 0xffffu) | (o[j][2] << 16), (e[j][2] >> 16) | (o[j][2] & 0xffff0000u),
                             (e[j][3] & 0xffffu) | (o[j][3] << 16), (e[j][3] >> 16) | (o[j][3] & 0xffff0000u)};
        *(u32x4a_t*)(cols + g * 8) = lo;
        *(u32x4a_t*)(cols + g * 8 + 4) = hi;
    }
    asm volatile("" ::: "memory");
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dy * a.dstep + (size_t)d0 * CN;
    for (int q = lane; q * 4 < np; q += 64) {                    // four destination pixels = 4 * CN * ISX columns, two per dword
        uint32_t r[2 * CN * ISX];
        typedef unsigned int u32x2a_t __attribute__((ext_vector_type(2), aligned(8)));
#pragma unroll
        for (int i = 0; i < CN * ISX; i++) {
            const u32x2a_t v = *(const u32x2a_t*)(cols + q * 2 * CN * ISX + 2 * i);
            r[2 * i] = v.x; r[2 * i + 1] = v.y;
        }
        uint32_t out[CN] = {};
#pragma unroll
        for (int pp = 0; pp < 4; pp++)
#pragma unroll
            for (int c = 0; c < CN; c++) {
                uint32_t sum = 0;
#pragma unroll
                for (int k = 0; k < ISX; k++) {
                    const int i = (pp * ISX + k) * CN + c;           // 16-bit slot inside r
                    sum += (i & 1) ? (r[i >> 1] >> 16) : (r[i >> 1] & 0xffffu);
                }
                const int ob = pp * CN + c;
                out[ob >> 2] = cvt_pk_u8(__fmul_rn((float)sum, scale), out[ob >> 2], ob & 3);
            }
        uint8_t* dq = D + (size_t)q * 4 * CN;
        if (q * 4 + 4 <= np) {
            typedef unsigned int u32xn_t __attribute__((ext_vector_type(CN), aligned(4)));
            u32xn_t ov;
#pragma unroll
            for (int i = 0; i < CN; i++) ov[i] = out[i];
            *(u32xn_t*)dq = ov;
        } else {
            for (int bidx = 0; bidx < (np - q * 4) * CN; bidx++) dq[bidx] = (uint8_t)(out[bidx >> 2] >> (8 * (bidx & 3)));
        }
    }
}

template <int CN, int ISX>
__global__ __launch_bounds__(256) void k_area_boxl(RArgs a, int isy, int P, int cpr, float scale) {
    __shared__ __attribute__((aligned(16))) uint32_t s_cols[4][BOXL_LINE];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    area_boxl_body<CN, ISX>(a, isy, P, cpr, scale, blockIdx.x * 4 + wv, blockIdx.y, s_cols[wv]);
}

// ------------------------------------------------------------------ AREA, general (float tables)
struct AreaDev {
    const int *xstart, *xcount, *xaoff; const float* xalpha;
    const int *ystart, *ycount, *yaoff; const float* yalpha;
};
#define AREA_ROWS 4

template <int CN>
__global__ __launch_bounds__(256) void k_resize_area(RArgs a, AreaDev t) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;      // (64-bit: a 2^30-pixel frame times a block size)
    if (idx >= (long long)a.dw * a.dh) return;
    const int dy = (int)(idx / a.dw), dx = (int)(idx - (long long)dy * a.dw);
    const uint8_t* S = a.src + (long long)blockIdx.y * a.src_stride;
    const int xs = t.xstart[dx], nx = t.xcount[dx];
    const float* xa = t.xalpha + t.xaoff[dx];
    const int ys = t.ystart[dy], ny = t.ycount[dy];
    const float* ya = t.yalpha + t.yaoff[dy];
    float sum[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) sum[c] = 0.f;
    for (int j = 0; j < ny; j++) {
        const uint8_t* row = S + (size_t)(ys + j) * a.sstep + (size_t)xs * CN;
        float buf[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) buf[c] = 0.f;
        for (int k = 0; k < nx; k++) {
            const float al = xa[k];
            if (CN == 4) {
                const uint32_t p = *(const uint32_t*)(row + k * 4);
                buf[0] = __fadd_rn(buf[0], __fmul_rn((float)(p & 0xff), al));
                buf[1] = __fadd_rn(buf[1], __fmul_rn((float)((p >> 8) & 0xff), al));
                buf[2] = __fadd_rn(buf[2], __fmul_rn((float)((p >> 16) & 0xff), al));
                buf[3] = __fadd_rn(buf[3], __fmul_rn((float)(p >> 24), al));
            } else {
#pragma unroll
                for (int c = 0; c < CN; c++) buf[c] = __fadd_rn(buf[c], __fmul_rn((float)row[k * CN + c], al));
            }
        }
        const float be = ya[j];
#pragma unroll
        for (int c = 0; c < CN; c++)
            sum[c] = (j == 0) ? __fmul_rn(be, buf[c]) : __fadd_rn(sum[c], __fmul_rn(be, buf[c]));
    }
    uint8_t* d = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)dy * a.dstep + (size_t)dx * CN;
    int out[CN];
#pragma unroll
    for (int c = 0; c < CN; c++) out[c] = sat_u8(__float2int_rn(sum[c]));
    if (CN == 4) *(uint32_t*)d = (uint32_t)out[0] | ((uint32_t)out[1] << 8) | ((uint32_t)out[2] << 16) | ((uint32_t)out[3] << 24);
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) d[c] = (uint8_t)out[c];
    }
}

// ------------------------------------------------------------------ AREA, general, weights computed in the kernel
// computeResizeAreaTab's cell arithmetic (imp_tables.cpp build_area_axis, the same doubles in the same order, IEEE
// divide, contraction off) evaluated by each lane for its own destination column and its group of AREA_ROWS rows:
// no per-geometry table, so nothing to build on the host, upload or cache when every request has its own size
// (BASELINE configs[4]).  The float sequence is resizeArea_'s, with zero weights
// where a source pixel does not belong to a cell.
struct AreaCell {                                      // one destination cell along one axis
    int s1, s2;                                        // whole source pixels [s1, s2)
    float af, am, al;                                  // weights of pixel s1 - 1 (if hf), of the whole ones, of pixel s2 (if hl)
    bool hf, hl;
    __device__ __forceinline__ float weight(int sp) const {
        float w = (sp >= s1 && sp < s2) ? am : 0.f;
        w = (hf && sp == s1 - 1) ? af : w;
        return (hl && sp == s2) ? al : w;
    }
    __device__ __forceinline__ int first() const { return hf ? s1 - 1 : ((s1 < s2 || hl) ? s1 : 0); }   // s1 == s2 when only hl
    __device__ __forceinline__ int end() const { return hl ? s2 + 1 : s2; }
};
__device__ __forceinline__ AreaCell area_cell(int d, int ssize, double scale) {
    AreaCell c;
    const double f1 = d * scale, f2 = f1 + scale;
    const double cell = fmin(scale, ssize - f1);
    int s1 = (int)ceil(f1), s2 = (int)floor(f2);
    if (s2 > ssize - 1) s2 = ssize - 1;
    if (s1 > s2) s1 = s2;
    c.s1 = s1; c.s2 = s2;
    c.hf = s1 - f1 > 1e-3;
    c.af = (float)((s1 - f1) / cell);
    c.am = (float)(1.0 / cell);
    c.hl = f2 - s2 > 1e-3;
    c.al = (float)(fmin(fmin(f2 - s2, 1.), cell) / cell);
    return c;
}

struct AreaGeom { double scale_x, scale_y; };

template <int CN, int NV, int R>
__device__ __forceinline__ void area_cells_body(const RArgs& a, const AreaGeom& gm, int frame, int blk) {
    const int ng = (a.dh + R - 1) / R;
    const int idx = blk * 256 + threadIdx.x;
    if (idx >= a.dw * ng) return;
    const int g = idx / a.dw, dx = idx - g * a.dw;
    const uint8_t* S = a.src + (long long)frame * a.src_stride;
    // this lane's column: a window of 4*NV pixels that holds the whole cell, clamped so it never leaves the row
    const AreaCell cx = area_cell(dx, a.sw, gm.scale_x);
    const int xs = min(cx.first(), a.sw - 4 * NV);
    float al[NV * 4];
#pragma unroll
    for (int k = 0; k < NV * 4; k++) al[k] = cx.weight(xs + k);
    AreaCell cy[R];
    int jend = 0;
#pragma unroll
    for (int k = 0; k < R; k++) {
        const int dy = min(g * R + k, a.dh - 1);
        cy[k] = area_cell(dy, a.sh, gm.scale_y);
        if (g * R + k >= a.dh) { cy[k].s1 = cy[k].s2 = -8; cy[k].hf = cy[k].hl = false; }      // no source row has weight in it
        else jend = max(jend, cy[k].end());
    }
    const int ys = cy[0].first();
    float acc[R][CN];
#pragma unroll
    for (int k = 0; k < R; k++)
#pragma unroll
        for (int c = 0; c < CN; c++) acc[k][c] = 0.f;
    for (int sy = ys; sy < jend; sy++) {
        float b[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) b[c] = 0.f;
        if constexpr (CN == 4) {
            const uint8_t* row = S + (size_t)sy * a.sstep + (size_t)xs * 4;
            uint32_t px[NV * 4];
            __builtin_memcpy(px, __builtin_assume_aligned(row, 4), NV * 16);
#pragma unroll
            for (int k = 0; k < NV * 4; k++) {
                b[0] = __fadd_rn(b[0], __fmul_rn((float)(px[k] & 0xff), al[k]));
                b[1] = __fadd_rn(b[1], __fmul_rn((float)((px[k] >> 8) & 0xff), al[k]));
                b[2] = __fadd_rn(b[2], __fmul_rn((float)((px[k] >> 16) & 0xff), al[k]));
                b[3] = __fadd_rn(b[3], __fmul_rn((float)(px[k] >> 24), al[k]));
            }
        } else {
            const uint8_t* row = S + (size_t)sy * a.sstep + (size_t)xs * 3;
            uint32_t w[NV * 3];
            load_bytes_aligned<NV * 3>(w, row);
#pragma unroll
            for (int k = 0; k < NV * 4; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int o = 3 * k + c;
                    b[c] = __fadd_rn(b[c], __fmul_rn((float)((w[o >> 2] >> (8 * (o & 3))) & 0xff), al[k]));
                }
        }
#pragma unroll
        for (int k = 0; k < R; k++) {
            const float be = cy[k].weight(sy);
#pragma unroll
            for (int c = 0; c < CN; c++) acc[k][c] = __fadd_rn(acc[k][c], __fmul_rn(be, b[c]));
        }
    }
    uint8_t* d = a.dst + (long long)frame * a.dst_stride + (size_t)(g * R) * a.dstep + (size_t)dx * CN;
#pragma unroll
    for (int k = 0; k < R; k++)
        if (g * R + k < a.dh) {
            uint8_t* q = d + (size_t)k * a.dstep;
            if constexpr (CN == 4)
                *(uint32_t*)q = (uint32_t)sat_u8(__float2int_rn(acc[k][0])) | ((uint32_t)sat_u8(__float2int_rn(acc[k][1])) << 8) |
                                ((uint32_t)sat_u8(__float2int_rn(acc[k][2])) << 16) | ((uint32_t)sat_u8(__float2int_rn(acc[k][3])) << 24);
            else {
#pragma unroll
                for (int c = 0; c < CN; c++) q[c] = (uint8_t)sat_u8(__float2int_rn(acc[k][c]));
            }
        }
}

template <int CN, int NV, int R>
__global__ __launch_bounds__(256) void k_resize_area_cells(RArgs a, AreaGeom gm, int bpf, int count) {
    int frame, blk;
    if (frame_block(bpf, count, &frame, &blk)) area_cells_body<CN, NV, R>(a, gm, frame, blk);
}

// ------------------------------------------------------------------ AREA, general, rows streamed through LDS (BGRA)
// resizeArea_'s own shape: walk the source rows once, reduce each horizontally into the destination columns, add the
// result into the destination row(s) it belongs to.  A WAVE owns 64 destination columns and a band of destination rows:
//   * it fetches its segment of a source row with CONTIGUOUS 16-byte loads (lane l takes granule l, l + 64, ...: 1 KB per
//     instruction, like a copy) one row ahead of the arithmetic, and parks the row in a wave-private LDS line -- no
//     barrier anywhere, a wave's LDS operations execute in order;
//   * every lane then reads ITS cell's window (4*NV pixels, weights in registers, zero where the window is wider than the
//     cell) from that line: the same float sequence as k_resize_area_cells, fed from LDS instead of lane-strided global
//     loads (which fetched every 128-byte line through up to nine different instructions);
//   * the vertical cell is the same for the whole wave, so the row walk is scalar control flow: a source row shared by
//     two destination rows is reduced once and added to both, a finished row is stored as 256 contiguous bytes.
// Source rows are read once per band (+ one shared row per band boundary), never re-read across lanes.
// What happens to a finished pixel: the Filter("rotate") and Watermark steps that follow Resize in a request
// (bridge.c:606-640) ride on the store -- the resized frame is a few hundred KB, so where its pixels land costs nothing
// next to the source walk, and the intermediate frames never exist.  rot = 0 / 90 / 180 / 270 (filters.c:111-133).
constexpr int MIX_NV = 5;                              // windows of up to 20 source columns: shrinks up to 18x (3840 -> 224 is 17.1x)
struct AreaTail { int rot; OverlayArgs wm; };
template <int CN = 4>      // channels of the frame the overlay lands on; the overlay itself is BGRA
__device__ __forceinline__ uint32_t overlay_px(const OverlayArgs& wm, uint32_t px, int row, int col) {
    if (wm.ov && row >= wm.ry && row < wm.ry + wm.maxrow && col >= wm.rx && col < wm.rx + wm.maxcol) {
        const uint32_t o = *(const uint32_t*)(wm.ov + (size_t)(row - wm.ry) * wm.ostep + (size_t)(col - wm.rx) * 4);
        px = CN == 4 ? blend_over_bgra(px, o, wm.alpha) : blend_over_bgr(px, o, wm.alpha);
    }
    return px;
}
__device__ __forceinline__ void store_bgr(uint8_t* q, uint32_t px) { q[0] = (uint8_t)px; q[1] = (uint8_t)(px >> 8); q[2] = (uint8_t)(px >> 16); }

// PAPER: the tail may end in BlendWithPaper (`flat`, BGRA only), after the overlay -- compiled in for the mixed tail kernel
// alone, so the other kernels that share this body keep their code.
template <int CN, int W, bool PAPER = false>
__device__ __forceinline__ void area_rows_body(const RArgs& a, const AreaGeom& gm, int frame, int item, int nstrips, int bh,
                                               uint32_t* __restrict__ line, const AreaTail& tail, uint32_t* __restrict__ tile,
                                               bool flat = false) {
    static_assert(CN == 3 || CN == 4, "interleaved BGR / BGRA");
    constexpr int NV = (W + 3) / 4;                              // 16-byte granules a lane fetches per source row
    const int lane = threadIdx.x & 63;
    const int band = item / nstrips, strip = item - band * nstrips;
    const int dy0 = band * bh;
    if (dy0 >= a.dh) return;
    const int dy1 = min(dy0 + bh, a.dh);
    const bool live = strip * 64 + lane < a.dw;
    const int dx = min(strip * 64 + lane, a.dw - 1);             // idle lanes shadow the last column
    const AreaCell cx = area_cell(dx, a.sw, gm.scale_x);
    const int xs = min(cx.first(), a.sw - W);
    float al[W];
#pragma unroll
    for (int k = 0; k < W; k++) al[k] = cx.weight(xs + k);
    // the wave's segment, in BYTES of the source row (rows are 4-byte aligned): from lane 0's window, rounded down to a
    // 16-byte granule, to the end of lane 63's
    // (a segment that starts inside the row's last 16 bytes starts a granule early, so the moved-back granule below never
    // lands in front of the line; the launcher guarantees rows of at least 16 bytes)
    const int row_end = (a.sw * CN + 3) & ~3;
    const int b0 = min((__builtin_amdgcn_readlane(xs, 0) * CN) & ~15, (row_end - 16) & ~15);
    const int ngran = ((__builtin_amdgcn_readlane(xs, 63) + W) * CN - b0 + 15) >> 4;  // <= 64 * NV (area_rows_plan)
    const int wofs = xs * CN - b0;                               // this lane's window in the parked line, in bytes
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)b0;
    // Every lane fetches a granule and parks it, with no predication: lanes past the segment repeat its last granule
    // (same address, same LDS slot, same data).  When the last granule would leave the row's padded end it is moved back
    // to end exactly there and parked dword by dword where those bytes belong (wave-uniform branch).
    const bool ragged = b0 + 16 * ngran > row_end;
    int gofs[NV], lofs[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int gi = min(j * 64 + lane, ngran - 1);
        gofs[j] = (ragged && gi == ngran - 1) ? row_end - 16 - b0 : gi * 16;
        lofs[j] = gofs[j] >> 2;
    }
    uint32_t nxt[NV][4];
    auto fetch = [&](int sy) {
        const uint8_t* row = S + (size_t)sy * a.sstep;
#pragma unroll
        for (int j = 0; j < NV; j++) load_stream<4>(nxt[j], row + gofs[j]);
    };
    float b[CN];
    auto reduce = [&]() {                                        // park the fetched row
        asm volatile("" ::: "memory");
        if (!ragged) {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                typedef unsigned int u32x4a_t __attribute__((ext_vector_type(4), aligned(16)));
                const u32x4a_t q = {nxt[j][0], nxt[j][1], nxt[j][2], nxt[j][3]};
                *(u32x4a_t*)(line + lofs[j]) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; j++)
#pragma unroll
                for (int t = 0; t < 4; t++) line[lofs[j] + t] = nxt[j][t];
        }
        asm volatile("" ::: "memory");
    };
    auto hsum = [&]() {
#pragma unroll
        for (int c = 0; c < CN; c++) b[c] = 0.f;
        if constexpr (CN == 4) {
            const uint32_t* win = line + (wofs >> 2);
#pragma unroll
            for (int k = 0; k < W; k++) {
                const uint32_t px = win[k];
                b[0] = __fadd_rn(b[0], __fmul_rn((float)(px & 0xff), al[k]));
                b[1] = __fadd_rn(b[1], __fmul_rn((float)((px >> 8) & 0xff), al[k]));
                b[2] = __fadd_rn(b[2], __fmul_rn((float)((px >> 16) & 0xff), al[k]));
                b[3] = __fadd_rn(b[3], __fmul_rn((float)(px >> 24), al[k]));
            }
        } else {
            // 3 W bytes at a byte offset: aligned dwords + v_alignbyte_b32, then every (pixel, channel) is a compile-time byte
            constexpr int ND = (3 * W + 3) / 4;
            const uint32_t* win = line + (wofs >> 2);
            const unsigned sh = (unsigned)wofs & 3u;
            uint32_t t[ND + 1], w[ND];
#pragma unroll
            for (int i = 0; i <= ND; i++) t[i] = win[i];
#pragma unroll
            for (int i = 0; i < ND; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], sh);
#pragma unroll
            for (int k = 0; k < W; k++)
#pragma unroll
                for (int c = 0; c < 3; c++) {
                    const int o = 3 * k + c;
                    b[c] = __fadd_rn(b[c], __fmul_rn((float)((w[o >> 2] >> (8 * (o & 3))) & 0xff), al[k]));
                }
        }
        asm volatile("" ::: "memory");
    };

    // rows: lane k works out the vertical cell of the band's k-th destination row once (bh <= 64); the walk below reads
    // them back with v_readlane, so everything in it is the same in all lanes -> scalar registers, scalar branches
    const AreaCell mine = area_cell(min(dy0 + lane, dy1 - 1), a.sh, gm.scale_y);
    const int sy_end = __builtin_amdgcn_readlane(mine.end(), dy1 - 1 - dy0);
    uint8_t* D = a.dst + (long long)frame * a.dst_stride;
    const bool quarter = tail.rot == 90 || tail.rot == 270;     // (kernel argument: scalar)
    int cur = -1;                                                // the source row `b` holds
    for (int dy = dy0; dy < dy1; dy++) {
        const int r = dy - dy0;
        const int s1 = __builtin_amdgcn_readlane(mine.s1, r), s2 = __builtin_amdgcn_readlane(mine.s2, r);
        const int hf = __builtin_amdgcn_readlane((int)mine.hf, r), hl = __builtin_amdgcn_readlane((int)mine.hl, r);
        const float yaf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.af), r));
        const float yam = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.am), r));
        const float yal = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.al), r));
        const int first = hf ? s1 - 1 : s1, end = hl ? s2 + 1 : s2;      // (s1 == s2 when the cell is its last partial row alone)
        if (cur < 0) { fetch(first); cur = first - 1; }
        float acc[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) acc[c] = 0.f;
        for (int sy = first; sy < end; sy++) {
            while (cur < sy) {                                   // (cells are contiguous: this runs once, or not at all for a shared row)
                cur++;
                reduce();
                if (cur + 1 < sy_end) fetch(cur + 1);
                hsum();
            }
            const float be = (hf && sy == s1 - 1) ? yaf : ((hl && sy == s2) ? yal : yam);
#pragma unroll
            for (int c = 0; c < CN; c++) acc[c] = __fadd_rn(acc[c], __fmul_rn(be, b[c]));
        }
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) px = cvt_pk_u8(acc[c], px, c);
        if (quarter) tile[(dy - dy0) * 65 + lane] = px;          // leaves with the band, turned (below)
        else if (live) {
            // R[i][j] = H[rh-1-i][rw-1-j] (180); H = the resized frame, dw x dh
            const int orow = tail.rot == 180 ? a.dh - 1 - dy : dy, ocol = tail.rot == 180 ? a.dw - 1 - dx : dx;
            uint32_t o = overlay_px<CN>(tail.wm, px, orow, ocol);
            if constexpr (PAPER && CN == 4) o = flat ? blend_paper_bgra(o) : o;
            if constexpr (CN == 4) *(uint32_t*)(D + (size_t)orow * a.dstep + (size_t)ocol * 4) = o;
            else store_bgr(D + (size_t)orow * a.dstep + (size_t)ocol * 3, o);
        }
    }
    if (quarter) {
        // R[i][j] = H[rh-1-j][i] (90), H[j][rw-1-i] (270): a destination row takes this band's pixels of ONE column, a
        // contiguous run of dy1 - dy0 pixels -- written 16 bytes per lane, four lanes per run of 16, once per band (a
        // scattered store per finished row would sit in front of every later source-row wait: one vmcnt for both)
        asm volatile("" ::: "memory");
        const int nb = dy1 - dy0, nq = (nb + 3) >> 2;
        const int ncol = min(64, a.dw - strip * 64);
        const int j0 = tail.rot == 90 ? a.dh - dy1 : dy0;        // first destination column of the run
        for (int t = lane; t < ncol * nq; t += 64) {
            const int col = t / nq, qi = t - col * nq;
            const int hx = strip * 64 + col;
            const int orow = tail.rot == 90 ? hx : a.dw - 1 - hx;
            uint32_t v[4];
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int k = 4 * qi + jj;                       // k-th pixel of the run
                const int r = tail.rot == 90 ? nb - 1 - k : k;   // band row it comes from
                v[jj] = overlay_px<CN>(tail.wm, tile[min(max(r, 0), nb - 1) * 65 + col], orow, j0 + k);
                if constexpr (PAPER && CN == 4) v[jj] = flat ? blend_paper_bgra(v[jj]) : v[jj];
            }
            uint8_t* q = D + (size_t)orow * a.dstep + (size_t)(j0 + 4 * qi) * CN;
            if constexpr (CN == 3) {                              // (a run of BGR pixels starts at any byte: byte stores)
                for (int jj = 0; jj < 4 && 4 * qi + jj < nb; jj++) store_bgr(q + 3 * jj, v[jj]);
            } else if (4 * qi + 4 <= nb) {
                const u32x4_t o4 = {v[0], v[1], v[2], v[3]};
                *(u32x4_t*)q = o4;
            } else {
                for (int jj = 0; 4 * qi + jj < nb; jj++) *(uint32_t*)(q + 4 * jj) = v[jj];
            }
        }
    }
}

template <int CN, int W>
__global__ __launch_bounds__(256) void k_resize_area_rows(RArgs a, AreaGeom gm, int nstrips, int bh, int nitems, int bpf, int count, AreaTail tail) {
    __shared__ __attribute__((aligned(16))) uint32_t s_line[4][64 * ((W + 3) / 4) * 4 + 4];      // + 4: a BGR window's look-ahead dword at the line's very end stays inside it
    __shared__ uint32_t s_tile[4][16 * 65];                      // quarter turns: a band (<= 16 rows) waits here to leave turned
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * 4 + wv;
    if (item < nitems) area_rows_body<CN, W>(a, gm, frame, item, nstrips, bh, s_line[wv], tail, s_tile[wv]);
}

// Small shrink factors (windows of at most 5 pixels: factors below ~3.9): 64 destination columns are only 64 * factor
// source pixels -- a few hundred bytes per wave and row, and the per-row work around the arithmetic (fetch, park, loop)
// shows (1.3x: 0.40 of the roofline).  Here a lane owns FOUR adjacent destination columns, a wave 256: the same walk, four
// windows per lane out of a segment four times as long, one 16-byte (BGRA) / 12-byte (BGR) store per lane and finished row.
template <int CN, int W>
__device__ __forceinline__ void area_rows4_body(const RArgs& a, const AreaGeom& gm, int frame, int item, int nstrips, int bh,
                                                uint32_t* __restrict__ line) {
    static_assert((CN == 3 || CN == 4) && W <= 5, "small windows only");
    constexpr int NV = 4;                                        // 64 * 4 granules hold 255 * 3.9 + W + 8 pixels
    const int lane = threadIdx.x & 63;
    const int band = item / nstrips, strip = item - band * nstrips;
    const int dy0 = band * bh;
    if (dy0 >= a.dh) return;
    const int dy1 = min(dy0 + bh, a.dh);
    const int dxf = strip * 256 + lane * 4;                      // this lane's first column
    int xs[4], wofs[4];
    float al[4][W];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const AreaCell cx = area_cell(min(dxf + p, a.dw - 1), a.sw, gm.scale_x);   // idle columns shadow the last one
        xs[p] = min(cx.first(), a.sw - W);
#pragma unroll
        for (int k = 0; k < W; k++) al[p][k] = cx.weight(xs[p] + k);
    }
    const int row_end = (a.sw * CN + 3) & ~3;
    const int b0 = min((__builtin_amdgcn_readlane(xs[0], 0) * CN) & ~15, (row_end - 16) & ~15);
    const int ngran = ((__builtin_amdgcn_readlane(xs[3], 63) + W) * CN - b0 + 15) >> 4;   // <= 256 (area_rows_plan)
#pragma unroll
    for (int p = 0; p < 4; p++) wofs[p] = xs[p] * CN - b0;
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)b0;
    const bool ragged = b0 + 16 * ngran > row_end;
    int gofs[NV], lofs[NV];
#pragma unroll
    for (int j = 0; j < NV; j++) {
        const int gi = min(j * 64 + lane, ngran - 1);
        gofs[j] = (ragged && gi == ngran - 1) ? row_end - 16 - b0 : gi * 16;
        lofs[j] = gofs[j] >> 2;
    }
    uint32_t nxt[NV][4];
    auto fetch = [&](int sy) {
        const uint8_t* row = S + (size_t)sy * a.sstep;
#pragma unroll
        for (int j = 0; j < NV; j++) load_stream<4>(nxt[j], row + gofs[j]);
    };
    float b[4][CN];
    auto reduce = [&]() {
        asm volatile("" ::: "memory");
        if (!ragged) {
#pragma unroll
            for (int j = 0; j < NV; j++) {
                typedef unsigned int u32x4a_t __attribute__((ext_vector_type(4), aligned(16)));
                const u32x4a_t q = {nxt[j][0], nxt[j][1], nxt[j][2], nxt[j][3]};
                *(u32x4a_t*)(line + lofs[j]) = q;
            }
        } else {
#pragma unroll
            for (int j = 0; j < NV; j++)
#pragma unroll
                for (int t = 0; t < 4; t++) line[lofs[j] + t] = nxt[j][t];
        }
        asm volatile("" ::: "memory");
    };
    auto hsum = [&]() {
#pragma unroll
        for (int p = 0; p < 4; p++) {
#pragma unroll
            for (int c = 0; c < CN; c++) b[p][c] = 0.f;
            const uint32_t* win = line + (wofs[p] >> 2);
            if constexpr (CN == 4) {
#pragma unroll
                for (int k = 0; k < W; k++) {
                    const uint32_t px = win[k];
                    b[p][0] = __fadd_rn(b[p][0], __fmul_rn((float)(px & 0xff), al[p][k]));
                    b[p][1] = __fadd_rn(b[p][1], __fmul_rn((float)((px >> 8) & 0xff), al[p][k]));
                    b[p][2] = __fadd_rn(b[p][2], __fmul_rn((float)((px >> 16) & 0xff), al[p][k]));
                    b[p][3] = __fadd_rn(b[p][3], __fmul_rn((float)(px >> 24), al[p][k]));
                }
            } else {
                constexpr int ND = (3 * W + 3) / 4;
                const unsigned sh = (unsigned)wofs[p] & 3u;
                uint32_t t[ND + 1], w[ND];
#pragma unroll
                for (int i = 0; i <= ND; i++) t[i] = win[i];
#pragma unroll
                for (int i = 0; i < ND; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], sh);
#pragma unroll
                for (int k = 0; k < W; k++)
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int o = 3 * k + c;
                        b[p][c] = __fadd_rn(b[p][c], __fmul_rn((float)((w[o >> 2] >> (8 * (o & 3))) & 0xff), al[p][k]));
                    }
            }
        }
        asm volatile("" ::: "memory");
    };
    const AreaCell mine = area_cell(min(dy0 + lane, dy1 - 1), a.sh, gm.scale_y);
    const int sy_end = __builtin_amdgcn_readlane(mine.end(), dy1 - 1 - dy0);
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dxf * CN;
    const int nlive = min(4, a.dw - dxf);                        // columns of this lane inside the frame (<= 0: none)
    int cur = -1;
    for (int dy = dy0; dy < dy1; dy++) {
        const int r = dy - dy0;
        const int s1 = __builtin_amdgcn_readlane(mine.s1, r), s2 = __builtin_amdgcn_readlane(mine.s2, r);
        const int hf = __builtin_amdgcn_readlane((int)mine.hf, r), hl = __builtin_amdgcn_readlane((int)mine.hl, r);
        const float yaf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.af), r));
        const float yam = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.am), r));
        const float yal = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.al), r));
        const int first = hf ? s1 - 1 : s1, end = hl ? s2 + 1 : s2;
        if (cur < 0) { fetch(first); cur = first - 1; }
        float acc[4][CN];
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int c = 0; c < CN; c++) acc[p][c] = 0.f;
        for (int sy = first; sy < end; sy++) {
            while (cur < sy) {
                cur++;
                reduce();
                if (cur + 1 < sy_end) fetch(cur + 1);
                hsum();
            }
            const float be = (hf && sy == s1 - 1) ? yaf : ((hl && sy == s2) ? yal : yam);
#pragma unroll
            for (int p = 0; p < 4; p++)
#pragma unroll
                for (int c = 0; c < CN; c++) acc[p][c] = __fadd_rn(acc[p][c], __fmul_rn(be, b[p][c]));
        }
        uint32_t out[CN] = {};
#pragma unroll
        for (int p = 0; p < 4; p++)
#pragma unroll
            for (int c = 0; c < CN; c++) {
                const int ob = p * CN + c;
                out[ob >> 2] = cvt_pk_u8(acc[p][c], out[ob >> 2], ob & 3);
            }
        uint8_t* q = D + (size_t)dy * a.dstep;
        if (nlive == 4 && !(((uintptr_t)q) & 3)) {
            typedef unsigned int u32xn_t __attribute__((ext_vector_type(CN), aligned(4)));
            u32xn_t ov;
#pragma unroll
            for (int i = 0; i < CN; i++) ov[i] = out[i];
            *(u32xn_t*)q = ov;
        } else {
            for (int bidx = 0; bidx < nlive * CN; bidx++) q[bidx] = (uint8_t)(out[bidx >> 2] >> (8 * (bidx & 3)));
        }
    }
}

template <int CN, int W>
__global__ __launch_bounds__(256) void k_resize_area_rows4(RArgs a, AreaGeom gm, int nstrips, int bh, int nitems, int bpf, int count) {
    __shared__ __attribute__((aligned(16))) uint32_t s_line[4][64 * 4 * 4 + 4];
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * 4 + wv;
    if (item < nitems) area_rows4_body<CN, W>(a, gm, frame, item, nstrips, bh, s_line[wv]);
}

// Cells wider than 20 source columns (shrinks past 18x: a 4032-wide photo at 200 and below): area_rows_body's walk with the
// window W a RUNTIME argument (the widest horizontal cell, 21..66).  What that changes:
//   * the weights are not held in registers: the horizontal reduction is a loop over the window, four pixels a turn, and
//     every weight is picked from the cell's first / whole / last split as it is used (zero where the window is wider
//     than the cell, and for the up to three pixels a turn of four reaches past the window);
//   * the wave's segment of a source row is 63 * scale_x + W pixels, up to 16.5 KB: the LDS line is dynamic shared memory
//     sized by the launcher (area_wide_plan), and a row comes in WIDE_PIECE granules per lane at a time -- the first piece
//     one row ahead of the arithmetic, as there, the rest (segments over 4 KB) when the row is parked;
//   * no tail: a finished row leaves as it is.
// The float sequence is resizeArea_'s, as in every body above.  `line_dw` = the line's length in dwords.
// Two ways to fetch a row (COVER, wave-uniform, area_wide_plan's verdict):
//   * aligned (BGRA; BGR whose pointer and pitch are 4-byte aligned): granules counted from a.src, the last one moved
//     back when it would pass the row's padded end (`ragged`);
//   * covering (gray; BGR off the 4-byte grid): area_rows_gray_body's scheme, which asks nothing of the source -- the
//     16-byte granules, aligned by absolute address, that cover the wave's segment of the row, and the segment's offset
//     inside its first granule (`dl`, wave-uniform, different from row to row when the pitch is no multiple of 16) added
//     to every lane's window place.  An aligned granule that holds one byte of the frame never leaves the frame's pages,
//     so no granule is moved.  A row's granule count follows its `dl`.
constexpr int WIDE_W_MIN = 4 * MIX_NV + 1, WIDE_W_MAX = 66;   // cells of 21..66 columns: factors up to 64
constexpr int WIDE_PIECE = 4;                                  // 16-byte granules of a row a lane holds at a time
template <int CN, bool COVER>
__device__ __forceinline__ void area_wide_impl(const RArgs& a, const AreaGeom& gm, int frame, int item, int nstrips, int bh,
                                               int W, int line_dw, uint32_t* __restrict__ line) {
    static_assert(CN == 1 || CN == 3 || CN == 4, "gray, or interleaved BGR / BGRA");
    static_assert(CN != 1 || COVER, "gray rows are always fetched by covering granules");
    static_assert(CN != 4 || !COVER, "BGRA rows are always 4-byte aligned");
    const int lane = threadIdx.x & 63;
    const int band = item / nstrips, strip = item - band * nstrips;
    const int dy0 = band * bh;
    if (dy0 >= a.dh) return;
    const int dy1 = min(dy0 + bh, a.dh);
    const bool live = strip * 64 + lane < a.dw;
    const int dx = min(strip * 64 + lane, a.dw - 1);             // idle lanes shadow the last column
    const AreaCell cx = area_cell(dx, a.sw, gm.scale_x);
    const int xs = min(cx.first(), a.sw - W);                    // the window holds the whole cell and never leaves the row
    // the cell in window places: whole pixels at [k1, k2), the partial ones at kf and kl (-1: none) -- cx.weight(xs + k)
    const int k1 = cx.s1 - xs, k2 = cx.s2 - xs;
    const int kf = cx.hf ? k1 - 1 : -1, kl = cx.hl ? k2 : -1;
    auto weight = [&](int k) {
        float w = (k >= k1 && k < k2) ? cx.am : 0.f;
        w = k == kf ? cx.af : w;
        return k == kl ? cx.al : w;
    };
    // the wave's segment in bytes of the source row, as in area_rows_body; covering: from lane 0's window to the end of
    // lane 63's, wherever that lies (a window never leaves the row, so neither does the segment)
    const int row_end = (a.sw * CN + 3) & ~3;
    const int x0b = __builtin_amdgcn_readlane(xs, 0) * CN;
    const int b0 = COVER ? x0b : min(x0b & ~15, (row_end - 16) & ~15);
    const int seglen = (__builtin_amdgcn_readlane(xs, 63) + W) * CN - b0;
    int ngran = ((COVER ? 15 : 0) + seglen + 15) >> 4;           // covering: the most a row can need (dl = 15); each row's own below
    if (ngran * 4 + 4 > line_dw) return;                         // (never: area_wide_plan sizes the line for the longest segment)
    const int wrel = xs * CN - b0;                               // this lane's window in the segment, in bytes
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)b0;
    // Every lane fetches whole pieces and parks them, with no predication: lanes past the segment repeat its last granule.
    // Aligned: when the last granule would leave the row's padded end it is moved back to end exactly there and the row is
    // parked dword by dword (wave-uniform branch).
    const bool ragged = !COVER && b0 + 16 * ngran > row_end;
    auto gran_ofs = [&](int j) {                                 // byte offset of this lane's j-th granule in the line
        const int gi = min(j * 64 + lane, ngran - 1);
        return (ragged && gi == ngran - 1) ? row_end - 16 - b0 : gi * 16;
    };
    int gofs[WIDE_PIECE];
    if constexpr (!COVER) {
#pragma unroll
        for (int j = 0; j < WIDE_PIECE; j++) gofs[j] = gran_ofs(j);
    }
    uint32_t nxt[WIDE_PIECE][4];                                 // the first piece of the row ahead
    int dnxt = 0, dcur = 0;                                      // covering: `dl` of the row in flight / of the parked row
    auto fetch = [&](int sy) {
        const uint8_t* row = S + (size_t)sy * a.sstep;
        if constexpr (COVER) {                                   // this row's granules: `ngran` holds until the row is parked
            dnxt = __builtin_amdgcn_readfirstlane((int)((uintptr_t)row & 15));
            ngran = (dnxt + seglen + 15) >> 4;
            row -= dnxt;
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++) load_stream<4>(nxt[j], row + gran_ofs(j));
        } else {
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++) load_stream<4>(nxt[j], row + gofs[j]);
        }
    };
    auto park = [&](const uint32_t (*q)[4], const int* ofs) {
        if (!ragged) {
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++) {
                typedef unsigned int u32x4a_t __attribute__((ext_vector_type(4), aligned(16)));
                const u32x4a_t v = {q[j][0], q[j][1], q[j][2], q[j][3]};
                *(u32x4a_t*)(line + (ofs[j] >> 2)) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++)
#pragma unroll
                for (int t = 0; t < 4; t++) line[(ofs[j] >> 2) + t] = q[j][t];
        }
    };
    float b[CN];
    auto reduce = [&](int sy) {                                  // park row sy: its first piece is in `nxt`, the rest comes now
        asm volatile("" ::: "memory");
        if constexpr (COVER) {                                   // (worked out again: four registers fewer across the row sum)
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++) gofs[j] = gran_ofs(j);
        }
        park(nxt, gofs);
        dcur = dnxt;
        const uint8_t* row = S + (size_t)sy * a.sstep - dcur;
        const int npieces = (ngran + 64 * WIDE_PIECE - 1) / (64 * WIDE_PIECE);
        for (int p = 1; p < npieces; p++) {
            uint32_t more[WIDE_PIECE][4];
            int mofs[WIDE_PIECE];
#pragma unroll
            for (int j = 0; j < WIDE_PIECE; j++) {
                mofs[j] = gran_ofs(p * WIDE_PIECE + j);
                load_stream<4>(more[j], row + mofs[j]);
            }
            park(more, mofs);
        }
        asm volatile("" ::: "memory");
    };
    auto hsum = [&]() {
#pragma unroll
        for (int c = 0; c < CN; c++) b[c] = 0.f;
        const int wofs = wrel + dcur;                            // this lane's window in the parked line, in bytes
        if constexpr (CN == 1) {
            // four pixels = one dword at a byte offset: two aligned dwords + v_alignbyte_b32
            const uint32_t* win = line + (wofs >> 2);
            const unsigned sh = (unsigned)wofs & 3u;
            for (int k = 0; k < W; k += 4, win++) {
                const uint32_t w = __builtin_amdgcn_alignbyte(win[1], win[0], sh);
#pragma unroll
                for (int t = 0; t < 4; t++) b[0] = __fadd_rn(b[0], __fmul_rn((float)((w >> (8 * t)) & 0xff), weight(k + t)));
            }
        } else if constexpr (CN == 4) {
            const uint32_t* win = line + (wofs >> 2);
            for (int k = 0; k < W; k += 4) {
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const uint32_t px = win[k + t];
                    const float al = weight(k + t);
                    b[0] = __fadd_rn(b[0], __fmul_rn((float)(px & 0xff), al));
                    b[1] = __fadd_rn(b[1], __fmul_rn((float)((px >> 8) & 0xff), al));
                    b[2] = __fadd_rn(b[2], __fmul_rn((float)((px >> 16) & 0xff), al));
                    b[3] = __fadd_rn(b[3], __fmul_rn((float)(px >> 24), al));
                }
            }
        } else {
            // four pixels = 12 bytes at a byte offset: four aligned dwords + v_alignbyte_b32, every (pixel, channel) a compile-time byte
            const uint32_t* win = line + (wofs >> 2);
            const unsigned sh = (unsigned)wofs & 3u;
            for (int k = 0; k < W; k += 4, win += 3) {
                uint32_t w[3];
#pragma unroll
                for (int i = 0; i < 3; i++) w[i] = __builtin_amdgcn_alignbyte(win[i + 1], win[i], sh);
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const float al = weight(k + t);
#pragma unroll
                    for (int c = 0; c < 3; c++) {
                        const int o = 3 * t + c;
                        b[c] = __fadd_rn(b[c], __fmul_rn((float)((w[o >> 2] >> (8 * (o & 3))) & 0xff), al));
                    }
                }
            }
        }
        asm volatile("" ::: "memory");
    };

    // rows: as in area_rows_body -- lane k works out the vertical cell of the band's k-th destination row (bh <= 64), the
    // walk reads them back with v_readlane: scalar registers, scalar branches
    const AreaCell mine = area_cell(min(dy0 + lane, dy1 - 1), a.sh, gm.scale_y);
    const int sy_end = __builtin_amdgcn_readlane(mine.end(), dy1 - 1 - dy0);
    uint8_t* D = a.dst + (long long)frame * a.dst_stride + (size_t)dx * CN;
    int cur = -1;                                                // the source row `b` holds
    for (int dy = dy0; dy < dy1; dy++) {
        const int r = dy - dy0;
        const int s1 = __builtin_amdgcn_readlane(mine.s1, r), s2 = __builtin_amdgcn_readlane(mine.s2, r);
        const int hf = __builtin_amdgcn_readlane((int)mine.hf, r), hl = __builtin_amdgcn_readlane((int)mine.hl, r);
        const float yaf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.af), r));
        const float yam = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.am), r));
        const float yal = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.al), r));
        const int first = hf ? s1 - 1 : s1, end = hl ? s2 + 1 : s2;
        if (cur < 0) { fetch(first); cur = first - 1; }
        float acc[CN];
#pragma unroll
        for (int c = 0; c < CN; c++) acc[c] = 0.f;
        for (int sy = first; sy < end; sy++) {
            while (cur < sy) {                                   // (cells are contiguous: this runs once, or not at all for a shared row)
                cur++;
                reduce(cur);
                if (cur + 1 < sy_end) fetch(cur + 1);
                hsum();
            }
            const float be = (hf && sy == s1 - 1) ? yaf : ((hl && sy == s2) ? yal : yam);
#pragma unroll
            for (int c = 0; c < CN; c++) acc[c] = __fadd_rn(acc[c], __fmul_rn(be, b[c]));
        }
        uint32_t px = 0;
#pragma unroll
        for (int c = 0; c < CN; c++) px = cvt_pk_u8(acc[c], px, c);
        if (live) {
            if constexpr (CN == 4) *(uint32_t*)(D + (size_t)dy * a.dstep) = px;
            else if constexpr (CN == 3) store_bgr(D + (size_t)dy * a.dstep, px);
            else D[(size_t)dy * a.dstep] = (uint8_t)px;
        }
    }
}

// `W` = the window; negative: a BGR frame that needs the covering fetch (gray always takes it, BGRA never).
template <int CN>
__device__ __forceinline__ void area_wide_body(const RArgs& a, const AreaGeom& gm, int frame, int item, int nstrips, int bh,
                                               int W, int line_dw, uint32_t* __restrict__ line) {
    if constexpr (CN == 1) area_wide_impl<1, true>(a, gm, frame, item, nstrips, bh, W, line_dw, line);
    else if constexpr (CN == 4) area_wide_impl<4, false>(a, gm, frame, item, nstrips, bh, W, line_dw, line);
    else if (W < 0) area_wide_impl<3, true>(a, gm, frame, item, nstrips, bh, -W, line_dw, line);   // (wave-uniform: a scalar branch)
    else area_wide_impl<3, false>(a, gm, frame, item, nstrips, bh, W, line_dw, line);
}

// `wpb` = waves per block (4; 2 when four of the longest lines would not fit 64 KB): a wave per item, a line per wave.
template <int CN>
__global__ __launch_bounds__(256) void k_resize_area_wide(RArgs a, AreaGeom gm, int W, int line_dw, int wpb, int nstrips, int bh, int nitems,
                                                          int bpf, int count) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_wide[];
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * wpb + wv;
    if (item < nitems) area_wide_body<CN>(a, gm, frame, item, nstrips, bh, W, line_dw, s_wide + wv * line_dw);
}

// Gray frames (one byte a pixel): the same walk with windows counted in BYTES.  A lane owns P adjacent destination columns
// (P = 4 while the windows are at most five pixels, as above; P = 1 past that), a wave 64 * P.  Nothing is asked of the
// source: a crop window starts at any byte and a gray pitch is any number, so every source row is fetched as the ALIGNED
// 16-byte granules that cover the wave's segment of it -- contiguous, 1 KB per instruction, and an aligned granule that
// holds one byte of the frame never leaves the frame's pages -- and the segment's offset inside its first granule (`dl`,
// the same for the whole wave, different from row to row when the pitch is no multiple of 16) is added to every window's
// place in the parked line.  Windows are read as aligned dwords + v_alignbyte_b32, like the BGR body's.
// The launcher (gray_rows_plan) guarantees 64 * P lanes' windows plus the 30 bytes of granule rounding fit NV KB.
constexpr int GRAY_W_MAX = 4 * MIX_NV;                         // the widest window, as for colour
constexpr int gray_rows_nv(int w, int p) { return (64 * p * w + 30 + 1023) / 1024; }
constexpr int GRAY_NV_MAX = 2;                                 // gray_rows_nv(20, 1) = gray_rows_nv(5, 4)
template <int W, int P>
__device__ __forceinline__ void area_rows_gray_body(const RArgs& a, const AreaGeom& gm, int item, int nstrips, int bh,
                                                    uint32_t* __restrict__ line) {
    static_assert((P == 1 && W <= GRAY_W_MAX) || (P == 4 && W <= 5), "four columns per lane for small windows only");
    constexpr int NV = gray_rows_nv(W, P);                       // 16-byte granules a lane fetches per source row
    static_assert(NV <= GRAY_NV_MAX, "the line holds GRAY_NV_MAX KB");
    const int lane = threadIdx.x & 63;
    const int band = item / nstrips, strip = item - band * nstrips;
    const int dy0 = band * bh;
    if (dy0 >= a.dh) return;
    const int dy1 = min(dy0 + bh, a.dh);
    const int dxf = (strip * 64 + lane) * P;                     // this lane's first column
    int xs[P];
    float al[P][W];
#pragma unroll
    for (int p = 0; p < P; p++) {
        const AreaCell cx = area_cell(min(dxf + p, a.dw - 1), a.sw, gm.scale_x);   // idle columns shadow the last one
        xs[p] = max(min(cx.first(), a.sw - W), 0);               // (a row narrower than the window: the window hangs over its end)
#pragma unroll
        for (int k = 0; k < W; k++) al[p][k] = cx.weight(xs[p] + k);             // zero past the cell, so past the row too
    }
    // the wave's segment of a source row: from lane 0's first window to the end of lane 63's last, in bytes
    const int x0 = __builtin_amdgcn_readlane(xs[0], 0);
    const int seglen = __builtin_amdgcn_readlane(xs[P - 1], 63) + W - x0;          // + 30 <= 1024 * NV (gray_rows_plan)
    const int segrow = min(seglen, a.sw - x0);                   // what of it lies inside the row: only that is fetched
    int wrel[P];
#pragma unroll
    for (int p = 0; p < P; p++) wrel[p] = xs[p] - x0;
    const uint8_t* S = a.src + (size_t)x0;
    // Every lane fetches NV granules and parks them, with no predication: lanes past the segment repeat its last granule
    // (same address, same LDS slot, same data).
    uint32_t nxt[NV][4];
    int nofs[NV];                                                // where the fetched granules go in the line, in dwords
    int dnxt = 0, dcur = 0;                                      // `dl` of the row in flight / of the parked row
    auto fetch = [&](int sy) {
        const uint8_t* row = S + (size_t)sy * a.sstep;
        dnxt = (int)((uintptr_t)row & 15);
        const int ngran = (dnxt + segrow + 15) >> 4;             // (bytes of the line past it keep old values: weight zero)
        const uint8_t* base = row - dnxt;
#pragma unroll
        for (int j = 0; j < NV; j++) {
            const int gi = min(j * 64 + lane, ngran - 1);
            nofs[j] = gi * 4;
            load_stream<4>(nxt[j], base + (size_t)gi * 16);
        }
    };
    float b[P];
    auto reduce = [&]() {                                        // park the fetched row
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < NV; j++) {
            typedef unsigned int u32x4a_t __attribute__((ext_vector_type(4), aligned(16)));
            const u32x4a_t q = {nxt[j][0], nxt[j][1], nxt[j][2], nxt[j][3]};
            *(u32x4a_t*)(line + nofs[j]) = q;
        }
        dcur = dnxt;
        asm volatile("" ::: "memory");
    };
    auto hsum = [&]() {
        constexpr int ND = (W + 3) / 4;
#pragma unroll
        for (int p = 0; p < P; p++) {
            const int wofs = wrel[p] + dcur;                     // this window in the parked line, in bytes
            const uint32_t* win = line + (wofs >> 2);
            const unsigned sh = (unsigned)wofs & 3u;
            uint32_t t[ND + 1], w[ND];
#pragma unroll
            for (int i = 0; i <= ND; i++) t[i] = win[i];
#pragma unroll
            for (int i = 0; i < ND; i++) w[i] = __builtin_amdgcn_alignbyte(t[i + 1], t[i], sh);
            b[p] = 0.f;
#pragma unroll
            for (int k = 0; k < W; k++) b[p] = __fadd_rn(b[p], __fmul_rn((float)((w[k >> 2] >> (8 * (k & 3))) & 0xff), al[p][k]));
        }
        asm volatile("" ::: "memory");
    };
    const AreaCell mine = area_cell(min(dy0 + lane, dy1 - 1), a.sh, gm.scale_y);
    const int sy_end = __builtin_amdgcn_readlane(mine.end(), dy1 - 1 - dy0);
    uint8_t* D = a.dst + (size_t)dxf;
    const int nlive = min(P, a.dw - dxf);                        // columns of this lane inside the frame (<= 0: none)
    int cur = -1;
    for (int dy = dy0; dy < dy1; dy++) {
        const int r = dy - dy0;
        const int s1 = __builtin_amdgcn_readlane(mine.s1, r), s2 = __builtin_amdgcn_readlane(mine.s2, r);
        const int hf = __builtin_amdgcn_readlane((int)mine.hf, r), hl = __builtin_amdgcn_readlane((int)mine.hl, r);
        const float yaf = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.af), r));
        const float yam = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.am), r));
        const float yal = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mine.al), r));
        const int first = hf ? s1 - 1 : s1, end = hl ? s2 + 1 : s2;
        if (cur < 0) { fetch(first); cur = first - 1; }
        float acc[P];
#pragma unroll
        for (int p = 0; p < P; p++) acc[p] = 0.f;
        for (int sy = first; sy < end; sy++) {
            while (cur < sy) {
                cur++;
                reduce();
                if (cur + 1 < sy_end) fetch(cur + 1);
                hsum();
            }
            const float be = (hf && sy == s1 - 1) ? yaf : ((hl && sy == s2) ? yal : yam);
#pragma unroll
            for (int p = 0; p < P; p++) acc[p] = __fadd_rn(acc[p], __fmul_rn(be, b[p]));
        }
        uint32_t out = 0;
#pragma unroll
        for (int p = 0; p < P; p++) out = cvt_pk_u8(acc[p], out, p);
        uint8_t* q = D + (size_t)dy * a.dstep;
        if (P == 4 && nlive == 4 && !(((uintptr_t)q) & 3)) *(uint32_t*)q = out;
        else
            for (int p = 0; p < nlive; p++) q[p] = (uint8_t)(out >> (8 * p));
    }
}

// ------------------------------------------------------------------ AREA over frames of DIFFERENT geometry (BASELINE configs[4])
// One launch for a run of requests whose frames all differ in size (bridge.c:588-604 calls Resize() on whatever arrives):
// a descriptor per frame -- its views and its two scale factors -- instead of launch arguments.  Blocks are dealt to the
// XCDs like frame_block deals them (block id mod 8 = XCD): descriptor list g holds the frames of XCD g back to back, each
// with the number of the first block it owns inside that list, and a block finds its frame by bisection over those.
// What `nv` means depends on the kernel and the body that reads the descriptor:
//   k_resize_area_mix<3 / 4>, nitems > 0   the window W in pixels (even); negative: four columns per lane, window -nv (2..5)
//   k_resize_area_mix<3>, nitems == 0      area_cells_body's NV: 16-byte granules of a lane's run
//   k_resize_area_mix<1>                   always nitems > 0: W in pixels = bytes (even, 2..20), or -W (2..5) with four columns per lane
//   k_resize_area_wide_mix<1 / 3 / 4>      W in pixels (21..66); <3>: -W when the frame needs the covering fetch
struct MixDesc { RArgs a; AreaGeom gm; int first, nblk, nv, rows, nstrips, nitems; };   // rows = band height (nitems > 0) or rows per lane group

template <int CN>
__global__ __launch_bounds__(256) void k_resize_area_mix(const MixDesc* __restrict__ d, MixIndex ix) {
    __shared__ __attribute__((aligned(16))) uint32_t s_line[4][64 * MIX_NV * 4 + 4];
    int blk;
    const int di = mix_pick(d, ix, &blk);              // (bisection over the first-block numbers of the XCD's list)
    if (di < 0) return;
    const MixDesc& m = d[di];
    if (m.nitems > 0 && m.nv < 0) {                    // small factors: four destination columns per lane (k_resize_area_rows4's body)
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int item = blk * 4 + wv;
        if (item >= m.nitems) return;
        switch (-m.nv) {
            case 2: area_rows4_body<CN, 2>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv]); break;
            case 3: area_rows4_body<CN, 3>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv]); break;
            case 4: area_rows4_body<CN, 4>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv]); break;
            default: area_rows4_body<CN, 5>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv]); break;
        }
    } else if (m.nitems > 0) {                         // (everything here is block-uniform: scalar branches)
        const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int item = blk * 4 + wv;
        if (item >= m.nitems) return;
        switch (m.nv) {
            case 2: area_rows_body<CN, 2>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 4: area_rows_body<CN, 4>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 6: area_rows_body<CN, 6>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 8: area_rows_body<CN, 8>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 10: area_rows_body<CN, 10>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 12: area_rows_body<CN, 12>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 14: area_rows_body<CN, 14>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 16: area_rows_body<CN, 16>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            case 18: area_rows_body<CN, 18>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
            default: area_rows_body<CN, 20>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], AreaTail{}, nullptr); break;
        }
    } else if constexpr (CN == 3) {                    // BGR rows that are not 4-byte aligned
        switch (m.nv * 2 + (m.rows == 1)) {
            case 2: area_cells_body<3, 1, AREA_ROWS>(m.a, m.gm, 0, blk); break;
            case 3: area_cells_body<3, 1, 1>(m.a, m.gm, 0, blk); break;
            case 4: area_cells_body<3, 2, AREA_ROWS>(m.a, m.gm, 0, blk); break;
            case 5: area_cells_body<3, 2, 1>(m.a, m.gm, 0, blk); break;
            case 6: area_cells_body<3, 3, AREA_ROWS>(m.a, m.gm, 0, blk); break;
            case 7: area_cells_body<3, 3, 1>(m.a, m.gm, 0, blk); break;
            case 8: area_cells_body<3, 4, AREA_ROWS>(m.a, m.gm, 0, blk); break;
            case 9: area_cells_body<3, 4, 1>(m.a, m.gm, 0, blk); break;
            case 10: area_cells_body<3, 5, AREA_ROWS>(m.a, m.gm, 0, blk); break;
            default: area_cells_body<3, 5, 1>(m.a, m.gm, 0, blk); break;
        }
    }
}

// Gray frames: every descriptor is a row-streaming one (nitems > 0) of area_rows_gray_body -- nv = the window W (even, 2..20)
// with one column per lane, or -W (2..5) with four.
template <>
__global__ __launch_bounds__(256) void k_resize_area_mix<1>(const MixDesc* __restrict__ d, MixIndex ix) {
    __shared__ __attribute__((aligned(16))) uint32_t s_line[4][64 * GRAY_NV_MAX * 4 + 4];   // + 4: a window's look-ahead dword
    int blk;
    const int di = mix_pick(d, ix, &blk);
    if (di < 0) return;
    const MixDesc& m = d[di];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * 4 + wv;
    if (item >= m.nitems) return;
    switch (m.nv) {                                    // (block-uniform: a scalar branch)
        case -2: area_rows_gray_body<2, 4>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
        case -3: area_rows_gray_body<3, 4>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
        case -4: area_rows_gray_body<4, 4>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
        case -5: area_rows_gray_body<5, 4>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
#define IMP_GRAY_W(W_) case W_: area_rows_gray_body<W_, 1>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
        IMP_GRAY_W(2) IMP_GRAY_W(4) IMP_GRAY_W(6) IMP_GRAY_W(8) IMP_GRAY_W(10) IMP_GRAY_W(12) IMP_GRAY_W(14) IMP_GRAY_W(16) IMP_GRAY_W(18)
#undef IMP_GRAY_W
        default: area_rows_gray_body<20, 1>(m.a, m.gm, item, m.nstrips, m.rows, s_line[wv]); break;
    }
}

// The same launch for requests whose Resize() is followed by more of RunJob's chain (bridge.c:606-656): a quarter or half
// turn (Filter "rotate"), the watermark and BlendWithPaper ride on the stores of the row-streaming body, exactly as in the
// lone launch_area_rotate, with the tail read from the frame's descriptor instead of the launch arguments.  A kernel of its
// own: the turned band's LDS tile (4 x 16 x 65 words, 16.6 KB a block) is not paid by k_resize_area_mix's bare batches.
// Every descriptor is a row-streaming one (nitems > 0, nv = the window, 1..20: area_tail_plan's, the lone launch's).
struct MixTailDesc { MixDesc m; AreaTail tail; int flat; };

template <int CN>
__global__ __launch_bounds__(256) void k_resize_area_mix_tail(const MixTailDesc* __restrict__ d, MixIndex ix) {
    __shared__ __attribute__((aligned(16))) uint32_t s_line[4][64 * MIX_NV * 4 + 4];
    __shared__ uint32_t s_tile[4][16 * 65];                      // quarter turns: a band (<= 16 rows) waits here to leave turned
    int blk;
    const int di = mix_pick(d, ix, &blk, [](const MixTailDesc& x) -> const MixDesc& { return x.m; });
    if (di < 0) return;
    const MixTailDesc& t = d[di];
    const MixDesc& m = t.m;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * 4 + wv;
    if (item >= m.nitems) return;
    const bool flat = t.flat != 0;
    switch (m.nv) {                                    // (block-uniform: a scalar branch)
#define IMP_TAIL_W(W_) \
        case W_: area_rows_body<CN, W_, true>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], t.tail, s_tile[wv], flat); break;
        IMP_TAIL_W(1) IMP_TAIL_W(2) IMP_TAIL_W(3) IMP_TAIL_W(4) IMP_TAIL_W(5) IMP_TAIL_W(6) IMP_TAIL_W(7) IMP_TAIL_W(8)
        IMP_TAIL_W(9) IMP_TAIL_W(10) IMP_TAIL_W(11) IMP_TAIL_W(12) IMP_TAIL_W(13) IMP_TAIL_W(14) IMP_TAIL_W(15) IMP_TAIL_W(16)
        IMP_TAIL_W(17) IMP_TAIL_W(18) IMP_TAIL_W(19)
#undef IMP_TAIL_W
        default: area_rows_body<CN, 20, true>(m.a, m.gm, 0, item, m.nstrips, m.rows, s_line[wv], t.tail, s_tile[wv], flat); break;
    }
}

// Frames whose cells span 21..66 source columns (area_wide_plan), of different geometry, in one launch: the descriptor
// scheme around area_wide_body.  nv = the window W (negative: a BGR frame off the 4-byte grid, fetched by covering
// granules: wide_nv), rows = the band height, nblk = ceil(nitems / wpb).  A kernel
// of its own: its lines are dynamic LDS sized for the longest segment of the launch (`line_dw` dwords each, `wpb` of them),
// which k_resize_area_mix's frames never pay.
template <int CN>
__global__ __launch_bounds__(256) void k_resize_area_wide_mix(const MixDesc* __restrict__ d, MixIndex ix, int line_dw, int wpb) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_wide_mix[];
    int blk;
    const int di = mix_pick(d, ix, &blk);
    if (di < 0) return;
    const MixDesc& m = d[di];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * wpb + wv;
    if (item >= m.nitems) return;
    area_wide_body<CN>(m.a, m.gm, 0, item, m.nstrips, m.rows, m.nv, line_dw, s_wide_mix + wv * line_dw);
}

// ------------------------------------------------------------------ whole-factor AREA and NN over frames of DIFFERENT geometry
// resizeAreaFast_ (both factors integers: 640x480, 1280x720, 1920x1080 ... at 320 wide) for a run of requests in one
// launch: the descriptor scheme of k_resize_area_mix around the bodies of the lone kernels above, so the bytes are the
// lone launch's.  A descriptor names its body (block-uniform: scalar branches) and how that body splits the frame:
//   IM_2X2    k_area2x2_v4 / k_area2x2_v3: a lane per four destination pixels, per_row = lanes per destination row
//   IM_BOXL   k_area_boxl<CN, isx>, isx = 2..8, at most 257 source pixels a box, 4-byte aligned rows and pointers:
//             a wave per run of P destination pixels, per_row = runs per destination row.  BGRA 8x, which alone runs
//             k_area_boxc<8>, takes area_boxl_body<4, 8> here: with it the BGRA kernel wanted 65 VGPRs (7 waves per
//             SIMD against BGR's 8), so the kernel is bounded to 8 waves -- 63 VGPRs, no scratch.
//   IM_PIXEL  k_resize_area_int: a lane per destination pixel -- factors of 1 or above 8, boxes over 257 pixels, BGR
//             rows that are not 4-byte aligned, gray
// The wave-private LDS lines of IM_BOXL are dynamic: a launch without such a frame asks for none.
enum { IM_PIXEL = 0, IM_2X2 = 1, IM_BOXL = 2 };
struct IntMixDesc { RArgs a; int isx, isy, cls, per_row, P, first, nblk; float scale; };

template <int CN>
__global__ __launch_bounds__(256, 8) void k_area_int_mix(const IntMixDesc* __restrict__ d, MixIndex ix) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_int_mix[];      // IM_BOXL: 4 lines of BOXL_LINE dwords
    int blk;
    const int di = mix_pick(d, ix, &blk);
    if (di < 0) return;
    const IntMixDesc& m = d[di];
    if constexpr (CN != 1) {
        if (m.cls == IM_BOXL) {
            const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
            uint32_t* cols = s_int_mix + wv * BOXL_LINE;
            const int gw = blk * 4 + wv;
            switch (m.isx) {
#define IMP_BOXL(I_) case I_: area_boxl_body<CN, I_>(m.a, m.isy, m.P, m.per_row, m.scale, gw, 0, cols); break;
                IMP_BOXL(2) IMP_BOXL(3) IMP_BOXL(4) IMP_BOXL(5) IMP_BOXL(6) IMP_BOXL(7)
#undef IMP_BOXL
                default: area_boxl_body<CN, 8>(m.a, m.isy, m.P, m.per_row, m.scale, gw, 0, cols); break;
            }
            return;
        }
        if (m.cls == IM_2X2) {
            if constexpr (CN == 4) area2x2_v4_body(m.a, m.per_row, blk * 256 + (int)threadIdx.x, 0);
            else area2x2_v3_body(m.a, m.per_row, blk * 256 + (int)threadIdx.x, 0);
            return;
        }
    }
    area_int_body<CN>(m.a, m.isx, m.isy, blk * 256 + (int)threadIdx.x, 0);
}

// cvResize INTER_NN (the `simple` requests: GIF answers) the same way: k_resize_nn's body per destination pixel.
struct NnMixDesc { RArgs a; double scale_x, scale_y; int first, nblk; };

template <int CN>
__global__ __launch_bounds__(256) void k_resize_nn_mix(const NnMixDesc* __restrict__ d, MixIndex ix) {
    int blk;
    const int di = mix_pick(d, ix, &blk);
    if (di < 0) return;
    const NnMixDesc& m = d[di];
    resize_nn_body<CN>(m.a, m.scale_x, m.scale_y, (long long)blk * 256 + threadIdx.x, 0);
}

// ------------------------------------------------------------------ per-geometry table cache
struct TableSet {
    void* blob = nullptr;     // one device allocation
    const int *xofs = nullptr, *yofs = nullptr;
    const short *xco = nullptr, *yco = nullptr;
    const int* srows = nullptr;   // per destination row {first footprint row, ksize weights, padding}: strip_row_ints(ksize) ints (k_resize_strip)
    const void* yrows = nullptr;  // CUBIC: per destination row {footprint advance, yco * 2^-22 as floats, first footprint row} (UpRow)
    int up_period = 0;        // CUBIC enlargement: P when exactly every P-th destination row advances the footprint (integer factor), else 0
    int strip_a0 = -1, strip_a1 = -1;   // the footprint advances by a0 rows after even destination rows and a1 after odd ones (k_resize_strip2), or -1
    bool ysym = false;        // step2 and the one set of row weights is mirror-symmetric (vpass_px's VSYM form)
    bool step2 = false;       // xofs[d] = xofs[0] + 2d and yofs[d] = yofs[0] + 2d: k_resize_2x_roll applies
    bool xuni = false;        // step2 and ONE set of column weights (k_resize_2x_dma's MF form)
    int x0 = 0;               // xofs[0]: the first source column of destination column 0
    AreaDev area{};
};
using Key = std::tuple<int, int, int, int, int>;

// One cache per lane (= per calling thread), owned by the lane and dropped with it: no lock, no shared state, nothing
// survives impgpu_env_destroy.  A miss builds the tables on the calling thread and sends them through the lane's
// pinned ring with hipMemcpyAsync; the blob is pool memory.  A mixed-size request stream (BASELINE configs[4]) misses
// on almost every request, so a miss must cost no lock, no hipMalloc and no device-wide wait.  Least-recently-used
// entries are evicted one at a time; their memory goes back to the pool in stream order.
struct TableEntry {
    TableSet ts;
    unsigned long long tick = 0;
    bool settled = false;                   // the upload is known to have completed
    std::vector<hipStream_t> foreign;       // caller-supplied streams that have read the blob (batch entry points)
};
struct TableCache : LaneCache {
    std::map<Key, TableEntry> m;
    unsigned long long tick = 0;
};
constexpr size_t TABLE_CACHE_ENTRIES = 256;

template <class T>
static size_t put(std::vector<uint8_t>& blob, const std::vector<T>& v) {
    while (blob.size() % 16) blob.push_back(0);
    size_t off = blob.size();
    const uint8_t* p = (const uint8_t*)v.data();
    blob.insert(blob.end(), p, p + v.size() * sizeof(T));
    return off;
}

static int table_use(TableEntry& e, hipStream_t s) {     // order `s` behind the entry's upload
    if (on_lane_stream(s)) return IMP_OK;                // the upload rode the lane stream: already ordered
    bool seen = false;
    for (hipStream_t f : e.foreign) seen = seen || f == s;
    if (!seen) e.foreign.push_back(s);
    if (e.settled) return IMP_OK;
    if (lane_stream_idle()) { e.settled = true; return IMP_OK; }
    return stream_join(s);
}

// The CUBIC enlargement kernels' row constants from the vertical axis of a geometry: an UpRow per destination row and a
// sentinel the kernels' one-row look-ahead may read.  *period = P when exactly every P-th row (P = 2, 3, 4) advances the
// footprint, else 0 (null: not asked for -- the walks over the axis that find it are skipped).  The one place they are made: get_tables (the lone launches, cached) and launch_up_mix (the mixed
// launch, whose tables travel with it) both call it.
static std::vector<UpRow> up_rows(const TapAxis& ty, int dh, int* period) {
    std::vector<UpRow> yr((size_t)dh + 1);
    for (int d = 0; d < dh; d++) {
        yr[d].first = ty.ofs[d] - 1;
        yr[d].adv = d ? ty.ofs[d] - ty.ofs[d - 1] : 0;
        for (int k = 0; k < 4; k++)     // the constants of VResizeCubicVec_32s8u's multiplies: one IEEE multiply each
            yr[d].bf[k] = (float)ty.coef[(size_t)d * 4 + k] * (1.f / (2048.f * 2048.f));
        yr[d].pad[0] = yr[d].pad[1] = 0;
    }
    yr[dh] = yr[dh - 1];
    yr[dh].adv = 0;
    if (!period) return yr;
    *period = 0;
    for (int per = 2; per <= 4 && !*period; per++) {   // rows p, p + per, p + 2 per ... advance by one, the others not at all
        int p0 = 1;
        while (p0 < dh && yr[p0].adv == 0) p0++;
        bool ok = p0 < dh;
        for (int d = 1; d < dh && ok; d++) ok = yr[d].adv == ((d >= p0 && (d - p0) % per == 0) ? 1 : 0);
        if (ok) *period = per;
    }
    return yr;
}

static int get_tables(int interp, int sw, int sh, int dw, int dh, double scale_x, double scale_y, hipStream_t s, TableSet* out) {
    LaneCache** slot = lane_cache_slot(0);
    if (!slot) { set_error("impgpu_env_start has not been called", hipErrorNotInitialized); return IMP_ERROR_DEVICE; }
    if (!*slot) *slot = new TableCache();
    TableCache& C = *static_cast<TableCache*>(*slot);
    Key key{interp, sw, sh, dw, dh};
    auto it = C.m.find(key);
    if (it != C.m.end()) {
        it->second.tick = ++C.tick;
        if (int rc = table_use(it->second, s)) return rc;
        *out = it->second.ts;
        return IMP_OK;
    }
    if (C.m.size() >= TABLE_CACHE_ENTRIES) {             // evict the least recently used geometry
        auto victim = C.m.begin();
        for (auto j = C.m.begin(); j != C.m.end(); ++j)
            if (j->second.tick < victim->second.tick) victim = j;
        for (hipStream_t f : victim->second.foreign)     // kernels on caller-supplied streams may still read it
            if (int rc = stream_join_back(f)) return rc;
        dev_free(victim->second.ts.blob);                // lane-stream order from here on
        C.m.erase(victim);
    }
    std::vector<uint8_t> blob;
    TableSet ts;
    size_t o[12] = {0};
    if (interp == IMP_INTER_AREA) {
        AreaAxis ax, ay;
        build_area_axis(sw, dw, scale_x, &ax);
        build_area_axis(sh, dh, scale_y, &ay);
        o[0] = put(blob, ax.start); o[1] = put(blob, ax.count); o[2] = put(blob, ax.aoff); o[3] = put(blob, ax.alpha);
        o[4] = put(blob, ay.start); o[5] = put(blob, ay.count); o[6] = put(blob, ay.aoff); o[7] = put(blob, ay.alpha);
    } else {
        TapAxis tx, ty;
        build_tap_axis(sw, dw, scale_x, interp, true, &tx);
        build_tap_axis(sh, dh, scale_y, interp, false, &ty);
        o[0] = put(blob, tx.ofs); o[1] = put(blob, tx.coef); o[2] = put(blob, ty.ofs); o[3] = put(blob, ty.coef);
        if (interp == IMP_INTER_CUBIC) {
            const std::vector<UpRow> yr = up_rows(ty, dh, &ts.up_period);
            while (blob.size() % 32) blob.push_back(0);
            o[4] = put(blob, yr);
        }
        {
            // the strip kernels' row constants: the footprint's first row, then the KS weights; for CUBIC again at [8..11] as
            // the floats b * 2^-22 of VResizeCubicVec_32s8u's multiplies.  And the advance pattern, when it has period two
            // (k_resize_strip2): A0 rows after every even destination row, A1 after every odd one.
            const int sr = strip_row_ints(ty.ksize), ks = ty.ksize;
            std::vector<int> rows((size_t)(dh + 1) * sr, 0);     // + a sentinel row
            for (int d = 0; d <= dh; d++) {
                const int dd = d < dh ? d : dh - 1;
                rows[(size_t)d * sr] = ty.ofs[dd] - (ks / 2 - 1);
                for (int k = 0; k < ks; k++) {
                    const int coef = ty.coef[(size_t)dd * ks + k];
                    rows[(size_t)d * sr + 1 + k] = coef;
                    if (interp == IMP_INTER_CUBIC) {
                        const float bf = (float)coef * (1.f / (2048.f * 2048.f));
                        __builtin_memcpy(&rows[(size_t)d * sr + 8 + k], &bf, 4);
                    }
                }
            }
            ts.strip_a0 = ts.strip_a1 = -1;
            if (dh >= 3) {
                const int a0 = ty.ofs[1] - ty.ofs[0], a1 = ty.ofs[2] - ty.ofs[1];
                bool ok = a0 >= 0 && a1 >= 0 && a0 <= 2 && a1 <= 2 && ((a0 + a1) & 1);
                for (int d = 1; d < dh && ok; d++) ok = ty.ofs[d] - ty.ofs[d - 1] == ((d & 1) ? a0 : a1);
                if (ok) { ts.strip_a0 = a0; ts.strip_a1 = a1; }
            }
            while (blob.size() % 64) blob.push_back(0);
            o[5] = put(blob, rows);
        }
        ts.step2 = true;
        for (int d = 1; d < dw && ts.step2; d++) ts.step2 = tx.ofs[d] == tx.ofs[0] + 2 * d;
        for (int d = 1; d < dh && ts.step2; d++) ts.step2 = ty.ofs[d] == ty.ofs[0] + 2 * d;
        for (int d = 1; d < dh && ts.step2; d++)          // and one set of row weights (true when the scale is exactly 2)
            for (int k = 0; k < ty.ksize; k++) ts.step2 = ts.step2 && ty.coef[(size_t)d * ty.ksize + k] == ty.coef[k];
        ts.ysym = ts.step2;
        for (int k = 0; k < ty.ksize && ts.ysym; k++) ts.ysym = ty.coef[k] == ty.coef[ty.ksize - 1 - k];
        ts.xuni = ts.step2;
        ts.x0 = tx.ofs[0];
        for (int d = 1; d < dw && ts.xuni; d++)
            for (int k = 0; k < tx.ksize; k++) ts.xuni = ts.xuni && tx.coef[(size_t)d * tx.ksize + k] == tx.coef[k];
    }
    void* devp = nullptr;
    if (int rc = upload_small(blob.data(), blob.size(), &devp, s)) return rc;     // asynchronous, ordered before later work on `s`
    uint8_t* dev = (uint8_t*)devp;
    ts.blob = dev;
    if (interp == IMP_INTER_AREA) {
        ts.area.xstart = (const int*)(dev + o[0]); ts.area.xcount = (const int*)(dev + o[1]);
        ts.area.xaoff = (const int*)(dev + o[2]);  ts.area.xalpha = (const float*)(dev + o[3]);
        ts.area.ystart = (const int*)(dev + o[4]); ts.area.ycount = (const int*)(dev + o[5]);
        ts.area.yaoff = (const int*)(dev + o[6]);  ts.area.yalpha = (const float*)(dev + o[7]);
    } else {
        ts.xofs = (const int*)(dev + o[0]); ts.xco = (const short*)(dev + o[1]);
        ts.yofs = (const int*)(dev + o[2]); ts.yco = (const short*)(dev + o[3]);
        ts.yrows = interp == IMP_INTER_CUBIC ? (const void*)(dev + o[4]) : nullptr;
        ts.srows = (const int*)(dev + o[5]);
    }
    TableEntry& e = C.m[key];
    e.ts = ts;
    e.tick = ++C.tick;
    if (!on_lane_stream(s)) e.foreign.push_back(s);
    *out = ts;
    return IMP_OK;
}

// ------------------------------------------------------------------ launcher
// Small host-side rules every launcher below shares.
// resizeAreaFast_'s test in OpenCV's resize: both factors are whole numbers -- the box kernels' arithmetic
static bool whole_factors(double scale_x, double scale_y) {
    return std::fabs(scale_x - std::lrint(scale_x)) < DBL_EPSILON && std::fabs(scale_y - std::lrint(scale_y)) < DBL_EPSILON;
}
// Destination rows per band of the row-streaming AREA bodies: 16, less while that leaves fewer than ~4096 waves (down to 4:
// a band re-reads one source row of its neighbour) or, for a lone request, fewer than ~1024 (down to 1: latency first).
static int area_band_height(long long frames, long long nstrips, int dh) {
    int b = 16;
    while (b > 4 && frames * nstrips * ((dh + b - 1) / b) < 4096) b /= 2;
    while (b > 1 && frames * nstrips * ((dh + b - 1) / b) < 1024) b /= 2;
    return b;
}
// A frame's split for the row-streaming bodies: strips of `cols` destination columns, bands of `bh` rows, an item (a wave's
// work) per strip and band, `wpb` items per block.
struct RowSplit { int nstrips, bh, nitems, nblk; };
static RowSplit row_split(int dw, int dh, int cols, int bh, int wpb = 4) {
    RowSplit r{};
    r.nstrips = (dw + cols - 1) / cols;
    r.bh = bh;
    r.nitems = r.nstrips * ((dh + bh - 1) / bh);
    r.nblk = (r.nitems + wpb - 1) / wpb;
    return r;
}
static unsigned round_up8(int count) { return (unsigned)((count + 7) / 8 * 8); }   // whole groups of 8 frames (frame-per-XCD order)
static RArgs rargs(const Frames& f) { return RArgs{f.src, f.src_stride, f.v.step, f.v.w, f.v.h, f.dst, f.dst_stride, f.dstep, f.dw, f.dh}; }
static RArgs rargs(const MixFrame& f) { return RArgs{f.src, 0, f.sstep, f.sw, f.sh, f.dst, 0, f.dstep, f.dw, f.dh}; }
static int launched() {
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}
// A runtime int in [Lo, Hi] as a compile-time constant: f(K) with K() == v; a value below the range takes Lo, one above it Hi.
template <int Lo, int Hi, class F>
static void with_const(int v, F f) {
    if constexpr (Lo == Hi) f(std::integral_constant<int, Lo>{});
    else if (v <= Lo) f(std::integral_constant<int, Lo>{});
    else with_const<Lo + 1, Hi>(v, f);
}

// k_resize_area_rows for this geometry?  *w = window (the widest horizontal cell, widened until a wave's segment fits its
// 64 * ceil(W/4) granules), *bh = destination rows per band (area_band_height).
static bool area_rows_plan(int sw, int sh, int dw, int dh, double scale_x, long long frames, bool even, int* w, int* bh) {
    (void)sh;
    int ww = area_max_count(sw, dw, scale_x);
    if (even) ww += ww & 1;                                // the mixed-geometry kernel carries the even windows only
    while (ww <= 4 * MIX_NV && 63 * scale_x + ww + 8 > 256 * ((ww + 3) / 4)) ww += even ? 2 : 1;
    if (ww < 1 || ww > 4 * MIX_NV || sw < ww || sw < 4) return false;
    *w = ww;
    *bh = area_band_height(frames, (dw + 63) / 64, dh);
    return true;
}

// area_rows_gray_body for this gray geometry?  *w = the window: the widest horizontal cell (even with one column per lane:
// the kernel carries those), widened until a wave's segment fits its granules; *p = columns per lane; *bh as area_rows_plan.
static bool gray_rows_plan(int sw, int dw, int dh, double scale_x, long long frames, int* w, int* p, int* bh) {
    auto fits = [&](int ww, int pp) { return (64 * pp - 1) * scale_x + ww + 2 + 30 <= 1024.0 * gray_rows_nv(ww, pp); };
    const int widest = std::max(area_max_count(sw, dw, scale_x), 2);
    int ww = widest, pp = 4;                               // four columns per lane while the windows are small and the rows long
    if (dw < 160 || ww > 5 || !fits(ww, 4)) {              // (fits(w, 4) holds for every w <= 5 whose scale is at most w: a guard, not a search)
        pp = 1;
        ww = widest + (widest & 1);
        while (ww <= GRAY_W_MAX && !fits(ww, 1)) ww += 2;
    }
    if (ww > GRAY_W_MAX) return false;                     // (a row narrower than the window is fine: the body clips its fetch)
    *w = ww;
    *p = pp;
    *bh = area_band_height(frames, (dw + 64 * pp - 1) / (64 * pp), dh);
    return true;
}

// area_wide_body for this frame?  The one acceptance rule of k_resize_area_wide (launch_cn) and k_resize_area_wide_mix
// (launch_resize_mixed): a general INTER_AREA shrink, of a gray, BGR or BGRA frame with any pointer and pitch, whose
// widest horizontal cell spans 21..66 source columns (factors up to 64; narrower cells belong to the bodies with
// compile-time windows, wider ones stay with k_resize_area and its tables).  *w = that widest cell, *bh as
// area_rows_plan picks it, *cover = the frame needs the covering fetch (gray; BGR off the 4-byte grid), *line_bytes = a
// wave's LDS line: the longest segment a strip can have -- lane 63's window starts less than 63 * scale_x + 2 pixels
// after lane 0's -- with the granule rounding at both ends (30 bytes: aligned, up to 15 in front of the segment and 15
// after it; covering, `dl` <= 15 and the same 15), plus the 16 bytes a last turn of four pixels and a window's look-ahead
// dword may read past it, rounded up.
static bool area_wide_plan(int sw, int sh, int dw, int dh, int cn, int interp, const uint8_t* src, int sstep, long long src_stride,
                           long long frames, int* w, int* bh, int* line_bytes, bool* cover) {
    (void)sh;
    if (interp != IMP_INTER_AREA || (cn != 1 && cn != 3 && cn != 4) || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || dw > sw || dh > sh)
        return false;
    const bool off_grid = (((uintptr_t)src | (uintptr_t)sstep | (uintptr_t)src_stride) & 3) != 0;
    if (cn == 4 && off_grid) return false;                 // (no caller passes one: BGRA pixels are dwords)
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    if (whole_factors(scale_x, scale_y)) return false;                                    // resizeAreaFast_: the box kernels' arithmetic
    if (scale_x > 70) return false;                        // (no cell of 66 columns or fewer: the axis need not be walked)
    const int ww = area_max_count(sw, dw, scale_x);
    if (ww < WIDE_W_MIN || ww > WIDE_W_MAX || sw < ww) return false;
    *w = ww;
    *bh = area_band_height(frames, (dw + 63) / 64, dh);
    *line_bytes = ((((int)std::ceil(63 * scale_x) + ww + 2) * cn + 30 + 15) & ~15) + 32;
    *cover = cn == 1 || off_grid;
    return true;
}
constexpr int wide_wpb(int line_bytes) { return 4 * line_bytes <= 65536 ? 4 : 2; }   // waves (= lines) per block: 64 KB of LDS at most
constexpr int wide_nv(int cn, int w, bool cover) { return cn == 3 && cover ? -w : w; }   // the window as area_wide_body reads it

template <int CN>
static void launch_area_rows(int w, const RowSplit& r, hipStream_t s, const RArgs& a, const AreaGeom& gm, int count, const AreaTail& tail) {
    with_const<1, 4 * MIX_NV>(w, [&](auto W) {
        hipLaunchKernelGGL((k_resize_area_rows<CN, W()>), dim3((unsigned)r.nblk, round_up8(count)), dim3(256), 0, s, a, gm, r.nstrips, r.bh,
                           r.nitems, r.nblk, count, tail);
    });
}

// Resize (general INTER_AREA, BGRA or BGR) + rotate + watermark (a BGRA overlay) in one pass; f.dw x f.dh is the RESIZED geometry, f.dst the final
// (rotated) frames.  IMP_ERROR_UNSUPPORTED when the geometry takes another resize kernel.
bool area_tail_plan(const Frames& f, int* w, int* bh) {
    const View& v = f.v;
    if ((v.c != 4 && v.c != 3) || f.count <= 0 || f.count > 65535 || f.dw <= 0 || f.dh <= 0 || f.dw > v.w || f.dh > v.h) return false;
    if (v.c == 3 && v.w < 6) return false;                 // (the BGR windows' aligned-dword reads need a few pixels of row)
    if (((uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)v.step | (uintptr_t)f.dstep | (uintptr_t)f.src_stride | (uintptr_t)f.dst_stride) & 3)
        return false;
    const double scale_x = 1. / ((double)f.dw / v.w), scale_y = 1. / ((double)f.dh / v.h);
    if (whole_factors(scale_x, scale_y)) return false;                                    // resizeAreaFast_: the box kernels' arithmetic
    if (!area_rows_plan(v.w, v.h, f.dw, f.dh, scale_x, f.count, false, w, bh)) return false;
    *bh = std::min(*bh, 16);                               // (the turned band's LDS tile)
    return true;
}

int launch_area_rotate(const Frames& f, int amount, const OverlayArgs* overlay, hipStream_t s) {
    const View& v = f.v;
    int w = 0, bh = 0;
    if (!area_tail_plan(f, &w, &bh)) return IMP_ERROR_UNSUPPORTED;
    const double scale_x = 1. / ((double)f.dw / v.w), scale_y = 1. / ((double)f.dh / v.h);
    const AreaGeom gm{scale_x, scale_y};
    AreaTail tail{};
    tail.rot = amount;
    if (overlay) tail.wm = *overlay;
    const RowSplit r = row_split(f.dw, f.dh, 64, bh);
    if (v.c == 4) launch_area_rows<4>(w, r, s, rargs(f), gm, f.count, tail);
    else launch_area_rows<3>(w, r, s, rargs(f), gm, f.count, tail);
    return launched();
}

// launch_cv_resize's launches, by channel count.  `grid`: a lane per destination pixel, a grid row per frame.
// Whole-factor INTER_AREA (whole_factors: resizeAreaFast_).
template <int CN>
static int launch_area_whole(const RArgs& a, int count, double scale_x, double scale_y, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    const int isx = (int)std::lrint(scale_x), isy = (int)std::lrint(scale_y);
    const bool rows4 = !(((uintptr_t)a.src | (uintptr_t)a.dst | (uintptr_t)a.sstep | (uintptr_t)a.dstep |
                          (uintptr_t)a.src_stride | (uintptr_t)a.dst_stride) & 3);
    if (isx == 2 && isy == 2 && (CN == 4 || CN == 3) && rows4 && a.sw == 2 * a.dw && a.sh >= 2 * a.dh) {
        const int qpr = (a.dw + 3) / 4;                  // lanes per destination row
        const dim3 qgrid((unsigned)(((long long)qpr * a.dh + 255) / 256), (unsigned)count);
        const int gpr2 = a.sw / 4;
        const dim3 cgrid2((unsigned)(((long long)gpr2 * a.dh + 511) / 512), (unsigned)count);
        if (CN == 4 && !(a.dw & 1)) hipLaunchKernelGGL(k_area2x2_c4, cgrid2, block, 0, s, a, gpr2);
        else if (CN == 4) hipLaunchKernelGGL(k_area2x2_v4, qgrid, block, 0, s, a, qpr);
        else hipLaunchKernelGGL(k_area2x2_v3, qgrid, block, 0, s, a, qpr);
    } else if (CN == 4 && rows4 && isx >= 3 && isx <= 8 && isy >= 1 && isx * isy <= 257 && a.sw == isx * a.dw && a.sh >= isy * a.dh) {
        const float scale = 1.f / (float)(isx * isy);
        const int cpr = a.sw / 4;                         // 16-byte granules per source row (k_area_boxc)
        const dim3 cgrid((unsigned)(((long long)cpr * a.dh + 1023) / 1024), (unsigned)count);
        const int P = (4096 / (4 * isx)) & ~3, lcpr = (a.dw + P - 1) / P;
        const dim3 lgrid((unsigned)(((long long)lcpr * a.dh + 3) / 4), (unsigned)count);
        if (isx == 8) hipLaunchKernelGGL((k_area_boxc<8>), cgrid, block, 0, s, a, isy, cpr, scale);
        else with_const<3, 7>(isx, [&](auto I) { hipLaunchKernelGGL((k_area_boxl<4, I()>), lgrid, block, 0, s, a, isy, P, lcpr, scale); });
    } else if (CN == 3 && rows4 && isx >= 2 && isx <= 8 && isy >= 1 && isx * isy <= 257 && !(isx == 2 && isy == 2) &&
               a.sw == isx * a.dw && a.sh >= isy * a.dh) {
        const int P = (4096 / (3 * isx)) & ~3, cpr = (a.dw + P - 1) / P;
        const dim3 bgrid((unsigned)(((long long)cpr * a.dh + 3) / 4), (unsigned)count);
        const float scale = 1.f / (float)(isx * isy);
        with_const<2, 8>(isx, [&](auto I) { hipLaunchKernelGGL((k_area_boxl<3, I()>), bgrid, block, 0, s, a, isy, P, cpr, scale); });
    } else
        hipLaunchKernelGGL((k_resize_area_int<CN>), grid, block, 0, s, a, isx, isy);
    return launched();
}

// Every other INTER_AREA shrink.
template <int CN>
static int launch_area_general(const RArgs& a, int count, int interp, double scale_x, double scale_y, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    // BGRA / BGR with cells of at most 20 source columns (shrinks up to 18x): source rows streamed through wave-private
    // LDS lines, weights computed in the kernel -- no per-geometry table to build, upload or cache.
    const AreaGeom gm{scale_x, scale_y};
    const bool rows4b = !(((uintptr_t)a.src | (uintptr_t)a.sstep | (uintptr_t)a.src_stride) & 3);
    if (CN == 4 || (CN == 3 && rows4b && a.sw >= 6)) {
        int w = 0, bh = 0;
        if (area_rows_plan(a.sw, a.sh, a.dw, a.dh, scale_x, count, false, &w, &bh)) {
            // four columns per lane while the windows are small and there are enough columns and waves for it
            const RowSplit r4 = row_split(a.dw, a.dh, 256, bh);
            const long long waves4 = (long long)count * r4.nitems;
            if (w >= 2 && w <= 5 && a.dw >= 160 && waves4 >= 2048 && 255 * scale_x + w + 8 <= (CN == 4 ? 1024 : 1340)) {
                constexpr int C34 = CN == 3 ? 3 : 4;
                with_const<2, 5>(w, [&](auto W) {
                    hipLaunchKernelGGL((k_resize_area_rows4<C34, W()>), dim3((unsigned)r4.nblk, round_up8(count)), block, 0, s, a, gm, r4.nstrips,
                                       bh, r4.nitems, r4.nblk, count);
                });
                return launched();
            }
            launch_area_rows<(CN == 3 ? 3 : 4)>(w, row_split(a.dw, a.dh, 64, bh), s, a, gm, count, AreaTail{});
            return launched();
        }
    }
    // BGR frames whose rows are not 4-byte aligned (never cvCreateImage's, but a caller's own buffer may be): a lane
    // per destination column, windows straight from global memory, weights computed in the kernel too
    const int bpf = (int)grid.x;                       // blocks per frame
    const dim3 fgrid(grid.x, round_up8(count));
    const int ng = (a.dh + AREA_ROWS - 1) / AREA_ROWS;
    const int gbpf = (int)(((long long)a.dw * ng + 255) / 256);
    const dim3 ggrid((unsigned)gbpf, round_up8(count));
    const bool big = (long long)gbpf * count >= 1024;
    const int nvx = CN == 3 ? (area_max_count(a.sw, a.dw, scale_x) + 3) / 4 : 0;
    if (nvx >= 1 && nvx <= MIX_NV && a.sw >= 4 * nvx) {
        with_const<1, MIX_NV>(nvx, [&](auto NV) {
            if (big) hipLaunchKernelGGL((k_resize_area_cells<3, NV(), AREA_ROWS>), ggrid, block, 0, s, a, gm, gbpf, count);
            else hipLaunchKernelGGL((k_resize_area_cells<3, NV(), 1>), fgrid, block, 0, s, a, gm, bpf, count);
        });
        return launched();
    }
    // cells of 21..66 source columns (shrinks past 18x, up to 64x), any channel count, pointer and pitch: the same walk
    // with a runtime window and a dynamic LDS line -- no table either
    {
        int w = 0, bh = 0, line_bytes = 0;
        bool cover = false;
        if (area_wide_plan(a.sw, a.sh, a.dw, a.dh, CN, interp, a.src, a.sstep, a.src_stride, count, &w, &bh, &line_bytes, &cover)) {
            const int wpb = wide_wpb(line_bytes);
            const RowSplit r = row_split(a.dw, a.dh, 64, bh, wpb);
            hipLaunchKernelGGL((k_resize_area_wide<CN>), dim3((unsigned)r.nblk, round_up8(count)), dim3(64 * wpb), (size_t)wpb * line_bytes, s, a, gm,
                               wide_nv(CN, w, cover), line_bytes / 4, wpb, r.nstrips, bh, r.nitems, r.nblk, count);
            return launched();
        }
    }
    // everything else (cells wider than 66 columns): run tables, one output per lane
    TableSet ts;
    if (int rc = get_tables(interp, a.sw, a.sh, a.dw, a.dh, scale_x, scale_y, s, &ts)) return rc;
    hipLaunchKernelGGL((k_resize_area<CN>), grid, block, 0, s, a, ts.area);
    return launched();
}

// The tapped interpolations (LINEAR, CUBIC, LANCZOS4), branch by branch.
// exact 2x decimation of a 3-channel frame: register-rolling strips
static void launch_2x_bgr(const RArgs& a, int count, int interp, const TableSet& ts, hipStream_t s) {
    const dim3 block(256);
    const int nstrips = (a.dh + ROLL_STRIP - 1) / ROLL_STRIP;
    const dim3 rgrid((a.dw + 255) / 256, nstrips, (unsigned)count);
    const bool dma3 = (a.sw & 15) == 0 && (long long)a.sh * a.sstep < (1LL << 32) && (long long)a.dh * a.dstep < (1LL << 32) &&
                      !(((uintptr_t)a.src | (uintptr_t)a.sstep | (uintptr_t)a.src_stride) & 15);
    const int nbx = (a.dw + 255) / 256, bpf = nbx * nstrips;
    const dim3 dgrid((unsigned)(bpf * 8), (unsigned)((count + 7) / 8));
    if (dma3 && interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_2x_dma3<4, M_CUBIC, 3, false>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, (a.dw * 3) & ~7, nbx, bpf, count);
    else if (dma3 && ts.ysym)
        hipLaunchKernelGGL((k_resize_2x_dma3<8, M_LANCZOS, 3, true>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0, nbx, bpf, count);
    else if (dma3)
        hipLaunchKernelGGL((k_resize_2x_dma3<8, M_LANCZOS, 3, false>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0, nbx, bpf, count);
    else if (interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_2x_roll3<4, M_CUBIC, false>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, (a.dw * 3) & ~7);
    else if (ts.ysym)
        hipLaunchKernelGGL((k_resize_2x_roll3<8, M_LANCZOS, true>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
    else
        hipLaunchKernelGGL((k_resize_2x_roll3<8, M_LANCZOS, false>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
}

// exact 2x decimation: register-rolling kernel, one wave per 64-column x ROLL_STRIP-row strip
static void launch_2x_bgra(const RArgs& a, int count, int interp, const TableSet& ts, hipStream_t s) {
    const dim3 block(256);
    const int nstrips = (a.dh + ROLL_STRIP - 1) / ROLL_STRIP;
    // LDS-DMA row ring, three iterations prefetched, when the 16-byte DMA granules line up with the rows (otherwise
    // the register-rolling kernel, which has no alignment demands)
    const bool dma_ok = interp != IMP_INTER_LINEAR && (a.sw & 3) == 0 &&
                        (long long)a.sh * a.sstep < (1LL << 32) && (long long)a.dh * a.dstep < (1LL << 32) &&
                        !(((uintptr_t)a.src | (uintptr_t)a.sstep | (uintptr_t)a.src_stride) & 15);
    const dim3 rgrid((a.dw + 255) / 256, nstrips, (unsigned)count);
    // four waves per block; they are independent (no barriers, private LDS rings)
    const int nbx = (a.dw + 255) / 256, bpf = nbx * nstrips;
    const dim3 dgrid((unsigned)(bpf * 8), (unsigned)((count + 7) / 8));
    // the horizontal pass on the matrix unit (k_resize_2x_dma's MF form) where every column has the same taps and the
    // strips' first tap is dword 1 of its 16-byte granule (xofs[0] = 0: sx00 = 2 dx0 - 3)
    const bool mf = dma_ok && ts.xuni && ts.ysym && interp == IMP_INTER_LANCZOS4 && ts.x0 == 0;
    if (mf) hipLaunchKernelGGL((k_resize_2x_dma<8, M_LANCZOS, 3, true, 4, true>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0, nbx, bpf, count);
    else if (dma_ok && interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_2x_dma<4, M_CUBIC, 3, false, 4>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, (a.dw * 4) & ~7, nbx, bpf, count);
    else if (dma_ok && ts.ysym)
        hipLaunchKernelGGL((k_resize_2x_dma<8, M_LANCZOS, 3, true, 4>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0, nbx, bpf, count);
    else if (dma_ok)
        hipLaunchKernelGGL((k_resize_2x_dma<8, M_LANCZOS, 3, false, 4>), dgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0, nbx, bpf, count);
    else if (interp == IMP_INTER_LINEAR)
        hipLaunchKernelGGL((k_resize_2x_roll<2, M_LINEAR>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
    else if (interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_2x_roll<4, M_CUBIC>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, (a.dw * 4) & ~7);
    else
        hipLaunchKernelGGL((k_resize_2x_roll<8, M_LANCZOS>), rgrid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
}

// Does the frame take the CUBIC enlargement kernels (k_resize_up_cubic3 / 4, alone or in a mixed launch)?  The one test:
// launch_tapped and classify_mixed both ask it.  y must not shrink (the footprint advances by at most one row per
// destination row), x may shrink up to 2x (a strip's source columns fit the LDS patch), and the kernels index a frame's
// destination bytes in 32 bits.
static bool up_cubic_takes(int cn, int interp, double scale_x, double scale_y, int sw, int dh, int dstep) {
    return (cn == 3 || cn == 4) && interp == IMP_INTER_CUBIC && scale_y <= 1.0 && scale_x <= 2.0 && sw >= 4 &&
           (long long)dh * dstep < (1LL << 32);
}

// Rows per wave chunk of the CUBIC enlargement kernels: as many as keep the chunk's source footprint (strip columns x
// footprint rows, from the bound floor(n * scale) + 1 on how far n + 1 sample positions spread, + 3 taps + 1) inside the
// wave's LDS patch, at most UP_ROWS -- mandatory, per frame; fewer when `frames` frames like this one would not fill the
// chip otherwise (a lone launch: its frame count; a mixed launch: the frames of the call).
static int up_rows_per_wave(int cn, int dw, int dh, double scale_x, double scale_y, long long frames) {
    const int nbx = (dw + 255) / 256;                   // four 64-column strips per block, one per wave
    const int wmax = (int)std::floor(63 * scale_x) + 6;
    const int pitch = cn == 3 ? ((wmax * 3 + 3) & ~3) + 4 : wmax, cap = cn == 3 ? UP_CAP3_BYTES : UP_CAP_PX;
    int rpw = UP_ROWS;
    while (rpw > 4 && ((int)std::floor((rpw - 1) * scale_y) + 6) * pitch > cap) rpw -= 4;
    while (rpw > 16 && (long long)nbx * 4 * ((dh + rpw - 1) / rpw) * frames < 8192) rpw -= rpw > 64 ? 64 : 16;
    return rpw;
}

// enlargement of a 3-channel frame (every JPEG): the BGRA kernel's structure on bytes
static void launch_up_cubic_bgr(const RArgs& a, int count, double scale_x, double scale_y, const TableSet& ts, hipStream_t s) {
    const int nbx = (a.dw + 255) / 256;
    const int rpw = up_rows_per_wave(3, a.dw, a.dh, scale_x, scale_y, count);
    const int ncy = (a.dh + rpw - 1) / rpw;
    with_const<1, 4>(ts.up_period, [&](auto K) {             // (see launch_up_cubic_bgra)
        constexpr int PS = K() == 1 ? 0 : K();
        hipLaunchKernelGGL(k_resize_up_cubic3<PS>, dim3((unsigned)(nbx * ncy), (unsigned)count), dim3(256), 0, s, a, ts.xofs, ts.xco, ts.yco,
                           (const UpRow*)ts.yrows, (a.dw * 3) & ~7, nbx, rpw);
    });
}

// enlargement (bridge.c:190's CUBIC case): wave-private strips, float H sums in a register ring
static void launch_up_cubic_bgra(const RArgs& a, int count, double scale_x, double scale_y, const TableSet& ts, hipStream_t s) {
    const int nbx = (a.dw + 255) / 256;                 // four 64-column strips per block, one per wave
    const int rpw = up_rows_per_wave(4, a.dw, a.dh, scale_x, scale_y, count);
    const int ncy = (a.dh + rpw - 1) / rpw;
    const dim3 ugrid((unsigned)(nbx * ncy), (unsigned)count);
    with_const<1, 4>(ts.up_period, [&](auto K) {             // 2, 3, 4 when every per-th row (and no other) advances the footprint; else 0
        constexpr int PS = K() == 1 ? 0 : K();
        hipLaunchKernelGGL(k_resize_up_cubic4<PS>, ugrid, dim3(256), 0, s, a, ts.xofs, ts.xco, ts.yco, (const UpRow*)ts.yrows, (a.dw * 4) & ~7, nbx, rpw);
    });
}

// every other scale up to 2 and every other enlargement: rolling strips with a dynamic footprint advance
// (BGR windows are fetched as aligned dwords: rows 4-byte aligned, which every frame of the library has)
template <int CN>
static void launch_strips(const RArgs& a, int count, int interp, const TableSet& ts, hipStream_t s) {
    const dim3 block(256);
    constexpr int C34 = CN == 3 ? 3 : 4;
    const int nsx = (a.dw + 255) / 256;
    int rps = 64;
    while (rps > 8 && (long long)count * nsx * 4 * ((a.dh + rps - 1) / rps) < 8192) rps /= 2;
    const dim3 sgrid((unsigned)nsx, (unsigned)((a.dh + rps - 1) / rps), (unsigned)count);
    const int ks = interp == IMP_INTER_LINEAR ? 2 : interp == IMP_INTER_CUBIC ? 4 : 8;
    const int pat = ts.strip_a0 * 4 + ts.strip_a1;          // (1,0) 4, (0,1) 1, (1,2) 6, (2,1) 9; rps is a multiple of the 2 * ks row block
    const bool periodic = ts.strip_a0 >= 0 && rps % (2 * ks) == 0;
    const int ve = interp == IMP_INTER_CUBIC ? (a.dw * CN) & ~7 : 0;
    // the patch stores are 16 bytes (BGR: 4) at row start + a multiple of 256 (192): rows and frames aligned to that
    const int wide = !(((uintptr_t)a.dst | (uintptr_t)a.dstep | (uintptr_t)a.dst_stride) & (CN == 4 ? 15 : 3));
#define IMP_STRIP2(KS_, MODE_, A0_, A1_) hipLaunchKernelGGL((k_resize_strip2<KS_, MODE_, C34, A0_, A1_>), sgrid, block, 0, s, a, ts.xofs, ts.xco, ts.srows, ve, rps, wide)
    if (periodic && interp == IMP_INTER_LINEAR && pat == 4) IMP_STRIP2(2, M_LINEAR, 1, 0);
    else if (periodic && interp == IMP_INTER_LINEAR && pat == 1) IMP_STRIP2(2, M_LINEAR, 0, 1);
    else if (periodic && interp == IMP_INTER_LINEAR && pat == 6) IMP_STRIP2(2, M_LINEAR, 1, 2);
    else if (periodic && interp == IMP_INTER_LINEAR && pat == 9) IMP_STRIP2(2, M_LINEAR, 2, 1);
    else if (periodic && interp == IMP_INTER_LANCZOS4 && pat == 4) IMP_STRIP2(8, M_LANCZOS, 1, 0);
    else if (periodic && interp == IMP_INTER_LANCZOS4 && pat == 1) IMP_STRIP2(8, M_LANCZOS, 0, 1);
    else if (periodic && interp == IMP_INTER_LANCZOS4 && pat == 6) IMP_STRIP2(8, M_LANCZOS, 1, 2);
    else if (periodic && interp == IMP_INTER_LANCZOS4 && pat == 9) IMP_STRIP2(8, M_LANCZOS, 2, 1);
    else if (periodic && interp == IMP_INTER_CUBIC && pat == 6) IMP_STRIP2(4, M_CUBIC, 1, 2);      // (CUBIC comes here only when y shrinks)
    else if (periodic && interp == IMP_INTER_CUBIC && pat == 9) IMP_STRIP2(4, M_CUBIC, 2, 1);
#undef IMP_STRIP2
    else if (interp == IMP_INTER_LINEAR)
        hipLaunchKernelGGL((k_resize_strip<2, M_LINEAR, C34>), sgrid, block, 0, s, a, ts.xofs, ts.xco, ts.srows, 0, rps);
    else if (interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_strip<4, M_CUBIC, C34>), sgrid, block, 0, s, a, ts.xofs, ts.xco, ts.srows, ve, rps);
    else
        hipLaunchKernelGGL((k_resize_strip<8, M_LANCZOS, C34>), sgrid, block, 0, s, a, ts.xofs, ts.xco, ts.srows, 0, rps);
}

template <int CN>
static void launch_taps(const RArgs& a, int interp, const TableSet& ts, dim3 grid, hipStream_t s) {
    const dim3 block(256);
    if (interp == IMP_INTER_LINEAR)
        hipLaunchKernelGGL((k_resize_taps<2, CN, M_LINEAR>), grid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
    else if (interp == IMP_INTER_CUBIC)
        hipLaunchKernelGGL((k_resize_taps<4, CN, M_CUBIC>), grid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco,
                           (a.dw * CN) & ~7);
    else
        hipLaunchKernelGGL((k_resize_taps<8, CN, M_LANCZOS>), grid, block, 0, s, a, ts.xofs, ts.xco, ts.yofs, ts.yco, 0);
}

template <int CN>
static int launch_tapped(const RArgs& a, int count, int interp, double scale_x, double scale_y, dim3 grid, hipStream_t s) {
    TableSet ts;
    if (int rc = get_tables(interp, a.sw, a.sh, a.dw, a.dh, scale_x, scale_y, s, &ts)) return rc;
    // both scales <= 2: neighbouring outputs share taps -> LDS-tiled separable kernel (BGRA)
    if (CN == 3 && ts.step2 && a.sw >= 8 && interp != IMP_INTER_LINEAR) launch_2x_bgr(a, count, interp, ts, s);
    else if (CN == 4 && ts.step2 && a.sw >= 8) launch_2x_bgra(a, count, interp, ts, s);
    else if (CN == 3 && up_cubic_takes(CN, interp, scale_x, scale_y, a.sw, a.dh, a.dstep)) launch_up_cubic_bgr(a, count, scale_x, scale_y, ts, s);
    else if (CN == 4 && up_cubic_takes(CN, interp, scale_x, scale_y, a.sw, a.dh, a.dstep)) launch_up_cubic_bgra(a, count, scale_x, scale_y, ts, s);
    else if ((CN == 4 || CN == 3) && scale_x <= 2.0 && scale_y <= 2.0 && a.sw >= 8 &&
             (CN == 4 || !(((uintptr_t)a.src | (uintptr_t)a.sstep | (uintptr_t)a.src_stride) & 3))) launch_strips<CN>(a, count, interp, ts, s);
    else launch_taps<CN>(a, interp, ts, grid, s);
    return launched();
}

template <int CN>
static int launch_cn(const RArgs& a, int count, int interp, double scale_x, double scale_y, hipStream_t s) {
    const dim3 block(256), grid((unsigned)(((long long)a.dw * a.dh + 255) / 256), (unsigned)count);
    if (interp == IMP_INTER_NN) {
        hipLaunchKernelGGL((k_resize_nn<CN>), grid, block, 0, s, a, scale_x, scale_y);
        return launched();
    }
    if (interp == IMP_INTER_AREA)
        return whole_factors(scale_x, scale_y) ? launch_area_whole<CN>(a, count, scale_x, scale_y, grid, s)
                                               : launch_area_general<CN>(a, count, interp, scale_x, scale_y, grid, s);
    return launch_tapped<CN>(a, count, interp, scale_x, scale_y, grid, s);
}

// ------------------------------------------------------------------ fused AREA 2x2 + rotate 90/270 (BGRA)
// cfg3's resize=960,540 followed by filter-rotate=90: cvResize(AREA) with both scales exactly 2 is
// (a+b+c+d+2)>>2 per channel, and the rotation (cvTranspose + cvFlip, filters.c:116-119) is a pure
// permutation, so the two are one pass: a block averages a TX x TY tile of the halved image (two 16-byte
// non-temporal loads per two outputs, all issued before the first use), parks it in an odd-pitch LDS
// tile and writes it transposed, 16 bytes per lane along destination rows.  The half-size intermediate
// never exists in HBM.  Measured on cfg3: reads alone run at 6.8 TB/s; the 2.1 GB of scattered stores
// add ~1.1 ms whatever their width, cache policy or run length (128x32 tiles are the best of four shapes).
__device__ __forceinline__ uint32_t box2x2(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t o = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
        const uint32_t sum = ((a >> (8 * ch)) & 0xff) + ((b >> (8 * ch)) & 0xff) + ((c >> (8 * ch)) & 0xff) + ((d >> (8 * ch)) & 0xff) + 2;
        o |= (sum >> 2) << (8 * ch);
    }
    return o;
}

template <int TX, int TY>      // tile of the halved image: TX columns x TY rows, 4096 pixels or a multiple
__global__ __launch_bounds__(256) void k_area2x2_rotate_bgra(RArgs a, int amount, int rw, int rh, int ntx, int nty, int count, OverlayArgs wm) {
    __shared__ uint32_t tile[TY][TX + 1];                     // odd pitch: the transposed read is bank-conflict free
    // Block order: a group of 8 frames is dealt one frame per XCD (linear id mod 8), and inside a frame the tiles of
    // one tile column are walked top to bottom back to back.  Vertically adjacent tiles store neighbouring column
    // segments of the SAME destination rows, so those partial rows meet in one L2 before they are written back.
    const long long lin = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const int tpf = ntx * nty;
    const long long q = lin >> 3;
    const int frame = (int)(q / tpf) * 8 + (int)(lin & 7);
    if (frame >= count) return;
    const int t = (int)(q % tpf);
    const int bx = t / nty, by = t - bx * nty;
    const uint8_t* S = a.src + (long long)frame * a.src_stride;
    uint8_t* D = a.dst + (long long)frame * a.dst_stride;
    const int rx0 = bx * TX, ry0 = by * TY;                   // tile origin in the halved (pre-rotation) image
    const int tid = threadIdx.x;
    {   // (1) each thread averages two neighbouring outputs per row from two 16-byte loads.  Addresses are clamped into
        // the frame so all loads of a batch issue back to back with no branch between them; only the LDS stores are
        // predicated.  Tiles of more than 4096 pixels take the rows in batches of eight passes (register budget).
        constexpr int LPR = TX / 2;                           // lanes per tile row
        constexpr int RPP = 256 / LPR;                        // rows per pass
        constexpr int NPT = TY / RPP;                         // passes in all
#ifndef CHAIN_NP
#define CHAIN_NP 8
#endif
        constexpr int NP = NPT < CHAIN_NP ? NPT : CHAIN_NP;   // passes per batch
        static_assert(NPT % NP == 0, "tile rows must split into whole batches");
        const int lx = (tid % LPR) * 2, ty = tid / LPR;
        const int rx = rx0 + lx;
        const int rxc = min(rx, rw - 2);                      // launcher guarantees rw >= 2
#pragma unroll 1
        for (int b0 = 0; b0 < NPT; b0 += NP) {
            uint32_t t0[NP][4], t1[NP][4];
#pragma unroll
            for (int r = 0; r < NP; r++) {
                const int ryc = min(ry0 + ty + RPP * (b0 + r), rh - 1);
                const uint8_t* p = S + (size_t)(2 * ryc) * a.sstep + (size_t)rxc * 8;
                load_stream<4>(t0[r], p);
                load_stream<4>(t1[r], p + a.sstep);
            }
#pragma unroll
            for (int r = 0; r < NP; r++) {
                const int ly = ty + RPP * (b0 + r);
                if (ry0 + ly < rh) {
                    if (rx + 1 < rw) {
                        tile[ly][lx] = box2x2(t0[r][0], t0[r][1], t1[r][0], t1[r][1]);
                        tile[ly][lx + 1] = box2x2(t0[r][2], t0[r][3], t1[r][2], t1[r][3]);
                    } else if (rx < rw) {                      // odd rw: the clamped window ends on this pixel
                        tile[ly][lx] = box2x2(t0[r][2], t0[r][3], t1[r][2], t1[r][3]);
                    }
                }
            }
        }
    }
    __syncthreads();
    // (2) destination: 90 -> R[i][j] = H[rh-1-j][i], 270 -> R[i][j] = H[j][rw-1-i]  (H = halved image; R is rh wide, rw tall).
    // A lane gathers FOUR consecutive destination pixels (four H rows of one H column) from the tile and stores them as
    // one 16-byte vector: TY/4 lanes cover a TY*4-byte run of a destination row.
    {
        constexpr int LPC = TY / 4;                           // lanes per H column
        constexpr int CPP = 256 / LPC;                        // H columns per pass
        constexpr int NP2 = TX / CPP;
        const int q = tid % LPC, col = tid / LPC;
#pragma unroll
        for (int r = 0; r < NP2; r++) {
            const int l = col + CPP * r;                       // H column inside the tile
            const int rx = rx0 + l;
            const int ryb = ry0 + 4 * q;                       // first of the four H rows
            if (rx >= rw || ryb >= rh) continue;
            uint32_t v[4];
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = tile[4 * q + j][l];
            const int dy = amount == 90 ? rx : rw - 1 - rx;
            uint8_t* drow = D + (size_t)dy * a.dstep;
            if (ryb + 3 < rh) {
                uint32_t o4[4];
                const int dx0 = amount == 90 ? rh - 1 - (ryb + 3) : ryb;      // dx = rh-1-ry descends for 90: reverse the four
#pragma unroll
                for (int j = 0; j < 4; j++) o4[j] = amount == 90 ? v[3 - j] : v[j];
                // Watermark (bridge.c:629-640, AlphaBlendOver filters.c:619-662) on the way out: the few tiles under the
                // overlay rectangle blend their pixels before the store; everyone else pays one wave-uniform-ish test
                if (wm.ov && dy >= wm.ry && dy < wm.ry + wm.maxrow && dx0 + 3 >= wm.rx && dx0 < wm.rx + wm.maxcol) {
                    const uint8_t* orow = wm.ov + (size_t)(dy - wm.ry) * wm.ostep;
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int ox = dx0 + j - wm.rx;
                        if (ox >= 0 && ox < wm.maxcol) o4[j] = blend_over_bgra(o4[j], *(const uint32_t*)(orow + (size_t)ox * 4), wm.alpha);
                    }
                }
                const u32x4_t o = {o4[0], o4[1], o4[2], o4[3]};
                *(u32x4_t*)(drow + (size_t)dx0 * 4) = o;
            } else {
                for (int j = 0; j < 4 && ryb + j < rh; j++) {
                    const int dx = amount == 90 ? rh - 1 - (ryb + j) : ryb + j;
                    uint32_t px = v[j];
                    if (wm.ov && dy >= wm.ry && dy < wm.ry + wm.maxrow && dx >= wm.rx && dx < wm.rx + wm.maxcol)
                        px = blend_over_bgra(px, *(const uint32_t*)(wm.ov + (size_t)(dy - wm.ry) * wm.ostep + (size_t)(dx - wm.rx) * 4), wm.alpha);
                    *(uint32_t*)(drow + (size_t)dx * 4) = px;
                }
            }
        }
    }
}

// Streaming form of the same chain (for even halved widths; odd ones take the block-tile kernel above): no block-wide phases.  A WAVE owns SW = 128 columns of the halved image and a band of BH = 32 rows; it reads its
// two source rows per halved row as one contiguous KB each, four halved rows per batch with the next batch already in
// flight, boxes them into a wave-private LDS band tile and, once the band is full, writes it out turned: BH pixels per
// destination row, 16 bytes per lane.  The four waves of a block take four consecutive bands of one strip, so a block
// leaves 4 * BH contiguous pixels in each destination row and the runs of neighbouring bands meet in one L2.  Measured on
// cfg3 (1024 frames): 64x64 block tiles 495-521 k img/s, this kernel 128x32 518-545 k (+4.5..7 %), 64x64 / 64x32 strips
// 465 k, 128x16 460 k, 128x64 376 k (132 KB of LDS: one block per CU), non-temporal stores 428 k.
template <int SW, int BH>      // strip width and band height in halved pixels
__global__ __launch_bounds__(256) void k_area2x2_turn(RArgs a, int amount, int rw, int rh, int nstrips, int nbands, int bpf, int count,
                                                      OverlayArgs wm) {
    constexpr int LPR = SW / 2;                                 // lanes per halved row (a lane boxes two neighbouring outputs)
    constexpr int RPI = 64 / LPR;                               // halved rows per wave-instruction
    extern __shared__ uint32_t s_dyn[];                         // [4 waves][BH][SW + 1]
    int frame, blk;
    if (!frame_block(bpf, count, &frame, &blk)) return;
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int item = blk * 4 + wv;                              // band fastest: the waves of a block are neighbours in y
    const int strip = item / nbands, band = item - strip * nbands;
    if (strip >= nstrips) return;
    uint32_t* tile = s_dyn + wv * (BH * (SW + 1));
    const int hx0 = strip * SW, hy0 = band * BH;
    const int nb = min(BH, rh - hy0);
    const int ncol = min(SW, rw - hx0);                         // even (launcher)
    const int rsub = lane / LPR, g = lane - rsub * LPR;         // this lane's row inside an instruction's group, its granule
    const bool have = 2 * g < ncol;
    const uint8_t* S = a.src + (long long)frame * a.src_stride + (size_t)(2 * hy0) * a.sstep + (size_t)(hx0 * 2 + (have ? g * 4 : 0)) * 4;
    uint32_t cur[4][2][4], nxt[4][2][4];
    auto fetch = [&](int r0, uint32_t (&v)[4][2][4]) {          // halved rows r0 .. r0 + 4 * RPI - 1 of the band (clamped: repeats are dropped later)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint8_t* p = S + (size_t)(2 * min(r0 + u * RPI + rsub, nb - 1)) * a.sstep;
            load_stream<4>(v[u][0], p);
            load_stream<4>(v[u][1], p + a.sstep);
        }
    };
    fetch(0, cur);
    for (int r0 = 0; r0 < nb; r0 += 4 * RPI) {
        if (r0 + 4 * RPI < nb) fetch(r0 + 4 * RPI, nxt);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int r = r0 + u * RPI + rsub;
            if (r < nb) {
                tile[r * (SW + 1) + 2 * g] = box2x2(cur[u][0][0], cur[u][0][1], cur[u][1][0], cur[u][1][1]);
                tile[r * (SW + 1) + 2 * g + 1] = box2x2(cur[u][0][2], cur[u][0][3], cur[u][1][2], cur[u][1][3]);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int t = 0; t < 4; t++) cur[u][h][t] = nxt[u][h][t];
    }
    asm volatile("" ::: "memory");
    // R[i][j] = H[rh-1-j][i] (90), H[j][rw-1-i] (270)
    uint8_t* D = a.dst + (long long)frame * a.dst_stride;
    const int nq = (nb + 3) >> 2;
    const int j0 = amount == 90 ? rh - (hy0 + nb) : hy0;
    for (int t = lane; t < ncol * nq; t += 64) {
        const int col = t / nq, qi = t - col * nq;
        const int hx = hx0 + col;
        const int orow = amount == 90 ? hx : rw - 1 - hx;
        uint32_t v[4];
#pragma unroll
        for (int jj = 0; jj < 4; jj++) {
            const int k = 4 * qi + jj;
            const int r = amount == 90 ? nb - 1 - k : k;
            v[jj] = overlay_px(wm, tile[min(max(r, 0), nb - 1) * (SW + 1) + col], orow, j0 + k);
        }
        uint8_t* q = D + (size_t)orow * a.dstep + (size_t)(j0 + 4 * qi) * 4;
        if (4 * qi + 4 <= nb) {
            const u32x4_t o4 = {v[0], v[1], v[2], v[3]};
            *(u32x4_t*)q = o4;                                  // (temporal on purpose: neighbouring bands' runs meet in L2; nt measured -20 %)
        } else {
            for (int jj = 0; 4 * qi + jj < nb; jj++) *(uint32_t*)(q + 4 * jj) = v[jj];
        }
    }
}

// src: sw x sh BGRA with sw = 2*rw, sh = 2*rh; dst: rh x rw (rotated).  Returns IMP_ERROR_UNSUPPORTED when the
// geometry is not the exact-2x BGRA case so the caller can fall back to resize + rotate.
int launch_area2x2_rotate(const Frames& f, int amount, const OverlayArgs* overlay, hipStream_t s) {
    const View& v = f.v;
    if (v.c != 4 || (amount != 90 && amount != 270) || (v.w & 1) || (v.h & 1)) return IMP_ERROR_UNSUPPORTED;
    const int rw = v.w / 2, rh = v.h / 2;
    if (rw < 2 || rh < 1) return IMP_ERROR_UNSUPPORTED;
    if (f.dw != rh || f.dh != rw || f.count <= 0 || f.count > 65535) return IMP_ERROR_UNSUPPORTED;
    if (((uintptr_t)f.src | (uintptr_t)v.step | (uintptr_t)f.src_stride) & 15) return IMP_ERROR_UNSUPPORTED;   // 16-byte loads
    if (((uintptr_t)f.dst | (uintptr_t)f.dstep | (uintptr_t)f.dst_stride) & 3) return IMP_ERROR_UNSUPPORTED;
    const RArgs a = rargs(f);
    const dim3 block(256);
    OverlayArgs wm{};
    if (overlay) wm = *overlay;
    if (!(rw & 1)) {
        constexpr int sw = 128, bh = 32;
        const int nstrips = (rw + sw - 1) / sw, nbands = (rh + bh - 1) / bh, bpf = (nstrips * nbands + 3) / 4;
        const dim3 sgrid((unsigned)bpf, round_up8(f.count));
        const size_t lds = (size_t)4 * bh * (sw + 1) * 4;
        hipError_t e = lds_limit_once<k_area2x2_turn<sw, bh>>();
        if (e == hipSuccess) {
            hipLaunchKernelGGL((k_area2x2_turn<sw, bh>), sgrid, block, lds, s, a, amount, rw, rh, nstrips, nbands, bpf, f.count, wm);
            e = hipGetLastError();
        }
        if (e != hipSuccess) { set_error("k_area2x2_turn", e); return IMP_ERROR_DEVICE; }
        return IMP_OK;
    }
    // odd halved widths: 64x64 block tiles, walked one tile column at a time (profiles/r01_chain_tiles.txt)
    const int ntx = (rw + 63) / 64, nty = (rh + 63) / 64;
    const dim3 grid((unsigned)(ntx * nty), round_up8(f.count));
    hipLaunchKernelGGL((k_area2x2_rotate_bgra<64, 64>), grid, block, 0, s, a, amount, rw, rh, ntx, nty, f.count, wm);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

int launch_cv_resize(const Frames& f, int interp, hipStream_t s) {
    if (f.count <= 0) return IMP_OK;
    if (f.count > 65535) return IMP_ERROR_INVALID_ARGS;
    if (interp < IMP_INTER_NN || interp > IMP_INTER_LANCZOS4) return IMP_ERROR_INVALID_ARGS;
    const View& v = f.v;
    if (!f.src || !f.dst || (v.c != 1 && v.c != 3 && v.c != 4)) return IMP_ERROR_INVALID_ARGS;
    // what the kernels index in 32 bits (pixels, row bytes, bytes inside a frame) has to fit: 64-bit checks, before any launch
    if (!view_fits(v.w, v.h, v.c, v.step) || !view_fits(f.dw, f.dh, v.c, f.dstep)) return IMP_ERROR_INVALID_ARGS;
    if (f.count > 1 && (f.src_stride < 0 || f.dst_stride < 0)) return IMP_ERROR_INVALID_ARGS;
    // cv::resize: scale = 1 / ((double)dsize / ssize)
    const double scale_x = 1. / ((double)f.dw / v.w), scale_y = 1. / ((double)f.dh / v.h);
    // the reference requests AREA only when neither axis grows (bridge.c:190)
    if (interp == IMP_INTER_AREA && !(scale_x >= 1 && scale_y >= 1)) return IMP_ERROR_INVALID_ARGS;
    if (v.c == 4 && (((uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)v.step | (uintptr_t)f.dstep |
                      (uintptr_t)f.src_stride | (uintptr_t)f.dst_stride) & 3))
        return IMP_ERROR_INVALID_ARGS;    // BGRA rows must be 4-byte aligned (cvCreateImage guarantees it)
    const RArgs a = rargs(f);
    switch (v.c) {
        case 1: return launch_cn<1>(a, f.count, interp, scale_x, scale_y, s);
        case 3: return launch_cn<3>(a, f.count, interp, scale_x, scale_y, s);
        case 4: return launch_cn<4>(a, f.count, interp, scale_x, scale_y, s);
    }
    return IMP_ERROR_INVALID_ARGS;
}

// Resize() over `count` frames of different geometry with as few launches as the mix allows.  Per frame the
// interpolation is the reference's (bridge.c:183-193) and the arithmetic is launch_cv_resize's.  classify_mixed names a
// frame's class and fills its descriptor: frames that take the general AREA path (every non-integer shrink whose cells
// span at most 20 source columns) are gathered into a k_resize_area_mix launch with their weights computed in the kernel,
// frames whose cells span 21..66 columns (area_wide_plan: shrinks past 18x, up to 64x; any channel count, pointer and
// pitch -- aligned and off-grid BGR frames ride the same launch, the fetch mode travels in the descriptor) into a
// k_resize_area_wide_mix launch, whole-factor AREA frames (any channel count) into a k_area_int_mix launch and NN frames
// into a k_resize_nn_mix launch, and BGR / BGRA enlargements (CUBIC, neither axis shrinking in y: up_cubic_takes) into a
// k_resize_up_cubic_mix launch that carries their tables -- five launches at most per channel count (an enlargement
// launch splits when its tables pass UP_MIX_BLOB_BYTES); a frame that is the only one of its class, and the rest (gray
// enlargements, frames of which one axis grows while y shrinks, enlargements whose x shrinks past 2x; extreme ratios:
// cells past 66 columns) go one launch each on the same stream.  Gray frames are gathered like colour ones: their
// general AREA shrinks ride k_resize_area_mix<1> whatever their pointers and pitches are.
// Blocks differ a hundredfold in work (a 4K source against a 256-pixel one, same 224-wide output): each launch deals its
// frames longest source first to the XCD list with the least source bytes so far (mix_launch), so each list starts with
// its heavy frames and the launch's tail is made of light ones.
template <class D, class L>
static int launch_by_source(std::vector<D>& v, hipStream_t s, L launch) {
    return mix_launch(v, [](D& d) { return (long long)d.a.sw * d.a.sh; }, s, launch);
}

static int launch_mix(std::vector<MixDesc>& v, int cn, hipStream_t s) {
    return launch_by_source(v, s, [&](dim3 grid, const MixDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_resize_area_mix<4>), grid, dim3(256), 0, s, dev, ix);
        else if (cn == 3) hipLaunchKernelGGL((k_resize_area_mix<3>), grid, dim3(256), 0, s, dev, ix);
        else hipLaunchKernelGGL((k_resize_area_mix<1>), grid, dim3(256), 0, s, dev, ix);
    });
}

// The descriptor of one whole-factor AREA frame.  Its body is the one launch_cn picks for the frame alone, with three
// exceptions (same bytes, the bodies being generic in CN and ISX): BGRA 2 x k (k != 2) and BGRA 8 x k run
// area_boxl_body<4, 2> / <4, 8>, instances no lone kernel has (alone: k_resize_area_int, k_area_boxc<8>), and BGRA 2 x 2
// of an even width runs k_area2x2_v4's body, not k_area2x2_c4's.
static IntMixDesc int_mix_desc(const MixFrame& f, int cn, int isx, int isy) {
    IntMixDesc d{};
    d.a = rargs(f);
    d.isx = isx;
    d.isy = isy;
    d.scale = 1.f / (float)(isx * isy);
    const bool rows4 = !(((uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)f.sstep | (uintptr_t)f.dstep) & 3);
    if (cn != 1 && rows4 && isx == 2 && isy == 2) {
        d.cls = IM_2X2;
        d.per_row = (f.dw + 3) / 4;
        d.nblk = (int)(((long long)d.per_row * f.dh + 255) / 256);
    } else if (cn != 1 && rows4 && isx >= 2 && isx <= 8 && (long long)isx * isy <= 257) {
        d.cls = IM_BOXL;
        d.P = (4096 / (cn * isx)) & ~3;
        d.per_row = (f.dw + d.P - 1) / d.P;
        d.nblk = (int)(((long long)d.per_row * f.dh + 3) / 4);
    } else {
        d.cls = IM_PIXEL;
        d.nblk = (int)(((long long)f.dw * f.dh + 255) / 256);
    }
    return d;
}

static int launch_int_mix(std::vector<IntMixDesc>& v, int cn, hipStream_t s) {
    size_t lds = 0;                                        // the largest any class present needs
    for (const IntMixDesc& d : v)
        if (d.cls == IM_BOXL) lds = 4 * BOXL_LINE * sizeof(uint32_t);
    return launch_by_source(v, s, [&](dim3 grid, const IntMixDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_area_int_mix<4>), grid, dim3(256), lds, s, dev, ix);
        else if (cn == 3) hipLaunchKernelGGL((k_area_int_mix<3>), grid, dim3(256), lds, s, dev, ix);
        else hipLaunchKernelGGL((k_area_int_mix<1>), grid, dim3(256), lds, s, dev, ix);
    });
}

static int launch_nn_mix(std::vector<NnMixDesc>& v, int cn, hipStream_t s) {
    return launch_by_source(v, s, [&](dim3 grid, const NnMixDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_resize_nn_mix<4>), grid, dim3(256), 0, s, dev, ix);
        else if (cn == 3) hipLaunchKernelGGL((k_resize_nn_mix<3>), grid, dim3(256), 0, s, dev, ix);
        else hipLaunchKernelGGL((k_resize_nn_mix<1>), grid, dim3(256), 0, s, dev, ix);
    });
}

// Frames area_wide_plan accepts, two or more: every line of the launch is as long as the longest one present.
static int launch_wide_mix(std::vector<MixDesc>& v, int cn, int line_bytes, hipStream_t s) {
    const int wpb = wide_wpb(line_bytes);
    for (MixDesc& d : v) d.nblk = (d.nitems + wpb - 1) / wpb;
    const size_t lds = (size_t)wpb * line_bytes;
    return launch_by_source(v, s, [&](dim3 grid, const MixDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_resize_area_wide_mix<4>), grid, dim3(64 * wpb), lds, s, dev, ix, line_bytes / 4, wpb);
        else if (cn == 3) hipLaunchKernelGGL((k_resize_area_wide_mix<3>), grid, dim3(64 * wpb), lds, s, dev, ix, line_bytes / 4, wpb);
        else hipLaunchKernelGGL((k_resize_area_wide_mix<1>), grid, dim3(64 * wpb), lds, s, dev, ix, line_bytes / 4, wpb);
    });
}

// Enlargements up_cubic_takes accepts, two or more.  Their tables TRAVEL WITH THE LAUNCH, in the blob behind the descriptor
// table, and are freed with it: nothing is put into, looked up in or evicted from the lane's TableCache, so a mixed stream
// of never-seen sizes costs no cache slot and no pool block per frame.  They are built exactly as get_tables builds them
// (build_tap_axis, up_rows; the built bytes of an axis are kept on the host: UpAxisMemo).  Within a launch frames share
// axes: one x table per (sw, dw), one y table per (sh, dh) -- a queue of same-size avatars uploads its tables once.
// UP_MIX_BLOB_BYTES bounds what one launch uploads, descriptors and tables together (a call holds up to 4096 requests and
// a 1080p destination's tables weigh 66 KB): when the next frame's tables would pass it, the frames gathered so far are
// launched and another launch begins.  Uploads past a ring segment (128 KB) go through the lane's staging buffers
// (upload_to), which start at 8 MB and wait for the device when they have to grow: half of that keeps every launch's
// upload inside a buffer that never regrows.  The launch's bytes are laid out before anything is built (a table's size
// follows from its axis), so every axis image is copied once into its place behind the space left for the descriptors and
// the whole leaves the host through one copy (mix_launch's `whole`).  A single frame whose own tables pass the bound (destinations past ~250 000 rows + columns) still goes, alone in its launch.
constexpr size_t UP_MIX_BLOB_BYTES = size_t(4) << 20;

// One axis of an enlargement as the bytes the mix kernel reads, in one piece: x -> xofs, then xco; y -> the UpRow rows
// (with their sentinel), then yco; every part a multiple of 16 bytes, the rows first so that a y image placed at a 32-byte
// multiple has them there.  Building one (build_tap_axis, up_rows: the float arithmetic of ~400 rows) is ~10 us, which for a
// call of a few dozen avatars was more than the launches it saved; a worker sees the same sizes again and again, so the
// images are kept per lane, HOST memory only (dropped with the lane; nothing on the device outlives a launch).  Bounded
// by UP_MEMO_BYTES: past it everything is dropped and the memo starts over -- a miss costs one build, as before.
constexpr size_t UP_MEMO_BYTES = size_t(16) << 20;
struct UpAxisMemo : LaneCache {
    std::map<std::tuple<int, int, bool>, std::vector<uint8_t>> m;
    size_t bytes = 0;
};
constexpr size_t up16(size_t n) { return (n + 15) & ~size_t(15); }
static size_t up_axis_bytes(int dsize, bool is_x) {
    return is_x ? up16((size_t)dsize * sizeof(int)) + up16((size_t)dsize * 4 * sizeof(short))
                : ((size_t)dsize + 1) * sizeof(UpRow) + up16((size_t)dsize * 4 * sizeof(short));
}
static void up_axis_build(int ssize, int dsize, bool is_x, std::vector<uint8_t>* out) {
    TapAxis ta;
    build_tap_axis(ssize, dsize, 1. / ((double)dsize / ssize), IMP_INTER_CUBIC, is_x, &ta);
    out->assign(up_axis_bytes(dsize, is_x), 0);
    if (is_x) {
        std::memcpy(out->data(), ta.ofs.data(), ta.ofs.size() * sizeof(int));
        std::memcpy(out->data() + up16((size_t)dsize * sizeof(int)), ta.coef.data(), ta.coef.size() * sizeof(short));
    } else {
        const std::vector<UpRow> yr = up_rows(ta, dsize, nullptr);     // (the mix kernel carries the generic advance only)
        std::memcpy(out->data(), yr.data(), yr.size() * sizeof(UpRow));
        std::memcpy(out->data() + yr.size() * sizeof(UpRow), ta.coef.data(), ta.coef.size() * sizeof(short));
    }
}
// copies the axis' image to `dst` (up_axis_bytes of it)
static void up_axis_put(int ssize, int dsize, bool is_x, uint8_t* dst) {
    LaneCache** slot = lane_cache_slot(1);
    if (!slot) {                                           // no lane: the upload will say so; build and forget
        std::vector<uint8_t> once;
        up_axis_build(ssize, dsize, is_x, &once);
        std::memcpy(dst, once.data(), once.size());
        return;
    }
    if (!*slot) *slot = new UpAxisMemo();
    UpAxisMemo& M = *static_cast<UpAxisMemo*>(*slot);
    auto it = M.m.find({ssize, dsize, is_x});
    if (it == M.m.end()) {
        const size_t n = up_axis_bytes(dsize, is_x);
        if (M.bytes + n > UP_MEMO_BYTES) { M.m.clear(); M.bytes = 0; }
        it = M.m.emplace(std::make_tuple(ssize, dsize, is_x), std::vector<uint8_t>()).first;
        up_axis_build(ssize, dsize, is_x, &it->second);
        M.bytes += n;
    }
    std::memcpy(dst, it->second.data(), it->second.size());
}

static int launch_up_mix(const std::vector<UpMixDesc>& frames, int cn, hipStream_t s) {
    size_t next = 0;
    while (next < frames.size()) {
        // the frames of this launch and where their axes will lie (sizes follow from the geometry: nothing is built yet)
        std::map<std::pair<int, int>, unsigned> xs, ys;    // (ssize, dsize) -> byte offset of the axis' image in the launch's tables
        std::vector<UpMixDesc> v;
        size_t tables = 0;
        for (; next < frames.size(); next++) {
            UpMixDesc d = frames[next];
            const std::pair<int, int> kx{d.a.sw, d.a.dw}, ky{d.a.sh, d.a.dh};
            auto ix = xs.find(kx), iy = ys.find(ky);
            size_t t = tables, xat = 0, yat = 0;
            if (ix == xs.end()) { xat = t; t += up_axis_bytes(d.a.dw, true); }
            if (iy == ys.end()) {
                t = (t + 31) & ~size_t(31);                // UpRow rows are read as 32-byte scalar rows (sizeof(UpMixDesc) % 32 == 0)
                yat = t;
                t += up_axis_bytes(d.a.dh, false);
            }
            if (!v.empty() && (v.size() + 1) * sizeof(UpMixDesc) + t > UP_MIX_BLOB_BYTES) break;
            if (ix == xs.end()) ix = xs.emplace(kx, (unsigned)xat).first;
            if (iy == ys.end()) iy = ys.emplace(ky, (unsigned)yat).first;
            tables = t;
            d.xofs = ix->second;
            d.xco = ix->second + (unsigned)up16((size_t)d.a.dw * sizeof(int));
            d.rows = iy->second;
            d.yco = iy->second + (unsigned)(((size_t)d.a.dh + 1) * sizeof(UpRow));
            v.push_back(d);
        }
        // descriptors in front (mix_launch writes them), every distinct axis once, straight into its place
        const size_t dbytes = mix_blob_offset<UpMixDesc>(v.size());
        std::vector<uint8_t> whole(dbytes + tables, 0);
        uint8_t* t = whole.data() + dbytes;
        for (const auto& x : xs) up_axis_put(x.first.first, x.first.second, true, t + x.second);
        for (const auto& y : ys) up_axis_put(y.first.first, y.first.second, false, t + y.second);
        const int rc = mix_launch(v, [](UpMixDesc& d) { return (long long)d.a.dw * d.a.dh; }, s,      // store- and VALU-bound: destination pixels
                                  [&](dim3 grid, const UpMixDesc* dev, const MixIndex& mi) {
            const uint8_t* dev_tables = (const uint8_t*)dev + dbytes;
            if (cn == 4) hipLaunchKernelGGL((k_resize_up_cubic_mix<4>), grid, dim3(256), 0, s, dev, mi, dev_tables);
            else hipLaunchKernelGGL((k_resize_up_cubic_mix<3>), grid, dim3(256), 0, s, dev, mi, dev_tables);
        }, nullptr, &whole);
        if (rc) return rc;
    }
    return IMP_OK;
}

// one frame of a mix through launch_cv_resize
static int launch_lone(const MixFrame& f, int cn, int interp, hipStream_t s) {
    Frames one{};
    one.src = f.src; one.src_stride = 0; one.v = View{f.src, f.sw, f.sh, cn, f.sstep};
    one.dst = f.dst; one.dst_stride = 0; one.dw = f.dw; one.dh = f.dh; one.dstep = f.dstep; one.count = 1;
    return launch_cv_resize(one, interp, s);
}

static void set_split(MixDesc* d, const RowSplit& r) { d->rows = r.bh; d->nstrips = r.nstrips; d->nitems = r.nitems; d->nblk = r.nblk; }

// The classes of a mixed launch, in the order they are launched, and the descriptor of a frame: the member its class names.
enum { MIX_LONE = -1, MIX_WHOLE = 0, MIX_NN, MIX_WIDE, MIX_ROWS, MIX_UP, MIX_CLASSES };
struct MixVerdict { MixDesc m; IntMixDesc whole; NnMixDesc nn; UpMixDesc up; int line_bytes; };

// The class of one frame of a mix of `count`, and its descriptor.  The rules are launch_cn's, except where a mix differs on
// purpose:
//  - four columns per lane needs `waves4 >= 2048` alone; a mix does not ask (its other frames fill the chip);
//  - the mix carries the even windows only (`even` of area_rows_plan): half the instances in one kernel;
//  - BGR rows that are not 4-byte aligned pick AREA_ROWS by `big` (blocks in the launch) alone and by `scale_y < 8` in a mix;
//  - the three whole-factor exceptions above int_mix_desc;
//  - a wide frame's `nblk` waits for launch_wide_mix: it follows the launch's longest line, known only once every frame is in;
//  - an enlargement (MIX_UP: exactly the frames launch_tapped sends to the CUBIC enlargement kernels, up_cubic_takes) runs
//    the generic footprint advance whatever its factor, and its table offsets wait for launch_up_mix, which builds the tables.
//    Its rows per wave are the lone launch's: the LDS bound per frame, the chip-fill reduction over the `count` frames of the call.
// MIX_LONE is what no descriptor launch takes: gray enlargements, frames of which one axis grows while y shrinks (the strip
// kernels), x shrinking past 2x beside a growing y, sources narrower than 4 columns, AREA cells past 66 columns.
static int classify_mixed(const MixFrame& f, int cn, int interp, int count, MixVerdict* out) {
    const double scale_x = 1. / ((double)f.dw / f.sw), scale_y = 1. / ((double)f.dh / f.sh);
    const bool whole = whole_factors(scale_x, scale_y);
    if (interp == IMP_INTER_NN) {
        NnMixDesc& d = out->nn = NnMixDesc{};
        d.a = rargs(f);
        d.scale_x = scale_x;
        d.scale_y = scale_y;
        d.nblk = (int)(((long long)f.dw * f.dh + 255) / 256);
        return MIX_NN;
    }
    if (interp == IMP_INTER_AREA && whole) {
        const int isx = (int)std::lrint(scale_x), isy = (int)std::lrint(scale_y);
        if ((long long)isx * f.dw == f.sw && (long long)isy * f.dh == f.sh) {      // (what `whole` means; the bodies' reads rest on it)
            out->whole = int_mix_desc(f, cn, isx, isy);
            return MIX_WHOLE;
        }
    }
    if (up_cubic_takes(cn, interp, scale_x, scale_y, f.sw, f.dh, f.dstep)) {
        UpMixDesc& u = out->up = UpMixDesc{};
        u.a = rargs(f);
        u.vec_end = (f.dw * cn) & ~7;
        u.nbx = (f.dw + 255) / 256;
        u.rows_per_wave = up_rows_per_wave(cn, f.dw, f.dh, scale_x, scale_y, count);
        u.nblk = u.nbx * ((f.dh + u.rows_per_wave - 1) / u.rows_per_wave);
        return MIX_UP;
    }
    if (interp != IMP_INTER_AREA || whole) return MIX_LONE;
    MixDesc& d = out->m = MixDesc{};
    d.a = rargs(f);
    d.gm = AreaGeom{scale_x, scale_y};
    if (cn == 1) {
        // gray: any pointer, any pitch (the bodies align their own fetches); the window decides -- up to 20 columns here,
        // past them area_wide_plan below
        int w1 = 0, p1 = 0, bh1 = 0;
        if (gray_rows_plan(f.sw, f.dw, f.dh, scale_x, count, &w1, &p1, &bh1)) {
            d.nv = p1 == 4 ? -w1 : w1;
            set_split(&d, row_split(f.dw, f.dh, 64 * p1, bh1));
            return MIX_ROWS;
        }
    }
    const bool aligned = !(((uintptr_t)f.src | (uintptr_t)f.sstep) & 3);
    const bool streams = cn == 4 || (cn == 3 && aligned && f.sw >= 6);      // area_rows_body / area_rows4_body take the frame
    int w4 = 0, bh4 = 0;
    if (streams && f.dw >= 160 && area_rows_plan(f.sw, f.sh, f.dw, f.dh, scale_x, count, false, &w4, &bh4) &&
        w4 >= 2 && w4 <= 5 && 255 * scale_x + w4 + 8 <= (cn == 4 ? 1024 : 1340)) {
        // windows of at most five pixels (factors below ~3.9): four destination columns per lane, like the uniform batches
        d.nv = -w4;
        set_split(&d, row_split(f.dw, f.dh, 256, bh4));
        return MIX_ROWS;
    }
    if (streams && area_rows_plan(f.sw, f.sh, f.dw, f.dh, scale_x, count, true, &d.nv, &d.rows)) {
        set_split(&d, row_split(f.dw, f.dh, 64, d.rows));
        return MIX_ROWS;
    }
    if (cn == 3) {
        // the widest cell decides the window: ceil(scale) <= widest <= floor(scale) + 2; the axis is walked only
        // when those two ends name different windows (a wider window than needed is still exact, only slower)
        const int nv_lo = ((int)std::ceil(scale_x) + 3) / 4, nv_hi = ((int)std::floor(scale_x) + 2 + 3) / 4;
        const int nv = nv_lo == nv_hi ? nv_hi : (area_max_count(f.sw, f.dw, scale_x) + 3) / 4;
        if (nv >= 1 && nv <= MIX_NV && f.sw >= 4 * nv) {
            d.nv = nv;
            d.rows = scale_y < 8 ? AREA_ROWS : 1;   // tall cells: sharing one boundary row in nine is not worth a quarter of the blocks
            d.nblk = (int)(((long long)f.dw * ((f.dh + d.rows - 1) / d.rows) + 255) / 256);
            d.nitems = 0;
            return MIX_ROWS;
        }
    }
    bool cover = false;
    if (area_wide_plan(f.sw, f.sh, f.dw, f.dh, cn, interp, f.src, f.sstep, 0, count, &d.nv, &d.rows, &out->line_bytes, &cover)) {
        d.nv = wide_nv(cn, d.nv, cover);
        set_split(&d, row_split(f.dw, f.dh, 64, d.rows));
        return MIX_WIDE;
    }
    return MIX_LONE;
}

int launch_resize_mixed(const MixFrame* fr, int count, int cn, int simple, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    if (!fr || (cn != 1 && cn != 3 && cn != 4)) return IMP_ERROR_INVALID_ARGS;
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every frame is well-formed
        const MixFrame& f = fr[i];
        if (!f.src || !f.dst || !view_fits(f.sw, f.sh, cn, f.sstep) || !view_fits(f.dw, f.dh, cn, f.dstep)) return IMP_ERROR_INVALID_ARGS;
        if (cn == 4 && (((uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)f.sstep | (uintptr_t)f.dstep) & 3)) return IMP_ERROR_INVALID_ARGS;
    }
    std::vector<IntMixDesc> whole_frames;                  // whole-factor AREA (resizeAreaFast_), any channel count
    std::vector<NnMixDesc> nn_frames;
    std::vector<MixDesc> wide_frames;                      // cells of 21..66 source columns (area_wide_plan)
    std::vector<MixDesc> rows_frames;                      // general AREA, cells of at most 20 columns
    int wide_line = 0;                                     // the longest LDS line among the wide frames, in bytes
    std::vector<UpMixDesc> up_frames;                      // CUBIC enlargements (up_cubic_takes)
    int members[MIX_CLASSES] = {0, 0, 0, 0, 0}, last[MIX_CLASSES] = {-1, -1, -1, -1, -1};   // frames of a class, and the latest of them
    rows_frames.reserve(count);
    for (int i = 0; i < count; i++) {
        const MixFrame& f = fr[i];
        const int interp = simple ? IMP_INTER_NN : ((f.dw > f.sw || f.dh > f.sh) ? IMP_INTER_CUBIC : IMP_INTER_AREA);   // bridge.c:188-192
        MixVerdict d;
        const int k = classify_mixed(f, cn, interp, count, &d);
        if (k == MIX_LONE) {
            if (int rc = launch_lone(f, cn, interp, s)) return rc;
            continue;
        }
        members[k]++;
        last[k] = i;
        if (k == MIX_WHOLE) whole_frames.push_back(d.whole);
        else if (k == MIX_NN) nn_frames.push_back(d.nn);
        else if (k == MIX_ROWS) rows_frames.push_back(d.m);
        else if (k == MIX_UP) up_frames.push_back(d.up);
        else {
            wide_frames.push_back(d.m);
            wide_line = std::max(wide_line, d.line_bytes);
        }
    }
    // a class of one keeps the lone launch and its tuned kernel; two or more share a descriptor launch.  The exception: a
    // single colour frame of MIX_ROWS rides k_resize_area_mix all the same (a gray one goes to k_resize_area<1> and its tables).
    for (int k = 0; k < MIX_CLASSES; k++) {
        int rc = IMP_OK;
        if (members[k] == 1 && (k != MIX_ROWS || cn == 1))
            rc = launch_lone(fr[last[k]], cn, k == MIX_NN ? IMP_INTER_NN : k == MIX_UP ? IMP_INTER_CUBIC : IMP_INTER_AREA, s);
        else if (k == MIX_WHOLE) rc = launch_int_mix(whole_frames, cn, s);
        else if (k == MIX_NN) rc = launch_nn_mix(nn_frames, cn, s);
        else if (k == MIX_WIDE) rc = launch_wide_mix(wide_frames, cn, wide_line, s);
        else if (k == MIX_UP) rc = launch_up_mix(up_frames, cn, s);
        else rc = launch_mix(rows_frames, cn, s);
        if (rc) return rc;
    }
    return IMP_OK;
}

int launch_area_tail_mixed(const TailItem* items, int count, int cn, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    if (!items || (cn != 3 && cn != 4)) return IMP_ERROR_INVALID_ARGS;
    std::vector<MixTailDesc> v((size_t)count);
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every item is one the lone launch takes
        const TailItem& it = items[i];
        if (it.v.c != cn || !it.v.d || !it.dst || !view_fits(it.v.w, it.v.h, cn, it.v.step)) return IMP_ERROR_INVALID_ARGS;
        if (it.rot != 0 && it.rot != 90 && it.rot != 180 && it.rot != 270) return IMP_ERROR_INVALID_ARGS;
        const bool swap = it.rot == 90 || it.rot == 270;
        if (!view_fits(swap ? it.dh : it.dw, swap ? it.dw : it.dh, cn, it.dstep)) return IMP_ERROR_INVALID_ARGS;
        if (it.has_wm && (!it.wm.ov || ((uintptr_t)it.wm.ov | (uintptr_t)it.wm.ostep) & 3)) return IMP_ERROR_INVALID_ARGS;
        Frames f{};
        f.src = it.v.d; f.v = it.v; f.dst = it.dst; f.dw = it.dw; f.dh = it.dh; f.dstep = it.dstep;
        f.count = count;                                   // (the band height follows the whole launch, as in launch_resize_mixed)
        int w = 0, bh = 0;
        if (!area_tail_plan(f, &w, &bh)) return IMP_ERROR_INVALID_ARGS;
        MixTailDesc& d = v[(size_t)i];
        d = MixTailDesc{};
        d.m.a = rargs(f);                                  // (strides 0: a frame per descriptor)
        d.m.gm = AreaGeom{1. / ((double)it.dw / it.v.w), 1. / ((double)it.dh / it.v.h)};
        d.m.nv = w;
        set_split(&d.m, row_split(it.dw, it.dh, 64, bh));
        d.tail.rot = it.rot;
        if (it.has_wm) d.tail.wm = it.wm;
        d.flat = it.flatten && cn == 4;
    }
    return mix_launch(v, [](MixTailDesc& d) -> MixDesc& { return d.m; }, [](MixTailDesc& d) { return (long long)d.m.a.sw * d.m.a.sh; }, s,
                      [&](dim3 grid, const MixTailDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_resize_area_mix_tail<4>), grid, dim3(256), 0, s, dev, ix);
        else hipLaunchKernelGGL((k_resize_area_mix_tail<3>), grid, dim3(256), 0, s, dev, ix);
    });
}

}  // namespace imp
