// imp_webp_lossy.h -- the lane code of the lossy WebP (VP8 key frame) encoder: what the five launches of imp_webp_lossy.hip
// run per lane, and what impgpu_webp_lossy_encode_host (imp_webp_lossy.cpp) runs one lane after the other (and under the
// sanitizers, tests/c/webp_lossy_fuzz.cpp).  The file is defined in include/impgpu.h ("LOSSY WEBP ANSWERS") and pinned by
// tests/webp_vp8_writer.py.
//
//   PLANES   vp8_planes_lane: a macroblock row of padded Y, U, V (and the alpha plane) from the frame, a gather per sample.
//   RECON    vp8_mb_phase: a macroblock in eight phases shared by 64 lanes through a Vp8Mb (LDS on the device): load, DC
//            values, partial mode costs, their sums, forward transforms, the Y2 block, quantise + reconstruct, store (the
//            samples come by vp8_mb_fetch, which the device issues a macroblock ahead).  The
//            lanes meet between phases; the rows of a frame meet through the border rows and progress counters of
//            k_vp8_recon.
//   TOKENS   vp8_mb_tokens: a macroblock's (probability, bit) records, contexts from the neighbours' stored flags.
//   BOOL     vp8_code_first, vp8_bool_put: a lane walks a partition's records through the boolean coder (Vp8Bool).
//   PACK     vp8_layout + vp8_write_headers: where the pieces go in the answer, and the bytes between them.
//
// Safe by construction: every index into a frame is clamped to w - 1 / h - 1; a record is dropped past VP8_MB_RECORDS and a
// coded byte past its region's size (neither happens: the bounds are the worst case of the token tree).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../include/impgpu.h"
#include "../../include/impgpu_vp8_tables.h"

#if defined(__HIPCC__)
#define IMP_VP8_HD __host__ __device__ __forceinline__
#else
#define IMP_VP8_HD inline
#endif

namespace imp {

constexpr int VP8_MAX_SIDE = 16383;
constexpr int VP8_WAVES = 8;                                           // macroblock rows k_vp8_recon keeps in flight at most
constexpr int VP8_BORDER_LDS = 112 * 1024;                             // its border rows' share of the LDS: fewer rows in flight past 7168 pixels a row
// records a macroblock makes at most: 25 blocks of a first "more?" bit and, per coefficient, 7 tree bits, 11 extra bits,
// the sign and the next "more?" bit
constexpr uint32_t VP8_MB_RECORDS = 25u * (1u + 16u * 20u);
constexpr uint32_t VP8_FIRST_RECORDS = 1094, VP8_MB_FIRST_RECORDS = 7; // the frame header's bits; skip flag + two modes
constexpr int VP8_PHASES = 8;
enum { VP8_DC = 0, VP8_V = 1, VP8_H = 2, VP8_TM = 3 };
// a macroblock's info word: bits 0..24 the blocks' non-zero flags (16 Y, 4 U, 4 V, Y2), 25..26 the luma mode, 27..28 chroma
constexpr uint32_t VP8_NZ_MASK = 0x1ffffffu;

struct Vp8Frame { const uint8_t* src; int w, h, c, step; };

IMP_VP8_HD uint8_t vp8_coef_prob(int type, int band, int ctx, int node) {
    static constexpr uint8_t T[1056] = IMPGPU_VP8_COEF_PROBS;
    return T[((type * 8 + band) * 3 + ctx) * 11 + node];
}
IMP_VP8_HD uint8_t vp8_update_prob(int i) {
    static constexpr uint8_t T[1056] = IMPGPU_VP8_UPDATE_PROBS;
    return T[i];
}
IMP_VP8_HD int vp8_dc_step(int qi) {
    static constexpr uint8_t T[128] = IMPGPU_VP8_DC_STEPS;
    return T[qi];
}
IMP_VP8_HD int vp8_ac_step(int qi) {
    static constexpr uint16_t T[128] = IMPGPU_VP8_AC_STEPS;
    return T[qi];
}
IMP_VP8_HD int vp8_zigzag(int i) {
    static constexpr uint8_t T[16] = {0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15};
    return T[i];
}
IMP_VP8_HD int vp8_band(int i) {
    static constexpr uint8_t T[17] = {0, 1, 2, 3, 6, 4, 5, 6, 6, 6, 6, 6, 6, 6, 6, 7, 0};
    return T[i];
}
IMP_VP8_HD uint8_t vp8_cat_prob(int cat, int i) {                       // categories 3..6
    static constexpr uint8_t T[4][11] = {{173, 148, 140}, {176, 155, 140, 135}, {180, 157, 141, 134, 130},
                                         {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129}};
    return T[cat - 3][i];
}

// ---------------------------------------------------------------- geometry, quantiser, sizes
inline int vp8_check_geometry(int w, int h, int c) {
    if (w <= 0 || h <= 0) return IMP_ERROR_INVALID_ARGS;
    if ((c != 1 && c != 3 && c != 4) || w > VP8_MAX_SIDE || h > VP8_MAX_SIDE) return IMP_ERROR_UNSUPPORTED;
    return IMP_OK;
}
IMP_VP8_HD int vp8_mbs(int side) { return (side + 15) >> 4; }
IMP_VP8_HD int vp8_partitions(int mbh) { return mbh >= 8 ? 8 : (mbh >= 4 ? 4 : (mbh >= 2 ? 2 : 1)); }
IMP_VP8_HD int vp8_quant_index(int quality) { return 127 - (127 * quality + 50) / 100; }
// q[]: y dc, y ac, y2 dc, y2 ac, uv dc, uv ac
IMP_VP8_HD void vp8_steps(int qi, int* q) {
    q[0] = vp8_dc_step(qi); q[1] = vp8_ac_step(qi);
    q[2] = vp8_dc_step(qi) * 2;
    q[3] = vp8_ac_step(qi) * 155 / 100;
    if (q[3] < 8) q[3] = 8;
    q[4] = vp8_dc_step(qi) > 132 ? 132 : vp8_dc_step(qi);
    q[5] = vp8_ac_step(qi);
}
IMP_VP8_HD void vp8_recips(const int* q, uint32_t* rq) {
    for (int k = 0; k < 6; k++) rq[k] = 0xffffffffu / (uint32_t)q[k];
}
// rows of partition p, and the bytes its coded form takes at most (a record codes to less than a byte; the flush is 4)
IMP_VP8_HD uint32_t vp8_partition_rows(int mbh, int nparts, int p) { return p < mbh ? (uint32_t)((mbh - p + nparts - 1) / nparts) : 0u; }
IMP_VP8_HD size_t vp8_partition_bound(int mbw, int mbh, int nparts, int p) {
    return (size_t)vp8_partition_rows(mbh, nparts, p) * (size_t)mbw * VP8_MB_RECORDS + 8u;
}
IMP_VP8_HD size_t vp8_first_bound(uint32_t nmb) { return (size_t)VP8_FIRST_RECORDS + (size_t)VP8_MB_FIRST_RECORDS * nmb + 8u; }
// impgpu_webp_lossy_encode_bound: the container at its longest (VP8X, ALPH with its pad byte), the frame header, the
// partition table, every partition at its bound, the pad byte
inline size_t vp8_file_bound(int w, int h, int c) {
    if (vp8_check_geometry(w, h, c) != IMP_OK) return 0;
    const int mbw = vp8_mbs(w), mbh = vp8_mbs(h), np = vp8_partitions(mbh);
    size_t n = 12u + 8u + 10u + vp8_first_bound((uint32_t)mbw * (uint32_t)mbh) + 3u * 7u + 1u;
    if (c == 4) n += 18u + 8u + 1u + (size_t)w * (size_t)h + 1u;
    for (int p = 0; p < np; p++) n += vp8_partition_bound(mbw, mbh, np, p);
    return n;
}

// ---------------------------------------------------------------- PLANES
IMP_VP8_HD void vp8_bgr_at(const Vp8Frame& f, int x, int y, int* b, int* g, int* r) {
    x = x < f.w ? x : f.w - 1;
    y = y < f.h ? y : f.h - 1;
    const uint8_t* p = f.src + (size_t)y * (size_t)f.step + (size_t)x * (size_t)f.c;
    if (f.c == 1) { *b = *g = *r = p[0]; }
    else { *b = p[0]; *g = p[1]; *r = p[2]; }
}
IMP_VP8_HD int vp8_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
// macroblock row `row` of the padded planes (wpad = 16 mbw a row of Y, wpad / 2 of U and V) and of the alpha plane (w a
// row, 4 channels alone); -> whether one of this lane's alpha bytes is not 255
IMP_VP8_HD bool vp8_planes_lane(const Vp8Frame& f, int mbw, int row, uint8_t* yp, uint8_t* up, uint8_t* vp, uint8_t* ap, int lane, int nlanes) {
    const int wpad = mbw * 16, cpad = mbw * 8;
    bool seen = false;
    for (int i = lane; i < 16 * wpad; i += nlanes) {
        const int x = i % wpad, y = row * 16 + i / wpad;
        int b, g, r;
        vp8_bgr_at(f, x, y, &b, &g, &r);
        yp[(size_t)y * (size_t)wpad + (size_t)x] = (uint8_t)((16839 * r + 33059 * g + 6420 * b + (16 << 16) + (1 << 15)) >> 16);
        if (ap && x < f.w && y < f.h) {
            const uint8_t a = f.src[(size_t)y * (size_t)f.step + (size_t)x * 4u + 3u];
            ap[(size_t)y * (size_t)f.w + (size_t)x] = a;
            seen |= a != 255;
        }
    }
    const int cw = (f.w + 1) >> 1, ch = (f.h + 1) >> 1;
    for (int i = lane; i < 8 * cpad; i += nlanes) {
        const int x = i % cpad, y = row * 8 + i / cpad;
        const int cx = x < cw ? x : cw - 1, cy = y < ch ? y : ch - 1;
        int bs = 0, gs = 0, rs = 0;
        for (int k = 0; k < 4; k++) {
            int b, g, r;
            vp8_bgr_at(f, 2 * cx + (k & 1), 2 * cy + (k >> 1), &b, &g, &r);
            bs += b; gs += g; rs += r;
        }
        up[(size_t)y * (size_t)cpad + (size_t)x] = (uint8_t)vp8_clip8((-9719 * rs - 19081 * gs + 28800 * bs + (128 << 18) + (1 << 17)) >> 18);
        vp[(size_t)y * (size_t)cpad + (size_t)x] = (uint8_t)vp8_clip8((28800 * rs - 24116 * gs - 4684 * bs + (128 << 18) + (1 << 17)) >> 18);
    }
    return seen;
}

// ---------------------------------------------------------------- transforms
IMP_VP8_HD void vp8_fdct(const int* d, int16_t* out) {                  // d: 16 differences in raster order
    int tmp[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = d[4 * i] + d[4 * i + 3], a1 = d[4 * i + 1] + d[4 * i + 2], a2 = d[4 * i + 1] - d[4 * i + 2], a3 = d[4 * i] - d[4 * i + 3];
        tmp[4 * i] = (a0 + a1) * 8;
        tmp[4 * i + 1] = (a2 * 2217 + a3 * 5352 + 1812) >> 9;
        tmp[4 * i + 2] = (a0 - a1) * 8;
        tmp[4 * i + 3] = (a3 * 2217 - a2 * 5352 + 937) >> 9;
    }
    for (int i = 0; i < 4; i++) {
        const int a0 = tmp[i] + tmp[12 + i], a1 = tmp[4 + i] + tmp[8 + i], a2 = tmp[4 + i] - tmp[8 + i], a3 = tmp[i] - tmp[12 + i];
        out[i] = (int16_t)((a0 + a1 + 7) >> 4);
        out[4 + i] = (int16_t)(((a2 * 2217 + a3 * 5352 + 12000) >> 16) + (a3 != 0));
        out[8 + i] = (int16_t)((a0 - a1 + 7) >> 4);
        out[12 + i] = (int16_t)((a3 * 2217 - a2 * 5352 + 51000) >> 16);
    }
}
IMP_VP8_HD void vp8_fwht(const int* in, int16_t* out) {
    int tmp[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = in[4 * i] + in[4 * i + 2], a1 = in[4 * i + 1] + in[4 * i + 3], a2 = in[4 * i + 1] - in[4 * i + 3], a3 = in[4 * i] - in[4 * i + 2];
        tmp[4 * i] = a0 + a1; tmp[4 * i + 1] = a3 + a2; tmp[4 * i + 2] = a3 - a2; tmp[4 * i + 3] = a0 - a1;
    }
    for (int i = 0; i < 4; i++) {
        const int a0 = tmp[i] + tmp[8 + i], a1 = tmp[4 + i] + tmp[12 + i], a2 = tmp[4 + i] - tmp[12 + i], a3 = tmp[i] - tmp[8 + i];
        out[i] = (int16_t)((a0 + a1) >> 1); out[4 + i] = (int16_t)((a3 + a2) >> 1);
        out[8 + i] = (int16_t)((a3 - a2) >> 1); out[12 + i] = (int16_t)((a0 - a1) >> 1);
    }
}
IMP_VP8_HD int vp8_mul1(int a) { return ((a * 20091) >> 16) + a; }
IMP_VP8_HD int vp8_mul2(int a) { return (a * 35468) >> 16; }
IMP_VP8_HD void vp8_idct(const int* c, int* res) {                      // res: 16 residuals in raster order
    int tmp[16];
    for (int i = 0; i < 4; i++) {
        const int a = c[i] + c[8 + i], b = c[i] - c[8 + i];
        const int cc = vp8_mul2(c[4 + i]) - vp8_mul1(c[12 + i]), d = vp8_mul1(c[4 + i]) + vp8_mul2(c[12 + i]);
        tmp[4 * i] = a + d; tmp[4 * i + 1] = b + cc; tmp[4 * i + 2] = b - cc; tmp[4 * i + 3] = a - d;
    }
    for (int i = 0; i < 4; i++) {
        const int dc = tmp[i] + 4, a = dc + tmp[8 + i], b = dc - tmp[8 + i];
        const int cc = vp8_mul2(tmp[4 + i]) - vp8_mul1(tmp[12 + i]), d = vp8_mul1(tmp[4 + i]) + vp8_mul2(tmp[12 + i]);
        res[4 * i] = (a + d) >> 3; res[4 * i + 1] = (b + cc) >> 3; res[4 * i + 2] = (b - cc) >> 3; res[4 * i + 3] = (a - d) >> 3;
    }
}
IMP_VP8_HD void vp8_iwht(const int* c, int16_t* out) {
    int tmp[16];
    for (int i = 0; i < 4; i++) {
        const int a0 = c[i] + c[12 + i], a1 = c[4 + i] + c[8 + i], a2 = c[4 + i] - c[8 + i], a3 = c[i] - c[12 + i];
        tmp[i] = a0 + a1; tmp[8 + i] = a0 - a1; tmp[4 + i] = a3 + a2; tmp[12 + i] = a3 - a2;
    }
    for (int i = 0; i < 4; i++) {
        const int dc = tmp[4 * i] + 3, a0 = dc + tmp[4 * i + 3], a1 = tmp[4 * i + 1] + tmp[4 * i + 2], a2 = tmp[4 * i + 1] - tmp[4 * i + 2],
                  a3 = dc - tmp[4 * i + 3];
        out[4 * i] = (int16_t)((a0 + a1) >> 3); out[4 * i + 1] = (int16_t)((a3 + a2) >> 3);
        out[4 * i + 2] = (int16_t)((a0 - a1) >> 3); out[4 * i + 3] = (int16_t)((a3 - a2) >> 3);
    }
}
// level = sign(c) * min(2047, (|c| + q/2) / q); r = 0xffffffff / q makes the division a multiplication and one correction
IMP_VP8_HD int vp8_quantise(int c, int q, uint32_t r) {
    const uint32_t a = (uint32_t)(c < 0 ? -c : c) + (uint32_t)q / 2u;
    uint32_t m = (uint32_t)(((uint64_t)a * r) >> 32);
    if ((m + 1u) * (uint32_t)q <= a) m++;
    if (m > 2047u) m = 2047u;
    return c < 0 ? -(int)m : (int)m;
}

// ---------------------------------------------------------------- RECON: a macroblock, 64 lanes, eight phases
struct Vp8Mb {
    uint32_t part[8][64];                                              // the lanes' partial costs: luma DC, V, H, TM, chroma DC, V, H, TM
    uint32_t cost[8];
    int dc[3];                                                         // the DC predictions of Y, U, V
    int16_t coef[25][16];                                              // 16 Y, 4 U, 4 V, Y2, raster order inside a block
    int16_t lev[25][16];
    int16_t ydc[16];                                                   // the Y blocks' DCs back from the Y2 block
    alignas(4) uint8_t src[384];                                       // Y 16x16, U 8x8, V 8x8
    uint8_t rec[384];
    uint8_t top[32], left[32];                                         // Y 16, U 8, V 8
    uint8_t tl[4];
    uint8_t nzf[28];
};
// what a macroblock row works on.  `above` / `border`: the reconstruction's last row of the macroblock row above (null in
// row 0) and of this one, Y (wpad), U, V (wpad / 2 each) in a row.  yrec / urec / vrec: the reconstructed planes, or null.
struct Vp8Row {
    const uint8_t *ysrc, *usrc, *vsrc;
    int mbw, my;
    int q[6];
    uint32_t rq[6];                                                    // 0xffffffff / q[]
    const uint8_t* above;
    uint8_t* border;
    int16_t* levels;                                                   // 400 a macroblock
    uint32_t* info;                                                    // a word a macroblock
    uint8_t *yrec, *urec, *vrec;
};
IMP_VP8_HD int vp8_plane_base(int p) { return p == 0 ? 0 : (p == 1 ? 16 : 24); }
IMP_VP8_HD int vp8_pred(const Vp8Mb& S, int p, int mode, int row, int col) {
    const int b = vp8_plane_base(p);
    if (mode == VP8_DC) return S.dc[p];
    if (mode == VP8_V) return S.top[b + col];
    if (mode == VP8_H) return S.left[b + row];
    return vp8_clip8((int)S.top[b + col] + (int)S.left[b + row] - (int)S.tl[p]);
}
IMP_VP8_HD int vp8_pick(const uint32_t* cost) {
    int m = 0;
    for (int k = 1; k < 4; k++)
        if (cost[k] < cost[m]) m = k;
    return m;
}
// block b of a macroblock: its plane, its side there, its first sample in src / rec
IMP_VP8_HD void vp8_block_at(int b, int* p, int* n, int* at) {
    if (b < 16) { *p = 0; *n = 16; *at = (b >> 2) * 64 + (b & 3) * 4; }
    else { const int k = (b - 16) & 3; *p = b < 20 ? 1 : 2; *n = 8; *at = (b < 20 ? 256 : 320) + (k >> 1) * 32 + (k & 1) * 4; }
}
// a lane's share of a macroblock's source samples, four at a time: Y samples 4 lane .. 4 lane + 3 of the 256, and for the
// lanes below 32 chroma samples 4 lane .. 4 lane + 3 of the 128 (U, then V).  The planes' rows are multiples of 8 bytes.
struct Vp8Fetch { uint32_t y, c; };
IMP_VP8_HD uint32_t vp8_load32(const uint8_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *(const uint32_t*)p;
#else
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
#endif
}
IMP_VP8_HD void vp8_store32(uint8_t* p, uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    *(uint32_t*)p = v;
#else
    memcpy(p, &v, 4);
#endif
}
IMP_VP8_HD Vp8Fetch vp8_mb_fetch(const Vp8Row& R, int mx, int lane) {
    const int wpad = R.mbw * 16, cpad = R.mbw * 8;
    Vp8Fetch f;
    f.y = vp8_load32(R.ysrc + (size_t)(R.my * 16 + (lane >> 2)) * (size_t)wpad + (size_t)(mx * 16 + (lane & 3) * 4));
    f.c = 0u;
    if (lane < 32) {
        const int k = lane & 15;
        f.c = vp8_load32((lane < 16 ? R.usrc : R.vsrc) + (size_t)(R.my * 8 + (k >> 1)) * (size_t)cpad + (size_t)(mx * 8 + (k & 1) * 4));
    }
    return f;
}
IMP_VP8_HD void vp8_mb_phase(int phase, Vp8Mb& S, const Vp8Row& R, int mx, int lane, const Vp8Fetch& in) {
    const int wpad = R.mbw * 16, cpad = R.mbw * 8;
    if (phase == 0) {                                                  // the source samples, the row above, the corner
        vp8_store32(S.src + lane * 4, in.y);
        if (lane < 32) vp8_store32(S.src + 256 + lane * 4, in.c);
        if (lane < 32) {
            const int at = lane < 16 ? mx * 16 + lane : (lane < 24 ? wpad + mx * 8 + lane - 16 : wpad + cpad + mx * 8 + lane - 24);
            S.top[lane] = R.above ? R.above[at] : 127;
            if (mx == 0) S.left[lane] = 129;
        } else if (lane < 35) {
            const int p = lane - 32;
            const int at = p == 0 ? mx * 16 - 1 : (p == 1 ? wpad + mx * 8 - 1 : wpad + cpad + mx * 8 - 1);
            S.tl[p] = !R.above ? 127 : (mx == 0 ? 129 : R.above[at]);
        }
    } else if (phase == 1) {                                           // the DC predictions
        if (lane < 3) {
            const int n = lane == 0 ? 16 : 8, b = vp8_plane_base(lane), sh = lane == 0 ? 4 : 3;
            int st = 0, sl = 0;
            for (int k = 0; k < n; k++) { st += S.top[b + k]; sl += S.left[b + k]; }
            const bool ht = R.above != nullptr, hl = mx > 0;
            S.dc[lane] = ht && hl ? (st + sl + n) >> (sh + 1) : (ht ? (st + n / 2) >> sh : (hl ? (sl + n / 2) >> sh : 128));
        }
    } else if (phase == 2) {                                           // every lane's share of the eight costs
        uint32_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < 4; j++) {
            const int i = lane * 4 + j;
            for (int m = 0; m < 4; m++) { const int d = vp8_pred(S, 0, m, i >> 4, i & 15) - (int)S.src[i]; c[m] += (uint32_t)(d * d); }
        }
        for (int p = 1; p < 3; p++)
            for (int m = 0; m < 4; m++) { const int d = vp8_pred(S, p, m, lane >> 3, lane & 7) - (int)S.src[192 + 64 * p + lane]; c[4 + m] += (uint32_t)(d * d); }
        for (int m = 0; m < 8; m++) S.part[m][lane] = c[m];
    } else if (phase == 3) {
        if (lane < 8) {
            uint32_t s = 0;
            for (int k = 0; k < 64; k++) s += S.part[lane][k];
            S.cost[lane] = s;
        }
    } else if (phase == 4) {                                           // the forward transform of block `lane`
        if (lane < 24) {
            int p, n, at;
            vp8_block_at(lane, &p, &n, &at);
            const int mode = vp8_pick(S.cost + (p ? 4 : 0)), r0 = (at - (p == 0 ? 0 : (p == 1 ? 256 : 320))) / n, c0 = at % n;
            int d[16];
            for (int k = 0; k < 16; k++) d[k] = (int)S.src[at + (k >> 2) * n + (k & 3)] - vp8_pred(S, p, mode, r0 + (k >> 2), c0 + (k & 3));
            vp8_fdct(d, S.coef[lane]);
        }
    } else if (phase == 5) {                                           // the Y2 block
        if (lane == 0) {
            int in[16], dq[16];
            for (int k = 0; k < 16; k++) in[k] = S.coef[k][0];
            vp8_fwht(in, S.coef[24]);
            bool nz = false;
            for (int k = 0; k < 16; k++) {
                const int q = k ? R.q[3] : R.q[2], l = vp8_quantise(S.coef[24][k], q, k ? R.rq[3] : R.rq[2]);
                S.lev[24][k] = (int16_t)l;
                dq[k] = l * q;
                nz |= l != 0;
            }
            vp8_iwht(dq, S.ydc);
            S.nzf[24] = nz;
        }
    } else if (phase == 6) {                                           // quantise, de-quantise, inverse transform, reconstruct
        if (lane < 24) {
            int p, n, at;
            vp8_block_at(lane, &p, &n, &at);
            const int mode = vp8_pick(S.cost + (p ? 4 : 0)), r0 = (at - (p == 0 ? 0 : (p == 1 ? 256 : 320))) / n, c0 = at % n;
            int dq[16], res[16];
            bool nz = false;
            for (int k = 0; k < 16; k++) {
                int l, v;
                if (p == 0 && k == 0) { l = 0; v = S.ydc[lane]; }
                else {
                    const int qk = p == 0 ? 1 : (k ? 5 : 4), q = R.q[qk];
                    l = vp8_quantise(S.coef[lane][k], q, R.rq[qk]);
                    v = l * q;
                }
                S.lev[lane][k] = (int16_t)l;
                dq[k] = v;
                nz |= l != 0;
            }
            vp8_idct(dq, res);
            for (int k = 0; k < 16; k++)
                S.rec[at + (k >> 2) * n + (k & 3)] = (uint8_t)vp8_clip8(vp8_pred(S, p, mode, r0 + (k >> 2), c0 + (k & 3)) + res[k]);
            S.nzf[lane] = nz;
        }
    } else {                                                           // what the macroblock leaves
        const size_t mb = (size_t)R.my * (size_t)R.mbw + (size_t)mx;
        for (int i = lane; i < 400; i += 64) R.levels[mb * 400u + (size_t)i] = S.lev[i >> 4][i & 15];
        if (lane < 32) {
            const int at = lane < 16 ? mx * 16 + lane : (lane < 24 ? wpad + mx * 8 + lane - 16 : wpad + cpad + mx * 8 + lane - 24);
            R.border[at] = lane < 16 ? S.rec[240 + lane] : (lane < 24 ? S.rec[256 + 56 + lane - 16] : S.rec[320 + 56 + lane - 24]);
        } else {
            const int k = lane - 32;
            S.left[k] = k < 16 ? S.rec[k * 16 + 15] : (k < 24 ? S.rec[256 + (k - 16) * 8 + 7] : S.rec[320 + (k - 24) * 8 + 7]);
        }
        if (lane == 0) {
            uint32_t w = 0;
            for (int b = 0; b < 25; b++) w |= (uint32_t)(S.nzf[b] != 0) << b;
            R.info[mb] = w | (uint32_t)vp8_pick(S.cost) << 25 | (uint32_t)vp8_pick(S.cost + 4) << 27;
        }
        if (R.yrec)
            for (int i = lane; i < 384; i += 64) {
                if (i < 256) R.yrec[(size_t)(R.my * 16 + (i >> 4)) * (size_t)wpad + (size_t)(mx * 16 + (i & 15))] = S.rec[i];
                else {
                    const int k = (i - 256) & 63;
                    (i < 320 ? R.urec : R.vrec)[(size_t)(R.my * 8 + (k >> 3)) * (size_t)cpad + (size_t)(mx * 8 + (k & 7))] = S.rec[i];
                }
            }
    }
}

// ---------------------------------------------------------------- TOKENS
struct Vp8Records { uint16_t* rec; uint32_t n; };
IMP_VP8_HD void vp8_rec(Vp8Records& r, int prob, int bit) {
    if (r.n < VP8_MB_RECORDS) r.rec[r.n] = (uint16_t)(prob | (bit ? 256 : 0));
    r.n++;
}
// one block: lev in raster order, coded in zigzag order from position `first`
IMP_VP8_HD void vp8_block_tokens(Vp8Records& r, const int16_t* lev, int type, int ctx, int first) {
    int last = -1;
    for (int i = 15; i >= first; i--)
        if (lev[vp8_zigzag(i)]) { last = i; break; }
    int n = first;
    vp8_rec(r, vp8_coef_prob(type, vp8_band(n), ctx, 0), last >= n);
    if (last < n) return;
    while (n < 16) {
        const int c = lev[vp8_zigzag(n)], b = vp8_band(n);
        n++;
        const int v = c < 0 ? -c : c;
        if (!v) {
            vp8_rec(r, vp8_coef_prob(type, b, ctx, 1), 0);
            ctx = 0;
            continue;
        }
        vp8_rec(r, vp8_coef_prob(type, b, ctx, 1), 1);
        if (v == 1) {
            vp8_rec(r, vp8_coef_prob(type, b, ctx, 2), 0);
            vp8_rec(r, 128, c < 0);
            ctx = 1;
        } else {
            vp8_rec(r, vp8_coef_prob(type, b, ctx, 2), 1);
            if (v <= 4) {
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 3), 0);
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 4), v != 2);
                if (v != 2) vp8_rec(r, vp8_coef_prob(type, b, ctx, 5), v == 4);
            } else if (v <= 10) {
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 3), 1);
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 6), 0);
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 7), v > 6);
                if (v <= 6) vp8_rec(r, 159, v == 6);
                else { vp8_rec(r, 165, v >= 9); vp8_rec(r, 145, !(v & 1)); }
            } else {
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 3), 1);
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 6), 1);
                const int cat = v < 19 ? 3 : (v < 35 ? 4 : (v < 67 ? 5 : 6));
                vp8_rec(r, vp8_coef_prob(type, b, ctx, 8), cat >= 5);
                vp8_rec(r, vp8_coef_prob(type, b, ctx, cat >= 5 ? 10 : 9), cat == 4 || cat == 6);
                const int bits = cat == 6 ? 11 : cat, extra = v - (3 + (8 << (cat - 3)));
                for (int k = 0; k < bits; k++) vp8_rec(r, vp8_cat_prob(cat, k), (extra >> (bits - 1 - k)) & 1);
            }
            vp8_rec(r, 128, c < 0);
            ctx = 2;
        }
        if (n == 16) return;
        vp8_rec(r, vp8_coef_prob(type, vp8_band(n), ctx, 0), n <= last);
        if (n > last) return;
    }
}
// a macroblock's records (none when it is skipped); left / up: the neighbours' info words, 0 outside the frame -> the count
IMP_VP8_HD uint32_t vp8_mb_tokens(const int16_t* lev, uint32_t info, uint32_t left, uint32_t up, uint16_t* rec) {
    Vp8Records r{rec, 0u};
    if (!(info & VP8_NZ_MASK)) return 0u;
    vp8_block_tokens(r, lev + 24 * 16, 1, (int)((left >> 24) & 1u) + (int)((up >> 24) & 1u), 0);
    for (int b = 0; b < 16; b++) {
        const uint32_t l = (b & 3) ? info >> (b - 1) : left >> (b + 3), t = (b >> 2) ? info >> (b - 4) : up >> (b + 12);
        vp8_block_tokens(r, lev + b * 16, 0, (int)(l & 1u) + (int)(t & 1u), 1);
    }
    for (int base = 16; base < 24; base += 4)
        for (int k = 0; k < 4; k++) {
            const int b = base + k;
            const uint32_t l = (k & 1) ? info >> (b - 1) : left >> (b + 1), t = (k >> 1) ? info >> (b - 2) : up >> (b + 2);
            vp8_block_tokens(r, lev + b * 16, 2, (int)(l & 1u) + (int)(t & 1u), 0);
        }
    return r.n < VP8_MB_RECORDS ? r.n : VP8_MB_RECORDS;
}

// ---------------------------------------------------------------- BOOL: RFC 6386 section 7.3, carries resolved in the lane's own output
struct Vp8Bool { uint8_t* out; size_t cap, n; uint32_t range, bottom; int count; };
IMP_VP8_HD Vp8Bool vp8_bool_begin(uint8_t* out, size_t cap) { return Vp8Bool{out, cap, 0u, 255u, 0u, 24}; }
IMP_VP8_HD void vp8_bool_carry(Vp8Bool& e) {
    size_t i = e.n < e.cap ? e.n : e.cap;
    while (i > 0) {
        i--;
        if (e.out[i] == 255) e.out[i] = 0;
        else { e.out[i]++; return; }
    }
}
IMP_VP8_HD void vp8_bool_byte(Vp8Bool& e, uint32_t v) {
    if (e.n < e.cap) e.out[e.n] = (uint8_t)v;
    e.n++;
}
IMP_VP8_HD void vp8_bool_put(Vp8Bool& e, int prob, int bit) {
    const uint32_t split = 1u + (((e.range - 1u) * (uint32_t)prob) >> 8);
    if (bit) { e.bottom += split; e.range -= split; }
    else e.range = split;
    while (e.range < 128u) {
        e.range <<= 1;
        if (e.bottom & 0x80000000u) vp8_bool_carry(e);
        e.bottom <<= 1;
        if (!--e.count) {
            vp8_bool_byte(e, e.bottom >> 24);
            e.bottom &= 0xffffffu;
            e.count = 8;
        }
    }
}
IMP_VP8_HD void vp8_bool_literal(Vp8Bool& e, int value, int bits) {
    for (int i = bits - 1; i >= 0; i--) vp8_bool_put(e, 128, (value >> i) & 1);
}
IMP_VP8_HD size_t vp8_bool_finish(Vp8Bool& e) {
    int c = e.count;
    uint32_t v = e.bottom;
    if (v & (1u << (32 - c))) vp8_bool_carry(e);
    v <<= c & 7;
    c >>= 3;
    while (--c >= 0) v <<= 8;
    for (c = 0; c < 4; c++) { vp8_bool_byte(e, v >> 24); v <<= 8; }
    return e.n;
}
// the first partition: the frame header, then every macroblock's skip flag and modes -> its bytes
IMP_VP8_HD size_t vp8_code_first(const uint32_t* info, uint32_t nmb, int qi, int nparts, uint8_t* out, size_t cap) {
    Vp8Bool e = vp8_bool_begin(out, cap);
    vp8_bool_literal(e, 0, 2);                                         // colour space, clamping type
    vp8_bool_literal(e, 0, 1);                                         // no segmentation
    vp8_bool_literal(e, 0, 10);                                        // filter type, level, sharpness
    vp8_bool_literal(e, 0, 1);                                         // no filter deltas
    vp8_bool_literal(e, nparts == 8 ? 3 : (nparts == 4 ? 2 : (nparts == 2 ? 1 : 0)), 2);
    vp8_bool_literal(e, qi, 7);
    vp8_bool_literal(e, 0, 5);                                         // no quantiser deltas
    vp8_bool_literal(e, 0, 1);                                         // refresh_entropy_probs
    for (int i = 0; i < 1056; i++) vp8_bool_put(e, vp8_update_prob(i), 0);
    vp8_bool_literal(e, 1, 1);                                         // mb_no_coeff_skip
    uint32_t coded = 0;
    for (uint32_t mb = 0; mb < nmb; mb++) coded += (info[mb] & VP8_NZ_MASK) != 0u;
    uint64_t ps = (256ull * coded + nmb / 2u) / nmb;
    const int pskip = ps < 1u ? 1 : (ps > 255u ? 255 : (int)ps);
    vp8_bool_literal(e, pskip, 8);
    for (uint32_t mb = 0; mb < nmb; mb++) {
        const uint32_t w = info[mb];
        const int ym = (int)((w >> 25) & 3u), um = (int)((w >> 27) & 3u);
        vp8_bool_put(e, pskip, !(w & VP8_NZ_MASK));
        vp8_bool_put(e, 145, 1);                                       // not B_PRED
        vp8_bool_put(e, 156, ym == VP8_H || ym == VP8_TM);
        if (ym == VP8_H || ym == VP8_TM) vp8_bool_put(e, 128, ym == VP8_TM);
        else vp8_bool_put(e, 163, ym == VP8_V);
        vp8_bool_put(e, 142, um != VP8_DC);
        if (um != VP8_DC) {
            vp8_bool_put(e, 114, um != VP8_V);
            if (um != VP8_V) vp8_bool_put(e, 183, um == VP8_TM);
        }
    }
    return vp8_bool_finish(e);
}
// ---------------------------------------------------------------- PACK
IMP_VP8_HD uint32_t vp8_len32(size_t n) { return n > 0xffffffffu ? 0xffffffffu : (uint32_t)n; }
struct Vp8Layout {
    uint32_t has_alpha, alph_at, vp8_at, first_at, table_at, part_at[8], vp8_len, file_len;
};
// file_len 0: the format cannot say the sizes (19 bits for the first partition, 24 for a token partition but the last, 32
// for the file)
IMP_VP8_HD Vp8Layout vp8_layout(int w, int h, bool alpha, uint32_t first_len, const uint32_t* part_len, int nparts) {
    Vp8Layout L;
    uint64_t at = 12u;
    L.has_alpha = alpha;
    L.alph_at = 0u;
    if (alpha) {
        at += 18u;                                                     // VP8X
        L.alph_at = (uint32_t)at;
        const uint32_t n = 1u + (uint32_t)w * (uint32_t)h;
        at += 8u + (uint64_t)n + (n & 1u);
    }
    L.vp8_at = (uint32_t)at;
    L.first_at = (uint32_t)at + 8u + 10u;
    L.table_at = L.first_at + first_len;
    uint64_t p_at = at + 18u + (uint64_t)first_len + 3u * (uint64_t)(nparts - 1);
    bool ok = first_len <= 0x7ffffu;
    for (int p = 0; p < 8; p++) {
        L.part_at[p] = (uint32_t)p_at;
        if (p < nparts) p_at += part_len[p];
        if (p + 1 < nparts && part_len[p] > 0xffffffu) ok = false;
    }
    L.vp8_len = (uint32_t)(p_at - (at + 8u));
    L.file_len = ok && p_at < 0xfffffff0ull ? (uint32_t)p_at + (L.vp8_len & 1u) : 0u;
    return L;
}
IMP_VP8_HD void vp8_put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24); }
IMP_VP8_HD void vp8_put24(uint8_t* p, uint32_t v) { p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); }
IMP_VP8_HD void vp8_tag(uint8_t* p, const char* t) { for (int i = 0; i < 4; i++) p[i] = (uint8_t)t[i]; }
// everything of the file but the alpha bytes, the first partition and the token partitions
IMP_VP8_HD void vp8_write_headers(uint8_t* out, const Vp8Layout& L, int w, int h, uint32_t first_len, const uint32_t* part_len, int nparts) {
    vp8_tag(out, "RIFF"); vp8_put32(out + 4, L.file_len - 8u); vp8_tag(out + 8, "WEBP");
    if (L.has_alpha) {
        uint8_t* x = out + 12;
        vp8_tag(x, "VP8X"); vp8_put32(x + 4, 10u);
        vp8_put32(x + 8, 0x10u);
        vp8_put24(x + 12, (uint32_t)w - 1u); vp8_put24(x + 15, (uint32_t)h - 1u);
        uint8_t* a = out + L.alph_at;
        const uint32_t n = 1u + (uint32_t)w * (uint32_t)h;
        vp8_tag(a, "ALPH"); vp8_put32(a + 4, n);
        a[8] = 0;
        if (n & 1u) a[8u + n] = 0;
    }
    uint8_t* v = out + L.vp8_at;
    vp8_tag(v, "VP8 "); vp8_put32(v + 4, L.vp8_len);
    vp8_put24(v + 8, (1u << 4) | (first_len << 5));                     // key frame, version 0, shown
    v[11] = 0x9d; v[12] = 0x01; v[13] = 0x2a;
    v[14] = (uint8_t)w; v[15] = (uint8_t)(w >> 8); v[16] = (uint8_t)h; v[17] = (uint8_t)(h >> 8);
    for (int p = 0; p + 1 < nparts; p++) vp8_put24(out + L.table_at + 3u * (uint32_t)p, part_len[p]);
    if (L.vp8_len & 1u) out[L.file_len - 1u] = 0;
}

// ---------------------------------------------------------------- impgpu_webp_lossy_encode_host: the lanes one after the other
// modes (2 bytes a macroblock: luma, chroma), levels (400 a macroblock) and the padded reconstructed planes may be null
inline int vp8_encode_host(const unsigned char* frame, int width, int height, int channels, int step, int quality, unsigned char* out, size_t capacity,
                           size_t* length, unsigned char* modes, short* levels_out, unsigned char* yrec, unsigned char* urec, unsigned char* vrec) {
    if (length) *length = 0;
    if (!frame || !length || quality < 0 || quality > 100) return IMP_ERROR_INVALID_ARGS;
    if (int rc = vp8_check_geometry(width, height, channels)) return rc;
    if ((long long)step < (long long)width * channels) return IMP_ERROR_INVALID_ARGS;
    const Vp8Frame f{frame, width, height, channels, step};
    const int mbw = vp8_mbs(width), mbh = vp8_mbs(height), nparts = vp8_partitions(mbh), wpad = mbw * 16, cpad = mbw * 8;
    const uint32_t nmb = (uint32_t)mbw * (uint32_t)mbh;
    std::vector<uint8_t> yp((size_t)wpad * mbh * 16), up((size_t)cpad * mbh * 8), vp((size_t)cpad * mbh * 8);
    std::vector<uint8_t> ap(channels == 4 ? (size_t)width * height : 0u);
    bool alpha = false;
    for (int r = 0; r < mbh; r++) alpha |= vp8_planes_lane(f, mbw, r, yp.data(), up.data(), vp.data(), ap.empty() ? nullptr : ap.data(), 0, 1);   // PLANES
    std::vector<int16_t> levels((size_t)nmb * 400u);
    std::vector<uint32_t> info(nmb);
    std::vector<uint8_t> borders((size_t)2 * wpad * 2);
    std::vector<Vp8Mb> mb(1);
    Vp8Row R;
    R.ysrc = yp.data(); R.usrc = up.data(); R.vsrc = vp.data();
    R.mbw = mbw;
    vp8_steps(vp8_quant_index(quality), R.q);
    vp8_recips(R.q, R.rq);
    R.levels = levels.data(); R.info = info.data();
    R.yrec = yrec; R.urec = urec; R.vrec = vrec;
    for (int my = 0; my < mbh; my++) {                                 // RECON
        R.my = my;
        R.above = my ? borders.data() + (size_t)((my - 1) & 1) * 2 * wpad : nullptr;
        R.border = borders.data() + (size_t)(my & 1) * 2 * wpad;
        for (int mx = 0; mx < mbw; mx++)
            for (int ph = 0; ph < VP8_PHASES; ph++)
                for (int lane = 0; lane < 64; lane++) vp8_mb_phase(ph, mb[0], R, mx, lane, vp8_mb_fetch(R, mx, lane));
    }
    if (modes)
        for (uint32_t i = 0; i < nmb; i++) { modes[2 * i] = (uint8_t)((info[i] >> 25) & 3u); modes[2 * i + 1] = (uint8_t)((info[i] >> 27) & 3u); }
    if (levels_out) memcpy(levels_out, levels.data(), levels.size() * sizeof(int16_t));
    std::vector<uint16_t> rec((size_t)mbw * VP8_MB_RECORDS);            // TOKENS and BOOL, a macroblock row at a time
    std::vector<uint32_t> nrec((size_t)mbw);
    std::vector<std::vector<uint8_t>> parts((size_t)nparts);
    std::vector<Vp8Bool> coders((size_t)nparts);
    uint32_t part_len[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int p = 0; p < nparts; p++) {
        parts[(size_t)p].resize(vp8_partition_bound(mbw, mbh, nparts, p));
        coders[(size_t)p] = vp8_bool_begin(parts[(size_t)p].data(), parts[(size_t)p].size());
    }
    for (int my = 0; my < mbh; my++) {
        Vp8Bool& e = coders[(size_t)(my % nparts)];
        for (int mx = 0; mx < mbw; mx++) {
            const size_t i = (size_t)my * mbw + mx;
            nrec[(size_t)mx] = vp8_mb_tokens(levels.data() + i * 400u, info[i], mx ? info[i - 1] : 0u, my ? info[i - (size_t)mbw] : 0u,
                                             rec.data() + (size_t)mx * VP8_MB_RECORDS);
        }
        for (int mx = 0; mx < mbw; mx++) {
            const uint16_t* r = rec.data() + (size_t)mx * VP8_MB_RECORDS;
            for (uint32_t k = 0; k < nrec[(size_t)mx]; k++) vp8_bool_put(e, r[k] & 255, r[k] >> 8);
        }
    }
    for (int p = 0; p < nparts; p++) part_len[p] = vp8_len32(vp8_bool_finish(coders[(size_t)p]));
    std::vector<uint8_t> first(vp8_first_bound(nmb));
    const uint32_t first_len = vp8_len32(vp8_code_first(info.data(), nmb, vp8_quant_index(quality), nparts, first.data(), first.size()));
    const Vp8Layout L = vp8_layout(width, height, alpha, first_len, part_len, nparts);   // PACK
    if (!L.file_len) return IMP_ERROR_UNSUPPORTED;
    *length = L.file_len;
    if (L.file_len > capacity || !out) return IMP_ERROR_MALLOC_FAILED;
    vp8_write_headers(out, L, width, height, first_len, part_len, nparts);
    if (alpha) memcpy(out + L.alph_at + 9u, ap.data(), ap.size());
    memcpy(out + L.first_at, first.data(), first_len);
    for (int p = 0; p < nparts; p++) memcpy(out + L.part_at[p], parts[(size_t)p].data(), part_len[p]);
    return IMP_OK;
}

// ---------------------------------------------------------------- the device block (imp_webp_lossy.cpp lays it out)
struct Vp8FrameDesc {
    const uint8_t* src;
    int w, h, c, step, mbw, mbh, nparts, qi;
    uint32_t nmb;
    unsigned long long out_bytes;
    long long y_off, u_off, v_off, alpha_off, lev_off, info_off, rec_off, nrec_off, first_off, part_off[8], out_off;
};
struct Vp8Work { uint32_t alpha_seen, first_len, part_len[8]; };       // zeroed before the launches
struct Vp8Rec { uint64_t file_len; };
struct Vp8RowItem { int frame, row; };
struct Vp8Dev {
    uint8_t* mem;
    const Vp8FrameDesc* frames;
    const Vp8RowItem* rows;                                            // every macroblock row of the call
    Vp8Work* works;
    Vp8Rec* recs;
    int nframes;
    int border_lds;                                                    // k_vp8_recon's dynamic LDS, set by the launcher
};
#if defined(__HIPCC__)
int launch_vp8_encode(Vp8Dev D, long long nrows, int max_wpad, uint32_t max_nmb, hipStream_t s);
#endif

}  // namespace imp
