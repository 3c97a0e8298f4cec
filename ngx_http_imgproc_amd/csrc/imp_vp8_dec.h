// imp_vp8_dec.h -- the lane code of the lossy WebP (VP8 key frame) decoder: what the launches of imp_vp8_dec.hip run per
// lane, and what impgpu_webp_decode_host_ex (imp_vp8_dec_host.h) runs one lane after the other (and under the sanitizers,
// tests/c/vp8_dec_test.cpp).  The frame is defined in include/impgpu.h ("WEBP UPLOADS in, LOSSY"); where libwebp and RFC 6386
// differ, libwebp is followed.
//
//   BOOL     VdBool: the boolean decoder, a byte at a time, with libwebp's end rule (eof once a byte past the end HAD to be
//            loaded; the first such load shifts a zero byte in, later ones only keep the window legal).
//   MODES    vd_mb_modes: a macroblock's segment, skip flag and intra modes out of the first partition.
//   TOKENS   vd_mb_residuals: the token tree with its contexts, de-quantised into 16-bit storage as libwebp does.
//   RECON    vd_mb_recon: prediction (16x16, chroma, the ten sub-block modes) plus inverse transforms, into the padded planes.
//   FILTER   vd_filter_step: both loop filters, a macroblock in eight steps shared by 32 lanes (16 luma lines, 8 + 8 chroma).
//   FRAME    vd_frame_pixel: fancy chroma upsampling and libwebp's YUV -> B,G,R,A, cropped to the frame.
//
// Safe by construction: every read of stream bytes is bounded by its partition's size; every loop over stream data is
// bounded by the macroblock count and by 16 coefficients a block; every plane index lies inside the padded planes.
#pragma once
#include "imp_webp_lossy.h"

namespace imp {

enum { VD_DC = 0, VD_TM = 1, VD_VE = 2, VD_HE = 3, VD_RD = 4, VD_VR = 5, VD_LD = 6, VD_VL = 7, VD_HD = 8, VD_HU = 9 };   // libwebp's order
enum { VD_OK = 0, VD_DAMAGED = 1 };

IMP_VP8_HD uint8_t vd_bmode_prob(int top, int left, int node) {         // RFC 6386 section 11.5, kf_bmode_probs
    static constexpr uint8_t T[900] = {
        231,120,48,89,115,113,120,152,112,152,179,64,126,170,118,46,70,95,175,69,143,80,85,82,72,155,103,56,58,10,
        171,218,189,17,13,152,114,26,17,163,44,195,21,10,173,121,24,80,195,26,62,44,64,85,144,71,10,38,171,213,
        144,34,26,170,46,55,19,136,160,33,206,71,63,20,8,114,114,208,12,9,226,81,40,11,96,182,84,29,16,36,
        134,183,89,137,98,101,106,165,148,72,187,100,130,157,111,32,75,80,66,102,167,99,74,62,40,234,128,41,53,9,
        178,241,141,26,8,107,74,43,26,146,73,166,49,23,157,65,38,105,160,51,52,31,115,128,104,79,12,27,217,255,
        87,17,7,87,68,71,44,114,51,15,186,23,47,41,14,110,182,183,21,17,194,66,45,25,102,197,189,23,18,22,
        88,88,147,150,42,46,45,196,205,43,97,183,117,85,38,35,179,61,39,53,200,87,26,21,43,232,171,56,34,51,
        104,114,102,29,93,77,39,28,85,171,58,165,90,98,64,34,22,116,206,23,34,43,166,73,107,54,32,26,51,1,
        81,43,31,68,25,106,22,64,171,36,225,114,34,19,21,102,132,188,16,76,124,62,18,78,95,85,57,50,48,51,
        193,101,35,159,215,111,89,46,111,60,148,31,172,219,228,21,18,111,112,113,77,85,179,255,38,120,114,40,42,1,
        196,245,209,10,25,109,88,43,29,140,166,213,37,43,154,61,63,30,155,67,45,68,1,209,100,80,8,43,154,1,
        51,26,71,142,78,78,16,255,128,34,197,171,41,40,5,102,211,183,4,1,221,51,50,17,168,209,192,23,25,82,
        138,31,36,171,27,166,38,44,229,67,87,58,169,82,115,26,59,179,63,59,90,180,59,166,93,73,154,40,40,21,
        116,143,209,34,39,175,47,15,16,183,34,223,49,45,183,46,17,33,183,6,98,15,32,183,57,46,22,24,128,1,
        54,17,37,65,32,73,115,28,128,23,128,205,40,3,9,115,51,192,18,6,223,87,37,9,115,59,77,64,21,47,
        104,55,44,218,9,54,53,130,226,64,90,70,205,40,41,23,26,57,54,57,112,184,5,41,38,166,213,30,34,26,
        133,152,116,10,32,134,39,19,53,221,26,114,32,73,255,31,9,65,234,2,15,1,118,73,75,32,12,51,192,255,
        160,43,51,88,31,35,67,102,85,55,186,85,56,21,23,111,59,205,45,37,192,55,38,70,124,73,102,1,34,98,
        125,98,42,88,104,85,117,175,82,95,84,53,89,128,100,113,101,45,75,79,123,47,51,128,81,171,1,57,17,5,
        71,102,57,53,41,49,38,33,13,121,57,73,26,1,85,41,10,67,138,77,110,90,47,114,115,21,2,10,102,255,
        166,23,6,101,29,16,10,85,128,101,196,26,57,18,10,102,102,213,34,20,43,117,20,15,36,163,128,68,1,26,
        102,61,71,37,34,53,31,243,192,69,60,71,38,73,119,28,222,37,68,45,128,34,1,47,11,245,171,62,17,19,
        70,146,85,55,62,70,37,43,37,154,100,163,85,160,1,63,9,92,136,28,64,32,201,85,75,15,9,9,64,255,
        184,119,16,86,6,28,5,64,255,25,248,1,56,8,17,132,137,255,55,116,128,58,15,20,82,135,57,26,121,40,
        164,50,31,137,154,133,25,35,218,51,103,44,131,131,123,31,6,158,86,40,64,135,148,224,45,183,128,22,26,17,
        131,240,154,14,1,209,45,16,21,91,64,222,7,1,197,56,21,39,155,60,138,23,102,213,83,12,13,54,192,255,
        68,47,28,85,26,85,85,128,128,32,146,171,18,11,7,63,144,171,4,4,246,35,27,10,146,174,171,12,26,128,
        190,80,35,99,180,80,126,54,45,85,126,47,87,176,51,41,20,32,101,75,128,139,118,146,116,128,85,56,41,15,
        176,236,85,37,9,62,71,30,17,119,118,255,17,18,138,101,38,60,138,55,70,43,26,142,146,36,19,30,171,255,
        97,27,20,138,45,61,62,219,1,81,188,64,32,41,20,117,151,142,20,21,163,112,19,12,61,195,128,48,4,24
    };
    return T[(top * 10 + left) * 9 + node];
}

// ---------------------------------------------------------------- BOOL
struct VdBool { const uint8_t* buf; uint32_t size, pos, value, range; int bits, eof; };
IMP_VP8_HD void vd_bool_load(VdBool& b) {
    if (b.pos < b.size) { b.value = (b.value << 8) | b.buf[b.pos++]; b.bits += 8; }
    else if (!b.eof) { b.value <<= 8; b.bits += 8; b.eof = 1; }
    else b.bits = 0;
}
IMP_VP8_HD void vd_bool_begin(VdBool& b, const uint8_t* buf, uint32_t size) {
    b.buf = buf; b.size = size; b.pos = 0; b.value = 0; b.range = 254; b.bits = -8; b.eof = 0;
    vd_bool_load(b);
}
IMP_VP8_HD int vd_bit(VdBool& b, int prob) {
    if (b.bits < 0) vd_bool_load(b);
    const int pos = b.bits;
    const uint32_t split = (b.range * (uint32_t)prob) >> 8;
    uint32_t r;
    int bit;
    if ((b.value >> pos) > split) { r = b.range - split; b.value -= (split + 1u) << pos; bit = 1; }
    else { r = split + 1u; bit = 0; }
    if (r > 255u || r == 0u) r = 1u;                                   // (only behind the end, where the window is no longer a stream)
    int shift = 0;
    while ((r << shift) < 128u) shift++;
    b.range = (r << shift) - 1u;
    b.bits -= shift;
    return bit;
}
IMP_VP8_HD int vd_value(VdBool& b, int bits) {
    int v = 0;
    while (bits-- > 0) v |= vd_bit(b, 128) << bits;
    return v;
}
IMP_VP8_HD int vd_signed_value(VdBool& b, int bits) {
    const int v = vd_value(b, bits);
    return vd_bit(b, 128) ? -v : v;
}

// ---------------------------------------------------------------- what the host front reads (imp_vp8_dec_host.h)
struct VdHdr {
    int w, h, mbw, mbh, nparts;
    int filter_type;                                                   // 0 off, 1 simple, 2 normal
    uint32_t feat;
    uint8_t update_map, use_skip, skip_p, pad0;
    uint8_t seg_prob[4];
    uint16_t dq[4][6];                                                 // per segment: y dc, y ac, y2 dc, y2 ac, uv dc, uv ac
    uint8_t fstr[4][2][4];                                             // per segment, per is-B_PRED: limit, inner level, hev threshold, inner
    uint8_t prob[4][8][3][11];
    uint32_t first_off, first_size;                                    // the first partition inside the chunk
    uint32_t br_pos, br_value, br_range;                               // its decoder behind the frame header
    int br_bits, br_eof;
    uint32_t part_off[8], part_size[8];
};

// what one file's macroblock walk keeps: the row above's contexts are arrays of mbw entries
struct VdWalk {
    VdBool br, parts[8];
    uint8_t *top_nz, *top_dc, *top_modes;                              // mbw, mbw, 4 mbw
    uint8_t left_nz, left_dc, left_modes[4];
    uint32_t feat, mode_mask;                                          // 16x16 modes 0..3, chroma 4..7, sub-block 8..17
};
struct VdPlanes { uint8_t *y, *u, *v; int ys, cs; };                   // padded: 16 mbw x 16 mbh, 8 mbw x 8 mbh
struct VdMb {
    int16_t coef[400];
    uint32_t nz_y, nz_uv;                                              // two bits a block, libwebp's codes: 3 full, 2 three coefficients, 1 DC
    uint8_t imodes[16];
    uint8_t is_i4, uvmode, segment, skip;
};

IMP_VP8_HD void vd_row_begin(VdWalk& W) {
    W.left_nz = 0; W.left_dc = 0;
    for (int i = 0; i < 4; i++) W.left_modes[i] = VD_DC;
}

// ---------------------------------------------------------------- MODES
IMP_VP8_HD void vd_mb_modes(const VdHdr& H, VdWalk& W, VdMb& M, int mx) {
    VdBool& br = W.br;
    uint8_t* top = W.top_modes + 4 * mx;
    M.segment = 0;
    if (H.update_map) M.segment = (uint8_t)(!vd_bit(br, H.seg_prob[0]) ? vd_bit(br, H.seg_prob[1]) : vd_bit(br, H.seg_prob[2]) + 2);
    M.skip = H.use_skip ? (uint8_t)vd_bit(br, H.skip_p) : 0;
    M.is_i4 = (uint8_t)!vd_bit(br, 145);
    if (!M.is_i4) {
        const int ym = vd_bit(br, 156) ? (vd_bit(br, 128) ? VD_TM : VD_HE) : (vd_bit(br, 163) ? VD_VE : VD_DC);
        M.imodes[0] = (uint8_t)ym;
        for (int i = 0; i < 4; i++) { top[i] = (uint8_t)ym; W.left_modes[i] = (uint8_t)ym; }
        W.mode_mask |= 1u << ym;
    } else {
        W.feat |= IMPGPU_VP8_DEC_F_BPRED;
        for (int y = 0; y < 4; y++) {
            int ym = W.left_modes[y];
            for (int x = 0; x < 4; x++) {
                const int t = top[x], l = ym;
                ym = !vd_bit(br, vd_bmode_prob(t, l, 0)) ? VD_DC
                   : !vd_bit(br, vd_bmode_prob(t, l, 1)) ? VD_TM
                   : !vd_bit(br, vd_bmode_prob(t, l, 2)) ? VD_VE
                   : !vd_bit(br, vd_bmode_prob(t, l, 3))
                         ? (!vd_bit(br, vd_bmode_prob(t, l, 4)) ? VD_HE : (!vd_bit(br, vd_bmode_prob(t, l, 5)) ? VD_RD : VD_VR))
                         : (!vd_bit(br, vd_bmode_prob(t, l, 6)) ? VD_LD
                            : (!vd_bit(br, vd_bmode_prob(t, l, 7)) ? VD_VL : (!vd_bit(br, vd_bmode_prob(t, l, 8)) ? VD_HD : VD_HU)));
                top[x] = (uint8_t)ym;
                M.imodes[4 * y + x] = (uint8_t)ym;
                W.mode_mask |= 1u << (8 + ym);
            }
            W.left_modes[y] = (uint8_t)ym;
        }
    }
    M.uvmode = (uint8_t)(!vd_bit(br, 142) ? VD_DC : !vd_bit(br, 114) ? VD_VE : vd_bit(br, 183) ? VD_TM : VD_HE);
    W.mode_mask |= 1u << (4 + M.uvmode);
}

// ---------------------------------------------------------------- TOKENS
IMP_VP8_HD int vd_large_value(VdBool& br, const uint8_t* p, uint32_t* feat) {
    int v;
    if (!vd_bit(br, p[3])) {
        if (!vd_bit(br, p[4])) v = 2;
        else v = 3 + vd_bit(br, p[5]);
    } else if (!vd_bit(br, p[6])) {
        if (!vd_bit(br, p[7])) v = 5 + vd_bit(br, 159);
        else { v = 7 + 2 * vd_bit(br, 165); v += vd_bit(br, 145); }
    } else {
        const int bit1 = vd_bit(br, p[8]), bit0 = vd_bit(br, p[9 + bit1]), cat = 2 * bit1 + bit0;
        const int nbits = cat == 3 ? 11 : cat + 3;
        if (cat == 3) *feat |= IMPGPU_VP8_DEC_F_CAT6;
        v = 0;
        for (int k = 0; k < nbits; k++) v += v + vd_bit(br, vp8_cat_prob(cat + 3, k));
        v += 3 + (8 << cat);
    }
    return v;
}
// one block from position n: out in raster order, already multiplied and cut to 16 bits -> libwebp's count
IMP_VP8_HD int vd_coeffs(VdBool& br, const VdHdr& H, int type, int ctx, int dc, int ac, int n, int16_t* out, uint32_t* feat) {
    const uint8_t* p = H.prob[type][vp8_band(n)][ctx];
    for (; n < 16; ++n) {
        if (!vd_bit(br, p[0])) return n;
        while (!vd_bit(br, p[1])) {
            p = H.prob[type][vp8_band(++n)][0];
            if (n == 16) return 16;
        }
        const int nb = vp8_band(n + 1);
        int v;
        if (!vd_bit(br, p[2])) { v = 1; p = H.prob[type][nb][1]; }
        else { v = vd_large_value(br, p, feat); p = H.prob[type][nb][2]; }
        if (vd_bit(br, 128)) v = -v;
        out[vp8_zigzag(n)] = (int16_t)(v * (n > 0 ? ac : dc));
    }
    return 16;
}
IMP_VP8_HD uint32_t vd_nz_code(uint32_t acc, int nz, int dc_nz) { return (acc << 2) | (uint32_t)(nz > 3 ? 3 : (nz > 1 ? 2 : dc_nz)); }
// a macroblock's coefficients (M.coef zeroed here) -> whether nothing is left to add (libwebp's `skip` behind the parse)
IMP_VP8_HD int vd_mb_residuals(const VdHdr& H, VdWalk& W, VdMb& M, VdBool& br, int mx) {
    const uint16_t* q = H.dq[M.segment];
    for (int i = 0; i < 400; i++) M.coef[i] = 0;
    int16_t* dst = M.coef;
    uint8_t& tnz_all = W.top_nz[mx];
    int first, type;
    if (!M.is_i4) {
        int16_t dc[16];
        for (int i = 0; i < 16; i++) dc[i] = 0;
        const int nz = vd_coeffs(br, H, 1, W.top_dc[mx] + W.left_dc, q[2], q[3], 0, dc, &W.feat);
        W.top_dc[mx] = W.left_dc = (uint8_t)(nz > 0);
        if (nz > 1) {
            int in[16];
            int16_t o[16];
            for (int i = 0; i < 16; i++) in[i] = dc[i];
            vp8_iwht(in, o);
            for (int i = 0; i < 16; i++) dst[16 * i] = o[i];
        } else {
            const int dc0 = (dc[0] + 3) >> 3;
            for (int i = 0; i < 16; i++) dst[16 * i] = (int16_t)dc0;
        }
        first = 1; type = 0;
    } else { first = 0; type = 3; }
    uint32_t tnz = tnz_all & 0x0fu, lnz = W.left_nz & 0x0fu, non_zero_y = 0, non_zero_uv = 0;
    for (int y = 0; y < 4; y++) {
        uint32_t l = lnz & 1u, codes = 0;
        for (int x = 0; x < 4; x++) {
            const int nz = vd_coeffs(br, H, type, (int)(l + (tnz & 1u)), q[0], q[1], first, dst, &W.feat);
            l = nz > first;
            tnz = (tnz >> 1) | (l << 7);
            codes = vd_nz_code(codes, nz, dst[0] != 0);
            dst += 16;
        }
        tnz >>= 4;
        lnz = (lnz >> 1) | (l << 7);
        non_zero_y = (non_zero_y << 8) | codes;
    }
    uint32_t out_t = tnz, out_l = lnz >> 4;
    for (int ch = 0; ch < 4; ch += 2) {
        uint32_t codes = 0;
        tnz = (uint32_t)tnz_all >> (4 + ch);
        lnz = (uint32_t)W.left_nz >> (4 + ch);
        for (int y = 0; y < 2; y++) {
            uint32_t l = lnz & 1u;
            for (int x = 0; x < 2; x++) {
                const int nz = vd_coeffs(br, H, 2, (int)(l + (tnz & 1u)), q[4], q[5], 0, dst, &W.feat);
                l = nz > 0;
                tnz = (tnz >> 1) | (l << 3);
                codes = vd_nz_code(codes, nz, dst[0] != 0);
                dst += 16;
            }
            tnz >>= 2;
            lnz = (lnz >> 1) | (l << 5);
        }
        non_zero_uv |= codes << (4 * ch);
        out_t |= (tnz << 4) << ch;
        out_l |= (lnz & 0xf0u) << ch;
    }
    tnz_all = (uint8_t)out_t;
    W.left_nz = (uint8_t)out_l;
    M.nz_y = non_zero_y;
    M.nz_uv = non_zero_uv;
    return !(non_zero_y | non_zero_uv);
}

// ---------------------------------------------------------------- RECON
// the sample at (x, y) of a plane for prediction: 127 above the frame (the corner too), 129 left of it
IMP_VP8_HD int vd_at(const uint8_t* p, int stride, int x, int y) {
    if (y < 0) return 127;
    if (x < 0) return 129;
    return p[(size_t)y * (size_t)stride + (size_t)x];
}
// libwebp's inverse DCT: `full` is its SSE2 form (every pass in 16-bit lanes), otherwise its C forms for blocks of at most
// three coefficients (plain int); the two agree wherever nothing leaves 16 bits
IMP_VP8_HD void vd_idct_add(const int16_t* in, uint8_t* dst, int stride, bool full) {
    int res[16];
    if (!full) {
        int c[16];
        for (int i = 0; i < 16; i++) c[i] = in[i];
        vp8_idct(c, res);
    } else {
        int tmp[16];
        for (int i = 0; i < 4; i++) {
            const int a = in[i] + in[8 + i], b = in[i] - in[8 + i];
            const int cc = vp8_mul2(in[4 + i]) - vp8_mul1(in[12 + i]), d = vp8_mul1(in[4 + i]) + vp8_mul2(in[12 + i]);
            tmp[4 * i] = (int16_t)(a + d); tmp[4 * i + 1] = (int16_t)(b + cc); tmp[4 * i + 2] = (int16_t)(b - cc); tmp[4 * i + 3] = (int16_t)(a - d);
        }
        for (int i = 0; i < 4; i++) {
            const int dc = tmp[i] + 4, a = dc + tmp[8 + i], b = dc - tmp[8 + i];
            const int cc = vp8_mul2(tmp[4 + i]) - vp8_mul1(tmp[12 + i]), d = vp8_mul1(tmp[4 + i]) + vp8_mul2(tmp[12 + i]);
            res[4 * i] = (int16_t)(a + d) >> 3; res[4 * i + 1] = (int16_t)(b + cc) >> 3;
            res[4 * i + 2] = (int16_t)(b - cc) >> 3; res[4 * i + 3] = (int16_t)(a - d) >> 3;
        }
    }
    for (int k = 0; k < 16; k++) {
        uint8_t* d = dst + (size_t)(k >> 2) * (size_t)stride + (size_t)(k & 3);
        *d = (uint8_t)vp8_clip8((int)*d + res[k]);
    }
}
// a 16x16 or 8x8 prediction with libwebp's edge forms of DC
IMP_VP8_HD void vd_pred_square(uint8_t* p, int stride, int x0, int y0, int n, int mode) {
    int dc = 0;
    if (mode == VD_DC) {
        const int sh = n == 16 ? 4 : 3;
        int st = 0, sl = 0;
        for (int k = 0; k < n; k++) { st += vd_at(p, stride, x0 + k, y0 - 1); sl += vd_at(p, stride, x0 - 1, y0 + k); }
        dc = y0 > 0 && x0 > 0 ? (st + sl + n) >> (sh + 1) : (y0 > 0 ? (st + n / 2) >> sh : (x0 > 0 ? (sl + n / 2) >> sh : 128));
    }
    const int tl = vd_at(p, stride, x0 - 1, y0 - 1);
    for (int r = 0; r < n; r++) {
        const int l = vd_at(p, stride, x0 - 1, y0 + r);
        for (int c = 0; c < n; c++) {
            const int t = vd_at(p, stride, x0 + c, y0 - 1);
            const int v = mode == VD_DC ? dc : (mode == VD_VE ? t : (mode == VD_HE ? l : vp8_clip8(t + l - tl)));
            p[(size_t)(y0 + r) * (size_t)stride + (size_t)(x0 + c)] = (uint8_t)v;
        }
    }
}
IMP_VP8_HD int vd_avg3(int a, int b, int c) { return (a + 2 * b + c + 2) >> 2; }
IMP_VP8_HD int vd_avg2(int a, int b) { return (a + b + 1) >> 1; }
// a 4x4 prediction: E[0] the corner, E[1..8] the row above and above-right, L[0..3] the left column -> o, raster
IMP_VP8_HD void vd_pred4(int mode, const int* E, const int* L, int* o) {
    const int X = E[0], A = E[1], B = E[2], C = E[3], D = E[4], Ee = E[5], F = E[6], G = E[7], Hh = E[8];
    const int I = L[0], J = L[1], K = L[2], Ll = L[3];
#define O(x, y) o[(y) * 4 + (x)]
    switch (mode) {
    case VD_DC: {
        const int dc = (A + B + C + D + I + J + K + Ll + 4) >> 3;
        for (int i = 0; i < 16; i++) o[i] = dc;
        break;
    }
    case VD_TM:
        for (int y = 0; y < 4; y++)
            for (int x = 0; x < 4; x++) O(x, y) = vp8_clip8(E[1 + x] + L[y] - X);
        break;
    case VD_VE:
        for (int y = 0; y < 4; y++) { O(0, y) = vd_avg3(X, A, B); O(1, y) = vd_avg3(A, B, C); O(2, y) = vd_avg3(B, C, D); O(3, y) = vd_avg3(C, D, Ee); }
        break;
    case VD_HE:
        for (int x = 0; x < 4; x++) { O(x, 0) = vd_avg3(X, I, J); O(x, 1) = vd_avg3(I, J, K); O(x, 2) = vd_avg3(J, K, Ll); O(x, 3) = vd_avg3(K, Ll, Ll); }
        break;
    case VD_RD:
        O(0, 3) = vd_avg3(J, K, Ll);
        O(1, 3) = O(0, 2) = vd_avg3(I, J, K);
        O(2, 3) = O(1, 2) = O(0, 1) = vd_avg3(X, I, J);
        O(3, 3) = O(2, 2) = O(1, 1) = O(0, 0) = vd_avg3(A, X, I);
        O(3, 2) = O(2, 1) = O(1, 0) = vd_avg3(B, A, X);
        O(3, 1) = O(2, 0) = vd_avg3(C, B, A);
        O(3, 0) = vd_avg3(D, C, B);
        break;
    case VD_VR:
        O(0, 0) = O(1, 2) = vd_avg2(X, A);
        O(1, 0) = O(2, 2) = vd_avg2(A, B);
        O(2, 0) = O(3, 2) = vd_avg2(B, C);
        O(3, 0) = vd_avg2(C, D);
        O(0, 3) = vd_avg3(K, J, I);
        O(0, 2) = vd_avg3(J, I, X);
        O(0, 1) = O(1, 3) = vd_avg3(I, X, A);
        O(1, 1) = O(2, 3) = vd_avg3(X, A, B);
        O(2, 1) = O(3, 3) = vd_avg3(A, B, C);
        O(3, 1) = vd_avg3(B, C, D);
        break;
    case VD_LD:
        O(0, 0) = vd_avg3(A, B, C);
        O(1, 0) = O(0, 1) = vd_avg3(B, C, D);
        O(2, 0) = O(1, 1) = O(0, 2) = vd_avg3(C, D, Ee);
        O(3, 0) = O(2, 1) = O(1, 2) = O(0, 3) = vd_avg3(D, Ee, F);
        O(3, 1) = O(2, 2) = O(1, 3) = vd_avg3(Ee, F, G);
        O(3, 2) = O(2, 3) = vd_avg3(F, G, Hh);
        O(3, 3) = vd_avg3(G, Hh, Hh);
        break;
    case VD_VL:
        O(0, 0) = vd_avg2(A, B);
        O(1, 0) = O(0, 2) = vd_avg2(B, C);
        O(2, 0) = O(1, 2) = vd_avg2(C, D);
        O(3, 0) = O(2, 2) = vd_avg2(D, Ee);
        O(0, 1) = vd_avg3(A, B, C);
        O(1, 1) = O(0, 3) = vd_avg3(B, C, D);
        O(2, 1) = O(1, 3) = vd_avg3(C, D, Ee);
        O(3, 1) = O(2, 3) = vd_avg3(D, Ee, F);
        O(3, 2) = vd_avg3(Ee, F, G);
        O(3, 3) = vd_avg3(F, G, Hh);
        break;
    case VD_HD:
        O(0, 0) = O(2, 1) = vd_avg2(I, X);
        O(0, 1) = O(2, 2) = vd_avg2(J, I);
        O(0, 2) = O(2, 3) = vd_avg2(K, J);
        O(0, 3) = vd_avg2(Ll, K);
        O(3, 0) = vd_avg3(A, B, C);
        O(2, 0) = vd_avg3(X, A, B);
        O(1, 0) = O(3, 1) = vd_avg3(I, X, A);
        O(1, 1) = O(3, 2) = vd_avg3(J, I, X);
        O(1, 2) = O(3, 3) = vd_avg3(K, J, I);
        O(1, 3) = vd_avg3(Ll, K, J);
        break;
    default:                                                           // VD_HU
        O(0, 0) = vd_avg2(I, J);
        O(2, 0) = O(0, 1) = vd_avg2(J, K);
        O(2, 1) = O(0, 2) = vd_avg2(K, Ll);
        O(1, 0) = vd_avg3(I, J, K);
        O(3, 0) = O(1, 1) = vd_avg3(J, K, Ll);
        O(3, 1) = O(1, 2) = vd_avg3(K, Ll, Ll);
        O(3, 2) = O(2, 2) = O(0, 3) = O(1, 3) = O(2, 3) = O(3, 3) = Ll;
        break;
    }
#undef O
}
// a macroblock into the planes.  Prediction reads the planes as reconstructed, never filtered: the filter is a later launch.
IMP_VP8_HD void vd_mb_recon(const VdHdr& H, const VdPlanes& P, const VdMb& M, int mx, int my) {
    const int x0 = mx * 16, y0 = my * 16;
    uint32_t bits = M.nz_y;
    if (M.is_i4) {
        int tr[4];                                                     // above-right of the macroblock: every sub-block of column 3 reads it
        for (int k = 0; k < 4; k++)
            tr[k] = my == 0 ? 127 : (mx < H.mbw - 1 ? P.y[(size_t)(y0 - 1) * (size_t)P.ys + (size_t)(x0 + 16 + k)] : P.y[(size_t)(y0 - 1) * (size_t)P.ys + (size_t)(x0 + 15)]);
        for (int n = 0; n < 16; n++, bits <<= 2) {
            const int bx = x0 + (n & 3) * 4, by = y0 + (n >> 2) * 4;
            int E[9], L[4], o[16];
            for (int k = 0; k < 5; k++) E[k] = vd_at(P.y, P.ys, bx - 1 + k, by - 1);
            for (int k = 0; k < 4; k++) {
                E[5 + k] = (n & 3) == 3 ? tr[k] : vd_at(P.y, P.ys, bx + 4 + k, by - 1);
                L[k] = vd_at(P.y, P.ys, bx - 1, by + k);
            }
            vd_pred4(M.imodes[n], E, L, o);
            uint8_t* d = P.y + (size_t)by * (size_t)P.ys + (size_t)bx;
            for (int k = 0; k < 16; k++) d[(size_t)(k >> 2) * (size_t)P.ys + (size_t)(k & 3)] = (uint8_t)o[k];
            if (bits >> 30) vd_idct_add(M.coef + n * 16, d, P.ys, (bits >> 30) == 3u);
        }
    } else {
        vd_pred_square(P.y, P.ys, x0, y0, 16, M.imodes[0]);
        for (int n = 0; n < 16; n++, bits <<= 2)
            if (bits >> 30) vd_idct_add(M.coef + n * 16, P.y + (size_t)(y0 + (n >> 2) * 4) * (size_t)P.ys + (size_t)(x0 + (n & 3) * 4), P.ys, (bits >> 30) == 3u);
    }
    for (int p = 0; p < 2; p++) {
        uint8_t* c = p ? P.v : P.u;
        const uint32_t b = (M.nz_uv >> (8 * p)) & 0xffu;
        vd_pred_square(c, P.cs, mx * 8, my * 8, 8, M.uvmode);
        if (!b) continue;
        const bool full = (b & 0xaau) != 0u;                           // one block past its DC: libwebp runs the full transform on all four
        for (int k = 0; k < 4; k++) {
            const int16_t* in = M.coef + (16 + 4 * p + k) * 16;
            if (full || in[0]) vd_idct_add(in, c + (size_t)(my * 8 + (k >> 1) * 4) * (size_t)P.cs + (size_t)(mx * 8 + (k & 1) * 4), P.cs, full);
        }
    }
}
// one file's macroblocks in raster order: modes, tokens, reconstruction; finfo: a word a macroblock for the filter
// (limit, inner level << 8, hev threshold << 16, inner << 24) -> VD_*
IMP_VP8_HD int vd_decode_mbs(const VdHdr& H, const uint8_t* chunk, VdWalk& W, VdMb& M, const VdPlanes& P, uint32_t* finfo) {
    W.br.buf = chunk + H.first_off; W.br.size = H.first_size; W.br.pos = H.br_pos; W.br.value = H.br_value; W.br.range = H.br_range;
    W.br.bits = H.br_bits; W.br.eof = H.br_eof;
    for (int p = 0; p < 8; p++) vd_bool_begin(W.parts[p], chunk + H.part_off[p], p < H.nparts ? H.part_size[p] : 0u);
    W.feat = 0; W.mode_mask = 0;
    for (int x = 0; x < H.mbw; x++) { W.top_nz[x] = 0; W.top_dc[x] = 0; }
    for (int x = 0; x < 4 * H.mbw; x++) W.top_modes[x] = VD_DC;
    for (int my = 0; my < H.mbh; my++) {
        VdBool& tb = W.parts[my & (H.nparts - 1)];
        vd_row_begin(W);
        for (int mx = 0; mx < H.mbw; mx++) {
            vd_mb_modes(H, W, M, mx);
            int skip = M.skip;
            if (!skip) skip = vd_mb_residuals(H, W, M, tb, mx);
            else {
                W.left_nz = W.top_nz[mx] = 0;
                if (!M.is_i4) W.left_dc = W.top_dc[mx] = 0;
                M.nz_y = M.nz_uv = 0;
            }
            if (tb.eof) return VD_DAMAGED;                             // libwebp: per macroblock
            vd_mb_recon(H, P, M, mx, my);
            const uint8_t* f = H.fstr[M.segment][M.is_i4];
            finfo[(size_t)my * (size_t)H.mbw + (size_t)mx] = (uint32_t)f[0] | (uint32_t)f[1] << 8 | (uint32_t)f[2] << 16 | (uint32_t)(f[3] | !skip) << 24;
        }
        if (W.br.eof) return VD_DAMAGED;                               // and per row for the first partition
    }
    return VD_OK;
}

// ---------------------------------------------------------------- FILTER
IMP_VP8_HD int vd_abs(int v) { return v < 0 ? -v : v; }
IMP_VP8_HD int vd_sclip1(int v) { return v < -128 ? -128 : (v > 127 ? 127 : v); }   // libwebp's tables as arithmetic
IMP_VP8_HD int vd_sclip2(int v) { return v < -16 ? -16 : (v > 15 ? 15 : v); }
IMP_VP8_HD void vd_filter2(uint8_t* p, ptrdiff_t s) {
    const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
    const int a = 3 * (q0 - p0) + vd_sclip1(p1 - q1);
    const int a1 = vd_sclip2((a + 4) >> 3), a2 = vd_sclip2((a + 3) >> 3);
    p[-s] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
}
IMP_VP8_HD void vd_filter4(uint8_t* p, ptrdiff_t s) {
    const int p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s];
    const int a = 3 * (q0 - p0);
    const int a1 = vd_sclip2((a + 4) >> 3), a2 = vd_sclip2((a + 3) >> 3), a3 = (a1 + 1) >> 1;
    p[-2 * s] = (uint8_t)vp8_clip8(p1 + a3);
    p[-s] = (uint8_t)vp8_clip8(p0 + a2);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[s] = (uint8_t)vp8_clip8(q1 - a3);
}
IMP_VP8_HD void vd_filter6(uint8_t* p, ptrdiff_t s) {
    const int p2 = p[-3 * s], p1 = p[-2 * s], p0 = p[-s], q0 = p[0], q1 = p[s], q2 = p[2 * s];
    const int a = vd_sclip1(3 * (q0 - p0) + vd_sclip1(p1 - q1));
    const int a1 = (27 * a + 63) >> 7, a2 = (18 * a + 63) >> 7, a3 = (9 * a + 63) >> 7;
    p[-3 * s] = (uint8_t)vp8_clip8(p2 + a3);
    p[-2 * s] = (uint8_t)vp8_clip8(p1 + a2);
    p[-s] = (uint8_t)vp8_clip8(p0 + a1);
    p[0] = (uint8_t)vp8_clip8(q0 - a1);
    p[s] = (uint8_t)vp8_clip8(q1 - a2);
    p[2 * s] = (uint8_t)vp8_clip8(q2 - a3);
}
IMP_VP8_HD bool vd_needs(const uint8_t* p, ptrdiff_t s, int t) {
    return 4 * vd_abs((int)p[-s] - (int)p[0]) + vd_abs((int)p[-2 * s] - (int)p[s]) <= t;
}
IMP_VP8_HD bool vd_needs2(const uint8_t* p, ptrdiff_t s, int t, int it) {
    if (!vd_needs(p, s, t)) return false;
    return vd_abs((int)p[-4 * s] - (int)p[-3 * s]) <= it && vd_abs((int)p[-3 * s] - (int)p[-2 * s]) <= it && vd_abs((int)p[-2 * s] - (int)p[-s]) <= it &&
           vd_abs((int)p[3 * s] - (int)p[2 * s]) <= it && vd_abs((int)p[2 * s] - (int)p[s]) <= it && vd_abs((int)p[s] - (int)p[0]) <= it;
}
IMP_VP8_HD bool vd_hev(const uint8_t* p, ptrdiff_t s, int t) {
    return vd_abs((int)p[-2 * s] - (int)p[-s]) > t || vd_abs((int)p[s] - (int)p[0]) > t;
}
constexpr int VD_FILTER_STEPS = 8, VD_FILTER_LANES = 32;
// Step `step` of macroblock (mx, my) for lane 0..31: steps 0..3 the edges between columns (the macroblock's left edge, then
// x = 4, 8, 12), steps 4..7 those between rows.  Lanes 0..15 take a luma line each, 16..23 a U line, 24..31 a V line (chroma:
// the macroblock edge and the one inner edge at 4, in steps 0, 2, 4, 6).  The lines of a step touch disjoint samples.
IMP_VP8_HD void vd_filter_step(const VdHdr& H, const VdPlanes& P, uint32_t info, int mx, int my, int step, int lane) {
    const int limit = (int)(info & 255u), ilevel = (int)((info >> 8) & 255u), hevt = (int)((info >> 16) & 255u), inner = (int)(info >> 24);
    if (!limit || lane >= VD_FILTER_LANES) return;
    const bool vertical = step >= 4;                                   // an edge between rows
    const int k = step & 3;
    if (k == 0 ? (vertical ? my == 0 : mx == 0) : !inner) return;
    const int lim = 2 * (limit + (k == 0 ? 4 : 0)) + 1;
    const bool luma = lane < 16;
    if (!luma && (H.filter_type == 1 || (k & 1))) return;
    uint8_t* plane = luma ? P.y : (lane < 24 ? P.u : P.v);
    const ptrdiff_t stride = luma ? P.ys : P.cs;
    const int n = luma ? 16 : 8, line = luma ? lane : (lane & 7), off = luma ? 4 * k : 2 * k;
    uint8_t* p = vertical ? plane + (ptrdiff_t)(my * n + off) * stride + (mx * n + line) : plane + (ptrdiff_t)(my * n + line) * stride + (mx * n + off);
    const ptrdiff_t s = vertical ? stride : 1;
    if (H.filter_type == 1) {
        if (vd_needs(p, s, lim)) vd_filter2(p, s);
    } else if (vd_needs2(p, s, lim, ilevel)) {
        if (vd_hev(p, s, hevt)) vd_filter2(p, s);
        else if (k == 0) vd_filter6(p, s);
        else vd_filter4(p, s);
    }
}

// ---------------------------------------------------------------- FRAME
IMP_VP8_HD int vd_up(const uint8_t* c, int cs, int cw, int ch, int x, int y) {      // the upsampled chroma at pixel (x, y)
    const int cx = x >> 1, cy = y >> 1;
    int ox = (x & 1) ? cx + 1 : cx - 1, oy = (y & 1) ? cy + 1 : cy - 1;
    ox = ox < 0 ? 0 : (ox > cw - 1 ? cw - 1 : ox);
    oy = oy < 0 ? 0 : (oy > ch - 1 ? ch - 1 : oy);
    const int near = c[(size_t)cy * (size_t)cs + (size_t)cx], horz = c[(size_t)cy * (size_t)cs + (size_t)ox];
    const int vert = c[(size_t)oy * (size_t)cs + (size_t)cx], diag = c[(size_t)oy * (size_t)cs + (size_t)ox];
    return (9 * near + 3 * vert + 3 * horz + diag + 8) >> 4;
}
IMP_VP8_HD int vd_mh(int a, int c) { return (a * c) >> 8; }
IMP_VP8_HD int vd_clip6(int v) { return (v & ~16383) == 0 ? v >> 6 : (v < 0 ? 0 : 255); }
IMP_VP8_HD uint32_t vd_frame_pixel(const VdPlanes& P, int w, int h, int x, int y) {
    const int cw = (w + 1) >> 1, ch = (h + 1) >> 1;
    const int yy = P.y[(size_t)y * (size_t)P.ys + (size_t)x], u = vd_up(P.u, P.cs, cw, ch, x, y), v = vd_up(P.v, P.cs, cw, ch, x, y);
    const int r = vd_clip6(vd_mh(yy, 19077) + vd_mh(v, 26149) - 14234);
    const int g = vd_clip6(vd_mh(yy, 19077) - vd_mh(u, 6419) - vd_mh(v, 13320) + 8708);
    const int b = vd_clip6(vd_mh(yy, 19077) + vd_mh(u, 33050) - 17685);
    return (uint32_t)b | (uint32_t)g << 8 | (uint32_t)r << 16 | 0xff000000u;
}

// ---------------------------------------------------------------- the device block (imp_webp_dec.cpp lays it out)
struct VdFileDesc {
    VdHdr hdr;
    long long chunk_off, y_off, u_off, v_off, finfo_off, ctx_off;      // ctx: 6 mbw bytes
    void* img;
};
#if defined(__HIPCC__)
int launch_vp8_decode(uint8_t* mem, const VdFileDesc* files, uint32_t* status, int nfiles, hipStream_t s);
#endif

}  // namespace imp
