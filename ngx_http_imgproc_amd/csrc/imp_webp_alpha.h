// imp_webp_alpha.h -- the alpha plane of a lossy WebP upload (VP8X + ALPH + `VP8 `): the lane code of k_webp_alpha
// (imp_webp_alpha.hip), which the host model runs too, and the host front that finds the plane.
//
// An ALPH chunk is a header byte -- bits 0-1 method (0 raw, 1 a VP8L stream without its five header bytes), bits 2-3 the
// filter (0 none, 1 horizontal, 2 vertical, 3 gradient), bits 4-5 pre-processing (0 or 1: nothing to undo), bits 6-7
// reserved -- and the plane's residuals: w * h bytes, or the green channel of the VP8L image.  The filter's inverse, all
// sums mod 256, `a` the alpha:
//   row 0 (every filter but none)   a[0][x] = r[0][x] + a[0][x-1], a[0][0] = r[0][0]
//   column 0 of the rows below      a[y][0] = r[y][0] + a[y-1][0]
//   elsewhere                       horizontal + a[y][x-1]; vertical + a[y-1][x];
//                                   gradient + clip(a[y][x-1] + a[y-1][x] - a[y-1][x-1], 0, 255)
// The alpha goes into byte 3 of the frame's pixels; nothing else of the frame is written.
//
// How the lanes share the work (WA_THREADS lanes a file):
//   none        a parallel copy.
//   horizontal  a[y][x] = a[y][0] + r[y][1] + .. + r[y][x]: column 0 is one prefix sum down the plane (a wave, 64 rows a
//               step, kept in LDS), then every row is a prefix sum of its own, a wave a row, 64 columns a step.
//   vertical    row 0 is a prefix sum (a wave, 64 columns a step), then a lane a column adds downwards: neighbouring lanes
//               read and write neighbouring bytes.
//   gradient    the clip makes it sequential: a[y][x] needs row y-1 through column x.  A wave takes a band of 64 rows, lane
//               j row row0 + j, skewed a column apart: at step s lane j is at column s - j.  Its left is its own last
//               value, its top the value lane j-1 made a step before (one cross-lane move), its top-left the top it was
//               handed a step before.  Lane 0's top is the last row of the band above, which that band's last lane left in
//               LDS.  w + 63 steps a band, h/64 bands one after the other: every loop is bounded by w and h.
#pragma once
#include <stdint.h>
#include <stddef.h>
#if defined(__HIPCC__)
#define IMP_WA_HD __host__ __device__ __forceinline__
#else
#define IMP_WA_HD inline
#endif

namespace imp {

constexpr int WA_THREADS = 256, WA_WAVE = 64;
constexpr int WA_MAX_SIDE = 16383;                                       // a VP8 frame's: what the LDS row / column holds
enum { WA_NONE = 0, WA_HORIZONTAL = 1, WA_VERTICAL = 2, WA_GRADIENT = 3 };

// the residuals: raw bytes (step 1, first 0) or byte 1, the green, of the lossless launches' ARGB words (step 4, first 1)
struct WaSrc {
    const uint8_t* p;
    int step, first;
};
IMP_WA_HD uint32_t wa_res(const WaSrc& s, size_t i) { return s.p[i * (size_t)s.step + (size_t)s.first]; }
IMP_WA_HD void wa_put(uint8_t* img, size_t i, uint32_t a) { img[i * 4u + 3u] = (uint8_t)a; }

IMP_WA_HD void wa_copy(const WaSrc& s, uint8_t* img, size_t npix, uint32_t lane, uint32_t nlanes) {
    for (size_t i = lane; i < npix; i += nlanes) wa_put(img, i, wa_res(s, i));
}

// vertical: column x below row 0, whose value is `top`
IMP_WA_HD void wa_column(const WaSrc& s, uint8_t* img, int w, int h, int x, uint32_t top) {
    uint32_t a = top;
    for (int y = 1; y < h; y++) {
        const size_t i = (size_t)y * (size_t)w + (size_t)x;
        a = (a + wa_res(s, i)) & 255u;
        wa_put(img, i, a);
    }
}

IMP_WA_HD uint32_t wa_gradient(uint32_t left, uint32_t top, uint32_t topleft) {
    const int g = (int)left + (int)top - (int)topleft;
    return g < 0 ? 0u : g > 255 ? 255u : (uint32_t)g;
}

// gradient: what a lane of a band carries from step to step
struct WaLane {
    uint32_t mine;                       // the value it made last: its left, and the top of the lane below a step later
    uint32_t topleft;                    // the top it was handed last
};
IMP_WA_HD int wa_band_steps(int w, int rows) { return w + rows - 1; }
// One step of lane `lane` of the band whose first row is row0: column step - lane of row row0 + lane, if there is one.
// `top` is a[y-1][x] (anything in row 0).  -> true: L.mine is the new a[y][x]
IMP_WA_HD bool wa_gradient_step(const WaSrc& s, uint8_t* img, int w, int h, int row0, int step, int lane, uint32_t top, WaLane& L) {
    const int x = step - lane, y = row0 + lane;
    if (x < 0 || x >= w || y >= h) return false;
    const size_t i = (size_t)y * (size_t)w + (size_t)x;
    const uint32_t pred = y == 0 ? (x == 0 ? 0u : L.mine) : x == 0 ? top : wa_gradient(L.mine, top, L.topleft);
    L.mine = (wa_res(s, i) + pred) & 255u;
    L.topleft = top;
    wa_put(img, i, L.mine);
    return true;
}

// ---------------------------------------------------------------- what the kernel reads (imp_webp_alpha.hip)
// a file with an alpha plane; src_off is into the group's device block
struct WaFileDesc {
    long long src_off;                   // the raw bytes, or the scratch plane the lossless launches wrote
    uint8_t* img;                        // the frame k_vp8_dec_frame wrote: w * 4 bytes a row
    int w, h, filter, method;
    int status_frame, status_stream;     // its status words: a file with one of them set is left alone (method 0: the same word)
};
#if defined(__HIPCC__)
int launch_webp_alpha(uint8_t* mem, const WaFileDesc* files, const uint32_t* status, int nfiles, hipStream_t s);
#endif

// ---------------------------------------------------------------- the host's run of the lanes
// the whole plane with no device: the kernel's phases, the lanes one after the other
inline void wa_unfilter_host(const WaSrc& s, uint8_t* img, int w, int h, int filter) {
    const size_t npix = (size_t)w * (size_t)h;
    if (filter == WA_NONE) {
        for (uint32_t j = 0; j < (uint32_t)WA_THREADS; j++) wa_copy(s, img, npix, j, (uint32_t)WA_THREADS);
    } else if (filter == WA_HORIZONTAL) {
        uint32_t col = 0;
        for (int y = 0; y < h; y++) {
            col = (col + wa_res(s, (size_t)y * (size_t)w)) & 255u;
            uint32_t a = col;
            wa_put(img, (size_t)y * (size_t)w, a);
            for (int x = 1; x < w; x++) {
                a = (a + wa_res(s, (size_t)y * (size_t)w + (size_t)x)) & 255u;
                wa_put(img, (size_t)y * (size_t)w + (size_t)x, a);
            }
        }
    } else if (filter == WA_VERTICAL) {
        uint32_t a = 0;
        for (int x = 0; x < w; x++) {
            a = (a + wa_res(s, (size_t)x)) & 255u;
            wa_put(img, (size_t)x, a);
            wa_column(s, img, w, h, x, a);
        }
    } else {
        uint8_t* last = new uint8_t[(size_t)w];                          // the band's last row, for the band below
        for (int row0 = 0; row0 < h; row0 += WA_WAVE) {
            const int rows = h - row0 < WA_WAVE ? h - row0 : WA_WAVE;
            WaLane L[WA_WAVE] = {};
            uint32_t top[WA_WAVE];
            for (int step = 0; step < wa_band_steps(w, rows); step++) {
                for (int j = 0; j < WA_WAVE; j++) top[j] = j ? L[j - 1].mine : (row0 && step < w ? last[step] : 0u);   // the cross-lane move
                for (int j = 0; j < rows; j++)
                    if (wa_gradient_step(s, img, w, h, row0, step, j, top[j], L[j]) && j == rows - 1) last[step - j] = (uint8_t)L[j].mine;
            }
        }
        delete[] last;
    }
}

}  // namespace imp
