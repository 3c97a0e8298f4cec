/*
 * impgpu_gif.h -- the GIF container walk, plain C99 over libc: ONE parser for libimpgpu.so (impgpu_image_decode_gif,
 * impgpu_gif_info, impgpu_gif_pages) and for a worker (glue/imp_gpu_client.c reads Frame.Time and Frame.Dispose, which
 * SaveGIF needs, advancedio.c:381-397, from it), fuzzed once (tests/c/gif_fuzz.cpp).
 *
 * The walk reads the header, the logical screen descriptor, the global colour table, the extensions and the image
 * descriptors up to the trailer, and DECOMPRESSES NOTHING: a page's record says where its LZW sub-blocks lie.  The
 * verdicts are conservative like the JPEG and PNG fronts': what is not provably what FreeImage would hand LoadGIF
 * (advancedio.c:103-274) goes back to the host decoder.
 *   IMP_ERROR_UNSUPPORTED     not GIF87a / GIF89a; a page with neither a local nor a global table; min_code_size outside
 *                             2..8; a page or canvas side above 4096; more than IMPB_MAX_GIF_PAGES pages; no page
 *   IMP_ERROR_DECODE_FAILED   a block or sub-block chain that runs past `size`; a page of zero width or height; an unknown
 *                             block introducer; no trailer
 *   IMP_ERROR_MALLOC_FAILED   more pages than `cap` records (*count is still the file's page count: call again)
 */
#ifndef IMPGPU_GIF_H
#define IMPGPU_GIF_H

#include <stddef.h>
#include <string.h>
#include "impgpu_broker.h"   /* IMPB_MAX_GIF_PAGES, the IMP_* codes */

#define IMPGPU_GIF_MAX_SIDE 4096

typedef struct impgpu_gif_desc {
    int left, top, width, height;      /* the image descriptor (advancedio.c:159-174 reads them as FrameLeft / FrameTop) */
    int interlaced;
    int dispose;                       /* of the nearest preceding graphic control extension (21 F9); 0 without one */
    int transparency_key;              /* -1 unless that extension's flag is set */
    int time_ms;                       /* its delay x 10 */
    size_t palette_at;                 /* the local colour table, else the global one: offset of its first R,G,B triple ... */
    int palette_entries;               /* ... and how many there are (2..256) */
    int min_code_size;
    size_t data_at;                    /* the first LZW sub-block (its length byte) */
    size_t data_bytes;                 /* the sum of the sub-block payloads */
} impgpu_gif_desc;

/* The sub-block chain at `at`: *end = the offset behind its terminator, *payload = the sum of the payloads.  0 when the
 * chain runs past `size`. */
static inline int impgpu_gif_chain(const unsigned char* blob, size_t size, size_t at, size_t* end, size_t* payload) {
    size_t sum = 0;
    for (;;) {
        if (at >= size) return 0;
        const size_t n = blob[at++];
        if (!n) break;
        if (n > size - at) return 0;
        at += n;
        sum += n;
    }
    *end = at;
    *payload = sum;
    return 1;
}

/* A page's sub-block payloads, one after the other, into `out` (desc->data_bytes bytes): the length bytes are dropped. */
static inline void impgpu_gif_gather(const unsigned char* blob, const impgpu_gif_desc* desc, unsigned char* out) {
    size_t at = desc->data_at, done = 0;
    while (done < desc->data_bytes) {
        const size_t n = blob[at++];
        if (!n) break;
        memcpy(out + done, blob + at, n);
        at += n;
        done += n;
    }
}

/* `pages` may be NULL with cap 0 (count and canvas only).  canvas = page 0's width x height (advancedio.c:134-137), not
 * the logical screen. */
static inline int impgpu_gif_walk(const unsigned char* blob, size_t size, impgpu_gif_desc* pages, int cap, int* count,
                                  int* canvas_w, int* canvas_h) {
    if (count) *count = 0;
    if (canvas_w) *canvas_w = 0;
    if (canvas_h) *canvas_h = 0;
    if (!blob || cap < 0 || (cap > 0 && !pages)) return IMP_ERROR_INVALID_ARGS;
    if (size < 6 || (memcmp(blob, "GIF87a", 6) != 0 && memcmp(blob, "GIF89a", 6) != 0)) return IMP_ERROR_UNSUPPORTED;
    if (size < 13) return IMP_ERROR_DECODE_FAILED;
    size_t at = 13, global_at = 0;
    int global_entries = 0;
    if (blob[10] & 0x80) {
        global_entries = 2 << (blob[10] & 7);
        global_at = at;
        if ((size_t)global_entries * 3 > size - at) return IMP_ERROR_DECODE_FAILED;
        at += (size_t)global_entries * 3;
    }
    int n = 0, dispose = 0, key = -1, time_ms = 0, cw = 0, ch = 0;
    for (;;) {
        if (at >= size) return IMP_ERROR_DECODE_FAILED;               /* no trailer */
        const unsigned char intro = blob[at++];
        if (intro == 0x3B) break;
        if (intro == 0x21) {                                          /* an extension: label, then a sub-block chain */
            if (at >= size) return IMP_ERROR_DECODE_FAILED;
            const unsigned char label = blob[at++];
            if (label == 0xF9 && at < size && blob[at] == 4 && size - at >= 5) {
                const unsigned char flags = blob[at + 1];
                dispose = (flags >> 2) & 7;
                time_ms = (blob[at + 2] | (blob[at + 3] << 8)) * 10;
                key = (flags & 1) ? blob[at + 4] : -1;
            }
            size_t end, payload;
            if (!impgpu_gif_chain(blob, size, at, &end, &payload)) return IMP_ERROR_DECODE_FAILED;
            at = end;
            continue;
        }
        if (intro != 0x2C) return IMP_ERROR_DECODE_FAILED;            /* an unknown block introducer */
        if (size - at < 9) return IMP_ERROR_DECODE_FAILED;
        impgpu_gif_desc d;
        d.left = blob[at] | (blob[at + 1] << 8);
        d.top = blob[at + 2] | (blob[at + 3] << 8);
        d.width = blob[at + 4] | (blob[at + 5] << 8);
        d.height = blob[at + 6] | (blob[at + 7] << 8);
        const unsigned char flags = blob[at + 8];
        at += 9;
        d.interlaced = (flags >> 6) & 1;
        d.dispose = dispose;
        d.transparency_key = key;
        d.time_ms = time_ms;
        if (flags & 0x80) {
            d.palette_entries = 2 << (flags & 7);
            d.palette_at = at;
            if ((size_t)d.palette_entries * 3 > size - at) return IMP_ERROR_DECODE_FAILED;
            at += (size_t)d.palette_entries * 3;
        } else {
            d.palette_entries = global_entries;
            d.palette_at = global_at;
        }
        if (at >= size) return IMP_ERROR_DECODE_FAILED;
        d.min_code_size = blob[at++];
        d.data_at = at;
        size_t end;
        if (!impgpu_gif_chain(blob, size, at, &end, &d.data_bytes)) return IMP_ERROR_DECODE_FAILED;
        at = end;
        if (d.width == 0 || d.height == 0) return IMP_ERROR_DECODE_FAILED;
        if (!d.palette_entries || d.min_code_size < 2 || d.min_code_size > 8 || d.width > IMPGPU_GIF_MAX_SIDE ||
            d.height > IMPGPU_GIF_MAX_SIDE)
            return IMP_ERROR_UNSUPPORTED;
        if (n == 0) { cw = d.width; ch = d.height; }
        if (n >= IMPB_MAX_GIF_PAGES) return IMP_ERROR_UNSUPPORTED;
        if (n < cap) pages[n] = d;
        n++;
        dispose = 0; key = -1; time_ms = 0;                           /* a graphic control extension serves ONE image */
    }
    if (n == 0) return IMP_ERROR_UNSUPPORTED;
    if (count) *count = n;
    if (canvas_w) *canvas_w = cw;
    if (canvas_h) *canvas_h = ch;
    return n > cap && pages ? IMP_ERROR_MALLOC_FAILED : IMP_OK;
}

#endif
