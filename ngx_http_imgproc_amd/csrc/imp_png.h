// imp_png.h -- the host side of the PNG front (imp_png.cpp), shared with the kernel file (imp_png.hip)
#pragma once
#include <cstddef>
#include <cstdint>

namespace imp {

constexpr int PNG_MAX_W = 4096;          // what k_png_unfilter's LDS layout holds
constexpr int PNG_MAX_H = 16384;

struct PngHeader {
    int w = 0, h = 0, bpp = 0;
    bool taken = false;                  // within what k_png_unfilter does
    int depth = 0, colour = 0, interlace = 0;
};

// IMP_OK with H filled; IMP_ERROR_UNSUPPORTED = not a PNG at all; IMP_ERROR_DECODE_FAILED = a PNG whose IHDR is damaged
int png_header(const unsigned char* blob, size_t size, PngHeader* H);
// the chunk walk (every CRC checked), the zlib stream of the IDAT chunks inflated into dst[h * (w * bpp + 1)], the filter
// bytes checked: IMP_OK or IMP_ERROR_DECODE_FAILED
// rows (optional) is called while the inflate goes, at the ends of deflate blocks: rows [0, complete) of dst are final and their
// filter bytes checked; a non-zero return stops the decode with that code.
typedef int (*png_rows_fn)(void* ctx, int complete);
int png_scanlines(const unsigned char* blob, size_t size, const PngHeader& H, unsigned char* dst, png_rows_fn rows = nullptr, void* ctx = nullptr);

// The part of a decode before the inflate, shared by the host route (png_scanlines*) and the device route (imp_png.hip,
// IMPGPU_PNG_DEVICE_INFLATE): the chunk walk of a file whose header png_header read, every CRC checked, and the IDAT payloads
// gathered, in order, into dst[0, cap) -- they are ONE zlib stream (PNG specification 10.1).  IMP_OK with *length, or
// IMP_ERROR_DECODE_FAILED (a damaged chunk, an unknown critical chunk, no IDAT, no IEND; cap too small cannot happen for
// cap >= size).
int png_gather_idat(const unsigned char* blob, size_t size, unsigned char* dst, size_t cap, size_t* length);

// ---- the device inflate (imp_png_inflate.hip): one descriptor per zlib stream, one workgroup of one wavefront each
struct PngInflateDesc {
    const uint8_t* in;                   // the compressed bytes: 16-byte aligned, in_cap (a multiple of 4) bytes readable, zero behind in_size
    uint32_t in_size, in_cap;
    uint8_t* out;                        // the scanline region: out_size bytes are inflated, `slack` more are cleared
    uint32_t out_size, slack;
    const uint32_t* pal;                 // a palette file: 256 words to copy to pal_dst (the end of its region); else null
    uint32_t* pal_dst;
    int nitems;                          // the stream's row layout: per item its rows and rowbytes + 1
    uint32_t rows[7], stride[7];
    uint32_t* status;                    // the stream's status word (imp_inflate_lanes.h: INF_*)
};

// ---- the kinds the _ex calls take besides (impgpu_*_png_ex: palette, 1/2/4-bit gray, Adam7)
// An ITEM is a run of filtered rows that the unfilter kernels take as one job: the whole file when it is not interlaced, one
// non-empty Adam7 pass otherwise (PNG specification 8.2: an empty pass has no rows at all, not even filter bytes).
struct PngItem {
    int w = 0, h = 0;                    // pixels of the pass (of the file)
    int pass = 0;                        // Adam7 pass 0..6 (0 when not interlaced)
    size_t rowbytes = 0;                 // ceil(w * bits per pixel / 8), the filter byte not counted
    size_t off = 0;                      // where its first filter byte lies in the inflated stream
};
struct PngLayout {
    bool plain = false;                  // one of k_png_unfilter's own kinds, not interlaced: decoded as before
    int channels = 0;                    // of the answer: 1 (gray), 3 (palette, RGB -> BGR), 4 (RGBA -> BGRA)
    int spp = 0;                         // samples per pixel in the file: 1 (gray, palette), 3, 4
    int depth = 8;
    int fu = 1;                          // the filter unit, max(1, bits per pixel / 8): 1, 3 or 4 bytes
    bool palette = false;
    int n = 0;                           // items
    PngItem item[7];
    size_t raw = 0;                      // bytes of the inflated stream: sum of h * (rowbytes + 1)
    uint32_t pal[256];                   // palette files: B | G << 8 | R << 16, zero past the PLTE entries
};
// The verdict of the _ex calls on a file whose header png_header read: IMP_OK with L filled (L.plain for today's kinds),
// IMP_ERROR_UNSUPPORTED for a kind outside `accept` (or outside every mask), IMP_ERROR_DECODE_FAILED for a palette file with a
// damaged chunk layout or a bad PLTE.  accept == 0 gives exactly the verdicts of impgpu_png_info.
int png_layout(const unsigned char* blob, size_t size, const PngHeader& H, int accept, PngLayout* L);
// png_scanlines for a layout: the items' filtered rows, back to back, into dst[L.raw]; every filter byte checked
int png_scanlines_items(const unsigned char* blob, size_t size, const PngLayout& L, unsigned char* dst);

}  // namespace imp
