// imp_png.cpp -- the host side of the PNG front: the file format (PNG specification, 2nd edition, section 5: signature,
// chunk layout, CRC; 11.2.2 IHDR; 10.1 the zlib stream across IDAT chunks; 9.2 filter types).  Host code only -- no HIP
// call -- so that tests/c/fuzz_host.cpp can run it under AddressSanitizer / UBSan on damaged files
// (tests/test_host_sanitizers.py); impgpu_image_decode_png (imp_png.hip) calls png_scanlines with the pinned staging buffer
// as its destination.  The inflate is imp_inflate.cpp's (1.6-1.9 x zlib 1.2.11 on scanlines).  The opt-in device inflate
// (IMPGPU_PNG_DEVICE_INFLATE, imp_png_inflate.hip) shares the chunk walk (png_gather_idat); its lanes' logic runs here on
// the host as a diagnostic (impgpu_png_inflate_lanes).
#include <zlib.h>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../include/impgpu.h"
#include "imp_inflate.h"
#include "imp_inflate_lanes.h"
#include "imp_png.h"

namespace imp {

static unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }

int png_header(const unsigned char* blob, size_t size, PngHeader* H) {
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    if (!blob || size < 8 || std::memcmp(blob, sig, 8) != 0) return IMP_ERROR_UNSUPPORTED;
    if (size < 8 + 25 || be32(blob + 8) != 13 || std::memcmp(blob + 12, "IHDR", 4) != 0) return IMP_ERROR_DECODE_FAILED;
    if (crc32_ieee(blob + 12, 17) != be32(blob + 29)) return IMP_ERROR_DECODE_FAILED;
    const unsigned w = be32(blob + 16), h = be32(blob + 20);
    const int depth = blob[24], colour = blob[25], compression = blob[26], filter = blob[27], interlace = blob[28];
    if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu || compression != 0 || filter != 0 || interlace > 1)
        return IMP_ERROR_DECODE_FAILED;
    H->w = (int)w; H->h = (int)h;
    H->depth = depth; H->colour = colour; H->interlace = interlace;
    H->bpp = colour == 0 ? 1 : colour == 2 ? 3 : colour == 6 ? 4 : 0;
    H->taken = depth == 8 && H->bpp != 0 && interlace == 0 && w <= (unsigned)PNG_MAX_W && h <= (unsigned)PNG_MAX_H;
    return IMP_OK;
}

namespace {
struct RowWatch {
    const PngHeader* H;
    unsigned char* dst;
    size_t rstride;
    int checked = 0;                     // rows whose filter byte has been looked at
    png_rows_fn rows;
    void* ctx;
    int code = IMP_OK;
};

// 9.2: filter types 0..4; rows are final once the inflate has passed their last byte
bool watch_rows(void* p, size_t produced) {
    RowWatch* W = (RowWatch*)p;
    const int complete = (int)(produced / W->rstride);
    for (; W->checked < complete; W->checked++)
        if (W->dst[(size_t)W->checked * W->rstride] > 4) { W->code = IMP_ERROR_DECODE_FAILED; return false; }
    if (W->rows && complete > 0) {
        W->code = W->rows(W->ctx, complete);
        if (W->code) return false;
    }
    return true;
}
}  // namespace

// The chunk walk behind the header: every CRC, the chunk rules, the IDAT payloads appended to `vec` or, when that is null,
// written to dst[0, cap)
static int png_walk(const unsigned char* blob, size_t size, std::vector<unsigned char>* vec, unsigned char* dst, size_t cap, size_t* length) {
    bool bad = false, seen_idat = false, seen_iend = false;
    size_t n = 0;
    for (size_t at = 8 + 25; !bad && !seen_iend;) {
        if (size - at < 12) { bad = true; break; }
        const unsigned len = be32(blob + at);
        const unsigned char* kind = blob + at + 4;
        if (len > 0x7fffffffu || size - at - 12 < len) { bad = true; break; }
        const bool critical = !(kind[0] & 0x20);
        // (libpng's default only warns about a damaged ANCILLARY chunk and skips it; such a file is left to the host decoder)
        if (crc32_ieee(kind, 4 + (size_t)len) != be32(blob + at + 8 + len)) { bad = true; break; }
        if (!std::memcmp(kind, "IDAT", 4)) {
            seen_idat = true;
            if (vec) vec->insert(vec->end(), blob + at + 8, blob + at + 8 + len);
            else if (cap - n < len) { bad = true; break; }
            else std::memcpy(dst + n, blob + at + 8, len);
            n += len;
        } else if (!std::memcmp(kind, "IEND", 4)) {
            seen_iend = true;
        } else if (critical && std::memcmp(kind, "PLTE", 4) != 0) {
            bad = true;                                                      // an unknown critical chunk (5.4)
        }
        at += 12 + (size_t)len;
    }
    if (bad || !seen_idat) return IMP_ERROR_DECODE_FAILED;
    if (length) *length = n;
    return IMP_OK;
}

int png_gather_idat(const unsigned char* blob, size_t size, unsigned char* dst, size_t cap, size_t* length) {
    if (size < 8 + 25) return IMP_ERROR_DECODE_FAILED;
    return png_walk(blob, size, nullptr, dst, cap, length);
}

// The IDAT payloads gathered and inflated into exactly raw_bytes of dst; watch(ctx, produced) as rows become final (see
// RowWatch), its false return ending the inflate with *code (or IMP_ERROR_DECODE_FAILED)
static int png_inflate(const unsigned char* blob, size_t size, unsigned char* dst, size_t raw_bytes, bool (*watch)(void*, size_t),
                       void* ctx, const int* code) {
    // the IDAT payloads are ONE zlib stream (10.1): gathered (a copy of the compressed bytes: 0.3 ms per 3 MB) so that the
    // inflate can run over one piece of memory
    static thread_local std::vector<unsigned char> stream;
    stream.clear();
    if (png_walk(blob, size, &stream, nullptr, 0, nullptr)) return IMP_ERROR_DECODE_FAILED;
    // exactly the image's bytes: a stream that ends early fails, whatever follows the last scanline is not read (libpng's rule)
    // IMPGPU_PNG_INFLATE=zlib (read per call): the audited library instead of this repository's one-shot inflate -- an operator's
    // choice for a worker that decompresses untrusted input; 1.3-1.6 x slower (profiles/r04_png_probe_zlib.json), same bytes
    const char* which = std::getenv("IMPGPU_PNG_INFLATE");
    int rc = IMP_OK;
    if (which && !std::strcmp(which, "zlib")) {
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (inflateInit(&z) != Z_OK) return IMP_ERROR_MALLOC_FAILED;
        size_t in_at = 0, produced = 0;
        bool ended = false;
        while (produced < raw_bytes && !ended && rc == IMP_OK) {
            // in pieces (the counters are 32-bit; and the rows behind a piece go to the device while the next is inflated)
            const size_t in_piece = stream.size() - in_at < (size_t(1) << 30) ? stream.size() - in_at : (size_t(1) << 30);
            const size_t out_piece = raw_bytes - produced < (size_t(1) << 20) ? raw_bytes - produced : (size_t(1) << 20);
            z.next_in = stream.data() + in_at; z.avail_in = (uInt)in_piece;
            z.next_out = dst + produced; z.avail_out = (uInt)out_piece;
            const int zr = inflate(&z, Z_NO_FLUSH);
            in_at += in_piece - z.avail_in;
            const size_t got = out_piece - z.avail_out;
            produced += got;
            if (zr == Z_STREAM_END) ended = true;
            else if (zr != Z_OK || (got == 0 && in_piece - z.avail_in == 0)) rc = IMP_ERROR_DECODE_FAILED;    // damaged, or no progress: the input ran out
            if (rc == IMP_OK && !watch(ctx, produced)) rc = *code ? *code : IMP_ERROR_DECODE_FAILED;
        }
        inflateEnd(&z);
        if (rc == IMP_OK && produced < raw_bytes) rc = IMP_ERROR_DECODE_FAILED;
    } else {
        if (inflate_exact(stream.data(), stream.size(), dst, raw_bytes, watch, ctx)) rc = *code ? *code : IMP_ERROR_DECODE_FAILED;
        else if (!watch(ctx, raw_bytes)) rc = *code;                 // the rows of the last block
    }
    // (the gather buffer is per thread and for life: one large file must not leave every worker thread holding its size)
    if (stream.capacity() > (size_t(4) << 20)) std::vector<unsigned char>().swap(stream);
    return rc;
}

int png_scanlines(const unsigned char* blob, size_t size, const PngHeader& H, unsigned char* dst, png_rows_fn rows, void* ctx) {
    const size_t rstride = (size_t)H.w * H.bpp + 1, raw_bytes = rstride * H.h;
    RowWatch W{&H, dst, rstride, 0, rows, ctx, IMP_OK};
    return png_inflate(blob, size, dst, raw_bytes, watch_rows, &W, &W.code);
}

// ---- palette, 1/2/4-bit gray, Adam7 (the _ex calls)
namespace {
// Adam7 (8.2): pass p holds the pixels x = X0[p] + k * XS[p], y = Y0[p] + j * YS[p]
constexpr int A7_X0[7] = {0, 4, 0, 2, 0, 1, 0}, A7_XS[7] = {8, 8, 4, 4, 2, 2, 1};
constexpr int A7_Y0[7] = {0, 0, 4, 0, 2, 0, 1}, A7_YS[7] = {8, 8, 8, 4, 4, 2, 2};

// the filter byte of every row of every item, as the inflate makes them final
struct ItemWatch {
    const PngLayout* L;
    const unsigned char* dst;
    int item = 0, row = 0;
    int code = IMP_OK;
};
bool watch_items(void* p, size_t produced) {
    ItemWatch* W = (ItemWatch*)p;
    while (W->item < W->L->n) {
        const PngItem& it = W->L->item[W->item];
        const size_t at = it.off + (size_t)W->row * (it.rowbytes + 1);
        if (at >= produced) return true;
        if (W->dst[at] > 4) { W->code = IMP_ERROR_DECODE_FAILED; return false; }
        if (++W->row == it.h) { W->row = 0; W->item++; }
    }
    return true;
}

// A palette file's chunks up to IEND: PLTE (5.6: before the first IDAT, once, 1..256 entries of 3 bytes, its CRC right) and
// whether a tRNS chunk is present.  The CRCs of the other chunks are png_inflate's to check.
int png_palette(const unsigned char* blob, size_t size, int depth, uint32_t pal[256]) {
    bool seen_idat = false, trns = false;
    int plte = 0;                                                    // PLTE chunks before the first IDAT
    size_t plte_at = 0, plte_len = 0;
    for (size_t at = 8 + 25;;) {
        if (size - at < 12) return IMP_ERROR_DECODE_FAILED;
        const unsigned len = be32(blob + at);
        const unsigned char* kind = blob + at + 4;
        if (len > 0x7fffffffu || size - at - 12 < len) return IMP_ERROR_DECODE_FAILED;
        if (!std::memcmp(kind, "IDAT", 4)) seen_idat = true;
        else if (!std::memcmp(kind, "IEND", 4)) break;
        else if (!std::memcmp(kind, "tRNS", 4)) trns = true;
        else if (!std::memcmp(kind, "PLTE", 4)) {
            if (seen_idat) return IMP_ERROR_DECODE_FAILED;          // libpng: "Invalid PLTE after IDAT"
            plte++; plte_at = at; plte_len = len;
        }
        at += 12 + (size_t)len;
    }
    // (OpenCV 2.4.9's channel count for a palette file with transparency cannot be pinned here: left to the host decoder)
    if (trns) return IMP_ERROR_UNSUPPORTED;
    if (plte != 1 || plte_len == 0 || plte_len > 768 || plte_len % 3) return IMP_ERROR_DECODE_FAILED;
    if (crc32_ieee(blob + plte_at + 4, 4 + plte_len) != be32(blob + plte_at + 8 + plte_len)) return IMP_ERROR_DECODE_FAILED;
    const int entries = (int)(plte_len / 3);
    if (entries > (1 << depth)) return IMP_ERROR_UNSUPPORTED;        // libpng's answer is a benign error: not pinned here
    // libpng 1.6's png_set_PLTE keeps a zero-filled palette of 256 entries, and the check of the indices against the PLTE's
    // length at png_read_end is only a benign warning on read: an index past the last entry reads (0, 0, 0).  This rests on
    // reading libpng's source; no decoder at hand pins it.
    const unsigned char* e = blob + plte_at + 8;
    for (int i = 0; i < 256; i++)
        pal[i] = i < entries ? (uint32_t)e[3 * i + 2] | (uint32_t)e[3 * i + 1] << 8 | (uint32_t)e[3 * i] << 16 : 0u;
    return IMP_OK;
}
}  // namespace

int png_layout(const unsigned char* blob, size_t size, const PngHeader& H, int accept, PngLayout* L) {
    L->plain = false;
    L->palette = false;
    L->n = 0;
    L->depth = H.depth;
    const int d = H.depth, ct = H.colour;
    if (H.taken || !accept) {
        if (!H.taken) return IMP_ERROR_UNSUPPORTED;
        // (L->pal is not read for such a file)
        L->plain = true;
        L->channels = L->spp = L->fu = H.bpp;
        L->n = 1;
        L->item[0] = PngItem{H.w, H.h, 0, (size_t)H.w * H.bpp, 0};
        L->raw = ((size_t)H.w * H.bpp + 1) * H.h;
        return IMP_OK;
    }
    int need = 0;
    if (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) { need = IMPGPU_PNG_PALETTE; L->spp = 1; L->channels = 3; L->palette = true; }
    else if (ct == 0 && (d == 1 || d == 2 || d == 4)) { need = IMPGPU_PNG_LOW_GRAY; L->spp = 1; L->channels = 1; }
    else if (d == 8 && (ct == 0 || ct == 2 || ct == 6)) { L->spp = L->channels = H.bpp; }        // interlaced: ADAM7 alone
    else return IMP_ERROR_UNSUPPORTED;
    if (H.interlace) need |= IMPGPU_PNG_ADAM7;
    if ((need & accept) != need || H.w > PNG_MAX_W || H.h > PNG_MAX_H) return IMP_ERROR_UNSUPPORTED;
    const int bits = L->spp * d;
    L->fu = bits >= 8 ? bits / 8 : 1;
    size_t off = 0;
    for (int p = 0; p < (H.interlace ? 7 : 1); p++) {
        const int x0 = H.interlace ? A7_X0[p] : 0, xs = H.interlace ? A7_XS[p] : 1;
        const int y0 = H.interlace ? A7_Y0[p] : 0, ys = H.interlace ? A7_YS[p] : 1;
        const int w = H.w > x0 ? (H.w - x0 + xs - 1) / xs : 0, h = H.h > y0 ? (H.h - y0 + ys - 1) / ys : 0;
        if (!w || !h) continue;
        PngItem& it = L->item[L->n++];
        it = PngItem{w, h, p, ((size_t)w * bits + 7) / 8, off};
        off += (it.rowbytes + 1) * (size_t)h;
    }
    L->raw = off;
    return L->palette ? png_palette(blob, size, d, L->pal) : IMP_OK;
}

int png_scanlines_items(const unsigned char* blob, size_t size, const PngLayout& L, unsigned char* dst) {
    ItemWatch W{&L, dst};
    return png_inflate(blob, size, dst, L.raw, watch_items, &W, &W.code);
}

}  // namespace imp

using namespace imp;

extern "C" {

int impgpu_png_info(const unsigned char* blob, size_t size, int* width, int* height, int* channels) {
    PngHeader H;
    const int rc = png_header(blob, size, &H);
    if (rc) return rc;
    if (!H.taken) return IMP_ERROR_UNSUPPORTED;
    if (width) *width = H.w;
    if (height) *height = H.h;
    if (channels) *channels = H.bpp;
    return IMP_OK;
}

int impgpu_png_scanlines(const unsigned char* blob, size_t size, unsigned char* out, size_t capacity, size_t* length) {
    PngHeader H;
    int rc = png_header(blob, size, &H);
    if (rc) return rc;
    if (!H.taken) return IMP_ERROR_UNSUPPORTED;
    const size_t raw_bytes = ((size_t)H.w * H.bpp + 1) * H.h;
    if (length) *length = raw_bytes;
    if (raw_bytes / 1032 > size) return IMP_ERROR_DECODE_FAILED;             // (zlib's best ratio: the file cannot hold that much)
    if (!out || capacity < raw_bytes) return IMP_ERROR_MALLOC_FAILED;
    return png_scanlines(blob, size, H, out);
}

int impgpu_png_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels) {
    accept &= ~IMPGPU_PNG_DEVICE_INFLATE;                            // (how a file is decoded, not which: nothing to do with its header)
    if (!accept) return impgpu_png_info(blob, size, width, height, channels);
    PngHeader H;
    int rc = png_header(blob, size, &H);
    if (rc) return rc;
    static thread_local PngLayout L;
    if ((rc = png_layout(blob, size, H, accept, &L))) return rc;
    if (width) *width = H.w;
    if (height) *height = H.h;
    if (channels) *channels = L.channels;
    return IMP_OK;
}

int impgpu_png_scanlines_ex(const unsigned char* blob, size_t size, int accept, unsigned char* out, size_t capacity, size_t* length) {
    accept &= ~IMPGPU_PNG_DEVICE_INFLATE;
    if (!accept) return impgpu_png_scanlines(blob, size, out, capacity, length);
    PngHeader H;
    int rc = png_header(blob, size, &H);
    if (rc) return rc;
    static thread_local PngLayout L;
    if ((rc = png_layout(blob, size, H, accept, &L))) return rc;
    if (length) *length = L.raw;
    if (L.raw / 1032 > size) return IMP_ERROR_DECODE_FAILED;
    if (!out || capacity < L.raw) return IMP_ERROR_MALLOC_FAILED;
    return png_scanlines_items(blob, size, L, out);
}

int impgpu_png_inflate_lanes(const unsigned char* in, size_t in_size, unsigned char* out, size_t out_size, int* status) {
    if (status) *status = INF_DAMAGED;
    if ((!in && in_size) || (!out && out_size) || in_size >= INF_MAX_IN || out_size >= INF_MAX_OUT) return IMP_ERROR_INVALID_ARGS;
    // the stream as the device holds it: word aligned, zero behind its last byte
    const uint32_t cap = (uint32_t)((in_size + 3) & ~(size_t)3);
    std::vector<uint32_t> staged(cap / 4 + 1, 0u);
    if (in_size) std::memcpy(staged.data(), in, in_size);
    std::vector<InfMem> mem(1);
    const int st = inf_lanes_host((const uint8_t*)staged.data(), cap, (uint32_t)in_size, out, (uint32_t)out_size, mem.data());
    if (status) *status = st;
    return st == INF_OK ? IMP_OK : IMP_ERROR_DECODE_FAILED;
}

}  // extern "C"
