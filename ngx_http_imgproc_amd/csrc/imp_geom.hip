// imp_geom.hip -- exact byte movers: the copy behind Crop (cvSetImageROI + cvCopy,
// bridge.c:130-135), cvFlip (filters.c:93-99, :126), cvTranspose + cvFlip as one rotation
// (filters.c:116-119) and cvCvtColor(GRAY2BGR) (bridge.c:613-618).  Bit-exact by nature.
//
// Rotation by 90 / 270 of BGRA goes through a 32x32-pixel LDS tile (33-dword row pitch, so
// the transposed read is bank-conflict free): global reads run along source rows, global
// writes along destination rows, both coalesced, in one pass instead of the reference's
// transpose + flip pair.
#include "imp_internal.h"

namespace imp {

struct GArgs {
    const uint8_t* src; long long src_stride; int sstep, sw, sh;
    uint8_t* dst; long long dst_stride; int dstep, dw, dh;
};

// ---- copy: a dword per thread when everything is dword aligned (k_copy<4>); 16-byte runs of each row when only the
// destination is (k_copy_run); a byte per thread otherwise (k_copy<1>) ----
template <int UNIT>
__global__ __launch_bounds__(256) void k_copy(GArgs a, int row_units) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)row_units * a.dh) return;
    const int y = (int)(idx / row_units), u = (int)(idx - (long long)y * row_units);
    const uint8_t* s = a.src + (long long)blockIdx.y * a.src_stride + (size_t)y * a.sstep + (size_t)u * UNIT;
    uint8_t* d = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)y * a.dstep + (size_t)u * UNIT;
    if (UNIT == 4) *(uint32_t*)d = *(const uint32_t*)s;
    else *d = *s;
}

// Windows that start or end off the dword grid (a BGR crop at x = 1, 2, 3 mod 4; a row of w * c bytes that is no multiple of
// 4): a lane moves 16 destination bytes of one row through copy_run16 instead of one byte.
__global__ __launch_bounds__(256) void k_copy_run(GArgs a, int rowbytes, int chunks) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)chunks * a.dh) return;
    const int y = (int)(idx / chunks), k = (int)(idx - (long long)y * chunks);
    copy_run16(a.src + (long long)blockIdx.y * a.src_stride + (size_t)y * a.sstep,
               a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)y * a.dstep, rowbytes, k);
}

// ---- cvFlip: mode 0 = vertical (around x axis), > 0 = horizontal, < 0 = both ----
// the source pixel of destination (x, y); shared by k_flip and k_geom_mix
__device__ __forceinline__ void flip_src(int mode, int sw, int sh, int x, int y, int* sx, int* sy) {
    *sy = mode <= 0 ? sh - 1 - y : y;
    *sx = mode != 0 ? sw - 1 - x : x;
}
// rotate 90 (clockwise): R[i][j] = S[H-1-j][i];  270: R[i][j] = S[j][W-1-i]  (filters.c:116-119); shared by k_rotate_* and k_geom_mix
__device__ __forceinline__ void turn_src(int amount, int sw, int sh, int i, int j, int* srow, int* scol) {
    *srow = amount == 90 ? sh - 1 - j : j;
    *scol = amount == 90 ? i : sw - 1 - i;
}

template <int CN>
__global__ __launch_bounds__(256) void k_flip(GArgs a, int mode) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.dw * a.dh) return;
    const int y = (int)(idx / a.dw), x = (int)(idx - (long long)y * a.dw);
    int sx, sy;
    flip_src(mode, a.sw, a.sh, x, y, &sx, &sy);
    const uint8_t* s = a.src + (long long)blockIdx.y * a.src_stride + (size_t)sy * a.sstep + (size_t)sx * CN;
    uint8_t* d = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)y * a.dstep + (size_t)x * CN;
    if (CN == 4) *(uint32_t*)d = *(const uint32_t*)s;
    else {
#pragma unroll
        for (int c = 0; c < CN; c++) d[c] = s[c];
    }
}

// ---- rotate 90 / 270 (turn_src) ----
__global__ __launch_bounds__(256) void k_rotate_bgra(GArgs a, int amount) {
    __shared__ uint32_t tile[32][33];
    const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 32;   // destination tile origin (x along dw = sh)
    const uint8_t* S = a.src + (long long)blockIdx.z * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride;
    const int li = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int lj = threadIdx.y + 8 * r;
        const int j = tx0 + lj, i = ty0 + li;                  // destination (x = j, y = i)
        if (j < a.dw && i < a.dh) {
            int srow, scol;
            turn_src(amount, a.sw, a.sh, i, j, &srow, &scol);
            tile[lj][li] = *(const uint32_t*)(S + (size_t)srow * a.sstep + (size_t)scol * 4);
        }
    }
    __syncthreads();
    const int lj = threadIdx.x;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int l = threadIdx.y + 8 * r;
        const int j = tx0 + lj, i = ty0 + l;
        if (j < a.dw && i < a.dh) *(uint32_t*)(D + (size_t)i * a.dstep + (size_t)j * 4) = tile[lj][l];
    }
}

// The same for 3-channel frames (every JPEG): a 32 x 32 pixel tile is 32 source row segments of 96 bytes.  Full,
// dword-aligned tiles move as dwords on both sides (24 per row segment) and the quarter turn happens in the byte
// gather out of LDS; border tiles and odd alignments take bytes on the global side.  LDS row pitch 100 bytes.
__global__ __launch_bounds__(256) void k_rotate_bgr(GArgs a, int amount) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[32][100];
    const int tx0 = blockIdx.x * 32, ty0 = blockIdx.y * 32;   // destination tile origin (x along dw = sh, y along dh = sw)
    const uint8_t* S = a.src + (long long)blockIdx.z * a.src_stride;
    uint8_t* D = a.dst + (long long)blockIdx.z * a.dst_stride;
    const int tid = threadIdx.y * 32 + threadIdx.x;
    const bool full = tx0 + 32 <= a.dw && ty0 + 32 <= a.dh;
    // source tile: rows srow0 .. srow0+31, columns scol0 .. scol0+31 (tile[r][3*c + ch])
    const int srow0 = amount == 90 ? a.sh - 32 - tx0 : tx0;
    const int scol0 = amount == 90 ? ty0 : a.sw - 32 - ty0;
    const bool vec = full && !(((uintptr_t)S | (uintptr_t)D | (uintptr_t)a.sstep | (uintptr_t)a.dstep | (uintptr_t)(scol0 * 3)) & 3);
    if (vec) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int e = tid + 256 * q;                       // 768 dwords: 32 rows x 24
            const int r = e / 24, d = e - r * 24;
            *(uint32_t*)&tile[r][4 * d] = *(const uint32_t*)(S + (size_t)(srow0 + r) * a.sstep + (size_t)scol0 * 3 + 4 * d);
        }
    } else {
        for (int e = tid; e < 32 * 32; e += 256) {
            const int r = e >> 5, c = e & 31;
            const int sr = srow0 + r, sc = scol0 + c;
            if (sr >= 0 && sr < a.sh && sc >= 0 && sc < a.sw) {
                const uint8_t* p = S + (size_t)sr * a.sstep + (size_t)sc * 3;
                tile[r][3 * c] = p[0]; tile[r][3 * c + 1] = p[1]; tile[r][3 * c + 2] = p[2];
            }
        }
    }
    __syncthreads();
    // destination pixel (row ty0 + li, column tx0 + lj) = tile[31 - lj][li] (90)  or  tile[lj][31 - li] (270)
    if (vec) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int e = tid + 256 * q;
            const int li = e / 24, d = e - li * 24;
            uint32_t o = 0;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                const int byte = 4 * d + b, lj = byte / 3, ch = byte - 3 * lj;
                const uint8_t v = amount == 90 ? tile[31 - lj][3 * li + ch] : tile[lj][3 * (31 - li) + ch];
                o |= (uint32_t)v << (8 * b);
            }
            *(uint32_t*)(D + (size_t)(ty0 + li) * a.dstep + (size_t)tx0 * 3 + 4 * d) = o;
        }
    } else {
        for (int e = tid; e < 32 * 32; e += 256) {
            const int li = e >> 5, lj = e & 31;
            if (ty0 + li < a.dh && tx0 + lj < a.dw) {
                const uint8_t* t = amount == 90 ? &tile[31 - lj][3 * li] : &tile[lj][3 * (31 - li)];
                uint8_t* p = D + (size_t)(ty0 + li) * a.dstep + (size_t)(tx0 + lj) * 3;
                p[0] = t[0]; p[1] = t[1]; p[2] = t[2];
            }
        }
    }
}

template <int CN>
__global__ __launch_bounds__(256) void k_rotate_any(GArgs a, int amount) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.dw * a.dh) return;
    const int i = (int)(idx / a.dw), j = (int)(idx - (long long)i * a.dw);
    int srow, scol;
    turn_src(amount, a.sw, a.sh, i, j, &srow, &scol);
    const uint8_t* s = a.src + (long long)blockIdx.y * a.src_stride + (size_t)srow * a.sstep + (size_t)scol * CN;
    uint8_t* d = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)i * a.dstep + (size_t)j * CN;
#pragma unroll
    for (int c = 0; c < CN; c++) d[c] = s[c];
}

__global__ __launch_bounds__(256) void k_gray2bgr(GArgs a) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)a.dw * a.dh) return;
    const int y = (int)(idx / a.dw), x = (int)(idx - (long long)y * a.dw);
    const uint8_t v = a.src[(long long)blockIdx.y * a.src_stride + (size_t)y * a.sstep + x];
    uint8_t* d = a.dst + (long long)blockIdx.y * a.dst_stride + (size_t)y * a.dstep + (size_t)x * 3;
    d[0] = v; d[1] = v; d[2] = v;
}

// IplToFI32 / IplToFI24 (advancedio.c:65-101): vertical flip + channel repack into FreeImage's row pitch.  The pixel `idx`
// (row-major in the bitmap) of a w x h frame: shared by k_pack_fi (one frame) and k_pack_fi_mix (many).
template <int SC, int DC>
__device__ __forceinline__ void pack_fi_pixel(const uint8_t* __restrict__ src, int sstep, int w, int h, uint8_t* __restrict__ dst,
                                              int dpitch, long long idx) {
    if (idx >= (long long)w * h) return;
    const int y = (int)(idx / w), x = (int)(idx - (long long)y * w);
    const uint8_t* s = src + (size_t)(h - 1 - y) * sstep + (size_t)x * SC;
    uint8_t* d = dst + (size_t)y * dpitch + (size_t)x * DC;
    if (SC == 4 && DC == 4) { *(uint32_t*)d = *(const uint32_t*)s; return; }
    d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    if (DC == 4) d[3] = SC == 4 ? s[3] : 255;
}

template <int SC, int DC>
__global__ __launch_bounds__(256) void k_pack_fi(const uint8_t* __restrict__ src, int sstep, int w, int h, uint8_t* __restrict__ dst, int dpitch) {
    pack_fi_pixel<SC, DC>(src, sstep, w, h, dst, dpitch, (long long)blockIdx.x * 256 + threadIdx.x);
}

int launch_pack_fi(const View& v, int bpp, uint8_t* dst, int dpitch, hipStream_t s) {
    if (v.c < 3 || (bpp != 24 && bpp != 32)) return IMP_ERROR_INVALID_ARGS;
    const dim3 grid((unsigned)(((long long)v.w * v.h + 255) / 256)), block(256);
    if (v.c == 4 && bpp == 32) {
        if (((uintptr_t)v.d | (uintptr_t)v.step | (uintptr_t)dst | (uintptr_t)dpitch) & 3) return IMP_ERROR_INVALID_ARGS;
        hipLaunchKernelGGL((k_pack_fi<4, 4>), grid, block, 0, s, v.d, v.step, v.w, v.h, dst, dpitch);
    } else if (v.c == 4) hipLaunchKernelGGL((k_pack_fi<4, 3>), grid, block, 0, s, v.d, v.step, v.w, v.h, dst, dpitch);
    else if (bpp == 32) hipLaunchKernelGGL((k_pack_fi<3, 4>), grid, block, 0, s, v.d, v.step, v.w, v.h, dst, dpitch);
    else hipLaunchKernelGGL((k_pack_fi<3, 3>), grid, block, 0, s, v.d, v.step, v.w, v.h, dst, dpitch);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

// ---- many frames, one launch (impgpu_batch_download_fi) ----
// A descriptor per frame, dealt like k_geom_mix's; a workgroup covers 256 bitmap pixels of ONE frame, a lane one pixel
// through pack_fi_pixel -- a dword in and out for BGRA -> 32 bits, bytes otherwise, exactly k_pack_fi's accesses.
struct PackFiDesc {
    const uint8_t* src; uint8_t* dst;
    int w, h, sstep, dpitch;
    int first, nblk;
};

template <int SC, int DC>
__global__ __launch_bounds__(256) void k_pack_fi_mix(const PackFiDesc* __restrict__ d, MixIndex ix) {
    int blk;
    const int i = mix_pick(d, ix, &blk);
    if (i < 0) return;
    pack_fi_pixel<SC, DC>(d[i].src, d[i].sstep, d[i].w, d[i].h, d[i].dst, d[i].dpitch, (long long)blk * 256 + threadIdx.x);
}

int launch_pack_fi_mixed(const PackFiItem* items, int count, int channels, int bpp, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    if (!items || (channels != 3 && channels != 4) || (bpp != 24 && bpp != 32)) return IMP_ERROR_INVALID_ARGS;
    std::vector<PackFiDesc> v;
    v.reserve((size_t)count);
    long long blocks = 0;
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every item is well-formed
        const PackFiItem& it = items[i];
        if (!it.src || !it.dst || !view_fits(it.w, it.h, channels, it.sstep) || !view_fits(it.w, it.h, bpp / 8, it.dpitch)) return IMP_ERROR_INVALID_ARGS;
        if (channels == 4 && bpp == 32 && (((uintptr_t)it.src | (uintptr_t)it.sstep | (uintptr_t)it.dst | (uintptr_t)it.dpitch) & 3)) return IMP_ERROR_INVALID_ARGS;
        PackFiDesc d{};
        d.src = it.src; d.dst = it.dst; d.w = it.w; d.h = it.h; d.sstep = it.sstep; d.dpitch = it.dpitch;
        d.nblk = (int)(((long long)it.w * it.h + 255) / 256);
        blocks += d.nblk;
        v.push_back(d);
    }
    if (blocks * 8 > 0x7fffffffLL) return IMP_ERROR_INVALID_ARGS;     // (the grid is 8 x the longest list: the caller splits first)
    return mix_launch(v, [](PackFiDesc& d) { return (long long)d.w * d.h; }, s, [&](dim3 grid, const PackFiDesc* dev, const MixIndex& ix) {
        if (channels == 4 && bpp == 32) hipLaunchKernelGGL((k_pack_fi_mix<4, 4>), grid, dim3(256), 0, s, dev, ix);
        else if (channels == 4) hipLaunchKernelGGL((k_pack_fi_mix<4, 3>), grid, dim3(256), 0, s, dev, ix);
        else if (bpp == 32) hipLaunchKernelGGL((k_pack_fi_mix<3, 4>), grid, dim3(256), 0, s, dev, ix);
        else hipLaunchKernelGGL((k_pack_fi_mix<3, 3>), grid, dim3(256), 0, s, dev, ix);
    });
}

// LoadGIF's compositing loop (advancedio.c:204-247) for the canvas pixel (x, y), walking the pages in order: the `master`
// index canvas of the destructive mode is that pixel's register.  Same definitions as the oracle where the reference is
// undefined (read one byte past the frame row at x == left + w; index < 0 -> colour 0).  Shared by k_gif_compose (one file)
// and k_gif_compose_mix (many): `blob` is what the pages' idx_off / pal_off count from.
__device__ __forceinline__ void gif_walk(const uint8_t* __restrict__ blob, const GifPageDev* __restrict__ pg,
                                         uint8_t* const* __restrict__ outs, int npages, int ostep, int destructive, int only,
                                         int x, int y) {
    int master = 0;
    for (int f = 0; f < npages; f++) {
        const GifPageDev p = pg[f];
        const int rowidx = p.h + p.top - y - 1;
        int coloridx;
        if (rowidx < 0 || x < p.left || y < p.top || x > p.left + p.w || y > p.top + p.h) {
            coloridx = p.key;
        } else {
            const long long o = (long long)rowidx * p.pitch + (x - p.left);
            coloridx = o < (long long)p.pitch * p.h ? (int)blob[p.idx_off + o] : p.key;
        }
        if (destructive) {
            if (p.dispose == 2) {
                if (coloridx == p.key) coloridx = 0;
                else master = coloridx;
            } else {
                if (coloridx == p.key && f > 0) coloridx = master;
                else master = coloridx;
            }
        }
        if (only >= 0 && f != only) continue;
        uint32_t px = 0;
        if (coloridx >= 0 && coloridx < 256) {
            const uint8_t* q = blob + p.pal_off + 4 * coloridx;
            px = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16);
        }
        if (coloridx != p.key) px |= 0xff000000u;
        *(uint32_t*)(outs[only >= 0 ? 0 : f] + (size_t)y * ostep + (size_t)x * 4) = px;
    }
}

// one file: one lane per canvas pixel
__global__ __launch_bounds__(256) void k_gif_compose(const uint8_t* __restrict__ blob, const GifPageDev* __restrict__ pg,
                                                     uint8_t* const* __restrict__ outs, int npages, int cw, int ch,
                                                     int ostep, int destructive, int only) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)cw * ch) return;
    const int y = (int)(idx / cw), x = (int)(idx - (long long)y * cw);
    gif_walk(blob, pg, outs, npages, ostep, destructive, only, x, y);
}

int launch_gif_compose(const uint8_t* blob, const GifPageDev* pages, uint8_t* const* outs, int npages, int cw, int ch,
                       int ostep, int destructive, int only, hipStream_t s) {
    const dim3 grid((unsigned)(((long long)cw * ch + 255) / 256)), block(256);
    hipLaunchKernelGGL(k_gif_compose, grid, block, 0, s, blob, pages, outs, npages, cw, ch, ostep, destructive, only);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

// ---- many files, one launch (impgpu_batch_gif_compose) ----
// A descriptor per album, dealt like k_geom_mix's; a workgroup covers 256 canvas pixels of ONE album and runs gif_walk for
// each.  Everything the walk reads travels behind the descriptor table in the same allocation (mix_launch's `staged`), so
// the table's address is what every offset -- the descriptors' and the pages' -- counts from.
struct GifMixDesc {
    long long pages_off, outs_off;       // GifPageDev[npages], uint8_t*[frames written]
    int npages, cw, ch, ostep, destructive, only;
    int first, nblk;
};

__global__ __launch_bounds__(256) void k_gif_compose_mix(const GifMixDesc* __restrict__ d, MixIndex ix) {
    int blk;
    const int i = mix_pick(d, ix, &blk);
    if (i < 0) return;
    const int cw = d[i].cw;
    const long long idx = (long long)blk * 256 + threadIdx.x;
    if (idx >= (long long)cw * d[i].ch) return;
    const int y = (int)(idx / cw), x = (int)(idx - (long long)y * cw);
    const uint8_t* base = (const uint8_t*)d;
    gif_walk(base, (const GifPageDev*)(base + d[i].pages_off), (uint8_t* const*)(base + d[i].outs_off), d[i].npages,
             d[i].ostep, d[i].destructive, d[i].only, x, y);
}

size_t gif_mix_table_bytes(int count) { return mix_blob_offset<GifMixDesc>((size_t)count); }

int launch_gif_compose_mixed(const GifMixItem* items, int count, const MixStaged& staged, size_t bytes, hipStream_t s) {
    // (whatever is refused here: the pieces already sent are fenced and the block goes back)
    auto refuse = [&]() { (void)stage_upload_part(staged.token, 0, staged.dev, 0, true); dev_free(staged.dev); return IMP_ERROR_INVALID_ARGS; };
    if (count <= 0 || !items || bytes < gif_mix_table_bytes(count)) return refuse();
    std::vector<GifMixDesc> v;
    v.reserve((size_t)count);
    long long blocks = 0;
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every item is well-formed
        const GifMixItem& it = items[i];
        const size_t nout = it.only >= 0 ? 1 : (size_t)it.npages;
        if (it.npages <= 0 || it.only >= it.npages || !view_fits(it.cw, it.ch, 4, it.ostep) || (it.ostep & 3) || ((it.pages_off | it.outs_off) & 7) ||
            it.pages_off + (size_t)it.npages * sizeof(GifPageDev) > bytes || it.outs_off + nout * sizeof(uint8_t*) > bytes)
            return refuse();
        GifMixDesc d{};
        d.pages_off = (long long)it.pages_off; d.outs_off = (long long)it.outs_off;
        d.npages = it.npages; d.cw = it.cw; d.ch = it.ch; d.ostep = it.ostep; d.destructive = it.destructive ? 1 : 0; d.only = it.only;
        d.nblk = (int)(((long long)it.cw * it.ch + 255) / 256);
        blocks += d.nblk;
        v.push_back(d);
    }
    if (blocks * 8 > 0x7fffffffLL) return refuse();                    // (the grid is 8 x the longest list: the caller splits first)
    return mix_launch(v, [](GifMixDesc& d) { return (long long)d.cw * d.ch * d.npages; }, s, [&](dim3 grid, const GifMixDesc* dev, const MixIndex& ix) {
        hipLaunchKernelGGL(k_gif_compose_mix, grid, dim3(256), 0, s, dev, ix);
    }, nullptr, nullptr, &staged);
}

static GArgs gargs(const Frames& f) {
    return GArgs{f.src, f.src_stride, f.v.step, f.v.w, f.v.h, f.dst, f.dst_stride, f.dstep, f.dw, f.dh};
}
static bool dword_ok(const Frames& f) {
    return !(((uintptr_t)f.src | (uintptr_t)f.dst | (uintptr_t)f.v.step | (uintptr_t)f.dstep |
              (uintptr_t)f.src_stride | (uintptr_t)f.dst_stride) & 3);
}
static unsigned blocks_for(long long n) { return (unsigned)((n + 255) / 256); }

int launch_copy(const Frames& f, hipStream_t s) {
    if (f.count <= 0) return IMP_OK;
    if (f.dw != f.v.w || f.dh != f.v.h || f.count > 65535) return IMP_ERROR_INVALID_ARGS;
    GArgs a = gargs(f);
    const int rowbytes = f.dw * f.v.c;
    if (dword_ok(f) && rowbytes % 4 == 0) {
        const int units = rowbytes / 4;
        hipLaunchKernelGGL((k_copy<4>), dim3(blocks_for((long long)units * f.dh), f.count), dim3(256), 0, s, a, units);
    } else if (!(((uintptr_t)f.dst | (uintptr_t)f.dstep | (uintptr_t)f.dst_stride) & 3)) {
        // dword-aligned destination rows (every pool frame): the source may start anywhere
        const int chunks = (rowbytes + 15) / 16;
        hipLaunchKernelGGL(k_copy_run, dim3(blocks_for((long long)chunks * f.dh), f.count), dim3(256), 0, s, a, rowbytes, chunks);
    } else {
        // destination rows off the dword grid -- the re-pitching copies into a caller's tight BGR pitch
        // (impgpu_image_download_pinned): a byte per thread, 64 contiguous bytes per wave instruction, as before
        hipLaunchKernelGGL((k_copy<1>), dim3(blocks_for((long long)rowbytes * f.dh), f.count), dim3(256), 0, s, a, rowbytes);
    }
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

int launch_flip(const Frames& f, int mode, hipStream_t s) {
    if (f.count <= 0) return IMP_OK;
    if (f.dw != f.v.w || f.dh != f.v.h || f.count > 65535) return IMP_ERROR_INVALID_ARGS;
    GArgs a = gargs(f);
    const dim3 grid(blocks_for((long long)f.dw * f.dh), f.count), block(256);
    if (f.v.c == 4 && dword_ok(f)) hipLaunchKernelGGL((k_flip<4>), grid, block, 0, s, a, mode);
    else if (f.v.c == 4) return IMP_ERROR_INVALID_ARGS;
    else if (f.v.c == 3) hipLaunchKernelGGL((k_flip<3>), grid, block, 0, s, a, mode);
    else hipLaunchKernelGGL((k_flip<1>), grid, block, 0, s, a, mode);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

int launch_rotate(const Frames& f, int amount, hipStream_t s) {
    if (f.count <= 0) return IMP_OK;
    if (amount == 180) return launch_flip(f, -1, s);
    if ((amount != 90 && amount != 270) || f.dw != f.v.h || f.dh != f.v.w || f.count > 65535) return IMP_ERROR_INVALID_ARGS;
    GArgs a = gargs(f);
    if (f.v.c == 4) {
        if (!dword_ok(f)) return IMP_ERROR_INVALID_ARGS;
        const dim3 grid((f.dw + 31) / 32, (f.dh + 31) / 32, f.count), block(32, 8);
        if (grid.y > 65535) return IMP_ERROR_INVALID_ARGS;
        hipLaunchKernelGGL(k_rotate_bgra, grid, block, 0, s, a, amount);
    } else if (f.v.c == 3 && (f.dh + 31) / 32 <= 65535) {
        const dim3 grid((f.dw + 31) / 32, (f.dh + 31) / 32, f.count), block(32, 8);
        hipLaunchKernelGGL(k_rotate_bgr, grid, block, 0, s, a, amount);
    } else {
        const dim3 grid(blocks_for((long long)f.dw * f.dh), f.count), block(256);
        if (f.v.c == 3) hipLaunchKernelGGL((k_rotate_any<3>), grid, block, 0, s, a, amount);
        else hipLaunchKernelGGL((k_rotate_any<1>), grid, block, 0, s, a, amount);
    }
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

// ---- flips and turns of frames of different geometry (impgpu_batch_run_ops' geometry segments) ----
// A descriptor per frame, dealt like k_resize_area_mix's; a workgroup covers GEOM_PIX destination pixels of one frame,
// each a gather through flip_src / turn_src (a half turn is cvFlip mode -1, as in launch_rotate).
#define GEOM_PIX (256 * 8)
struct GeomDesc {
    const uint8_t* src; int sw, sh, sstep;
    uint8_t* dst; int dw, dh, dstep;
    int kind, mode;              // 0: flip (mode), 1: turn 90 / 270
    int first, nblk;
};

template <int CN>
__global__ __launch_bounds__(256) void k_geom_mix(const GeomDesc* __restrict__ descs, MixIndex ix) {
    int blk;
    const int di = mix_pick(descs, ix, &blk);
    if (di < 0) return;
    const GeomDesc* m = descs + di;
    const int dw = m->dw, kind = m->kind, mode = m->mode;
    const long long npix = (long long)dw * m->dh;
    const long long first = (long long)blk * GEOM_PIX + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < GEOM_PIX / 256; it++) {
        const long long idx = first + (long long)it * 256;
        if (idx >= npix) break;
        const int y = (int)(idx / dw), x = (int)(idx - (long long)y * dw);
        int sx, sy;
        if (kind == 0) flip_src(mode, m->sw, m->sh, x, y, &sx, &sy);
        else turn_src(mode, m->sw, m->sh, y, x, &sy, &sx);
        const uint8_t* s = m->src + (size_t)sy * m->sstep + (size_t)sx * CN;
        uint8_t* d = m->dst + (size_t)y * m->dstep + (size_t)x * CN;
        if (CN == 4) *(uint32_t*)d = *(const uint32_t*)s;
        else {
#pragma unroll
            for (int c = 0; c < CN; c++) d[c] = s[c];
        }
    }
}

int launch_geom_mixed(const GeomItem* items, int count, int cn, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    if (!items || (cn != 3 && cn != 4)) return IMP_ERROR_INVALID_ARGS;
    std::vector<GeomDesc> v;
    v.reserve((size_t)count);
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every item is well-formed
        const GeomItem& it = items[i];
        if (!it.src || !it.dst || !view_fits(it.sw, it.sh, cn, it.sstep) || !view_fits(it.dw, it.dh, cn, it.dstep)) return IMP_ERROR_INVALID_ARGS;
        if (cn == 4 && (((uintptr_t)it.src | (uintptr_t)it.dst | (uintptr_t)it.sstep | (uintptr_t)it.dstep) & 3)) return IMP_ERROR_INVALID_ARGS;
        GeomDesc d{};
        d.src = it.src; d.sw = it.sw; d.sh = it.sh; d.sstep = it.sstep;
        d.dst = it.dst; d.dw = it.dw; d.dh = it.dh; d.dstep = it.dstep;
        if (it.kind == 0 || (it.kind == 1 && it.mode == 180)) {
            if (it.dw != it.sw || it.dh != it.sh) return IMP_ERROR_INVALID_ARGS;
            d.kind = 0;
            d.mode = it.kind == 0 ? it.mode : -1;
        } else if (it.kind == 1 && (it.mode == 90 || it.mode == 270)) {
            if (it.dw != it.sh || it.dh != it.sw) return IMP_ERROR_INVALID_ARGS;
            d.kind = 1;
            d.mode = it.mode;
        } else {
            return IMP_ERROR_INVALID_ARGS;
        }
        d.nblk = (int)(((long long)it.dw * it.dh + GEOM_PIX - 1) / GEOM_PIX);
        v.push_back(d);
    }
    return mix_launch(v, [](GeomDesc& d) { return (long long)d.dw * d.dh; }, s, [&](dim3 grid, const GeomDesc* dev, const MixIndex& ix) {
        if (cn == 4) hipLaunchKernelGGL((k_geom_mix<4>), grid, dim3(256), 0, s, dev, ix);
        else hipLaunchKernelGGL((k_geom_mix<3>), grid, dim3(256), 0, s, dev, ix);
    });
}

// ---- cvCvtColor(GRAY2BGR) of frames of different geometry (the gray requests of impgpu_batch_run_ops) ----
// k_gray2bgr's bytes through a descriptor per frame: a lane takes four adjacent pixels of one row -- one dword in, three
// out when both rows are 4-byte aligned (pool frames are), bytes otherwise and at a row's ragged end.
#define G2B_GROUPS (256 * 4)                               // groups of four pixels a workgroup covers
struct Gray2BgrDesc {
    const uint8_t* src; uint8_t* dst;
    int w, h, sstep, dstep;
    int first, nblk;
};

__global__ __launch_bounds__(256) void k_gray2bgr_mix(const Gray2BgrDesc* __restrict__ descs, MixIndex ix) {
    int blk;
    const int di = mix_pick(descs, ix, &blk);
    if (di < 0) return;
    const Gray2BgrDesc* m = descs + di;
    const int w = m->w, gpr = (w + 3) >> 2;                // groups per row
    const long long ngroups = (long long)gpr * m->h;
    const bool words = !(((uintptr_t)m->src | (uintptr_t)m->dst | (uintptr_t)m->sstep | (uintptr_t)m->dstep) & 3);
    const long long first = (long long)blk * G2B_GROUPS + threadIdx.x;
#pragma unroll 1
    for (int it = 0; it < G2B_GROUPS / 256; it++) {
        const long long idx = first + (long long)it * 256;
        if (idx >= ngroups) break;
        const int y = (int)(idx / gpr), x = (int)(idx - (long long)y * gpr) * 4;
        const uint8_t* sp = m->src + (size_t)y * m->sstep + x;
        uint8_t* d = m->dst + (size_t)y * m->dstep + (size_t)x * 3;
        if (words && x + 4 <= w) {
            const uint32_t v = *(const uint32_t*)sp;
            const uint32_t b0 = v & 0xff, b1 = (v >> 8) & 0xff, b2 = (v >> 16) & 0xff, b3 = v >> 24;
            uint32_t* q = (uint32_t*)d;
            q[0] = b0 * 0x010101u | (b1 << 24);
            q[1] = b1 * 0x0101u | (b2 * 0x01010000u);
            q[2] = b2 | (b3 * 0x01010100u);
        } else {
            const int n = min(4, w - x);
            for (int k = 0; k < n; k++) {
                const uint8_t g = sp[k];
                d[3 * k] = g; d[3 * k + 1] = g; d[3 * k + 2] = g;
            }
        }
    }
}

int launch_gray2bgr_mixed(const Gray2BgrItem* items, int count, hipStream_t s) {
    if (count <= 0) return IMP_OK;
    if (!items) return IMP_ERROR_INVALID_ARGS;
    std::vector<Gray2BgrDesc> v;
    v.reserve((size_t)count);
    for (int i = 0; i < count; i++) {                      // nothing is launched unless every item is well-formed
        const Gray2BgrItem& it = items[i];
        if (!it.src || !it.dst || !view_fits(it.w, it.h, 1, it.sstep) || !view_fits(it.w, it.h, 3, it.dstep)) return IMP_ERROR_INVALID_ARGS;
        Gray2BgrDesc d{};
        d.src = it.src; d.dst = it.dst; d.w = it.w; d.h = it.h; d.sstep = it.sstep; d.dstep = it.dstep;
        d.nblk = (int)(((long long)((it.w + 3) / 4) * it.h + G2B_GROUPS - 1) / G2B_GROUPS);
        v.push_back(d);
    }
    return mix_launch(v, [](Gray2BgrDesc& d) { return (long long)d.w * d.h; }, s, [&](dim3 grid, const Gray2BgrDesc* dev, const MixIndex& ix) {
        hipLaunchKernelGGL(k_gray2bgr_mix, grid, dim3(256), 0, s, dev, ix);
    });
}

int launch_gray2bgr(const Frames& f, hipStream_t s) {
    if (f.count <= 0) return IMP_OK;
    if (f.v.c != 1 || f.dw != f.v.w || f.dh != f.v.h || f.count > 65535) return IMP_ERROR_INVALID_ARGS;
    GArgs a = gargs(f);
    hipLaunchKernelGGL(k_gray2bgr, dim3(blocks_for((long long)f.dw * f.dh), f.count), dim3(256), 0, s, a);
    IMP_HIP(hipGetLastError());
    return IMP_OK;
}

}  // namespace imp
