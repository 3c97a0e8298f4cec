// imp_png_enc.hip -- the PNG side of the answer: cvEncodeImage(".png", image, {CV_IMWRITE_PNG_COMPRESSION, q}) at
// bridge.c:704 (q from bridge.c:487-497) for the frame the operator chain leaves in HBM, so that the compressed file crosses
// the link instead of the pixels.  What OpenCV 2.4.9's PngEncoder asks libpng 1.6 for: compression level q, strategy Z_RLE,
// libpng's own filter choice, png_set_bgr, 8-bit gray / RGB / RGBA, no interlace, IHDR + IDAT + IEND -- and the output is
// the same FILE, byte for byte (tests/golden/png_enc is pinned against libpng 1.6.37 + zlib 1.2.11).  Under Z_RLE every
// level from 1 to 9 runs the same deflate_rle, so the file does not depend on q.
//
//   k_png_filter   one workgroup per row: the five filters of PNG 9.2 scored as libpng's heuristic does (sum of
//                  v < 128 ? v : 256 - v, first strictly smallest wins), the chosen row written with its filter byte, and
//                  the row's Adler-32 pieces
//   k_png_edges    one lane per 128-byte segment of an image's filtered stream: its first and last run boundaries
//   k_png_runs     one workgroup per image: where the runs crossing each segment's edges begin and end (max / min scans),
//                  and the stream's Adler-32 from the row pieces
//   k_png_count    one lane per segment: the deflate_rle symbols that start in it (imp_png_deflate.h png_run_count)
//   k_png_symscan  one workgroup per image: the segments' first symbol indices (exclusive scan); 16383 symbols per block
//   k_png_symbols  one lane per segment: every symbol written out, its block's literal/length histogram counted
//   k_png_tree     one workgroup per block, one lane of it busy: trees.c in LDS (plan_block), the block's kind, header bits,
//                  code table and length
//   k_png_place    one lane per image: the blocks' bit offsets (stored blocks byte-align, so this walk is serial), the
//                  Adler-32 trailer
//   k_png_emit     one workgroup per block: lane bit offsets by a block scan, bits OR-ed into the zeroed stream words
// The host writes the signature, IHDR, the zlib header (libpng's CINFO rule for short streams), the IDAT framing of
// 8192-byte chunks with their CRCs, and IEND.
#include <algorithm>
#include <cstring>
#include <vector>
#include "imp_internal.h"
#include "imp_enc_host.h"
#include "imp_inflate.h"
#include "imp_png_deflate.h"

namespace imp {

namespace {

using namespace png;

constexpr int PNG_SEG = 128;                                    // bytes of filtered stream per segment lane
constexpr int PNG_MAX_SIDE = 1000000;                           // libpng's write-side user limits (PNG_USER_WIDTH_MAX / HEIGHT_MAX)
constexpr int PNG_MAX_BATCH = 256;
constexpr uint64_t PNG_MAX_BYTES = 1ull << 28;                  // filtered bytes of one frame the device takes
constexpr int PNG_HDR_WORDS = 80;                               // a dynamic block's tree description: < 2300 bits
constexpr int PNG_TAB = L_CODES + 1;
constexpr uint32_t NONE = 0xffffffffu;

struct PngJob {
    const uint8_t* src;
    int w, h, c, step;
    uint32_t rowlen, n;                 // 1 + w c, h rowlen
    uint32_t row0, seg0, nseg, blk0, maxblk;
    uint32_t zwords;
    uint8_t* f;                         // filtered stream (n bytes)
    uint32_t* syms;                     // one word per symbol (at most n)
    uint32_t* z;                        // the zlib stream's words, zeroed
};
struct PngBlk {
    uint32_t kind, start, end, sym0, nsym, hdr_bits;
    uint64_t bits;                      // non-stored: 3 + the tree description + the symbols + END_BLOCK
    uint64_t off;                       // bit offset of the block's 3 header bits in the stream
};
// per image, filled on the device: [0] symbols, [1] blocks, [2] stream bytes, [3] Adler-32, [4] status (0 = fine)
constexpr int PNG_RES = 8;

struct PngDev {
    const PngJob* jobs;
    int njobs;
    uint32_t *rowA, *rowB;
    uint32_t *segF, *segL, *segRS, *segRE, *segCnt, *segBase;
    uint32_t *hist, *blkStart, *tabs, *hdrs;
    PngBlk* blk;
    uint32_t* res;
};

template <int FIELD>
__device__ inline int find_job(const PngJob* jobs, int njobs, uint32_t g) {
    int lo = 0, hi = njobs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const uint32_t v = FIELD == 0 ? jobs[mid].row0 : FIELD == 1 ? jobs[mid].seg0 : jobs[mid].blk0;
        if (v <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// the filtered stream's byte i of row y, before filtering: R, G, B[, A] from B, G, R[, A] (png_set_bgr)
__device__ inline int raw_at(const PngJob& J, int y, int i) {
    const int x = i / J.c, ch = i - x * J.c;
    const int sch = (J.c >= 3 && ch < 3) ? 2 - ch : ch;
    return J.src[(size_t)y * J.step + (size_t)x * J.c + sch];
}
__device__ inline int paeth(int a, int b, int c) {
    const int p = b - c, q = a - c;
    const int pa = p < 0 ? -p : p, pb = q < 0 ? -q : q, pc = (p + q) < 0 ? -(p + q) : p + q;
    return (pa <= pb && pa <= pc) ? a : (pb <= pc) ? b : c;
}
__device__ inline uint32_t score(int v) { v &= 255; return v < 128 ? v : 256 - v; }

template <class T, class Op>
__device__ inline T block_reduce(T v, T* lds, Op op) {          // blockDim.x == 256
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) lds[t] = op(lds[t], lds[t + s]);
        __syncthreads();
    }
    const T r = lds[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void k_png_filter(PngDev D) {
    __shared__ uint32_t s_sum[5][256];
    __shared__ uint64_t s_ab[256];
    const int jb = find_job<0>(D.jobs, D.njobs, blockIdx.x);
    const PngJob& J = D.jobs[jb];
    const int y = (int)(blockIdx.x - J.row0), t = threadIdx.x, wc = J.w * J.c, c = J.c;
    uint32_t sum[5] = {0, 0, 0, 0, 0};
    for (int i = t; i < wc; i += 256) {
        const int x = raw_at(J, y, i), b = y ? raw_at(J, y - 1, i) : 0;
        const int a = i >= c ? raw_at(J, y, i - c) : 0, d = (i >= c && y) ? raw_at(J, y - 1, i - c) : 0;
        sum[0] += score(x); sum[1] += score(x - a); sum[2] += score(x - b);
        sum[3] += score(x - ((a + b) >> 1)); sum[4] += score(x - paeth(a, b, d));
    }
    for (int k = 0; k < 5; k++) s_sum[k][t] = sum[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s)
            for (int k = 0; k < 5; k++) s_sum[k][t] += s_sum[k][t + s];
        __syncthreads();
    }
    // png_write_find_filter: None, Sub, Up, Average, Paeth; the first strictly smallest sum.  One row: no Up / Average /
    // Paeth; one pixel wide: no Sub / Average / Paeth.
    int best = 0;
    uint32_t mins = s_sum[0][0];
    for (int k = 1; k < 5; k++) {
        if (J.h == 1 && (k == 2 || k == 3 || k == 4)) continue;
        if (J.w == 1 && (k == 1 || k == 3 || k == 4)) continue;
        if (s_sum[k][0] < mins) { mins = s_sum[k][0]; best = k; }
    }
    uint8_t* row = J.f + (size_t)y * J.rowlen;
    const uint32_t L = J.rowlen;
    uint64_t A = 0, B = 0;
    if (t == 0) { row[0] = (uint8_t)best; A = (uint64_t)best; B = (uint64_t)L * best; }
    for (int i = t; i < wc; i += 256) {
        const int x = raw_at(J, y, i);
        int v = x;
        if (best) {
            const int b = y ? raw_at(J, y - 1, i) : 0, a = i >= c ? raw_at(J, y, i - c) : 0;
            v = best == 1 ? x - a : best == 2 ? x - b : best == 3 ? x - ((a + b) >> 1)
                                                       : x - paeth(a, b, (i >= c && y) ? raw_at(J, y - 1, i - c) : 0);
        }
        v &= 255;
        row[1 + i] = (uint8_t)v;
        A += (uint64_t)v;
        B += (uint64_t)(L - 1 - i) * (uint64_t)v;                 // byte k = 1 + i weighs L - k
    }
    A = block_reduce(A, s_ab, [](uint64_t p, uint64_t q) { return p + q; });
    B = block_reduce(B, s_ab, [](uint64_t p, uint64_t q) { return p + q; });
    if (t == 0) { D.rowA[blockIdx.x] = (uint32_t)(A % ADLER_MOD); D.rowB[blockIdx.x] = (uint32_t)(B % ADLER_MOD); }
}

__global__ __launch_bounds__(256) void k_png_edges(PngDev D, uint32_t nseg) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nseg) return;
    const PngJob& J = D.jobs[find_job<1>(D.jobs, D.njobs, g)];
    const uint32_t lo = (g - J.seg0) * PNG_SEG, hi = min(lo + (uint32_t)PNG_SEG, J.n);
    uint32_t first = NONE, last = NONE;
    int prev = lo ? J.f[lo - 1] : -1;
    for (uint32_t i = lo; i < hi; i++) {
        const int v = J.f[i];
        if (v != prev) { if (first == NONE) first = i; last = i; }
        prev = v;
    }
    D.segF[g] = first;
    D.segL[g] = last;
}

// Inclusive scan of one value per thread over 1024 threads (Hillis-Steele in LDS).
template <class Op>
__device__ inline uint32_t scan1024(uint32_t v, uint32_t* lds, Op op) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
    for (int s = 1; s < 1024; s <<= 1) {
        const uint32_t o = t >= s ? lds[t - s] : 0;
        const bool has = t >= s;
        __syncthreads();
        if (has) lds[t] = op(lds[t], o);
        __syncthreads();
    }
    const uint32_t r = lds[t];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(1024) void k_png_runs(PngDev D) {
    __shared__ uint32_t s[1024];
    __shared__ uint32_t s_a[1024], s_b[1024], s_n[1024];
    const PngJob& J = D.jobs[blockIdx.x];
    const int t = threadIdx.x;
    const uint32_t per = (J.nseg + 1023) / 1024, s0 = min(t * per, J.nseg), s1 = min(s0 + per, J.nseg);
    // run starts: exclusive max of the segments' last boundaries (position 0 is a boundary, so 0 is the identity)
    uint32_t m = 0;
    for (uint32_t k = s0; k < s1; k++) if (D.segL[J.seg0 + k] != NONE) m = max(m, D.segL[J.seg0 + k]);
    (void)scan1024(m, s, [](uint32_t p, uint32_t q) { return max(p, q); });
    uint32_t run = t ? s[t - 1] : 0;                            // exclusive: through the threads before (s = inclusive)
    __syncthreads();
    for (uint32_t k = s0; k < s1; k++) {
        const uint32_t lo = k * PNG_SEG, g = J.seg0 + k;
        D.segRS[g] = D.segF[g] == lo ? lo : run;
        if (D.segL[g] != NONE) run = max(run, D.segL[g]);
    }
    // run ends: the first boundary at or after the segment's end (J.n past the last one), a min scan from the right
    const int r = 1023 - t;                                     // thread r takes the mirrored range
    const uint32_t q0 = min(r * per, J.nseg), q1 = min(q0 + per, J.nseg);
    uint32_t mn = J.n;
    for (uint32_t k = q0; k < q1; k++) if (D.segF[J.seg0 + k] != NONE) mn = min(mn, D.segF[J.seg0 + k]);
    (void)scan1024(mn, s, [](uint32_t p, uint32_t q) { return min(p, q); });   // in mirrored order: segments after
    uint32_t after = t ? s[t - 1] : J.n;                        // min over the ranges of threads r' > r
    __syncthreads();
    for (uint32_t k = q1; k-- > q0;) {
        const uint32_t g = J.seg0 + k;
        D.segRE[g] = after;
        if (D.segF[g] != NONE) after = min(after, D.segF[g]);
    }
    // Adler-32: the rows' (A, B) pieces combine as (A1 + A2, B1 + B2 + L A2) in row order -- every row has L bytes
    const uint32_t rper = (J.h + 1023) / 1024, r0 = min(t * rper, (uint32_t)J.h), r1 = min(r0 + rper, (uint32_t)J.h);
    uint32_t A = 0, B = 0, N = 0;
    for (uint32_t k = r0; k < r1; k++) {
        const uint32_t a2 = D.rowA[J.row0 + k], b2 = D.rowB[J.row0 + k];
        B = (uint32_t)(((uint64_t)B + b2 + (uint64_t)(J.rowlen % ADLER_MOD) * A) % ADLER_MOD);
        A = (A + a2) % ADLER_MOD;
        N = (uint32_t)(((uint64_t)N + J.rowlen) % ADLER_MOD);
    }
    s_a[t] = A; s_b[t] = B; s_n[t] = N;
    __syncthreads();
    for (int st = 1; st < 1024; st <<= 1) {
        if ((t & (2 * st - 1)) == 0) {
            const uint32_t a1 = s_a[t], b1 = s_b[t], a2 = s_a[t + st], b2 = s_b[t + st], n2 = s_n[t + st];
            s_b[t] = (uint32_t)(((uint64_t)b1 + b2 + (uint64_t)n2 * a1) % ADLER_MOD);
            s_a[t] = (a1 + a2) % ADLER_MOD;
            s_n[t] = (s_n[t] + n2) % ADLER_MOD;
        }
        __syncthreads();
    }
    if (t == 0) {
        const uint32_t a = (1 + s_a[0]) % ADLER_MOD, b = (uint32_t)(((uint64_t)s_b[0] + (uint64_t)J.n) % ADLER_MOD);
        D.res[blockIdx.x * PNG_RES + 3] = b << 16 | a;
    }
}

// The runs crossing [lo, hi): f(a, b, byte) for each, in order.
template <class F>
__device__ inline void walk_runs(const PngJob& J, uint32_t lo, uint32_t hi, uint32_t rs, uint32_t re, F&& f) {
    uint32_t a = rs;
    int prev = J.f[lo];
    for (uint32_t i = lo + 1; i < hi; i++) {
        const int v = J.f[i];
        if (v != prev) { f(a, i, prev); a = i; prev = v; }
    }
    f(a, re, prev);
}

__global__ __launch_bounds__(256) void k_png_count(PngDev D, uint32_t nseg) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nseg) return;
    const PngJob& J = D.jobs[find_job<1>(D.jobs, D.njobs, g)];
    const uint32_t lo = (g - J.seg0) * PNG_SEG, hi = min(lo + (uint32_t)PNG_SEG, J.n);
    uint32_t n = 0;
    walk_runs(J, lo, hi, D.segRS[g], D.segRE[g], [&](uint32_t a, uint32_t b, int) { n += png_run_count(a, b, lo, hi); });
    D.segCnt[g] = n;
}

__global__ __launch_bounds__(1024) void k_png_symscan(PngDev D) {
    __shared__ uint32_t s[1024];
    const PngJob& J = D.jobs[blockIdx.x];
    const int t = threadIdx.x;
    const uint32_t per = (J.nseg + 1023) / 1024, s0 = min(t * per, J.nseg), s1 = min(s0 + per, J.nseg);
    uint32_t sum = 0;
    for (uint32_t k = s0; k < s1; k++) sum += D.segCnt[J.seg0 + k];
    const uint32_t inc = scan1024(sum, s, [](uint32_t p, uint32_t q) { return p + q; });
    uint32_t base = inc - sum;
    for (uint32_t k = s0; k < s1; k++) { D.segBase[J.seg0 + k] = base; base += D.segCnt[J.seg0 + k]; }
    if (t == 1023) {
        D.res[blockIdx.x * PNG_RES + 0] = inc;
        D.res[blockIdx.x * PNG_RES + 1] = inc / BLOCK_SYMS + 1;
    }
}

__global__ __launch_bounds__(256) void k_png_symbols(PngDev D, uint32_t nseg) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= nseg) return;
    const PngJob& J = D.jobs[find_job<1>(D.jobs, D.njobs, g)];
    const uint32_t lo = (g - J.seg0) * PNG_SEG, hi = min(lo + (uint32_t)PNG_SEG, J.n);
    uint32_t at = D.segBase[g];
    uint32_t pend_key = NONE, pend_n = 0;                       // consecutive equal (block, symbol) counts share one atomic
    uint32_t* hist = D.hist + (size_t)J.blk0 * L_CODES;
    walk_runs(J, lo, hi, D.segRS[g], D.segRE[g], [&](uint32_t a, uint32_t b, int byte) {
        png_run_symbols(a, b, byte, lo, hi, [&](uint32_t pos, uint32_t sym) {
            J.syms[at] = sym;
            const uint32_t blk = at / BLOCK_SYMS;
            if (at - blk * BLOCK_SYMS == 0) D.blkStart[J.blk0 + blk] = pos;
            const uint32_t key = blk * L_CODES + (sym & 511);
            if (key != pend_key) {
                if (pend_n) atomicAdd(&hist[pend_key], pend_n);
                pend_key = key;
                pend_n = 0;
            }
            pend_n++;
            at++;
        });
    });
    if (pend_n) atomicAdd(&hist[pend_key], pend_n);
}

__global__ __launch_bounds__(64) void k_png_tree(PngDev D) {
    __shared__ BlockTrees T;
    const int jb = find_job<2>(D.jobs, D.njobs, blockIdx.x);
    const PngJob& J = D.jobs[jb];
    const uint32_t b = blockIdx.x - J.blk0, nsym = D.res[jb * PNG_RES + 0], nblk = D.res[jb * PNG_RES + 1];
    if (b >= nblk || threadIdx.x) return;
    const uint32_t sym0 = b * BLOCK_SYMS;
    const uint32_t start = sym0 < nsym ? D.blkStart[blockIdx.x] : J.n;
    const uint32_t end = (b + 1) * BLOCK_SYMS < nsym ? D.blkStart[blockIdx.x + 1] : J.n;   // (a final empty block starts at J.n)
    const int kind = plan_block(T, D.hist + (size_t)blockIdx.x * L_CODES, end - start);
    PngBlk& B = D.blk[blockIdx.x];
    B.kind = (uint32_t)kind; B.start = start; B.end = end; B.sym0 = sym0; B.nsym = min(nsym - sym0, (uint32_t)BLOCK_SYMS);
    B.hdr_bits = 0;
    B.bits = 3 + (kind == BT_DYN ? T.opt_len : T.static_len);
    if (kind == BT_STORED) return;
    code_table(T, kind, D.tabs + (size_t)blockIdx.x * PNG_TAB);
    if (kind == BT_DYN) {
        uint32_t* h = D.hdrs + (size_t)blockIdx.x * PNG_HDR_WORDS;
        for (int k = 0; k < PNG_HDR_WORDS; k++) h[k] = 0;
        BitWords o{h, 0};
        send_all_trees(o, T);
        B.hdr_bits = (uint32_t)o.at;
    }
}

__global__ __launch_bounds__(64) void k_png_place(PngDev D) {
    const PngJob& J = D.jobs[blockIdx.x];
    if (threadIdx.x) return;
    uint32_t* res = D.res + blockIdx.x * PNG_RES;
    const uint32_t nblk = res[1];
    uint64_t bit = 16;
    for (uint32_t b = 0; b < nblk; b++) {
        PngBlk& B = D.blk[J.blk0 + b];
        B.off = bit;
        if (B.kind == BT_STORED) bit = ((bit + 3 + 7) & ~(uint64_t)7) + 32 + 8 * (uint64_t)(B.end - B.start);
        else bit += B.bits;
    }
    const uint64_t bytes = ((bit + 7) >> 3) + 4;
    res[2] = (uint32_t)bytes;
    res[4] = bytes > (uint64_t)J.zwords * 4 ? 1u : 0u;
    if (res[4]) return;
    const uint32_t adler = res[3];
    const uint64_t at = (bit + 7) >> 3;                         // the trailer, most significant byte first
    for (int k = 0; k < 4; k++) atomicOr(&J.z[(at + k) >> 2], ((adler >> (24 - 8 * k)) & 0xffu) << (8 * ((at + k) & 3)));
}

__device__ inline void or_bits(uint32_t* z, uint64_t at, uint64_t v, int n) {
    if (!n) return;
    const uint32_t sh = (uint32_t)(at & 31);
    const uint64_t lo = v << sh;                                // n <= 32: fits with the shift
    atomicOr(&z[at >> 5], (uint32_t)lo);
    if (sh + n > 32) atomicOr(&z[(at >> 5) + 1], (uint32_t)(lo >> 32));
}

__global__ __launch_bounds__(256) void k_png_emit(PngDev D) {
    __shared__ uint32_t tab[PNG_TAB];
    __shared__ uint32_t s[256];
    const int jb = find_job<2>(D.jobs, D.njobs, blockIdx.x);
    const PngJob& J = D.jobs[jb];
    const uint32_t* res = D.res + jb * PNG_RES;
    const uint32_t b = blockIdx.x - J.blk0, nblk = res[1];
    if (b >= nblk || res[4]) return;
    const PngBlk& B = D.blk[blockIdx.x];
    const int t = threadIdx.x;
    const uint32_t last = b + 1 == nblk;
    if (B.kind == BT_STORED) {
        const uint32_t len = B.end - B.start;
        const uint64_t db = ((B.off + 3 + 7) >> 3);            // LEN's byte
        if (t == 0) {
            or_bits(J.z, B.off, last, 3);
            or_bits(J.z, db * 8, (uint64_t)(len & 0xffff) | (uint64_t)(~len & 0xffff) << 16, 32);
        }
        const uint64_t d0 = db + 4, d1 = d0 + len;             // bytes [d0, d1) <- f[start, end)
        for (uint64_t ww = (d0 >> 2) + t; ww <= (d1 - 1) >> 2; ww += 256) {
            uint32_t v = 0;
            for (int k = 0; k < 4; k++) {
                const uint64_t p = ww * 4 + k;
                if (p >= d0 && p < d1) v |= (uint32_t)J.f[B.start + (p - d0)] << (8 * k);
            }
            atomicOr(&J.z[ww], v);
        }
        return;
    }
    for (int k = t; k < PNG_TAB; k += 256) tab[k] = D.tabs[(size_t)blockIdx.x * PNG_TAB + k];
    __syncthreads();
    const uint64_t body = B.off + 3 + B.hdr_bits;
    if (t == 0) {
        or_bits(J.z, B.off, (uint64_t)(B.kind << 1 | last), 3);
        const uint32_t* h = D.hdrs + (size_t)blockIdx.x * PNG_HDR_WORDS;
        for (uint32_t k = 0; k * 32 < B.hdr_bits; k++) {
            const int n = (int)min(32u, B.hdr_bits - k * 32);
            or_bits(J.z, B.off + 3 + k * 32, h[k] & (n == 32 ? 0xffffffffu : ((1u << n) - 1)), n);
        }
    }
    const uint32_t per = (B.nsym + 255) / 256, k0 = min(t * per, B.nsym), k1 = min(k0 + per, B.nsym);
    const uint32_t* sy = J.syms + B.sym0;
    uint32_t bits = 0;
    for (uint32_t k = k0; k < k1; k++) { uint64_t v; bits += (uint32_t)sym_bits(sy[k], tab, &v); }
    // exclusive block scan of the lanes' bit counts
    s[t] = bits;
    __syncthreads();
    for (int st = 1; st < 256; st <<= 1) {
        const uint32_t o = t >= st ? s[t - st] : 0;
        __syncthreads();
        s[t] += o;
        __syncthreads();
    }
    uint64_t at = body + (s[t] - bits);
    const uint64_t endb = body + s[255];
    for (uint32_t k = k0; k < k1; k++) {
        uint64_t v;
        const int n = sym_bits(sy[k], tab, &v);
        or_bits(J.z, at, v, n);
        at += (uint64_t)n;
    }
    if (t == 0) or_bits(J.z, endb, tab[END_BLOCK] & 0xffff, (int)(tab[END_BLOCK] >> 16));
}

// ---------------------------------------------------------------- host
bool png_geom(int w, int h, int c, uint64_t* n) {
    if (w <= 0 || h <= 0 || w > PNG_MAX_SIDE || h > PNG_MAX_SIDE) return false;   // (libpng refuses those: cvEncodeImage fails)
    *n = (uint64_t)h * (1 + (uint64_t)w * (uint64_t)c);
    return *n <= PNG_MAX_BYTES;
}
uint64_t zlib_bound(uint64_t n) { return 2 + n + 6 * (n / BLOCK_SYMS + 2) + 4 + 16; }   // a block costs at most its bytes + 5.25
uint64_t file_len(uint64_t zbytes) { return 8 + 25 + zbytes + 12 * ((zbytes + 8191) / 8192) + 12; }

void put32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// signature, IHDR, the zlib stream in IDAT chunks of 8192 bytes, IEND
void write_file(uint8_t* o, int w, int h, int c, const uint8_t* zs, uint64_t zbytes) {
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0d, 0x0a, 0x1a, 0x0a};
    std::memcpy(o, sig, 8);
    put32(o + 8, 13);
    std::memcpy(o + 12, "IHDR", 4);
    put32(o + 16, (uint32_t)w); put32(o + 20, (uint32_t)h);
    o[24] = 8; o[25] = c == 1 ? 0 : c == 3 ? 2 : 6; o[26] = 0; o[27] = 0; o[28] = 0;
    put32(o + 29, crc32_ieee(o + 12, 17));
    uint8_t* p = o + 33;
    for (uint64_t z = 0; z < zbytes; z += 8192) {
        const uint32_t len = (uint32_t)std::min<uint64_t>(8192, zbytes - z);
        put32(p, len);
        std::memcpy(p + 4, "IDAT", 4);
        std::memcpy(p + 8, zs + z, len);
        put32(p + 8 + len, crc32_ieee(p + 4, 4 + (size_t)len));
        p += 12 + len;
    }
    put32(p, 0);
    std::memcpy(p + 4, "IEND", 4);
    put32(p + 8, 0xae426082u);
}

int encode_group(const impgpu_image* const* images, int count, int level, unsigned char* const* outs, const size_t* caps,
                 size_t* lens, int* codes) {
    hipStream_t s = env_stream();
    std::vector<PngJob> jobs;
    std::vector<int> owner;
    uint64_t f_bytes = 0, sym_words = 0, z_words = 0;
    uint32_t rows = 0, segs = 0, blks = 0;
    std::vector<uint64_t> o_f, o_s, o_z;
    for (int i = 0; i < count; i++) {
        lens[i] = 0;
        const impgpu_image* im = images[i];
        uint64_t n = 0;
        if (!im || !outs[i]) codes[i] = IMP_ERROR_INVALID_ARGS;
        else if (level == 0) codes[i] = IMP_ERROR_UNSUPPORTED;
        else if (level < 0 || level > 9) codes[i] = IMP_ERROR_INVALID_ARGS;
        else if (im->c == 2) codes[i] = IMP_ERROR_UNSUPPORTED;
        else if (im->c != 1 && im->c != 3 && im->c != 4) codes[i] = IMP_ERROR_INVALID_ARGS;
        else if (!png_geom(im->w, im->h, im->c, &n)) codes[i] = im->w > 0 && im->h > 0 ? IMP_ERROR_UNSUPPORTED : IMP_ERROR_INVALID_ARGS;
        else codes[i] = IMP_OK;
        if (codes[i] != IMP_OK) continue;
        PngJob J{};
        J.src = im->d; J.w = im->w; J.h = im->h; J.c = im->c; J.step = im->step;
        J.rowlen = (uint32_t)(1 + im->w * im->c); J.n = (uint32_t)n;
        J.row0 = rows; rows += (uint32_t)im->h;
        J.nseg = (uint32_t)((n + PNG_SEG - 1) / PNG_SEG); J.seg0 = segs; segs += J.nseg;
        J.maxblk = (uint32_t)(n / BLOCK_SYMS + 1); J.blk0 = blks; blks += J.maxblk;
        J.zwords = (uint32_t)((zlib_bound(n) + 3) / 4);
        o_f.push_back(f_bytes); f_bytes += up256(n);
        o_s.push_back(sym_words); sym_words += (n + 63) & ~uint64_t(63);
        o_z.push_back(z_words); z_words += ((uint64_t)J.zwords + 63) & ~uint64_t(63);
        jobs.push_back(J);
        owner.push_back(i);
    }
    const int nj = (int)jobs.size();
    if (!nj) return IMP_OK;
    // one pool block: filtered streams | symbols | zlib words | row pieces | segment records | block records | results
    BlockLayout L;
    const size_t a_f = L.take(f_bytes);                                 // the filtered streams
    const size_t a_s = L.take(sym_words * 4);                           // the symbols
    const size_t a_z = L.take(z_words * 4);                             // the zlib words (zeroed)
    const size_t a_rows = L.take((size_t)rows * 8);                     // row pieces: rowA, rowB
    const size_t a_seg = L.take((size_t)segs * 24);                     // six words a segment
    const size_t a_hist = L.take((size_t)blks * L_CODES * 4);           // the blocks' histograms (zeroed)
    const size_t a_bs = L.take((size_t)blks * 4 + 4);                   // the blocks' starts
    const size_t a_tab = L.take((size_t)blks * PNG_TAB * 4);            // ... code tables
    const size_t a_hdr = L.take((size_t)blks * PNG_HDR_WORDS * 4);      // ... headers
    const size_t a_blk = L.take((size_t)blks * sizeof(PngBlk));         // ... records
    const size_t a_res = L.take((size_t)nj * PNG_RES * 4);              // the results (zeroed)
    DevBlock block, table;                                              // the block, and the jobs table uploaded beside it
    if (int rc = dev_alloc(L.size(), &block.p)) return rc;
    uint8_t* m = block.bytes();
    for (int k = 0; k < nj; k++) {
        jobs[k].f = m + a_f + o_f[k];
        jobs[k].syms = (uint32_t*)(m + a_s) + o_s[k];
        jobs[k].z = (uint32_t*)(m + a_z) + o_z[k];
    }
    if (int rc = upload_small(jobs.data(), jobs.size() * sizeof(PngJob), &table.p, s)) return rc;
    PngDev D;
    D.jobs = (const PngJob*)table.p; D.njobs = nj;
    D.rowA = (uint32_t*)(m + a_rows); D.rowB = D.rowA + rows;
    D.segF = (uint32_t*)(m + a_seg); D.segL = D.segF + segs; D.segRS = D.segL + segs; D.segRE = D.segRS + segs;
    D.segCnt = D.segRE + segs; D.segBase = D.segCnt + segs;
    D.hist = (uint32_t*)(m + a_hist); D.blkStart = (uint32_t*)(m + a_bs); D.tabs = (uint32_t*)(m + a_tab);
    D.hdrs = (uint32_t*)(m + a_hdr); D.blk = (PngBlk*)(m + a_blk); D.res = (uint32_t*)(m + a_res);
    hipError_t e = hipMemsetAsync(m + a_z, 0, z_words * 4, s);
    if (e == hipSuccess) e = hipMemsetAsync(m + a_hist, 0, a_bs - a_hist, s);
    if (e == hipSuccess) e = hipMemsetAsync(m + a_res, 0, L.size() - a_res, s);
    const unsigned sg = (segs + 255) / 256;
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_png_filter, dim3(rows), dim3(256), 0, s, D);
        hipLaunchKernelGGL(k_png_edges, dim3(sg), dim3(256), 0, s, D, segs);
        hipLaunchKernelGGL(k_png_runs, dim3(nj), dim3(1024), 0, s, D);
        hipLaunchKernelGGL(k_png_count, dim3(sg), dim3(256), 0, s, D, segs);
        hipLaunchKernelGGL(k_png_symscan, dim3(nj), dim3(1024), 0, s, D);
        hipLaunchKernelGGL(k_png_symbols, dim3(sg), dim3(256), 0, s, D, segs);
        hipLaunchKernelGGL(k_png_tree, dim3(blks), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_png_place, dim3(nj), dim3(64), 0, s, D);
        hipLaunchKernelGGL(k_png_emit, dim3(blks), dim3(256), 0, s, D);
        e = hipGetLastError();
    }
    if (e != hipSuccess) { set_error("png encode", e); return drained(IMP_ERROR_DEVICE); }
    std::vector<uint32_t> res((size_t)nj * PNG_RES);
    if (int rc = fetch_records(D.res, res.size() * 4, res.data(), "png encode")) return rc;      // the first wait
    // the streams that fit their callers' buffers, in one pinned area
    AnswerFetch answers;
    std::vector<int> piece((size_t)nj, -1);
    for (int k = 0; k < nj; k++) {
        const int i = owner[k];
        const uint32_t* r = &res[(size_t)k * PNG_RES];
        if (r[4]) { codes[i] = IMP_ERROR_DEVICE; set_error_text("png encode: a stream outgrew its bound"); continue; }
        if (answer_fits((size_t)file_len(r[2]), caps[i], &codes[i], &lens[i])) piece[k] = answers.add(jobs[k].z, r[2]);
    }
    const int rc = answers.run("png encode download");                 // the second wait
    for (int k = 0; k < nj && !rc; k++) {
        if (piece[k] < 0) continue;
        const PngJob& J = jobs[k];
        uint8_t* zs = answers.at(piece[k]);
        zlib_header(J.n, zs);                                   // (the kernels leave the first two bytes to the host)
        write_file(outs[owner[k]], J.w, J.h, J.c, zs, res[(size_t)k * PNG_RES + 2]);
    }
    return rc;
}

}  // namespace

}  // namespace imp

using namespace imp;

extern "C" {

size_t impgpu_png_encode_bound(int width, int height, int channels) {
    uint64_t n;
    if ((channels != 1 && channels != 3 && channels != 4) || !png_geom(width, height, channels, &n)) return 0;
    return (size_t)file_len(zlib_bound(n));
}

int impgpu_batch_encode_png(const impgpu_image* const* images, int count, int level, unsigned char* const* outs,
                            const size_t* capacities, size_t* lengths, int* codes) {
    if (count < 0 || count > PNG_MAX_BATCH || (count && (!images || !outs || !capacities || !lengths || !codes))) return IMP_ERROR_INVALID_ARGS;
    if (int rc = need_env()) return rc;
    TraceRange tr("IMP_STEP_ENCODE");                           // bridge.c:679-710
    IMP_FAULT_POINT(IMP_STEP_ENCODE);
    return encode_group(images, count, level, outs, capacities, lengths, codes);
}

int impgpu_image_encode_png(const impgpu_image* image, int level, unsigned char* out, size_t capacity, size_t* length) {
    if (!image || !out || !length) return IMP_ERROR_INVALID_ARGS;
    int code = IMP_OK;
    if (int rc = impgpu_batch_encode_png(&image, 1, level, &out, &capacity, length, &code)) return rc;
    return code;
}

int impgpu_png_deflate(const unsigned char* data, size_t size, unsigned char* out, size_t capacity, size_t* length) {
    if ((!data && size) || !length) return IMP_ERROR_INVALID_ARGS;
    *length = 0;
    if (size > PNG_MAX_BYTES) return IMP_ERROR_UNSUPPORTED;
    std::vector<uint32_t> words((size_t)(zlib_bound(size) + 3) / 4 + 2, 0), hist(L_CODES), syms(BLOCK_SYMS);
    std::vector<BlockTrees> T(1);
    const uint64_t n = deflate_serial(data, (uint32_t)size, words.data(), T[0], hist.data(), syms.data());
    *length = (size_t)n;
    if (capacity < n || !out) return IMP_ERROR_MALLOC_FAILED;
    std::memcpy(out, words.data(), (size_t)n);
    return IMP_OK;
}

}  // extern "C"
