// inflate_lanes_test.cpp -- the host form of the wave's inflate (csrc/imp_inflate_lanes.h: the rounds of k_png_inflate, one
// lane after the other) against zlib and against imp::inflate_exact, built with AddressSanitizer / UBSan
// (tests/test_inflate_lanes_sanitizers.py).  Seeded random streams of every block type and content class, each decoded
// at the exact size, at fewer and at more bytes than it holds; every truncation of small streams; flipped bits; the header
// cases.  The output buffer is exactly out_size bytes of heap (ASan guards its end) and the input is copied into a buffer
// of exactly the capacity the decoder is told it may read.
//   inflate_lanes_test_asan [iterations]      prints "<cases> cases, <bad> bad"
#include "imp_inflate.h"
#include "imp_inflate_lanes.h"
#include <zlib.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
using namespace imp;

static std::vector<uint8_t> deflate_with(const std::vector<uint8_t>& src, int level, int strategy, int flush_every, int flush_kind) {
    z_stream zs; memset(&zs, 0, sizeof zs);
    deflateInit2(&zs, level, Z_DEFLATED, 15, 8, strategy);
    std::vector<uint8_t> out(deflateBound(&zs, src.size()) * 2 + src.size() + (flush_every ? src.size() / flush_every * 16 : 0) + 65536);
    zs.next_out = out.data(); zs.avail_out = out.size();
    size_t at = 0;
    while (at < src.size()) {
        size_t n = flush_every ? std::min<size_t>(flush_every, src.size() - at) : src.size() - at;
        zs.next_in = (Bytef*)src.data() + at; zs.avail_in = n;
        deflate(&zs, at + n == src.size() ? Z_FINISH : flush_kind);
        at += n;
    }
    if (src.empty()) { zs.next_in = (Bytef*)""; zs.avail_in = 0; deflate(&zs, Z_FINISH); }
    out.resize(zs.total_out);
    deflateEnd(&zs);
    return out;
}

static unsigned rnd_state = 777;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }

static std::unique_ptr<InfMem> g_mem(new InfMem());

// the lanes on z[0, zn) into exactly `want` bytes; the bytes in *got
static int lanes(const uint8_t* z, size_t zn, size_t want, std::vector<uint8_t>* got) {
    const uint32_t cap = (uint32_t)((zn + 3) & ~(size_t)3);
    uint32_t* in = cap ? (uint32_t*)malloc(cap) : (uint32_t*)malloc(4);          // exactly in_cap bytes: ASan sees a read past it
    memset(in, 0, cap ? cap : 4);
    if (zn) memcpy(in, z, zn);
    uint8_t* out = (uint8_t*)malloc(want ? want : 1);                            // exactly out_size bytes
    memset(out, 0xEE, want ? want : 1);
    const int st = inf_lanes_host((const uint8_t*)in, cap, (uint32_t)zn, out, (uint32_t)want, g_mem.get());
    got->assign(out, out + want);
    free(out);
    free(in);
    return st;
}

static long cases = 0, bad = 0;

// one input: the lanes' verdict and bytes against inflate_exact's (always) and zlib's (where zlib delivers `want` bytes)
static void check(const char* what, int iter, const std::vector<uint8_t>& z, size_t want) {
    std::vector<uint8_t> got, ref(want + 1, 0xEE), zl(want + 1, 0xEE);
    const int st = lanes(z.data(), z.size(), want, &got);
    const int rc = inflate_exact(z.data(), z.size(), ref.data(), want);
    cases++;
    if ((st != 0) != (rc != 0)) { bad++; printf("FAIL %s iter %d: lanes %d, inflate_exact %d (in %zu, want %zu)\n", what, iter, st, rc, z.size(), want); return; }
    if (st == 0 && want && memcmp(got.data(), ref.data(), want) != 0) { bad++; printf("FAIL %s iter %d: bytes differ from inflate_exact\n", what, iter); return; }
    if (z.size() < 2) return;
    z_stream zs; memset(&zs, 0, sizeof zs); inflateInit(&zs);
    zs.next_in = (Bytef*)z.data(); zs.avail_in = (uInt)z.size(); zs.next_out = zl.data(); zs.avail_out = (uInt)want;
    const int zr = inflate(&zs, Z_SYNC_FLUSH);
    const size_t n = zs.total_out; inflateEnd(&zs);
    if (want && n == want && zr != Z_DATA_ERROR && zr != Z_NEED_DICT) {
        if (st != 0 || memcmp(got.data(), zl.data(), want) != 0) { bad++; printf("FAIL %s iter %d: zlib delivered %zu bytes, lanes %d\n", what, iter, n, st); }
    } else if (want && n < want && st == 0) { bad++; printf("FAIL %s iter %d: zlib stopped at %zu of %zu (%d), lanes accepted\n", what, iter, n, want, zr); }
}

int main(int argc, char** argv) {
    const int iterations = argc > 1 ? atoi(argv[1]) : 300;
    for (int iter = 0; iter < iterations; iter++) {
        const int kind = rnd() % 7;
        size_t n = kind == 5 ? rnd() % 40 : rnd() % 90000;
        std::vector<uint8_t> src(n);
        for (size_t i = 0; i < n; i++) {
            switch (kind) {
                case 0: src[i] = rnd(); break;
                case 1: src[i] = (uint8_t)(i * 7 + (rnd() % 3)); break;
                case 2: src[i] = i >= 3 && rnd() % 10 ? src[i - 1 - rnd() % 3] : rnd(); break;                 // short distances
                case 3: src[i] = i >= 40000 && rnd() % 50 ? src[i - 32768 + (rnd() % 5)] : (rnd() % 4); break; // far matches
                case 4: src[i] = (rnd() % 100) ? 0 : rnd(); break;                                            // long runs
                case 6: { unsigned v = 0; while (v < 39 && (rnd() & 1)) v++; src[i] = (uint8_t)v; break; }     // a steep histogram: the longest codes
                default: src[i] = rnd(); break;
            }
        }
        const int level = rnd() % 10;
        const int strategy = (rnd() % 4 == 0) ? Z_FIXED : (rnd() % 5 == 0 ? Z_HUFFMAN_ONLY : rnd() % 5 == 0 ? Z_RLE : Z_DEFAULT_STRATEGY);
        const std::vector<uint8_t> z = deflate_with(src, level, strategy, rnd() % 3 ? 0 : 1 + rnd() % 20000, rnd() % 2 ? Z_FULL_FLUSH : Z_SYNC_FLUSH);
        {
            std::vector<uint8_t> got;
            const int st = lanes(z.data(), z.size(), n, &got);
            cases++;
            if (st != 0 || (n && memcmp(got.data(), src.data(), n) != 0)) { bad++; printf("FAIL exact iter %d kind %d n %zu level %d strategy %d status %d\n", iter, kind, n, level, strategy, st); }
        }
        if (n > 10) check("partial", iter, z, 1 + rnd() % (n - 1));
        check("more", iter, z, n + 5);
        for (int t = 0; t < 3 && z.size() > 3; t++) {
            std::vector<uint8_t> zc(z.begin(), z.begin() + rnd() % z.size());
            check("cut", iter, zc, n);
        }
        for (int t = 0; t < 6 && z.size() > 3; t++) {
            std::vector<uint8_t> zc(z);
            zc[rnd() % zc.size()] ^= 1u << (rnd() % 8);
            check("flip", iter, zc, n);
            if (n > 10) check("flip-partial", iter, zc, 1 + rnd() % (n - 1));
        }
    }
    // every truncation and every flipped bit of small streams of each block type
    for (int which = 0; which < 4; which++) {
        std::vector<uint8_t> src(which == 3 ? 700 : 300);
        for (size_t i = 0; i < src.size(); i++) src[i] = (uint8_t)(i % 11 == 0 ? rnd() : (i * 3) & 63);
        const std::vector<uint8_t> z = deflate_with(src, which == 0 ? 0 : 6, which == 1 ? Z_FIXED : Z_DEFAULT_STRATEGY, which == 3 ? 100 : 0, Z_SYNC_FLUSH);
        for (size_t cut = 0; cut <= z.size(); cut++) check("every-cut", which, std::vector<uint8_t>(z.begin(), z.begin() + cut), src.size());
        for (size_t bit = 0; bit < z.size() * 8; bit++) {
            std::vector<uint8_t> zc(z);
            zc[bit >> 3] ^= 1u << (bit & 7);
            check("every-bit", which, zc, src.size());
            check("every-bit-partial", which, zc, src.size() / 2);
        }
        // garbage behind a full output, and a wanted size of zero
        std::vector<uint8_t> zg(z);
        for (int i = 0; i < 40; i++) zg.push_back((uint8_t)rnd());
        check("trailing", which, zg, src.size());
        check("nothing", which, z, 0);
    }
    // the header: method, window, FCHECK, FDICT, and inputs shorter than it
    {
        std::vector<uint8_t> src(64, 7);
        const std::vector<uint8_t> z = deflate_with(src, 6, Z_DEFAULT_STRATEGY, 0, Z_SYNC_FLUSH);
        for (int a = 0; a < 256; a++)
            for (int b = 0; b < 256; b += (a == 0x78 ? 1 : 17)) {
                std::vector<uint8_t> zc(z);
                zc[0] = (uint8_t)a; zc[1] = (uint8_t)b;
                std::vector<uint8_t> got;
                const int st = lanes(zc.data(), zc.size(), src.size(), &got);
                std::vector<uint8_t> ref(src.size());
                const int rc = inflate_exact(zc.data(), zc.size(), ref.data(), src.size());
                cases++;
                if ((st != 0) != (rc != 0)) { bad++; printf("FAIL header %02x %02x: lanes %d, inflate_exact %d\n", a, b, st, rc); }
            }
    }
    printf("%ld cases, %ld bad\n", cases, bad);
    return bad != 0;
}
