// gif_enc_fuzz.cpp -- the GIF encoder's host code under AddressSanitizer + UBSan (tests/test_gif_encode_sanitizers.py):
// impgpu_gif_encode_host's body (csrc/imp_gif_enc.h: the lane code of k_gif_enc_sets / _tables / _index / _lzw / _pack,
// run one lane after the other) sees random albums.  One album per line of stdin: "w h channels frames segment loop" and
// the frames' bytes in hex.  The file is written into a heap block of exactly its size, then read back with the library's
// plain host decoder (imp_gif.h, how = 0) and compared with the frames pixel by pixel.  One line of answers each: the
// code, the file's size, a checksum of the file, and whether the read-back agreed (1; 0 for a refused album).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "imp_gif_enc.h"

static unsigned long long mix(unsigned long long s, unsigned long long v) { return (s * 31 + v) & 0xFFFFFFFFFFFFFFFFull; }
static int nib(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }

// the file's pages against the frames: B,G,R where the frame is not transparent, the transparency key where it is
static bool reads_back(const unsigned char* blob, size_t size, const std::vector<unsigned char*>& frames, int w, int h, int c) {
    std::vector<impgpu_gif_desc> pages(frames.size());
    int count = 0, cw = 0, ch = 0;
    if (impgpu_gif_walk(blob, size, pages.data(), (int)pages.size(), &count, &cw, &ch) != IMP_OK) return false;
    if (count != (int)frames.size() || cw != w || ch != h) return false;
    size_t need = 0;
    if (imp::gif_pages_host(blob, size, 0, nullptr, 0, &need) != IMP_ERROR_MALLOC_FAILED) return false;
    unsigned char* planes = (unsigned char*)std::malloc(need ? need : 1);
    bool ok = imp::gif_pages_host(blob, size, 0, planes, need, &need) == IMP_OK;
    const int pitch = imp::gif_pitch(w);
    for (int f = 0; f < count && ok; f++) {
        const impgpu_gif_desc& d = pages[(size_t)f];
        ok = d.width == w && d.height == h && d.left == 0 && d.top == 0 && !d.interlaced;
        const unsigned char* plane = planes + (size_t)f * pitch * h;
        bool holes = false;
        for (int y = 0; y < h && ok; y++)
            for (int x = 0; x < w && ok; x++) {
                const unsigned char* px = frames[(size_t)f] + ((size_t)y * w + x) * c;
                const int idx = plane[(size_t)(h - 1 - y) * pitch + x];
                if (c == 4 && px[3] == 0) { holes = true; ok = idx == d.transparency_key; continue; }
                const unsigned char* rgb = blob + d.palette_at + 3 * (size_t)idx;
                ok = idx < d.palette_entries && idx != d.transparency_key && rgb[0] == px[2] && rgb[1] == px[1] && rgb[2] == px[0];
            }
        if (ok && !holes) ok = d.transparency_key == -1;
    }
    std::free(planes);
    return ok;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int w = 0, h = 0, c = 0, n = 0, segment = 0, loop = 0;
        std::string hex;
        in >> w >> h >> c >> n >> segment >> loop >> hex;
        const size_t each = (size_t)w * h * c;
        if (hex.size() != 2 * each * (size_t)n) { std::printf("-1 0 0 0\n"); continue; }
        std::vector<unsigned char*> frames;
        std::vector<int> time_ms, dispose;
        for (int f = 0; f < n; f++) {                                // every frame a heap block of exactly its size
            unsigned char* p = (unsigned char*)std::malloc(each ? each : 1);
            for (size_t i = 0; i < each; i++) p[i] = (unsigned char)(nib(hex[2 * (f * each + i)]) << 4 | nib(hex[2 * (f * each + i) + 1]));
            frames.push_back(p);
            time_ms.push_back(37 * f);
            dispose.push_back(f & 3);
        }
        size_t need = 0;
        int rc = imp::gif_encode_host(frames.data(), n, w, h, c, w * c, time_ms.data(), dispose.data(), loop, segment, nullptr, 0, &need);
        unsigned long long sum = 0;
        int back = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            size_t got = 0;
            rc = imp::gif_encode_host(frames.data(), n, w, h, c, w * c, time_ms.data(), dispose.data(), loop, segment, out, need, &got);
            if (rc == IMP_OK && got == need) {
                for (size_t i = 0; i < need; i++) sum = mix(sum, out[i]);
                back = reads_back(out, need, frames, w, h, c) ? 1 : 0;
            }
            std::free(out);
        }
        std::printf("%d %zu %llu %d\n", rc, need, sum, back);
        for (unsigned char* p : frames) std::free(p);
    }
    return 0;
}
