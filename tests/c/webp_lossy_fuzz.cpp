// webp_lossy_fuzz.cpp -- the lossy WebP encoder's host code under AddressSanitizer + UBSan
// (tests/test_webp_lossy_sanitizers.py): impgpu_webp_lossy_encode_host's body (csrc/imp_webp_lossy.h: the lane code of
// k_vp8_planes / _recon / _tokens / _bool / _pack, run one lane after the other) sees the cases and random frames.  One frame
// per line of stdin: "w h channels pad quality" and the frame's rows in hex (each row w * channels + pad bytes, the last
// without its padding).  The frame lives in a heap block of exactly its size, the file is written into a heap block of
// exactly its size.  One line of answers each: the code, the file's size, a checksum of the file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "imp_webp_lossy.h"

static unsigned long long mix(unsigned long long s, unsigned long long v) { return (s * 31 + v) & 0xFFFFFFFFFFFFFFFFull; }
static int nib(char c) { return c <= '9' ? c - '0' : (c | 32) - 'a' + 10; }
static unsigned char* from_hex(const std::string& hex, size_t n) {
    unsigned char* p = (unsigned char*)std::malloc(n ? n : 1);
    for (size_t i = 0; i < n; i++) p[i] = (unsigned char)(nib(hex[2 * i]) << 4 | nib(hex[2 * i + 1]));
    return p;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int w = 0, h = 0, c = 0, pad = 0, quality = 0;
        std::string hex;
        in >> w >> h >> c >> pad >> quality >> hex;
        const int step = w * c + pad;
        const size_t bytes = (size_t)step * (size_t)(h - 1) + (size_t)w * c;
        if (w <= 0 || h <= 0 || hex.size() != 2 * bytes) { std::printf("-1 0 0\n"); continue; }
        unsigned char* frame = from_hex(hex, bytes);
        size_t need = 0;
        int rc = imp::vp8_encode_host(frame, w, h, c, step, quality, nullptr, 0, &need, nullptr, nullptr, nullptr, nullptr, nullptr);
        unsigned long long sum = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            size_t got = 0;
            rc = imp::vp8_encode_host(frame, w, h, c, step, quality, out, need, &got, nullptr, nullptr, nullptr, nullptr, nullptr);
            if (rc == IMP_OK && got == need)
                for (size_t i = 0; i < need; i++) sum = mix(sum, out[i]);
            else if (rc == IMP_OK) rc = -2;
            std::free(out);
        }
        std::printf("%d %zu %llu\n", rc, need, sum);
        std::free(frame);
    }
    return 0;
}
