// webp_lz_fuzz.cpp -- the WebP encoder's host code WITH backward references under AddressSanitizer + UBSan
// (tests/test_webp_lz_sanitizers.py): impgpu_webp_encode_host_flags' body (csrc/imp_webp_enc.h: the lane code of the seven
// launches, the parse's equality words, skips and lengths among it, run one lane after the other) sees planted matches and
// random frames.  One frame per line of stdin: "w h channels pad forced flags" and the frame's rows in hex (each row
// w * channels + pad bytes), then, when forced is 1, a mode byte per tile in hex.  The frame lives in a heap block of exactly
// its size -- the parse reads residuals, never the frame, behind a position -- and the file is written into a heap block
// of exactly its size.  One line of answers each: the code, the file's size, a checksum of the file.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "imp_webp_enc.h"

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
        int w = 0, h = 0, c = 0, pad = 0, forced = 0, flags = 0;
        std::string hex, mhex;
        in >> w >> h >> c >> pad >> forced >> flags >> hex;
        if (forced) in >> mhex;
        const int step = w * c + pad;
        // the last row carries no padding: the block ends with the last pixel
        const size_t bytes = (size_t)step * (size_t)(h - 1) + (size_t)w * c;
        const size_t ntiles = (size_t)imp::webp_tiles(w, IMPGPU_WEBP_TILE_BITS) * (size_t)imp::webp_tiles(h, IMPGPU_WEBP_TILE_BITS);
        if (w <= 0 || h <= 0 || hex.size() != 2 * bytes || (forced && mhex.size() != 2 * ntiles)) { std::printf("-1 0 0\n"); continue; }
        unsigned char* frame = from_hex(hex, bytes);
        unsigned char* modes = forced ? from_hex(mhex, ntiles) : nullptr;
        size_t need = 0;
        int rc = imp::webp_encode_host(frame, w, h, c, step, modes, nullptr, 0, &need, flags);
        unsigned long long sum = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            if (need > imp::webp_file_bound_flags(w, h, c, flags)) rc = -3;
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            size_t got = 0;
            if (rc != -3) rc = imp::webp_encode_host(frame, w, h, c, step, modes, out, need, &got, flags);
            if (rc == IMP_OK && got == need)
                for (size_t i = 0; i < need; i++) sum = mix(sum, out[i]);
            else if (rc == IMP_OK) rc = -2;
            std::free(out);
        }
        std::printf("%d %zu %llu\n", rc, need, sum);
        std::free(frame);
        std::free(modes);
    }
    return 0;
}
