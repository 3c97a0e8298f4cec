// gif_quant_fuzz.cpp -- the GIF quantiser's host code under AddressSanitizer + UBSan (tests/test_gif_quant_sanitizers.py):
// the bodies of impgpu_gif_encode_host_ex and impgpu_gif_quantize_host (csrc/imp_gif_enc.h: the lane code of
// k_gif_enc_hist and k_gif_enc_cut, and of the launches they feed, run one lane after the other) see the cases and random
// albums.  One album per line of stdin: "w h channels frames segment loop flags" and the frames' bytes in hex.  Every
// buffer is a heap block of exactly its size.  One line of answers each: the code, the file's size, a checksum of the
// file, and a checksum of what impgpu_gif_quantize_host gives for every frame (code, entries, transparent index, table
// and indices).
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

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int w = 0, h = 0, c = 0, n = 0, segment = 0, loop = 0, flags = 0;
        std::string hex;
        in >> w >> h >> c >> n >> segment >> loop >> flags >> hex;
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
        int rc = imp::gif_encode_host_ex(frames.data(), n, w, h, c, w * c, time_ms.data(), dispose.data(), loop, segment, flags, nullptr, 0, &need);
        unsigned long long sum = 0, qsum = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            size_t got = 0;
            rc = imp::gif_encode_host_ex(frames.data(), n, w, h, c, w * c, time_ms.data(), dispose.data(), loop, segment, flags, out, need, &got);
            if (rc == IMP_OK && got == need)
                for (size_t i = 0; i < need; i++) sum = mix(sum, out[i]);
            std::free(out);
        }
        for (int f = 0; f < n; f++) {
            unsigned char* table = (unsigned char*)std::malloc(768);
            unsigned char* indices = (unsigned char*)std::malloc((size_t)w * h ? (size_t)w * h : 1);
            int entries = 0, tkey = 0;
            const int qrc = imp::gif_quantize_host(frames[(size_t)f], w, h, c, w * c, table, &entries, &tkey, indices);
            qsum = mix(mix(mix(qsum, (unsigned)qrc), (unsigned)entries), (unsigned)(tkey + 1));
            if (qrc == IMP_OK) {
                for (int i = 0; i < 3 * entries; i++) qsum = mix(qsum, table[i]);
                for (size_t i = 0; i < (size_t)w * h; i++) qsum = mix(qsum, indices[i]);
            }
            std::free(table);
            std::free(indices);
        }
        std::printf("%d %zu %llu %llu\n", rc, need, sum, qsum);
        for (unsigned char* p : frames) std::free(p);
    }
    return 0;
}
