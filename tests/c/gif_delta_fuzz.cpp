// gif_delta_fuzz.cpp -- the GIF encoder's delta-frame host code under AddressSanitizer + UBSan
// (tests/test_gif_delta_sanitizers.py): the body of impgpu_gif_encode_host_ex2 (csrc/imp_gif_enc.h: the lane code of
// k_gif_enc_delta -- the held rule, the held plane, the window's bounds -- and of the launches behind it reading through the
// window, run one lane after the other) sees the cases and random albums.  One album per line of stdin:
// "w h channels frames segment loop flags dispose" -- dispose a string of one digit per frame -- and the frames' bytes in
// hex.  Every buffer is a heap block of exactly its size.  One line of answers each: the code, the file's size and a
// checksum of the file.
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
        std::string dis, hex;
        in >> w >> h >> c >> n >> segment >> loop >> flags >> dis >> hex;
        const size_t each = (size_t)w * h * c;
        if (hex.size() != 2 * each * (size_t)n || dis.size() != (size_t)n) { std::printf("-1 0 0\n"); continue; }
        std::vector<unsigned char*> frames;
        int* time_ms = (int*)std::malloc(sizeof(int) * (size_t)(n ? n : 1));
        int* dispose = (int*)std::malloc(sizeof(int) * (size_t)(n ? n : 1));
        for (int f = 0; f < n; f++) {                                // every frame a heap block of exactly its size
            unsigned char* p = (unsigned char*)std::malloc(each ? each : 1);
            for (size_t i = 0; i < each; i++) p[i] = (unsigned char)(nib(hex[2 * (f * each + i)]) << 4 | nib(hex[2 * (f * each + i) + 1]));
            frames.push_back(p);
            time_ms[f] = 37 * f;
            dispose[f] = dis[(size_t)f] - '0';
        }
        size_t need = 0;
        int rc = imp::gif_encode_host_ex2(frames.data(), n, w, h, c, w * c, time_ms, dispose, loop, segment, flags, nullptr, 0, &need);
        unsigned long long sum = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            size_t got = 0;
            rc = imp::gif_encode_host_ex2(frames.data(), n, w, h, c, w * c, time_ms, dispose, loop, segment, flags, out, need, &got);
            if (rc == IMP_OK && got == need)
                for (size_t i = 0; i < need; i++) sum = mix(sum, out[i]);
            std::free(out);
        }
        std::printf("%d %zu %llu\n", rc, need, sum);
        for (unsigned char* p : frames) std::free(p);
        std::free(time_ms);
        std::free(dispose);
    }
    return 0;
}
