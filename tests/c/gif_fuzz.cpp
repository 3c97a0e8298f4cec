// gif_fuzz.cpp -- the GIF front's host code under AddressSanitizer + UBSan (tests/test_gif_decode_sanitizers.py): the
// container walk of include/impgpu_gif.h and both decoders of csrc/imp_gif.h -- the plain one and the wave's rounds, the
// kernel's own lane code -- see files somebody uploaded.  One file per line of stdin, in hex; one line of answers each:
//   walk's code, its page count and canvas, a checksum of its records; then per decoder the code of impgpu_gif_pages'
//   body and a checksum of the planes.  The planes are written into a heap block of exactly their size, so a byte
//   outside them is the sanitizer's to report.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "imp_gif.h"

static unsigned long long mix(unsigned long long s, unsigned long long v) { return (s * 31 + v) & 0xFFFFFFFFFFFFFFFFull; }

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<unsigned char> file(line.size() / 2);
        for (size_t i = 0; i < file.size(); i++) file[i] = (unsigned char)std::stoi(line.substr(2 * i, 2), nullptr, 16);
        // (an exact-size heap copy: a read past the file's end is the sanitizer's to report too)
        unsigned char* blob = (unsigned char*)std::malloc(file.size() ? file.size() : 1);
        for (size_t i = 0; i < file.size(); i++) blob[i] = file[i];
        std::vector<impgpu_gif_desc> recs(8);
        int count = -1, cw = -1, ch = -1;
        int rc = impgpu_gif_walk(blob, file.size(), recs.data(), (int)recs.size(), &count, &cw, &ch);
        if (rc == IMP_ERROR_MALLOC_FAILED) {
            recs.resize((size_t)count);
            rc = impgpu_gif_walk(blob, file.size(), recs.data(), count, &count, &cw, &ch);
        }
        unsigned long long sum = 0;
        if (rc == IMP_OK)
            for (int f = 0; f < count; f++) {
                const impgpu_gif_desc& d = recs[(size_t)f];
                const long long v[] = {d.left, d.top, d.width, d.height, d.interlaced, d.dispose, d.transparency_key, d.time_ms, (long long)d.palette_at,
                                       d.palette_entries, d.min_code_size, (long long)d.data_at, (long long)d.data_bytes};
                for (long long x : v) sum = mix(sum, (unsigned long long)x);
            }
        std::printf("%d %d %d %d %llu", rc, count, cw, ch, sum);
        for (int how = 0; how < 2; how++) {
            size_t need = 0;
            int rcp = imp::gif_pages_host(blob, file.size(), how, nullptr, 0, &need);
            unsigned long long psum = 0;
            if (rcp == IMP_ERROR_MALLOC_FAILED && need <= (size_t(64) << 20)) {
                unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
                for (size_t i = 0; i < need; i++) out[i] = 0xA5;
                rcp = imp::gif_pages_host(blob, file.size(), how, out, need, &need);
                if (rcp == IMP_OK)
                    for (size_t i = 0; i < need; i++) psum = mix(psum, out[i]);
                std::free(out);
            }
            std::printf(" %d %llu", rcp, psum);
        }
        std::printf("\n");
        std::free(blob);
    }
    return 0;
}
