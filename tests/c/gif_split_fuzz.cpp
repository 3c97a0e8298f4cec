// gif_split_fuzz.cpp -- the split route's host code under AddressSanitizer + UBSan (tests/test_gif_split_sanitizers.py):
// the scan that cuts a page at its clear codes, the length pass and the emit pass of csrc/imp_gif.h -- the lane code of
// k_gif_lzw_scan / _len / _emit, run one lane after the other -- see files somebody uploaded.  One file per line of stdin,
// in hex; one line of answers each: the code of impgpu_gif_pages_split's body, a checksum of the planes (0 unless the code
// is IMP_OK), the page count and a checksum of the pages' segment counts.  The planes are written into a heap block of
// exactly their size and the counts into one of exactly the page count, so a byte outside them is the sanitizer's to report.
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
        const size_t size = line.size() / 2;
        unsigned char* blob = (unsigned char*)std::malloc(size ? size : 1);
        for (size_t i = 0; i < size; i++) blob[i] = (unsigned char)std::stoi(line.substr(2 * i, 2), nullptr, 16);
        size_t need = 0;
        int rc = imp::gif_pages_split_host(blob, size, nullptr, 0, &need, nullptr, 0);
        unsigned long long psum = 0, ssum = 0;
        int count = 0;
        if (rc == IMP_ERROR_MALLOC_FAILED && need <= (size_t(64) << 20)) {
            int cw = 0, ch = 0;
            (void)impgpu_gif_walk(blob, size, nullptr, 0, &count, &cw, &ch);
            unsigned char* out = (unsigned char*)std::malloc(need ? need : 1);
            int* segs = (int*)std::malloc(sizeof(int) * (size_t)(count > 0 ? count : 1));
            for (size_t i = 0; i < need; i++) out[i] = 0xA5;
            for (int f = 0; f < count; f++) segs[f] = -7;
            rc = imp::gif_pages_split_host(blob, size, out, need, &need, segs, count);
            if (rc == IMP_OK)
                for (size_t i = 0; i < need; i++) psum = mix(psum, out[i]);
            for (int f = 0; f < count; f++) ssum = mix(ssum, (unsigned long long)(long long)segs[f]);
            std::free(segs);
            std::free(out);
        }
        std::printf("%d %llu %d %llu\n", rc, psum, count, ssum);
        std::free(blob);
    }
    return 0;
}
