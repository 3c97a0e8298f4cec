// fuzz_jpeg_prog.cpp -- driver for the AddressSanitizer + UBSan build of the progressive JPEG front's host code
// (imp_jpeg.cpp: the multi-scan marker walk and the progression checks; imp_jpeg_prog.cpp / imp_jpeg_prog.h: every scan
// unstuffed and cut into items, the plain decoder, and the device's lane code run item by item).  CPU only.
//
// stdin: one hex-encoded file per line  ->  rc of impgpu_jpeg_info_ex, rc of the plain decoder, rc of the lane code,
// a checksum of each decoder's coefficients
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "../../include/impgpu.h"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        // an exact-size heap copy: an over-read of the file by one byte is an AddressSanitizer report
        std::vector<unsigned char> file;
        for (size_t i = 0; i + 1 < line.size(); i += 2) file.push_back((unsigned char)std::strtol(line.substr(i, 2).c_str(), nullptr, 16));
        int w = 0, h = 0, c = 0;
        const int rci = impgpu_jpeg_info_ex(file.data(), file.size(), IMPGPU_JPEG_PROGRESSIVE, &w, &h, &c);
        int rc0 = rci, rc1 = rci, info[12] = {0};
        unsigned long long sum0 = 0, sum1 = 0;
        if (!rci && (long long)w * h <= 4000000) {
            // exact size too: one coefficient past the planes is a report
            const size_t cap = (size_t)((w + 15) / 16 * 16) * ((h + 15) / 16 * 16) * 3;
            std::vector<short> out(cap);
            rc0 = impgpu_jpeg_coefficients_ex(file.data(), file.size(), 0, IMPGPU_JPEG_PROGRESSIVE, out.data(), out.size(), info);
            if (!rc0) for (int i = 0; i < info[0]; i++) sum0 = sum0 * 31u + (unsigned short)out[(size_t)i];
            rc1 = impgpu_jpeg_coefficients_ex(file.data(), file.size(), 1, IMPGPU_JPEG_PROGRESSIVE, out.data(), out.size(), info);
            if (!rc1) for (int i = 0; i < info[0]; i++) sum1 = sum1 * 31u + (unsigned short)out[(size_t)i];
        }
        std::printf("%d %d %d %llu %llu\n", rci, rc0, rc1, sum0, sum1);
    }
    return 0;
}
