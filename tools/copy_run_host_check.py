#!/usr/bin/env python3
"""copy_run16 (csrc/imp_internal.h) as HOST code under AddressSanitizer: a stand-alone program, built here from the header's
own text, calls it for every source alignment (0..3), destination alignment (0..3), row length 1..70 and source pitch with
0..3 spare bytes.  The source rows live in an exact-size heap block, so a load of a byte before the first row or behind the
last ends the run; every row must arrive byte for byte and every destination byte outside a row must keep its fill.  No GPU.
    python tools/copy_run_host_check.py"""
import os, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc", "imp_internal.h")
CLANG = os.environ.get("CXX_HOST") or "/opt/rocm/llvm/bin/clang++"      # (the vector extension types are clang's)

text = open(HEADER).read()
i = text.index("__device__ __forceinline__ uint32_t row_dword")
j = text.index("#endif", i)
body = text[i:j].replace("__device__ __forceinline__", "static inline")
program = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
// v_alignbyte_b32: the low dword of {hi, lo} >> 8 * (s & 3)
static inline uint32_t __builtin_amdgcn_alignbyte(uint32_t hi, uint32_t lo, unsigned s) {
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * (s & 3)));
}
""" + body + r"""
int main() {
    long cases = 0;
    for (int soff = 0; soff < 4; soff++)
        for (int doff = 0; doff < 4; doff++)
            for (int n = 1; n <= 70; n++)
                for (int spare = 0; spare < 4; spare++) {
                    const int h = 3, sstep = n + spare, dstep = ((n + 3) & ~3) + 4;
                    // malloc returns 16-byte aligned memory: the first row starts `soff` bytes into a block that ends with
                    // the last row's last byte, and the rows between start at every alignment the pitch gives them
                    const size_t slen = (size_t)soff + (size_t)sstep * (h - 1) + n;
                    uint8_t* sp = (uint8_t*)malloc(slen);
                    for (size_t b = 0; b < slen; b++) sp[b] = (uint8_t)rand();
                    std::vector<uint8_t> dst((size_t)dstep * h + 8, 0xA5);
                    uint8_t* d0 = dst.data();
                    while (((uintptr_t)d0 & 3) != (unsigned)doff) d0++;
                    const int chunks = (n + 15) / 16;
                    for (int y = 0; y < h; y++)
                        for (int k = 0; k <= chunks; k++)          // (one lane past the row's end, as a full workgroup has)
                            copy_run16(sp + soff + (size_t)y * sstep, d0 + (size_t)y * dstep, n, k);
                    for (int y = 0; y < h; y++) {
                        if (memcmp(d0 + (size_t)y * dstep, sp + soff + (size_t)y * sstep, n)) { printf("row differs: soff %d doff %d n %d y %d\n", soff, doff, n, y); return 1; }
                        for (int b = n; b < dstep && (size_t)y * dstep + b < (size_t)dstep * h; b++)
                            if (d0[(size_t)y * dstep + b] != 0xA5) { printf("stored outside a row: soff %d doff %d n %d y %d byte %d\n", soff, doff, n, y, b); return 1; }
                    }
                    free(sp);
                    cases++;
                }
    printf("copy_run16: %ld cases, every row equal, no byte outside a row read or written\n", cases);
    return 0;
}
"""
with tempfile.TemporaryDirectory() as d:
    src, exe = os.path.join(d, "copy_run_host_check.cpp"), os.path.join(d, "copy_run_host_check")
    open(src, "w").write(program)
    subprocess.check_call([CLANG, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize=alignment", "-o", exe, src])
    sys.exit(subprocess.call([exe]))
