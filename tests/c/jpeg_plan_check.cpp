// jpeg_plan_check.cpp -- the JPEG entropy work area's layout (csrc/imp_jpeg_plan.h) under AddressSanitizer + UBSan
// (tests/test_jpeg_plan_host.py builds and runs it; CPU only).  For a sweep of chunk counts, lanes per chunk, blocks per MCU
// and frame sizes: every array the kernels are handed lies inside the area at the length imp_jpeg.h documents for it, none
// overlaps another, each is aligned for its element; offsets and size are what the code computed before the layout had a
// header of its own; and every array is written from end to end through the pointers jpeg_job_bind_work sets, into a heap
// block of exactly `bytes`.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../ngx_http_imgproc_amd/csrc/imp_jpeg_plan.h"

using namespace imp;

namespace {

struct Arr { const char* name; size_t off, count, elem; void* ptr; };
size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }

int fail(const char* what, const char* name, unsigned nc, unsigned ws, int bpm, unsigned slots) {
    std::printf("FAIL %s %s: nchunks %u wsplit %u bpm %d total_slots %u\n", what, name, nc, ws, bpm, slots);
    return 1;
}

int check(unsigned nc, unsigned ws, int bpm, unsigned slots) {
    const JpegWorkLayout L = jpeg_work_layout(nc, ws, bpm, slots);
    const size_t NC = nc, NU = NC * ws, NB = NC * (size_t)bpm, EB = jpeg_entropy_blocks((unsigned)NU);
    // ---- the offsets and the size as commit 93cb3b7 spelt them (imp_jpeg_api.cpp:354-355 the size, :442-467 the pointers)
    const size_t cd = up(NC * 24 + NU * 20, 8) + EB * 32, tabs = cd + NB * 64, ext = tabs + up(sizeof(JpegHuffTabs), 64);
    const uint32_t ext_cap = (uint32_t)(NC / 8 + 16);
    const size_t dcadd = ext + up((size_t)ext_cap * JPEG_EXT_WORDS * 4, 64);
    const size_t bytes = up(NC * (24 + 20 * (size_t)ws + 64 * (size_t)bpm) + 8 + EB * 32 + sizeof(JpegHuffTabs) + 64 + ((size_t)NC / 8 + 16) * JPEG_EXT_WORDS * 4 +
                            up((size_t)slots / 64 * 2, 64) + 64, 256);
    const size_t was[21] = {0, NC * 8, NC * 16, NC * 20, NC * 24, NC * 24 + NU * 4, NC * 24 + NU * 20, cd, cd + NB * 8, cd + NB * 16, cd + NB * 24, cd + NB * 32,
                            cd + NB * 40, cd + NB * 44, cd + NB * 48, cd + NB * 52, cd + NB * 56, cd + NB * 60, tabs, ext, dcadd};
    JpegJob J;
    std::memset(&J, 0, sizeof J);
    // (the arithmetic checks need no memory: the largest areas are bound to a null base)
    const bool touch = nc <= 4096;
    uint8_t* base = touch ? (uint8_t*)std::malloc(L.bytes) : nullptr;
    if (touch && !base) return fail("malloc", "", nc, ws, bpm, slots);
    if (touch) jpeg_job_bind_work(J, base, L);
    // ---- the arrays at their documented lengths (imp_jpeg.h, JpegJob), in the order of `was`
    Arr A[21] = {
        {"chunk_entry", L.chunk_entry, NC, 8, J.chunk_entry}, {"chunk_mid", L.chunk_mid, NC, 8, J.chunk_mid}, {"chunk_n", L.chunk_n, NC, 4, J.chunk_n},
        {"chunk_nmid", L.chunk_nmid, NC, 4, J.chunk_nmid}, {"chunk_slot0", L.chunk_slot0, NU, 4, J.chunk_slot0}, {"chunk_dc", L.chunk_dc, NU * 4, sizeof(int), J.chunk_dc},
        {"wg_dc", L.wg_dc, EB * 8, sizeof(int), J.wg_dc}, {"cand_in", L.cand_in, NB, 8, J.cand_in}, {"cand_out", L.cand_out, NB, 8, J.cand_out},
        {"rep_out", L.rep_out, NB, 8, J.rep_out}, {"cand_mid", L.cand_mid, NB, 8, J.cand_mid}, {"rep_mid", L.rep_mid, NB, 8, J.rep_mid},
        {"cand_n", L.cand_n, NB, 4, J.cand_n}, {"rep_n", L.rep_n, NB, 4, J.rep_n}, {"cand_nmid", L.cand_nmid, NB, 4, J.cand_nmid},
        {"rep_nmid", L.rep_nmid, NB, 4, J.rep_nmid}, {"cand_nib", L.cand_nib, NB, 1, J.cand_nib}, {"ext_idx", L.ext_idx, NB, 4, J.ext_idx},
        {"tabs", L.tabs, 1, sizeof(JpegHuffTabs), J.tabs}, {"ext", L.ext, (size_t)L.ext_cap * JPEG_EXT_WORDS, 4, J.ext},
        {"dcadd", L.dcadd, (size_t)slots / 64, sizeof(int16_t), J.dcadd},
    };
    int bad = 0;
    if (L.bytes != bytes || L.bytes % 256) bad |= fail("bytes", "", nc, ws, bpm, slots);
    if (L.ext_cap != ext_cap) bad |= fail("ext_cap", "", nc, ws, bpm, slots);
    for (int i = 0; i < 21; i++) {
        const size_t align = A[i].elem > 8 ? alignof(JpegHuffTabs) : A[i].elem;
        if (A[i].off != was[i]) bad |= fail("moved", A[i].name, nc, ws, bpm, slots);
        if (A[i].off % align) bad |= fail("alignment", A[i].name, nc, ws, bpm, slots);
        if (A[i].off > L.bytes || A[i].count * A[i].elem > L.bytes - A[i].off) bad |= fail("outside", A[i].name, nc, ws, bpm, slots);
        if (touch && A[i].ptr != base + A[i].off) bad |= fail("bound elsewhere", A[i].name, nc, ws, bpm, slots);
    }
    std::vector<Arr> sorted(A, A + 21);
    std::sort(sorted.begin(), sorted.end(), [](const Arr& a, const Arr& b) { return a.off < b.off; });
    for (int i = 0; i + 1 < 21; i++)
        if (sorted[i].off + sorted[i].count * sorted[i].elem > sorted[i + 1].off) bad |= fail("overlap", sorted[i].name, nc, ws, bpm, slots);
    if (touch && J.ext_cap != ext_cap) bad |= fail("J.ext_cap", "", nc, ws, bpm, slots);
    // ---- every array written whole through the job's pointers: a byte past the block is AddressSanitizer's to report
    if (touch && !bad)
        for (int i = 0; i < 21; i++) std::memset(A[i].ptr, 0xA5, A[i].count * A[i].elem);
    std::free(base);
    return bad;
}

}  // namespace

int main() {
    const unsigned chunks[] = {1, 2, 7, 8, 9, 255, 256, 257, 511, 512, 513, 4096, 65537};
    const unsigned lanes[] = {1, 2};
    const int blocks[] = {1, 3, 4, 6};
    const unsigned slots[] = {64, 192, 64 * 6 * 5, 64 * 6 * 1021, 64u * ((1u << 20) + 1)};
    int bad = 0, n = 0;
    for (unsigned nc : chunks)
        for (unsigned ws : lanes)
            for (int bpm : blocks)
                for (unsigned sl : slots) { bad |= check(nc, ws, bpm, sl); n++; }
    std::printf("%s %d layouts\n", bad ? "FAILED" : "ok", n);
    return bad;
}
