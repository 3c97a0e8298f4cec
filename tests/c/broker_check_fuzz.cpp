// broker_check_fuzz.cpp -- impb::check_gif (csrc/imp_broker_check.h) on seeded mutations of valid IMPB_IN_GIF inputs, for
// tests/test_broker_album_host.py, which compiles it with -fsanitize=address,undefined and holds every verdict against a
// slow check of its own.  The input lives in a heap block of EXACTLY in_bytes, so a read past it is a sanitizer report; for
// an accepted request every byte the records name is read as well, as the compose call would.
//   broker_check_fuzz <cases> <seed>
// One line per case: slot_bytes in_bytes in_pages in_page verdict nrec {indices_at palette_at width height pitch}*nrec
// (nrec = in_pages when the table is one the check may read -- 1..IMPB_MAX_GIF_PAGES records inside in_bytes -- else 0).
#include "imp_broker_check.h"

#include <cinttypes>
#include <cstdio>
#include <cstdlib>

static uint64_t g_state;
static uint64_t rnd() {                                    // xorshift64*
    g_state ^= g_state >> 12; g_state ^= g_state << 25; g_state ^= g_state >> 27;
    return g_state * 0x2545F4914F6CDD1DULL;
}
static int pick(int n) { return (int)(rnd() % (uint64_t)n); }

int main(int argc, char** argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 1000;
    g_state = argc > 2 ? strtoull(argv[2], nullptr, 10) | 1 : 88172645463325252ULL;
    unsigned long sink = 0;
    for (int c = 0; c < cases; c++) {
        // a valid input: records, then per page a palette and a plane
        int32_t pages = c % 97 == 0 ? IMPB_MAX_GIF_PAGES : 1 + pick(6);
        int32_t in_page = pick(4) == 0 ? pick(pages + 2) : -1;
        std::vector<impb_gif_page> rec((size_t)pages);
        uint64_t at = (uint64_t)pages * sizeof(impb_gif_page);
        for (impb_gif_page& p : rec) {
            p.width = 1 + pick(40); p.height = 1 + pick(30); p.pitch = p.width + pick(5);
            p.left = pick(9) - 4; p.top = pick(9) - 4; p.dispose = pick(4); p.transparency_key = pick(258) - 1; p.pad = 0;
            p.palette_at = at; at += 1024;
            p.indices_at = at; at += (uint64_t)p.pitch * (uint64_t)p.height;
        }
        uint64_t in_bytes = at;
        const uint64_t frames = in_page >= 0 ? 1 : (uint64_t)pages;
        const uint64_t answer = frames * (uint64_t)rec[0].width * 4 * (uint64_t)rec[0].height;
        uint64_t slot_bytes = ((in_bytes + 63) & ~uint64_t(63)) + answer + (uint64_t)pick(3) * 64;
        // one mutation (or none)
        impb_gif_page& v = rec[(size_t)pick(pages)];
        const uint64_t plane = (uint64_t)v.pitch * (uint64_t)v.height;
        switch (pick(24)) {
        case 0: v.indices_at = in_bytes - plane; break;                        // ends exactly at the end: fine
        case 1: v.indices_at = in_bytes - plane + 1; break;                    // one byte past it
        case 2: v.indices_at = in_bytes; break;
        case 3: v.indices_at = in_bytes + 1 + rnd() % 4096; break;
        case 4: v.indices_at = ~uint64_t(0) - plane + 1 + (uint64_t)pick(3); break;   // indices_at + plane wraps around 2^64
        case 5: v.indices_at = ~uint64_t(0) - (uint64_t)pick(2); break;
        case 6: v.palette_at = in_bytes - 1024; break;
        case 7: v.palette_at = in_bytes - 1023; break;
        case 8: v.palette_at = in_bytes; break;
        case 9: v.palette_at = ~uint64_t(0) - 1023 + (uint64_t)pick(1024); break;
        case 10: v.pitch = 0x7fffffff; v.height = 0x7fffffff; break;           // a plane of 2^62 bytes ...
        case 11: v.pitch = 0x7fffffff; v.height = 0x7fffffff; v.indices_at = ~uint64_t(0) - (uint64_t(1) << 61); break;   // ... that wraps
        case 12: pages = 0; break;
        case 13: pages = IMPB_MAX_GIF_PAGES + 1; break;                        // (the table is not even inside in_bytes)
        case 14: pages = -1 - pick(3); break;
        case 15: v.width = -v.width; break;
        case 16: v.height = pick(2) ? 0 : -v.height; break;
        case 17: v.pitch = pick(2) ? v.width - 1 : -v.pitch; break;
        case 18: in_page = -2 - pick(3); break;
        case 19: in_page = 0x7fffffff; break;
        case 20: slot_bytes = ((in_bytes + 63) & ~uint64_t(63)) + answer - 1; break;   // the answer is one byte too large
        case 21: slot_bytes = ((in_bytes + 63) & ~uint64_t(63)) + answer; break;       // ... and fits exactly
        case 22: slot_bytes = in_bytes - 1 - (uint64_t)pick(64); break;        // in_bytes past the slot
        default: break;
        }
        uint8_t* in = (uint8_t*)malloc((size_t)in_bytes);
        if (!in) return 3;
        for (uint64_t i = 0; i < in_bytes; i++) in[i] = (uint8_t)(i * 7 + (uint64_t)c);
        memcpy(in, rec.data(), rec.size() * sizeof(impb_gif_page));
        std::vector<impb_gif_page> table;
        int got_frames = -1;
        uint64_t frame_bytes = 0;
        const impb::GifVerdict verdict = impb::check_gif(in, in_bytes, slot_bytes, pages, in_page, &table, &got_frames, &frame_bytes);
        if (verdict == impb::GIF_OK) {
            if (table.size() != (size_t)pages) return 4;
            for (const impb_gif_page& p : table) {
                for (uint64_t i = 0; i < (uint64_t)p.pitch * (uint64_t)p.height; i++) sink += in[p.indices_at + i];
                for (uint64_t i = 0; i < 1024; i++) sink += in[p.palette_at + i];
            }
            if ((uint64_t)got_frames != (in_page >= 0 ? 1 : (uint64_t)pages) || frame_bytes != (uint64_t)table[0].width * 4 * (uint64_t)table[0].height) return 5;
        }
        const bool readable = pages >= 1 && pages <= IMPB_MAX_GIF_PAGES && (uint64_t)pages * sizeof(impb_gif_page) <= in_bytes && (size_t)pages <= rec.size();
        printf("%" PRIu64 " %" PRIu64 " %d %d %d %d", slot_bytes, in_bytes, pages, in_page, (int)verdict, readable ? pages : 0);
        if (readable)
            for (int i = 0; i < pages; i++)
                printf(" %" PRIu64 " %" PRIu64 " %d %d %d", rec[(size_t)i].indices_at, rec[(size_t)i].palette_at, rec[(size_t)i].width, rec[(size_t)i].height, rec[(size_t)i].pitch);
        printf("\n");
        free(in);
    }
    fprintf(stderr, "sink %lu\n", sink);
    return 0;
}
