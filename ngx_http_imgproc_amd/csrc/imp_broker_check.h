// imp_broker_check.h -- what the broker asks of an IMPB_IN_GIF request before anything reads through its records.
// Plain C++, no HIP, header only: imp_broker.cpp includes it, and tests/c/broker_check_fuzz.cpp compiles it on its own
// under the sanitizers.  The slot is shared memory that a worker may rewrite at any time: the record table is copied out
// ONCE, every check is made on the copy, and the copy is what the broker goes on to use.
#pragma once
#include <impgpu_broker.h>

#include <cstring>
#include <vector>

namespace impb {

enum GifVerdict {
    GIF_OK = 0,
    GIF_INVALID = 1,        // the request itself is wrong: IMP_ERROR_INVALID_ARGS at IMP_STEP_DECODE
    GIF_TOO_LARGE = 2,      // a sound request whose answer cannot lie behind it in the slot: the oversized answer's code
};

// `in` .. `in + in_bytes`: the request's input as the slot holds it; `slot_bytes`: the slot's whole data area.  On GIF_OK
// (and GIF_TOO_LARGE) *table holds the `in_pages` checked records, *frames the number of frames the compose call makes and
// *frame_bytes the size of one (the canvas is the first page's, four channels, rows of width * 4 bytes).
inline GifVerdict check_gif(const uint8_t* in, uint64_t in_bytes, uint64_t slot_bytes, int32_t in_pages, int32_t in_page,
                            std::vector<impb_gif_page>* table, int* frames, uint64_t* frame_bytes) {
    table->clear();
    if (in_bytes > slot_bytes) return GIF_INVALID;
    if (in_pages < 1 || in_pages > IMPB_MAX_GIF_PAGES || in_page < -1) return GIF_INVALID;
    const uint64_t table_bytes = (uint64_t)in_pages * sizeof(impb_gif_page);
    if (table_bytes > in_bytes) return GIF_INVALID;
    table->resize((size_t)in_pages);
    std::memcpy(table->data(), in, (size_t)table_bytes);
    for (const impb_gif_page& p : *table) {
        if (p.width <= 0 || p.height <= 0 || p.pitch <= 0 || p.pitch < p.width) return GIF_INVALID;
        const uint64_t plane = (uint64_t)p.pitch * (uint64_t)p.height;            // two positive 32-bit values: below 2^62
        if (p.indices_at > in_bytes || plane > in_bytes - p.indices_at) return GIF_INVALID;
        if (p.palette_at > in_bytes || 1024 > in_bytes - p.palette_at) return GIF_INVALID;
    }
    const impb_gif_page& first = (*table)[0];
    *frames = in_page >= 0 ? 1 : in_pages;
    *frame_bytes = (uint64_t)first.width * 4 * (uint64_t)first.height;            // below 2^64: 2^31 * 4 * 2^31
    const uint64_t out_offset = (in_bytes + 63) & ~uint64_t(63);
    if (out_offset > slot_bytes) return GIF_TOO_LARGE;
    if (*frame_bytes > (slot_bytes - out_offset) / (uint64_t)*frames) return GIF_TOO_LARGE;
    return GIF_OK;
}

}  // namespace impb
