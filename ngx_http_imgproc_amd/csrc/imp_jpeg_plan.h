// imp_jpeg_plan.h -- where the arrays of one file's entropy work area lie (JpegJob's chunk_*, cand_*, rep_*, ext*, tabs,
// dcadd: imp_jpeg.h).  The one place that spells these offsets: imp_jpeg_api.cpp sizes the area, fills the job table and
// reads its traces back through it, and tests/c/jpeg_plan_check.cpp runs it under AddressSanitizer.  Host arithmetic only,
// no HIP call.
#pragma once
#include "imp_jpeg_core.h"

namespace imp {

struct JpegWorkLayout {                             // byte offsets from the file's work_off
    size_t chunk_entry, chunk_mid, chunk_n, chunk_nmid, chunk_slot0, chunk_dc, wg_dc;
    size_t cand_in, cand_out, rep_out, cand_mid, rep_mid;
    size_t cand_n, rep_n, cand_nmid, rep_nmid, cand_nib;
    size_t ext_idx, tabs, ext, dcadd;
    uint32_t ext_cap;                               // records `ext` has room for
    size_t bytes;                                   // the whole area: a multiple of 256, so that the next file's is aligned as well
};

// The arrays in the order the kernels were first handed them, laid out by a running cursor.  `reserved` is what the area is
// sized by: every array's length, and for every padding its worst case instead of what the offsets came to need -- a few
// dozen bytes more than the last array's end.  That is how the area has been sized since it exists; it stays, so that a
// launch asks the pool for the very bytes it always did.
inline JpegWorkLayout jpeg_work_layout(unsigned nchunks, unsigned wsplit, int bpm, unsigned total_slots) {
    const size_t NC = nchunks, NU = NC * wsplit, NB = NC * (size_t)bpm;
    size_t at = 0, reserved = 0, last = 0;
    auto take = [&](size_t count, size_t elem) { last = at; at += count * elem; reserved += count * elem; return last; };
    auto align = [&](size_t a) { at = (at + a - 1) / a * a; reserved += a; };                       // the next array starts on a multiple of `a`
    auto pad = [&](size_t a) { at = last + (at - last + a - 1) / a * a; reserved += a; };           // the last array's LENGTH becomes a multiple of `a`
    JpegWorkLayout L;
    L.chunk_entry = take(NC, 8);
    L.chunk_mid = take(NC, 8);
    L.chunk_n = take(NC, 4);
    L.chunk_nmid = take(NC, 4);
    L.chunk_slot0 = take(NU, 4);
    L.chunk_dc = take(NU * 4, sizeof(int));
    L.wg_dc = take((size_t)jpeg_entropy_blocks((unsigned)NU) * 8, sizeof(int));
    align(8);                                       // (the candidates' 64-bit states; an odd number of 4-byte entries can lie before them)
    L.cand_in = take(NB, 8);
    L.cand_out = take(NB, 8);
    L.rep_out = take(NB, 8);
    L.cand_mid = take(NB, 8);
    L.rep_mid = take(NB, 8);
    L.cand_n = take(NB, 4);
    L.rep_n = take(NB, 4);
    L.cand_nmid = take(NB, 4);
    L.rep_nmid = take(NB, 4);
    L.cand_nib = take(NB, 4);                       // a byte each is used: the area has always kept four, and ext_idx starts behind them
    L.ext_idx = take(NB, 4);
    L.tabs = take(1, sizeof(JpegHuffTabs));
    pad(64);
    static_assert(sizeof(JpegHuffTabs) % 64 == 0, "the tables end on their own 64-byte multiple: the padding behind them is none");
    L.ext_cap = (uint32_t)(NC / 8 + 16);
    L.ext = take((size_t)L.ext_cap * JPEG_EXT_WORDS, 4);
    pad(64);                                        // (of the records' length, not to a boundary: `tabs` starts on a multiple of 8 only)
    L.dcadd = take(((size_t)total_slots / 64 * 2 + 63) / 64 * 32, sizeof(int16_t));                 // a short per block, the length rounded up to 64 bytes
    L.bytes = (reserved + 255) / 256 * 256;
    return L;
}

inline void jpeg_job_bind_work(JpegJob& J, uint8_t* base, const JpegWorkLayout& L) {
    J.chunk_entry = (uint64_t*)(base + L.chunk_entry);
    J.chunk_mid = (uint64_t*)(base + L.chunk_mid);
    J.chunk_n = (uint32_t*)(base + L.chunk_n);
    J.chunk_nmid = (uint32_t*)(base + L.chunk_nmid);
    J.chunk_slot0 = (uint32_t*)(base + L.chunk_slot0);
    J.chunk_dc = (int*)(base + L.chunk_dc);
    J.wg_dc = (int*)(base + L.wg_dc);
    J.cand_in = (uint64_t*)(base + L.cand_in);
    J.cand_out = (uint64_t*)(base + L.cand_out);
    J.rep_out = (uint64_t*)(base + L.rep_out);
    J.cand_mid = (uint64_t*)(base + L.cand_mid);
    J.rep_mid = (uint64_t*)(base + L.rep_mid);
    J.cand_n = (uint32_t*)(base + L.cand_n);
    J.rep_n = (uint32_t*)(base + L.rep_n);
    J.cand_nmid = (uint32_t*)(base + L.cand_nmid);
    J.rep_nmid = (uint32_t*)(base + L.rep_nmid);
    J.cand_nib = base + L.cand_nib;
    J.ext_idx = (uint32_t*)(base + L.ext_idx);
    J.tabs = (JpegHuffTabs*)(base + L.tabs);
    J.ext = (uint32_t*)(base + L.ext);
    J.ext_cap = L.ext_cap;
    J.dcadd = (int16_t*)(base + L.dcadd);
}

}  // namespace imp
