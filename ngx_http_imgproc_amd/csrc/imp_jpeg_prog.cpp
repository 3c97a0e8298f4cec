// imp_jpeg_prog.cpp -- host side of the progressive JPEG front (imp_jpeg_prog.h): every scan unstuffed into one staging
// area and cut into items, the tables the kernels read, a plain sequential decoder of the whole file (the reference the
// lane code is checked against) and the lane code run item by item.  No HIP runtime calls: builds with g++ for the
// sanitizer fuzz (tests/c/).  The marker walk itself is jpeg_parse_ex in imp_jpeg.cpp.
#include <algorithm>
#include <cstring>
#include "imp_jpeg_prog.h"

namespace imp {

size_t jpeg_prog_capacity(const JpegProg& P) {
    // every interval: its bytes, up to 3 bytes to the word boundary, the guard words
    return P.data_bytes + P.max_items * (4 + 4 * JPEG_PROG_GUARD_WORDS) + 64;
}

int jpeg_prog_prepare(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, uint8_t* out, size_t cap,
                      std::vector<JpegProgItem>* items, std::vector<uint32_t>* level_first) {
    (void)H;
    items->clear();
    size_t o = 0;
    for (size_t si = 0; si < P.scans.size(); si++) {
        const JpegProgScan& sc = P.scans[si];
        if (sc.data_end > size || sc.data_begin > sc.data_end) return IMP_ERROR_DECODE_FAILED;
        size_t at = sc.data_begin, seg_begin = o;
        uint32_t seg = 0;
        int expect_rst = 0;
        auto close_segment = [&]() -> bool {
            if (o == seg_begin || seg >= sc.nsegs) return false;     // an interval with no data, or one more than the scan has units for
            const uint32_t per = sc.restart_interval ? (uint32_t)sc.restart_interval : sc.nunits;
            const uint32_t unit0 = seg * per, n = std::min(per, sc.nunits - unit0);
            if ((uint64_t)(o - seg_begin) * 8 >= (1ull << 32) || seg_begin / 4 >= (1ull << 32)) return false;
            items->push_back(JpegProgItem{0u, (uint32_t)si, (uint32_t)(seg_begin / 4), (uint32_t)((o - seg_begin) * 8), unit0, n});
            const size_t padded = (o + 3) / 4 * 4 + 4 * JPEG_PROG_GUARD_WORDS;
            std::memset(out + o, 0xFF, padded - o);
            o = seg_begin = padded;
            seg++;
            return true;
        };
        while (at < sc.data_end) {
            const uint8_t* ff = (const uint8_t*)std::memchr(blob + at, 0xFF, sc.data_end - at);
            const size_t run = (ff ? (size_t)(ff - blob) : sc.data_end) - at;
            if (o + run + 16 + 4 * JPEG_PROG_GUARD_WORDS > cap) return IMP_ERROR_DECODE_FAILED;
            std::memcpy(out + o, blob + at, run);
            o += run;
            at += run;
            if (!ff) break;
            size_t m = at + 1;
            while (m < sc.data_end && blob[m] == 0xFF) m++;           // fill bytes
            if (m >= sc.data_end) break;                              // (the FF of the marker that ends the scan is data_end itself)
            const int code = blob[m];
            if (code == 0x00 && m == at + 1) {
                out[o++] = 0xFF;
                at = m + 1;
            } else if (code >= 0xD0 && code <= 0xD7) {
                if (!sc.restart_interval || code != 0xD0 + expect_rst) return IMP_ERROR_DECODE_FAILED;
                if (!close_segment()) return IMP_ERROR_DECODE_FAILED;
                expect_rst = (expect_rst + 1) & 7;
                at = m + 1;
            } else return IMP_ERROR_DECODE_FAILED;                    // FF FF 00 and the like: not a sequence an encoder writes
        }
        if (o + 16 + 4 * JPEG_PROG_GUARD_WORDS > cap) return IMP_ERROR_DECODE_FAILED;
        if (o != seg_begin) { if (!close_segment()) return IMP_ERROR_DECODE_FAILED; }
        if (seg != sc.nsegs) return IMP_ERROR_DECODE_FAILED;          // intervals missing (a marker behind the last one is allowed: nothing follows it)
    }
    // by level, then by decoder kind: a wave's lanes run the same decoder
    std::stable_sort(items->begin(), items->end(), [&](const JpegProgItem& a, const JpegProgItem& b) {
        const JpegProgScan &x = P.scans[a.scan], &y = P.scans[b.scan];
        return x.level != y.level ? x.level < y.level : x.kind < y.kind;
    });
    level_first->assign((size_t)P.nlevels + 1, 0u);
    for (const JpegProgItem& it : *items) (*level_first)[(size_t)P.scans[it.scan].level + 1]++;
    for (int l = 0; l < P.nlevels; l++) (*level_first)[(size_t)l + 1] += (*level_first)[(size_t)l];
    return IMP_OK;
}

void jpeg_prog_file_dev(const JpegHeader& H, const JpegFrame& F, JpegProgFileDev* D) {
    std::memset(D, 0, sizeof *D);
    D->ncomp = H.ncomp; D->mcux = H.mcux; D->mcuy = H.mcuy;
    for (int i = 0; i < 3; i++) { D->h[i] = D->v[i] = D->bw[i] = D->cbw[i] = D->cbh[i] = 1; }
    for (int i = 0; i < H.ncomp; i++) {
        D->h[i] = H.comp[i].h; D->v[i] = H.comp[i].v; D->bw[i] = H.comp[i].bw;
        D->cbw[i] = (H.comp[i].dsw + 7) / 8; D->cbh[i] = (H.comp[i].dsh + 7) / 8;
        D->coef_off[i] = F.coef_off[i];
    }
    D->total_slots = F.total_slots;
}

void jpeg_prog_scans_dev(const JpegProg& P, JpegProgScanDev* out) {
    for (size_t i = 0; i < P.scans.size(); i++) {
        const JpegProgScan& s = P.scans[i];
        JpegProgScanDev d{};
        d.ncomp = (uint8_t)s.ncomp; d.ss = (uint8_t)s.ss; d.se = (uint8_t)s.se; d.ah = (uint8_t)s.ah; d.al = (uint8_t)s.al; d.kind = (uint8_t)s.kind;
        for (int k = 0; k < 3; k++) { d.comp[k] = (uint8_t)(k < s.ncomp ? s.comp[k] : 0); d.tab[k] = (uint8_t)(k < s.ncomp ? s.tab[k] : 0); }
        out[i] = d;
    }
}

int jpeg_prog_emulate(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, const JpegFrame& F, int16_t* coef, unsigned* status) {
    std::vector<uint8_t> buf((jpeg_prog_capacity(P) + 3) / 4 * 4);
    std::vector<JpegProgItem> items;
    std::vector<uint32_t> level_first;
    if (int rc = jpeg_prog_prepare(blob, size, H, P, buf.data(), buf.size(), &items, &level_first)) return rc;
    std::vector<JpegHuffDev> tabs(P.tables.size() + 1);
    for (size_t k = 0; k < P.tables.size(); k++)
        if (int rc = jpeg_build_table(P.tables[k], P.table_is_dc[k] != 0, &tabs[k])) return rc;
    std::vector<JpegProgScanDev> scans(P.scans.size());
    jpeg_prog_scans_dev(P, scans.data());
    JpegProgFileDev D;
    jpeg_prog_file_dev(H, F, &D);
    D.coef = coef;
    D.tables = tabs.data();
    D.scans = scans.data();
    const uint8_t* bytes = buf.data();
    *status = 0;
    for (const JpegProgItem& it : items) {                            // (sorted by level: the order the launches give)
        const uint8_t* base = bytes + (size_t)it.word0 * 4;
        auto word = [base](uint32_t i) -> uint32_t {
            const uint8_t* q = base + (size_t)i * 4;
            return ((uint32_t)q[3] << 24) | ((uint32_t)q[2] << 16) | ((uint32_t)q[1] << 8) | q[0];
        };
        *status |= jpeg_prog_item(D, scans[it.scan], word, it.nbits, it.unit0, it.nunits);
    }
    return IMP_OK;
}

// ---- the reference: the file's bytes as they are, scan after scan, one bit at a time (T.81 annex G read literally; codes
// looked up by the canonical limits of annex F.2.2.3 -- no table shared with the lane code but the DHT content)
namespace {
const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                             41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                             30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct RefBits {
    const uint8_t* p;
    size_t at, end;
    int left = 0;            // bits of `cur` not yet given out
    unsigned cur = 0;
    bool bad = false;
    int bit() {
        if (left == 0) {
            if (at >= end) { bad = true; return 0; }
            cur = p[at++];
            if (cur == 0xFF) {
                if (at < end && p[at] == 0x00) at++;
                else { bad = true; return 0; }                        // a marker inside the interval
            }
            left = 8;
        }
        left--;
        return (int)(cur >> left) & 1;
    }
    int bits(int n) { int v = 0; for (int i = 0; i < n; i++) v = (v << 1) | bit(); return v; }
};
struct RefTable {
    int mincode[17], maxcode[17], valptr[17];
    const uint8_t* vals;
    bool ok = true;
    explicit RefTable(const JpegHuffSpec& t) : vals(t.vals) {
        int code = 0, k = 0;
        for (int l = 1; l <= 16; l++) {
            valptr[l] = k; mincode[l] = code;
            code += t.bits[l]; k += t.bits[l];
            maxcode[l] = t.bits[l] ? code - 1 : -1;
            if (code > (1 << l)) ok = false;
            code <<= 1;
        }
    }
    int symbol(RefBits& b) const {
        int code = 0;
        for (int l = 1; l <= 16; l++) {
            code = (code << 1) | b.bit();
            if (b.bad) return -1;
            if (maxcode[l] >= 0 && code <= maxcode[l] && code >= mincode[l]) return vals[valptr[l] + code - mincode[l]];
        }
        return -1;
    }
};
inline int ref_extend(int v, int s) { return s == 0 ? 0 : (v < (1 << (s - 1)) ? v - (1 << s) + 1 : v); }
}  // namespace

int jpeg_prog_reference(const uint8_t* blob, size_t size, const JpegHeader& H, const JpegProg& P, const JpegFrame& F, int16_t* coef) {
    for (const JpegProgScan& sc : P.scans) {
        if (sc.data_end > size) return IMP_ERROR_DECODE_FAILED;
        std::vector<RefTable> T;
        for (int i = 0; i < sc.ncomp; i++) {
            if (sc.kind == JPEG_PROG_DC_REFINE) break;
            T.emplace_back(P.tables[(size_t)sc.tab[i]]);
            if (!T.back().ok) return IMP_ERROR_DECODE_FAILED;
            if (sc.kind == JPEG_PROG_DC_FIRST)
                for (int k = 0; k < P.tables[(size_t)sc.tab[i]].nvals; k++) if (P.tables[(size_t)sc.tab[i]].vals[k] > 15) return IMP_ERROR_DECODE_FAILED;
        }
        // the interval boundaries: RSTn markers in order
        std::vector<std::pair<size_t, size_t>> segs;
        {
            size_t a = sc.data_begin, q = a;
            int expect = 0;
            while (q + 1 < sc.data_end) {
                if (blob[q] != 0xFF) { q++; continue; }
                size_t m = q + 1;
                while (m < sc.data_end && blob[m] == 0xFF) m++;
                if (m >= sc.data_end) break;
                if (blob[m] == 0x00 && m == q + 1) { q = m + 1; continue; }
                if (blob[m] >= 0xD0 && blob[m] <= 0xD7) {
                    if (!sc.restart_interval || blob[m] != 0xD0 + expect) return IMP_ERROR_DECODE_FAILED;
                    expect = (expect + 1) & 7;
                    segs.push_back({a, q});
                    a = q = m + 1;
                    continue;
                }
                return IMP_ERROR_DECODE_FAILED;
            }
            if (a < sc.data_end) segs.push_back({a, sc.data_end});
        }
        if (segs.size() != sc.nsegs) return IMP_ERROR_DECODE_FAILED;
        const uint32_t per = sc.restart_interval ? (uint32_t)sc.restart_interval : sc.nunits;
        for (size_t sg = 0; sg < segs.size(); sg++) {
            if (segs[sg].first == segs[sg].second) return IMP_ERROR_DECODE_FAILED;
            RefBits b{blob, segs[sg].first, segs[sg].second};
            int pred[3] = {0, 0, 0};
            unsigned eobrun = 0;
            const uint32_t u0 = (uint32_t)sg * per, u1 = std::min(sc.nunits, u0 + per);
            for (uint32_t u = u0; u < u1; u++) {
                // the unit's blocks
                for (int i = 0; i < sc.ncomp; i++) {
                    const JpegComp& c = H.comp[sc.comp[i]];
                    const int hh = sc.ncomp == 1 ? 1 : c.h, vv = sc.ncomp == 1 ? 1 : c.v;
                    for (int by = 0; by < vv; by++)
                        for (int bx = 0; bx < hh; bx++) {
                            size_t row, col;
                            if (sc.ncomp == 1) { const uint32_t cbw = (uint32_t)(c.dsw + 7) / 8; row = u / cbw; col = u % cbw; }
                            else { row = (size_t)(u / (uint32_t)H.mcux) * (size_t)vv + (size_t)by; col = (size_t)(u % (uint32_t)H.mcux) * (size_t)hh + (size_t)bx; }
                            int16_t* blk = coef + F.coef_off[sc.comp[i]] + (row * (size_t)c.bw + col) * 64;
                            if (sc.kind == JPEG_PROG_DC_FIRST) {
                                const int s = T[(size_t)i].symbol(b);
                                if (s < 0 || s > 15) return IMP_ERROR_DECODE_FAILED;
                                pred[i] += ref_extend(b.bits(s), s);
                                blk[0] = (int16_t)(pred[i] * (1 << sc.al));
                            } else if (sc.kind == JPEG_PROG_DC_REFINE) {
                                if (b.bit()) blk[0] = (int16_t)(blk[0] | (1 << sc.al));
                            } else if (sc.kind == JPEG_PROG_AC_FIRST) {
                                if (eobrun) { eobrun--; continue; }
                                for (int k = sc.ss; k <= sc.se; k++) {
                                    const int rs = T[0].symbol(b);
                                    if (rs < 0) return IMP_ERROR_DECODE_FAILED;
                                    const int r = rs >> 4, s = rs & 15;
                                    if (s) {
                                        k += r;
                                        if (k > sc.se) return IMP_ERROR_DECODE_FAILED;
                                        blk[kZigzag[k]] = (int16_t)(ref_extend(b.bits(s), s) * (1 << sc.al));
                                    } else if (r == 15) {
                                        k += 15;
                                        if (k > sc.se) return IMP_ERROR_DECODE_FAILED;
                                    } else {
                                        eobrun = (1u << r) + (unsigned)b.bits(r) - 1;
                                        break;
                                    }
                                }
                            } else {
                                const int p1 = 1 << sc.al;
                                int k = sc.ss;
                                auto correct = [&](int16_t& c2) {
                                    if (b.bit() && (c2 & p1) == 0) c2 = (int16_t)(c2 + (c2 > 0 ? p1 : -p1));
                                };
                                if (!eobrun) {
                                    while (k <= sc.se) {
                                        const int rs = T[0].symbol(b);
                                        if (rs < 0) return IMP_ERROR_DECODE_FAILED;
                                        int r = rs >> 4;
                                        const int s = rs & 15;
                                        int val = 0;
                                        if (s) {
                                            if (s != 1) return IMP_ERROR_DECODE_FAILED;
                                            val = b.bit() ? p1 : -p1;
                                        } else if (r != 15) {
                                            eobrun = (1u << r) + (unsigned)b.bits(r);
                                            break;
                                        }
                                        bool placed = false;
                                        for (; k <= sc.se && !placed; k++) {
                                            int16_t& c2 = blk[kZigzag[k]];
                                            if (c2) correct(c2);
                                            else if (r-- == 0) { if (s) c2 = (int16_t)val; placed = true; }
                                        }
                                        if (!placed) return IMP_ERROR_DECODE_FAILED;
                                    }
                                }
                                if (eobrun) {
                                    for (; k <= sc.se; k++) if (blk[kZigzag[k]]) correct(blk[kZigzag[k]]);
                                    eobrun--;
                                }
                            }
                            if (b.bad) return IMP_ERROR_DECODE_FAILED;
                        }
                }
            }
            if (eobrun) return IMP_ERROR_DECODE_FAILED;
            // what is left must be the encoder's padding: fewer than 8 bits
            size_t rest = 0;
            for (size_t q = b.at; q < b.end; q++) { rest++; if (blob[q] == 0xFF) q++; }
            if (rest) return IMP_ERROR_DECODE_FAILED;
        }
    }
    return IMP_OK;
}

}  // namespace imp

using namespace imp;

extern "C" {

int impgpu_jpeg_info_ex(const unsigned char* blob, size_t size, int accept, int* width, int* height, int* channels) {
    JpegHeader H;
    JpegProg P;
    if (int rc = jpeg_parse_ex(blob, size, &H, (accept & IMPGPU_JPEG_PROGRESSIVE) ? &P : nullptr)) return rc;
    if (width) *width = H.width;
    if (height) *height = H.height;
    if (channels) *channels = H.ncomp;
    return IMP_OK;
}

int impgpu_jpeg_coefficients_ex(const unsigned char* blob, size_t size, int how, int accept, short* out, size_t capacity, int* info) {
    if (!blob || !out) return IMP_ERROR_INVALID_ARGS;
    JpegHeader H;
    JpegProg P;
    if (int rc = jpeg_parse_ex(blob, size, &H, (accept & IMPGPU_JPEG_PROGRESSIVE) ? &P : nullptr)) return rc;
    if (P.scans.empty()) return impgpu_jpeg_coefficients(blob, size, how, out, capacity, info);
    JpegFrame F;
    int dc_ids[2], ac_ids[2];
    for (int i = 0; i < H.ncomp; i++) H.comp[i].td = H.comp[i].ta = 0;       // (a progressive file's tables belong to its scans)
    if (int rc = jpeg_frame_setup(H, &F, dc_ids, ac_ids)) return rc;
    if ((size_t)F.total_slots > capacity) return IMP_ERROR_INVALID_ARGS;
    std::memset(out, 0, (size_t)F.total_slots * sizeof(short));
    unsigned status = 0;
    const int rc0 = how == 0 ? jpeg_prog_reference(blob, size, H, P, F, out) : jpeg_prog_emulate(blob, size, H, P, F, out, &status);
    if (info) {
        info[0] = (int)F.total_slots; info[1] = (int)status; info[2] = P.nlevels;
        for (int i = 0; i < 3; i++) { info[3 + i] = (int)F.coef_off[i]; info[6 + i] = F.bw[i]; info[9 + i] = F.bh[i]; }
    }
    return rc0 ? rc0 : status ? IMP_ERROR_DECODE_FAILED : IMP_OK;
}

}  // extern "C"
