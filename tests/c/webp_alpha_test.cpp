// webp_alpha_test.cpp -- the alpha route of the lossy WebP decoder (csrc/imp_vp8_dec_host.h: va_container, va_plane, the
// headerless lossless parse wd_parse_stream; csrc/imp_webp_alpha.h: what k_webp_alpha runs, one lane after the other) built
// with AddressSanitizer / UBSan (tests/test_webp_alpha_decode_sanitizers.py).  Every file of tests/golden/webp_alpha_dec,
// then seeded single-byte mutations and truncations of each, mutations aimed at the ALPH chunk, and every prefix of the
// small files.  The file lies in a heap block of exactly its size and the frame in one of exactly width * height * 4 bytes:
// a read or a write outside either ends the run.
//   webp_alpha_test_asan <fixture directory> [mutations per file]
// prints "frame <name> <fnv-1a 64 of the frame>" per fixture, "code <name> <code> <info code>" per refused or damaged
// file, then "<cases> cases, <bad> bad" (bad: a fixture that did not decode, a frame whose size is not the header's, a
// foreign code, an info call that disagrees with the route).
#include "imp_vp8_dec_host.h"
#include <dirent.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
using namespace imp;

static unsigned rnd_state = 90210;
static unsigned rnd() { rnd_state = rnd_state * 1664525u + 1013904223u; return rnd_state >> 8; }
static long cases = 0, bad = 0;
static const int ACCEPT = IMPGPU_WEBP_ACCEPT_LOSSY | IMPGPU_WEBP_ACCEPT_ALPHA;

static std::vector<uint8_t> slurp(const std::string& path) {
    std::vector<uint8_t> v;
    if (FILE* f = fopen(path.c_str(), "rb")) {
        uint8_t buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
        fclose(f);
    }
    return v;
}

// one input: the file in exactly `n` bytes of heap, the frame in exactly what the header asks for; -> the code
static int run(const uint8_t* data, size_t n, uint64_t* fnv, int* info_code) {
    cases++;
    uint8_t* blob = (uint8_t*)malloc(n ? n : 1);
    if (n) memcpy(blob, data, n);
    int w = 0, h = 0;
    size_t cap = 0;
    if (vd_info(blob, n, ACCEPT, &w, &h) == IMP_OK) cap = std::min<size_t>((size_t)w * (size_t)h * 4u, (size_t)1 << 22);   // (a mutated size: bounded)
    uint8_t* out = (uint8_t*)malloc(cap ? cap : 1);
    int ww = 0, hh = 0, info[IMPGPU_WEBP_DEC_INFO_WORDS], ainfo[4] = {0, 0, 0, 0};
    const int rc = vd_decode_host_any(blob, n, ACCEPT, out, cap, &ww, &hh, info);
    const int arc = va_info(blob, n, ainfo);
    if (info_code) *info_code = arc;
    if (rc == IMP_OK) {
        if (ww != w || hh != h) bad++;
        if (arc != IMP_OK && arc != IMP_ERROR_UNSUPPORTED) bad++;         // a file that decodes has a sound plane or none
        uint64_t hsh = 1469598103934665603ull;
        for (size_t i = 0; i < (size_t)w * (size_t)h * 4u; i++) hsh = (hsh ^ out[i]) * 1099511628211ull;
        if (fnv) *fnv = hsh;
    } else if (rc != IMP_ERROR_UNSUPPORTED && rc != IMP_ERROR_DECODE_FAILED && rc != IMP_ERROR_MALLOC_FAILED) {
        bad++;
    }
    // without the new bit the file is what it was: a file with an ALPH chunk in front of its image is refused
    (void)vd_decode_host_any(blob, n, IMPGPU_WEBP_ACCEPT_LOSSY, out, cap, &ww, &hh, info);
    free(out);
    free(blob);
    return rc;
}

// where the ALPH chunk's payload lies in a canonical file (0: none)
static size_t alph_at(const std::vector<uint8_t>& b, size_t* n) {
    for (size_t at = 12; at + 8 <= b.size();) {
        const size_t len = (size_t)b[at + 4] | (size_t)b[at + 5] << 8 | (size_t)b[at + 6] << 16 | (size_t)b[at + 7] << 24;
        if (!memcmp(&b[at], "ALPH", 4)) { *n = std::min(len, b.size() - at - 8); return at + 8; }
        at += 8 + len + (len & 1);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string dir = argv[1];
    const int mutations = argc > 2 ? atoi(argv[2]) : 12;
    std::vector<std::string> names;
    if (DIR* d = opendir(dir.c_str())) {
        while (dirent* e = readdir(d)) {
            const std::string f = e->d_name;
            if (f.size() > 5 && f.substr(f.size() - 5) == ".webp") names.push_back(f.substr(0, f.size() - 5));
        }
        closedir(d);
    }
    std::sort(names.begin(), names.end());
    for (const std::string& name : names) {
        const std::vector<uint8_t> blob = slurp(dir + "/" + name + ".webp");
        const bool fixture = name[1] == '_' && (name[0] == 'p' || name[0] == 'h');
        uint64_t fnv = 0;
        int arc = 0;
        const int rc = run(blob.data(), blob.size(), &fnv, &arc);
        if (fixture) {
            if (rc != IMP_OK) bad++;
            printf("frame %s %016llx\n", name.c_str(), (unsigned long long)fnv);
        } else {
            printf("code %s %d %d\n", name.c_str(), rc, arc);
        }
        const bool large = blob.size() > 20000;                          // (the 16383-long frames: fewer variants)
        size_t an = 0;
        const size_t aat = alph_at(blob, &an);
        std::vector<uint8_t> v;
        for (int k = 0; k < (large ? 2 : mutations); k++) {
            v = blob;
            v[rnd() % v.size()] ^= (uint8_t)(1u + rnd() % 255u);
            (void)run(v.data(), v.size(), nullptr, nullptr);
            (void)run(blob.data(), rnd() % blob.size(), nullptr, nullptr);
            if (aat && an) {                                             // the header byte, the stream's first bytes, anywhere in the chunk, its size
                v = blob;
                v[aat + (k < 4 ? (size_t)k % an : rnd() % an)] ^= (uint8_t)(1u + rnd() % 255u);
                (void)run(v.data(), v.size(), nullptr, nullptr);
                v = blob;
                v[aat - 4 + (size_t)(k & 1)] ^= (uint8_t)(1u + rnd() % 255u);
                (void)run(v.data(), v.size(), nullptr, nullptr);
            }
        }
        if (blob.size() < 400)
            for (size_t n = 0; n < blob.size(); n++) (void)run(blob.data(), n, nullptr, nullptr);
    }
    printf("%ld cases, %ld bad\n", cases, bad);
    return bad ? 1 : 0;
}
