"""The alpha route of the lossy WebP decoder -- the container walk, the ALPH header, the headerless lossless parse and
k_webp_alpha's lane code (csrc/imp_vp8_dec_host.h, imp_webp_alpha.h) -- under AddressSanitizer / UBSan:
tests/c/webp_alpha_test.cpp has its own main and is built with g++ -fsanitize=address,undefined.  It decodes every file of
tests/golden/webp_alpha_dec, seeded mutations and truncations of each (some aimed at the ALPH chunk) and every prefix of the
small files, with the file and the frame in heap blocks of exactly their sizes.  The frames' checksums must be those of
Pillow's frames.  CPU only: nothing is loaded into Python under a sanitizer."""
import os
import subprocess

import webp_alpha_dec_fixtures as F
from conftest import ROOT

CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "webp_alpha_test_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "webp_alpha_test.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("imp_webp_alpha.h", "imp_vp8_dec.h", "imp_vp8_dec_host.h", "imp_webp_lossy.h", "imp_webp_dec.h", "imp_webp_dec_host.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + CSRC, src, "-o", DRIVER])


def fnv(data):
    h = 1469598103934665603
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_the_alpha_route_and_the_lanes_under_sanitizers():
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER, F.HERE, "10"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    lines = p.stdout.strip().splitlines()
    cases, bad = int(lines[-1].split()[0]), int(lines[-1].split()[2])
    assert cases > 5000 and bad == 0, lines[-1]
    frames = {ln.split()[1]: int(ln.split()[2], 16) for ln in lines if ln.startswith("frame ")}
    fixtures = F.load()
    assert set(frames) == {name for name, _, _ in fixtures}
    small = [(name, e) for name, _, e in fixtures if e.size <= 70 * 66 * 4]              # (the checksum in Python: the small frames)
    assert len(small) > 100
    for name, expected in small:
        assert frames[name] == fnv(expected.tobytes()), name
    # the refused and damaged files were run, and gave the host model's codes from the route and from the info call
    codes = {ln.split()[1]: (int(ln.split()[2]), int(ln.split()[3])) for ln in lines if ln.startswith("code ")}
    want = {name: (F.IMP_ERROR_UNSUPPORTED,) * 2 for name, _ in F.refused()}
    want.update({name: (F.IMP_ERROR_DECODE_FAILED,) * 2 for name, _ in F.damaged()})
    assert codes == want
