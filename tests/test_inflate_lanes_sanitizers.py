"""csrc/imp_inflate_lanes.h (the device inflate's lanes, run on the host one after the other) under AddressSanitizer / UBSan:
tests/c/inflate_lanes_test.cpp has its own main and is built with g++ -fsanitize=address,undefined -- seeded random streams
of every block type and content class at the exact size, at fewer and at more bytes than they hold, cut at random places
and with random bits flipped; every truncation and every single-bit flip of four small streams; the header's 2 x 256 values.
The input lies in a heap block of exactly the capacity the lanes are told they may read and the output in one of exactly
out_size bytes, so a read or a write outside either ends the run.  The verdict must be imp::inflate_exact's on every input
and zlib's wherever zlib delivers the bytes.  CPU only: nothing is loaded into Python under a sanitizer."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "inflate_lanes_test_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "inflate_lanes_test.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("imp_inflate_lanes.h", "imp_inflate.h", "imp_inflate.cpp")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + CSRC, src, os.path.join(CSRC, "imp_inflate.cpp"), "-lz", "-o", DRIVER])


def test_the_lanes_match_inflate_exact_and_zlib_under_sanitizers():
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER, "150"], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, (p.stdout[-2000:], p.stderr[-3000:])
    summary = [line for line in p.stdout.strip().splitlines() if line.endswith(" bad")][0]
    cases, bad = int(summary.split()[0]), int(summary.split()[2])
    assert cases > 20000 and bad == 0, summary
