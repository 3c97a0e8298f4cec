"""The GIF front's host code under AddressSanitizer + UBSan (the pattern of test_jpeg_prog_sanitizers.py): the container
walk and both LZW decoders -- the plain one and the device's lane code run on the host -- see the bytes of files somebody
uploaded.  tests/c/gif_fuzz.cpp has its own main, is built with g++ -fsanitize=address,undefined and fed the written
files and seeded damage of them; every verdict must equal what the regular library returns, and the planes go into a heap
block of exactly their size.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gif_decode_host import album_file, damaged_file, damaged_streams, pin_cases

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_gif.h"), os.path.join(ROOT, "include", "impgpu_gif.h"), os.path.join(ROOT, "include", "impgpu_broker.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(files):
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(f.hex() for f in files) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(files)
    return [[int(v) for v in line.split()] for line in out]


def checksum(data):
    s = 0
    for v in data:
        s = (s * 31 + v) & 0xFFFFFFFFFFFFFFFF
    return s


def check(files):
    for k, (f, (rc, count, cw, ch, _, rc0, sum0, rc1, sum1)) in enumerate(zip(files, drive(files))):
        want_rc, (n, w, h) = imp.gif_info(f)
        assert (rc, count, cw, ch) == (want_rc, n, w, h), k
        for how, got_rc, got_sum in ((0, rc0, sum0), (1, rc1, sum1)):
            want_rc, planes = imp.gif_pages(f, how)
            assert got_rc == want_rc, (k, how)
            if want_rc == 0:
                assert got_sum == checksum(planes), (k, how)


def seeded_damage(blob, seed, n):
    """n damaged copies: a byte changed, a byte run changed, a cut, a cut with a trailer put back"""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        b = bytearray(blob)
        kind = k % 4
        at = int(rng.integers(6, len(b)))
        if kind == 0:
            b[at] ^= 1 << int(rng.integers(0, 8))
        elif kind == 1:
            for j in range(at, min(len(b), at + int(rng.integers(1, 9)))):
                b[j] = int(rng.integers(0, 256))
        elif kind == 2:
            b = b[:at]
        else:
            b = b[:at] + b"\x00\x3b"
        out.append(bytes(b))
    return out


def test_written_files_under_sanitizers():
    cases = pin_cases()
    names = [n for n in cases if n.startswith(("1x1", "3x5", "19x37_m2", "19x37_m8", "130x120_m4_i1", "130x120_m8_i0_c1", "200x200", "130x120_runs"))]
    files = [cases[n][0] for n in names] + [album_file()[0]]
    files += [damaged_file(s, t) for s in damaged_streams().values() for t in (False, True)]
    check(files)


@pytest.mark.parametrize("name", ["19x37_m3_i1_c1", "130x120_m8_i0_c0", "200x200_runs_never_clear", "album"])
def test_seeded_damage_under_sanitizers(name):
    blob = album_file()[0] if name == "album" else pin_cases()[name][0]
    check(seeded_damage(blob, len(name), 60))
