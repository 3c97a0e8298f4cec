"""The lossy WebP encoder's host code under AddressSanitizer + UBSan (the pattern of test_webp_encode_sanitizers.py): the
lane code of csrc/imp_webp_lossy.h -- planes, the macroblock phases, the token records, the boolean coder and the packing, as
impgpu_webp_lossy_encode_host runs them -- sees the cases of test_webp_vp8_writer and random frames with padded rows.
tests/c/webp_lossy_fuzz.cpp has its own main, is built with g++ -fsanitize=address,undefined, keeps every frame and every
file in a heap block of exactly its size; its verdicts, sizes and checksums must equal the regular library's
impgpu_webp_lossy_encode_host.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gif_decode_sanitizers import checksum
from test_webp_lossy_host import random_frames
from test_webp_vp8_writer import CASES

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "webp_lossy_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "webp_lossy_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_webp_lossy.h"), os.path.join(ROOT, "include", "impgpu.h"), os.path.join(ROOT, "include", "impgpu_vp8_tables.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(items):
    """items: [(frame, pad, quality)] -> the driver's [code, size, checksum] per frame"""
    build()
    lines = []
    for frame, pad, q in items:
        h, w, c = frame.shape
        rows = np.zeros((h, w * c + pad), np.uint8)
        rows[:, : w * c] = frame.reshape(h, w * c)
        data = rows.reshape(-1)[: (w * c + pad) * (h - 1) + w * c]
        lines.append("%d %d %d %d %d %s" % (w, h, c, pad, q, data.tobytes().hex()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(items)
    return [[int(v) for v in line.split()] for line in out]


def check(items):
    for k, ((frame, pad, q), (rc, size, csum)) in enumerate(zip(items, drive(items))):
        want_rc, blob, length, intact = imp.encode_webp_lossy_host(frame, q)
        assert rc == want_rc and intact, k
        if want_rc == 0:
            assert size == length and csum == checksum(blob), k


def test_the_cases_under_sanitizers():
    items = [(CASES[name][0], 0, CASES[name][1]) for name in sorted(CASES)]
    items += [(np.zeros((3, 5, 2), np.uint8), 0, 75), (np.zeros((3, 5, 3), np.uint8), 0, 101)]      # refused
    check(items)


def test_random_frames_under_sanitizers():
    check(random_frames(11, 25))
