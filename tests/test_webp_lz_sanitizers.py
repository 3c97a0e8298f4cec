"""The WebP encoder's host code with backward references under AddressSanitizer + UBSan (the pattern of
test_webp_encode_sanitizers.py): the lane code of csrc/imp_webp_enc.h with IMPGPU_WEBP_ENC_BACKREFS -- the candidates'
equality words, the skips and lengths read from them, the token plane, the 280-symbol green code and the distance code
through zlib's build_tree, the tokens' symbols and their packing, as impgpu_webp_encode_host_flags runs them -- sees the
cases of test_webp_lz_writer (planted matches, the shapes around an item's end) and random frames with padded rows and
forced modes.  tests/c/webp_lz_fuzz.cpp has its own main, is built with g++ -fsanitize=address,undefined, keeps every frame
and every file in a heap block of exactly its size; its verdicts, sizes and checksums must equal the regular library's
impgpu_webp_encode_host_flags.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import webp_writer as W
from conftest import ROOT
from test_gif_decode_sanitizers import checksum
from test_webp_encode_host import random_frames
from test_webp_lz_writer import CASES

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "webp_lz_fuzz_asan")
LZF = imp.WEBP_ENC_BACKREFS


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "webp_lz_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_webp_enc.h"), os.path.join(CSRC, "imp_png_deflate.h"), os.path.join(ROOT, "include", "impgpu.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(items):
    """items: [(frame, pad, forced modes or None, flags)] -> the driver's [code, size, checksum] per frame"""
    build()
    lines = []
    for frame, pad, modes, flags in items:
        h, w, c = frame.shape
        rows = np.zeros((h, w * c + pad), np.uint8)
        rows[:, : w * c] = frame.reshape(h, w * c)
        data = rows.reshape(-1)[: (w * c + pad) * (h - 1) + w * c]
        line = "%d %d %d %d %d %d %s" % (w, h, c, pad, int(modes is not None), flags, data.tobytes().hex())
        if modes is not None:
            line += " " + np.asarray(modes, np.uint8).tobytes().hex()
        lines.append(line)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(items)
    return [[int(v) for v in line.split()] for line in out]


def check(items):
    for k, ((frame, pad, modes, flags), (rc, size, csum)) in enumerate(zip(items, drive(items))):
        want_rc, blob, length, intact = imp.encode_webp_host(frame, forced_modes=modes, flags=flags)
        assert rc == want_rc and intact, k
        if want_rc == 0:
            assert size == length and csum == checksum(blob), k


def test_the_cases_under_sanitizers():
    items = [(CASES[name][0], 0, CASES[name][1], LZF) for name in sorted(CASES)]
    items += [(CASES["rows2_41x25"][0], 0, CASES["rows2_41x25"][1], 0)]           # flags 0: the flag-less body
    items += [(np.zeros((3, 5, 2), np.uint8), 0, None, LZF), (np.zeros((3, 5, 3), np.uint8), 0, None, 2)]   # refused
    check(items)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_frames_under_sanitizers(seed):
    rng = np.random.default_rng(17 + seed)
    items = []
    for frame, pad in random_frames(30 + seed, 25):
        h, w, _ = frame.shape
        tx, ty = W.tiles_of(w, h)
        items.append((frame, pad, rng.integers(0, W.MODES, tx * ty).astype(np.uint8) if rng.integers(0, 3) == 0 else None, LZF))
    check(items)
