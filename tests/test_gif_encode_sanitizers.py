"""The GIF encoder's host code under AddressSanitizer + UBSan (the pattern of test_gif_decode_sanitizers.py): the lane code
of csrc/imp_gif_enc.h -- colour sets, tables, index planes, the segmented LZW and the pack, as impgpu_gif_encode_host runs
them -- sees random albums.  tests/c/gif_enc_fuzz.cpp has its own main, is built with g++ -fsanitize=address,undefined, writes
every file into a heap block of exactly its size, reads it back with the library's plain host decoder and compares the pixels;
its verdicts, sizes and checksums must equal the regular library's impgpu_gif_encode_host.  CPU only: sanitizers do not run
on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gif_decode_sanitizers import checksum
from test_gif_encode_host import CASES, frame_of, palette, refused_frames

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_enc_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_enc_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_gif.h"), os.path.join(CSRC, "imp_gif_enc.h")] + [os.path.join(ROOT, "include", h) for h in ("impgpu.h", "impgpu_gif.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(albums):
    """albums: [(frames, segment, loop)] -> the driver's [code, size, checksum, read back] per album"""
    build()
    lines = []
    for frames, segment, loop in albums:
        h, w, c = frames[0].shape
        lines.append("%d %d %d %d %d %d %s" % (w, h, c, len(frames), segment, loop, b"".join(np.ascontiguousarray(f).tobytes() for f in frames).hex()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(albums)
    return [[int(v) for v in line.split()] for line in out]


def check(albums):
    accepted = 0
    for k, ((frames, segment, loop), (rc, size, csum, back)) in enumerate(zip(albums, drive(albums))):
        n = len(frames)
        want_rc, blob, length, intact = imp.encode_gif_host(frames, time_ms=[37 * f for f in range(n)], dispose=[f & 3 for f in range(n)],
                                                            loop_count=loop, segment=segment)
        assert rc == want_rc and intact, k
        if want_rc == 0:
            assert size == length and csum == checksum(blob) and back == 1, k
            accepted += 1
        else:
            assert want_rc == 1 and back == 0, k
    return accepted


def random_albums(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w, h = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        n = int(rng.integers(1, 4))
        alpha = bool(rng.integers(0, 2))
        colours = int(rng.integers(1, 301)) if w * h >= 300 else int(rng.integers(1, w * h + 1))
        pal = palette(rng, colours)
        share = int(rng.integers(0, 3))                             # frames of one table, of overlapping ones, of tables of their own
        frames = []
        for f in range(n):
            lo = 0 if share == 0 else (f * colours // (2 * n) if share == 1 else f * colours // n)
            sub = pal[lo: max(lo + 1, lo + colours // (1 if share == 0 else n))]
            frames.append(frame_of(rng, w, h, sub[: w * h], transparent=float(rng.choice([0.0, 0.0, 0.3])) if alpha else 0.0, alpha=alpha))
        out.append((frames, int(rng.choice([0, 256, 257, 1000, 4096, 8192])), int(rng.choice([-1, 0, 7]))))
    return out


def test_the_cases_under_sanitizers():
    albums = [(frames, kw.get("segment", 0), kw.get("loop_count", -1)) for frames, kw in CASES.values()]
    albums += [(frames, 0, -1) for _, frames in refused_frames()]
    albums += [([np.zeros((1, 1, 3), np.uint8)], 256, -1), ([np.zeros((1, 1, 4), np.uint8)], 256, 0)]
    assert check(albums) == len(CASES) + 2


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_albums_under_sanitizers(seed):
    assert check(random_albums(seed, 40)) >= 10
