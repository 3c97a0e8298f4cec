"""The GIF quantiser's host code under AddressSanitizer + UBSan (the pattern of test_gif_encode_sanitizers.py): the lane code
csrc/imp_gif_enc.h adds for IMPGPU_GIF_ENC_QUANTIZE -- the workgroup's cell table, the histogram, the summed-volume table,
the cuts, the colours and the cell -> index table, as impgpu_gif_encode_host_ex and impgpu_gif_quantize_host run them -- sees
the cases and random albums that mix frames under and over 256 colours, with and without transparency.
tests/c/gif_quant_fuzz.cpp has its own main and is built with g++ -fsanitize=address,undefined; its codes, sizes and checksums
must equal the regular library's.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gif_decode_sanitizers import checksum
from test_gif_encode_host import CASES as EXACT_CASES, frame_of, palette
from gif_quant_model import CASES

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_quant_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_quant_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_gif.h"), os.path.join(CSRC, "imp_gif_enc.h")] + [os.path.join(ROOT, "include", h) for h in ("impgpu.h", "impgpu_gif.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(albums):
    """albums: [(frames, segment, loop, flags)] -> the driver's [code, size, checksum, quantiser checksum] per album"""
    build()
    lines = []
    for frames, segment, loop, flags in albums:
        h, w, c = frames[0].shape
        lines.append("%d %d %d %d %d %d %d %s" % (w, h, c, len(frames), segment, loop, flags, b"".join(np.ascontiguousarray(f).tobytes() for f in frames).hex()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(albums)
    return [[int(v) for v in line.split()] for line in out]


def quantiser_checksum(frames):
    s = 0
    for f in frames:
        rc, table, tkey, indices = imp.gif_quantize_host(np.ascontiguousarray(f))
        for v in (rc, len(table), tkey + 1):
            s = (s * 31 + v) & 0xFFFFFFFFFFFFFFFF
        for v in table.tobytes() + indices.tobytes():
            s = (s * 31 + v) & 0xFFFFFFFFFFFFFFFF
    return s


def check(albums):
    """-> how many albums were accepted, how many of them held a quantised frame"""
    accepted = quantised = 0
    for k, ((frames, segment, loop, flags), (rc, size, csum, qsum)) in enumerate(zip(albums, drive(albums))):
        n = len(frames)
        want_rc, blob, length, intact = imp.encode_gif_host(frames, time_ms=[37 * f for f in range(n)], dispose=[f & 3 for f in range(n)],
                                                            loop_count=loop, segment=segment, flags=flags)
        assert rc == want_rc and intact, k
        assert qsum == quantiser_checksum(frames), k
        if want_rc == 0:
            assert size == length and csum == checksum(blob), k
            accepted += 1
            plain = imp.encode_gif_host(frames, segment=segment)[0]
            quantised += plain == 1
        else:
            assert want_rc == 1 and flags == 0 and csum == 0, k
    return accepted, quantised


def random_albums(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w, h = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        n = int(rng.integers(1, 4))
        alpha = bool(rng.integers(0, 2))
        frames = []
        for f in range(n):
            most = min(w * h, int(rng.choice([8, 200, 256, 257, 400, 3000])))
            colours = int(rng.integers(1, most + 1))
            if rng.integers(0, 3) == 0:                              # colours crowded into a corner of the cube: few cells, flat boxes
                pal = np.unique(rng.integers(0, 40, (colours, 3)).astype(np.uint8), axis=0)
            else:
                pal = palette(rng, colours)
            frames.append(frame_of(rng, w, h, pal[: w * h], transparent=float(rng.choice([0.0, 0.0, 0.3])) if alpha else 0.0, alpha=alpha))
        out.append((frames, int(rng.choice([0, 256, 257, 1000, 4096, 8192])), int(rng.choice([-1, 0, 7])), int(rng.choice([1, 1, 1, 0]))))
    return out


def test_the_cases_under_sanitizers():
    albums = [(frames, kw.get("segment", 0), kw.get("loop_count", -1), 1) for frames, kw in CASES.values()]
    albums += [(frames, kw.get("segment", 0), kw.get("loop_count", -1), 0) for frames, kw in CASES.values()]         # refused without the flag
    albums += [(frames, kw.get("segment", 0), kw.get("loop_count", -1), 1) for frames, kw in EXACT_CASES.values()]
    albums += [([np.zeros((1, 1, 3), np.uint8)], 256, -1, 1), ([np.zeros((1, 1, 4), np.uint8)], 256, 0, 1)]
    assert check(albums) == (len(CASES) + len(EXACT_CASES) + 2, len(CASES))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_albums_under_sanitizers(seed):
    accepted, quantised = check(random_albums(seed, 40))
    assert accepted >= 25 and quantised >= 5
