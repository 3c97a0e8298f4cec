"""The GIF encoder's delta-frame host code under AddressSanitizer + UBSan (the pattern of test_gif_quant_sanitizers.py): the
lane code csrc/imp_gif_enc.h adds for IMPGPU_GIF_ENC_DELTA -- the held rule and the held plane, the window's bounds, the set
of written keys, the choice, and index, histogram and LZW reading through the window, as impgpu_gif_encode_host_ex2 runs them
-- sees the cases and seeded random albums in which a patch moves over a still background, with every disposal.
tests/c/gif_delta_fuzz.cpp has its own main and is built with g++ -fsanitize=address,undefined; its codes, sizes and checksums
must equal the regular library's.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gif_decode_sanitizers import checksum
from test_gif_encode_host import CASES as EXACT_CASES, frame_of, palette
from gif_quant_model import CASES as QUANT_CASES
from gif_delta_model import CASES

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_delta_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_delta_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_gif.h"), os.path.join(CSRC, "imp_gif_enc.h")] + [os.path.join(ROOT, "include", h) for h in ("impgpu.h", "impgpu_gif.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def drive(albums):
    """albums: [(frames, segment, loop, flags, dispose)] -> the driver's [code, size, checksum] per album"""
    build()
    lines = []
    for frames, segment, loop, flags, dispose in albums:
        h, w, c = frames[0].shape
        lines.append("%d %d %d %d %d %d %d %s %s" % (w, h, c, len(frames), segment, loop, flags, "".join(str(d) for d in dispose),
                                                     b"".join(np.ascontiguousarray(f).tobytes() for f in frames).hex()))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(albums)
    return [[int(v) for v in line.split()] for line in out]


def check(albums):
    """-> how many albums were accepted, how many of those files the bit made smaller"""
    accepted = smaller = 0
    for k, ((frames, segment, loop, flags, dispose), (rc, size, csum)) in enumerate(zip(albums, drive(albums))):
        n = len(frames)
        assert flags & imp.GIF_ENC_DELTA
        want_rc, blob, length, intact = imp.encode_gif_host(frames, time_ms=[37 * f for f in range(n)], dispose=list(dispose), loop_count=loop,
                                                            segment=segment, flags=flags & ~imp.GIF_ENC_DELTA, delta=True)
        assert rc == want_rc and intact, k
        plain = imp.encode_gif_host(frames, dispose=list(dispose), loop_count=loop, segment=segment, flags=flags & ~imp.GIF_ENC_DELTA)
        assert plain[0] == want_rc or (plain[0] == 1 and want_rc == 0), k    # the bit refuses nothing the call without it takes
        if want_rc == 0:
            assert size == length and csum == checksum(blob), k
            accepted += 1
            smaller += length < plain[2]
        else:
            assert want_rc == 1 and csum == 0, k
    return accepted, smaller


def random_albums(seed, count):
    """a patch of fresh pixels moves over a background that stands still (or, one time in four, does not)"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w, h = int(rng.integers(1, 81)), int(rng.integers(1, 81))
        n = int(rng.integers(2, 5))
        alpha = bool(rng.integers(0, 2))
        colours = int(rng.choice([4, 60, 250, 256, 257, 1200]))
        pal = palette(rng, colours)
        back = frame_of(rng, w, h, pal[: min(colours, w * h)], transparent=float(rng.choice([0.0, 0.2])) if alpha else 0.0, alpha=alpha)
        frames = [back]
        for f in range(1, n):
            g = frames[-1].copy() if rng.integers(0, 4) else frame_of(rng, w, h, pal[: min(colours, w * h)], alpha=alpha)
            pw, ph = int(rng.integers(1, w + 1)), int(rng.integers(1, h + 1))
            x, y = int(rng.integers(0, w - pw + 1)), int(rng.integers(0, h - ph + 1))
            if rng.integers(0, 3):
                g[y:y + ph, x:x + pw, :3] = pal[rng.integers(0, colours, (ph, pw))]
            if alpha and rng.integers(0, 2):
                g[y:y + ph, x:x + 1, 3] = 0
            frames.append(g)
        dispose = [int(rng.choice([0, 1, 0, 1, 2, 3])) for _ in range(n)]
        out.append((frames, int(rng.choice([0, 256, 257, 1000, 4096])), int(rng.choice([-1, 0, 7])), 2 | int(rng.choice([1, 1, 0])), dispose))
    return out


def test_the_cases_under_sanitizers():
    albums = []
    for frames, kw, quantize in CASES.values():
        albums.append((frames, kw.get("segment", 0), kw.get("loop_count", -1), 3 if quantize else 2, kw.get("dispose") or [0] * len(frames)))
        if quantize:                                                  # refused without IMPGPU_GIF_ENC_QUANTIZE
            albums.append((frames, kw.get("segment", 0), kw.get("loop_count", -1), 2, kw.get("dispose") or [0] * len(frames)))
    for frames, kw in list(EXACT_CASES.values()) + list(QUANT_CASES.values()):
        albums.append((frames, kw.get("segment", 0), kw.get("loop_count", -1), 3, kw.get("dispose") or [0] * len(frames)))
    albums += [([np.zeros((1, 1, 3), np.uint8)] * 3, 256, -1, 2, [0, 0, 0]), ([np.zeros((1, 1, 4), np.uint8)] * 2, 256, 0, 3, [1, 1])]
    accepted, smaller = check(albums)
    assert accepted == len(albums) - 1 and smaller >= len(CASES) - 4


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_albums_under_sanitizers(seed):
    accepted, smaller = check(random_albums(seed, 40))
    assert accepted >= 25 and smaller >= 10
