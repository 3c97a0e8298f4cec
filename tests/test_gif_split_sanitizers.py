"""The split route's host code under AddressSanitizer + UBSan (the pattern of test_gif_decode_sanitizers.py): the scan, the
length pass and the emit pass of csrc/imp_gif.h -- the kernels' lane code run on the host -- see the bytes of files somebody
uploaded.  tests/c/gif_split_fuzz.cpp has its own main, is built with g++ -fsanitize=address,undefined and fed the written
files, the pages made to be cut, the damage behind a cut and seeded damage of four files; every verdict, checksum and
segment count must equal the regular library's impgpu_gif_pages_split, and the planes go into a heap block of exactly
their size.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from test_gif_decode_host import album_file, damaged_file, damaged_streams, pin_cases
from test_gif_decode_sanitizers import checksum, seeded_damage
from test_gif_split_host import cut_cases, damage_behind_a_cut

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_split_fuzz_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_split_fuzz.cpp")
    deps = [src, os.path.join(CSRC, "imp_gif.h")] + [os.path.join(ROOT, "include", h) for h in ("impgpu.h", "impgpu_gif.h", "impgpu_broker.h")]
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


def check(files):
    for k, (f, (rc, psum, count, ssum)) in enumerate(zip(files, drive(files))):
        want_rc, planes, segs = imp.gif_pages_split(f)
        assert rc == want_rc, k
        if want_rc == 0:
            assert psum == checksum(planes), k
        if segs is not None:
            assert count == len(segs) and ssum == checksum(segs), k


def test_written_files_under_sanitizers():
    cases = pin_cases()
    names = [n for n in cases if n.startswith(("1x1", "3x5", "19x37_m2", "19x37_m8", "130x120_m4_i1", "130x120_m8_i0_c1", "200x200", "130x120_runs"))]
    files = [cases[n][0] for n in names] + [album_file()[0]]
    files += [damaged_file(s, t) for s in damaged_streams().values() for t in (False, True)]
    files += [blob for blob, _ in cut_cases().values()] + [blob for blob, _ in damage_behind_a_cut().values()]
    check(files)


@pytest.mark.parametrize("name", ["19x37_m3_i1_c1", "130x120_noise_m8", "130x120_noise_m8_clear_every_1000", "album"])
def test_seeded_damage_under_sanitizers(name):
    blob = album_file()[0] if name == "album" else cut_cases()[name][0] if name in cut_cases() else pin_cases()[name][0]
    check(seeded_damage(blob, len(name), 60))
