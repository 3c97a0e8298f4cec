"""The progressive JPEG front's host code under AddressSanitizer + UBSan (the pattern of test_host_sanitizers.py): the
multi-scan marker walk, the progression checks, the unstuffing of every scan into items and both decoders -- the plain one
and the device's lane code run on the host -- see the bytes of files somebody uploaded.  tests/c/fuzz_jpeg_prog.cpp is
built with g++ -fsanitize=address,undefined and fed the fixtures, the written files and seeded damage of them; every
answer must equal what the regular library returns.  CPU only: sanitizers do not run on the GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_prog_writer as W
from conftest import ROOT
from test_jpeg_prog_host import NAMES, coefficients_ex, damaged_files, fixture, old_fixture, written, written_cases

import ngx_http_imgproc_amd as imp

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "fuzz_jpeg_prog_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    srcs = [os.path.join(ROOT, "tests", "c", "fuzz_jpeg_prog.cpp"), os.path.join(CSRC, "imp_jpeg.cpp"), os.path.join(CSRC, "imp_jpeg_prog.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("imp_jpeg_prog.h", "imp_jpeg_core.h", "imp_jpeg.h", "imp_internal.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include")] + srcs + ["-o", DRIVER])


def drive(files):
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], input="\n".join(f.hex() for f in files) + "\n", capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.strip().split("\n")
    assert len(out) == len(files)
    return [[int(v) for v in line.split()] for line in out]


def checksum(a):
    s = 0
    for v in a.astype(np.uint16).tolist():
        s = (s * 31 + v) & 0xFFFFFFFFFFFFFFFF
    return s


def check(files):
    for f, (rci, rc0, rc1, sum0, sum1) in zip(files, drive(files)):
        assert rci == imp.jpeg_info_ex(f, imp.JPEG_PROGRESSIVE)[0]
        for how, rc, s in ((0, rc0, sum0), (1, rc1, sum1)):
            want_rc, got, _ = coefficients_ex(f, how)
            if rci == 0:
                assert rc == want_rc
                if rc == 0:
                    assert s == checksum(got)


def test_fixtures_and_written_files_under_sanitizers():
    files = [fixture(n, "prog") for n in NAMES if n not in ("gray_q75_640x480", "c420_q50_400x300")]
    files += [written(src, script) for _, src, script in written_cases()]
    s = W.Source(old_fixture("c420_q90_67x45"))
    files += [W.write(s, sc) for sc in W.illegal_scripts(3).values()]
    check(files)


@pytest.mark.parametrize("name", ["c420_q90_dri4_95x51", "gray_q90_57x43", "c444_q100_noise_64x48", "c422_q85_49x37"])
def test_damaged_files_under_sanitizers(name):
    check(damaged_files(name))
