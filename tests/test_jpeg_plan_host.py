"""The JPEG entropy work area's layout (csrc/imp_jpeg_plan.h) under AddressSanitizer + UBSan (the pattern of
test_gif_delta_sanitizers.py): tests/c/jpeg_plan_check.cpp has its own main and is built with g++
-fsanitize=address,undefined.  It sweeps chunk counts, lanes per chunk, blocks per MCU and frame sizes; for each, every array
a kernel is handed lies inside the area, apart from the others and aligned, where it lay before the layout had a header of
its own, and is written whole through the job's pointers into a block of exactly the area's size.  CPU only: sanitizers do
not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "jpeg_plan_check_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "jpeg_plan_check.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("imp_jpeg_plan.h", "imp_jpeg_core.h", "imp_jpeg.h", "imp_internal.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def test_the_work_area_layout_under_sanitizers():
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
    assert p.stdout.strip().split("\n")[-1] == "ok %d layouts" % (13 * 2 * 4 * 5)
