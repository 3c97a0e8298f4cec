"""The GIF compose / decode calls' device blob (csrc/imp_gif_plan.h) under AddressSanitizer + UBSan (the pattern of
test_jpeg_plan_host.py): tests/c/gif_plan_check.cpp has its own main and is built with g++ -fsanitize=address,undefined.  It
sweeps entries per group, pages per entry, page sizes and pitches, page requests and table sizes, and on the decode route
compressed sizes with and without IMPGPU_GIF_SPLIT; for each, the blob is laid out and filled through the header into heap
blocks of exactly its two sizes, every offset is where the hand-written expressions put it before the header existed, the
regions lie in their zones, apart and aligned, the group cut agrees with the old loops under three caps, and the pieces leave
where the old loops sent them.  CPU only: sanitizers do not run on the GPU, and no Python runs under them."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ with libasan / libubsan")
CSRC = os.path.join(ROOT, "ngx_http_imgproc_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "c", "_build")
DRIVER = os.path.join(OUT, "gif_plan_check_asan")


def build():
    os.makedirs(OUT, exist_ok=True)
    src = os.path.join(ROOT, "tests", "c", "gif_plan_check.cpp")
    deps = [src] + [os.path.join(CSRC, h) for h in ("imp_gif_plan.h", "imp_gif.h", "imp_internal.h")]
    if os.path.exists(DRIVER) and all(os.path.getmtime(d) <= os.path.getmtime(DRIVER) for d in deps):
        return
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), src, "-o", DRIVER])


def test_the_gif_blob_layout_under_sanitizers():
    build()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([DRIVER], capture_output=True, text=True, env=env, timeout=600)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, (p.stdout[-3000:], p.stderr[-3000:])
    # entries x pages x (sizes x pitches) x requests x tables, each once for the compose route and data_bytes x split times for the decode route
    assert p.stdout.strip().split("\n")[-1] == "ok %d layouts" % (3 * 3 * (4 * 2) * 4 * 2 * (1 + 6 * 2))
