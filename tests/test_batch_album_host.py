"""impgpu_batch_download_fi and impgpu_batch_album_download answer malformed arguments on the host, before they look for a
device, and belong to the C ABI like every other entry point (runs without a GPU)."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("impgpu_batch_download_fi", "impgpu_batch_album_download")


def _fresh_process(body):
    """The argument checks in a process of their own: no env has been started there, whatever this session did before."""
    script = "import sys\nsys.path.insert(0, %r)\nimport ctypes as C\nimport ngx_http_imgproc_amd as imp\nlib = imp.lib\n" % ROOT + body
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


COMMON = """
OK, INV, DEV = imp.IMP_OK, imp.IMP_ERROR_INVALID_ARGS, imp.IMP_ERROR_DEVICE
n = 3
bufs = [(C.c_ubyte * 64)() for _ in range(n)]
# stand-ins for three handles: never dereferenced, the call refuses or misses the device first
images = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in bufs])
maps = [(C.c_ubyte * 64)(*[0xA5] * 64) for _ in range(n)]
bits = (C.c_void_p * n)(*[C.addressof(m) for m in maps])
pitches = (C.c_int * n)(16, 16, 16)
codes = (C.c_int * n)(*[-1] * n)
"""

DOWNLOAD_FI = COMMON + """
bpps = (C.c_int * n)(32, 24, 32)
launches = C.c_int(-1)
run = lib.impgpu_batch_download_fi
assert run(None, bpps, n, bits, pitches, codes, C.byref(launches)) == INV
assert launches.value == 0
assert run(images, None, n, bits, pitches, codes, None) == INV
assert run(images, bpps, n, None, pitches, codes, None) == INV
assert run(images, bpps, n, bits, None, codes, None) == INV
assert run(images, bpps, n, bits, pitches, None, None) == INV
assert run(images, bpps, -1, bits, pitches, codes, None) == INV
assert run(images, bpps, 257, bits, pitches, codes, None) == INV
assert list(codes) == [-1] * n                                       # nothing answered for a malformed call
launches.value = -1
assert run(images, bpps, 0, bits, pitches, codes, C.byref(launches)) == OK      # nothing asked
assert run(None, None, 0, None, None, None, None) == OK
assert launches.value == 0 and list(codes) == [-1] * n
# well-formed: only now is the device missed
launches.value = -1
assert run(images, bpps, n, bits, pitches, codes, C.byref(launches)) == DEV
assert list(codes) == [DEV] * n and launches.value == 0
assert all(bytes(m) == b"\\xa5" * 64 for m in maps)
print("download_fi ok")
"""

ALBUM_DOWNLOAD = COMMON + """
run = lib.impgpu_batch_album_download
assert run(None, n, bits, pitches, codes) == INV
assert run(images, n, None, pitches, codes) == INV
assert run(images, n, bits, None, codes) == INV
assert run(images, n, bits, pitches, None) == INV
assert run(images, -1, bits, pitches, codes) == INV
assert run(images, 257, bits, pitches, codes) == INV
assert list(codes) == [-1] * n
assert run(images, 0, bits, pitches, codes) == OK
assert run(None, 0, None, None, None) == OK
assert list(codes) == [-1] * n
assert run(images, n, bits, pitches, codes) == DEV
assert list(codes) == [DEV] * n
assert all(bytes(m) == b"\\xa5" * 64 for m in maps)
print("album_download ok")
"""


def test_batch_download_fi_judges_its_arguments_before_the_device():
    assert "download_fi ok" in _fresh_process(DOWNLOAD_FI)


def test_batch_album_download_judges_its_arguments_before_the_device():
    assert "album_download ok" in _fresh_process(ALBUM_DOWNLOAD)


def test_the_new_calls_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "impgpu.h")).read()
    binding = open(os.path.join(ROOT, "ngx_http_imgproc_amd", "_lib.py")).read()
    import ngx_http_imgproc_amd as imp

    for name in NEW:
        assert re.search(r"\b%s\(" % name, header), name
        assert '"%s"' % name in binding, name
        assert hasattr(imp.lib, name), name
    assert callable(imp.batch_download_fi) and callable(imp.batch_album_download)
