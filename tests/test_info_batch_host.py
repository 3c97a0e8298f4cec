"""impgpu_batch_calc_perceived_brightness and impgpu_batch_ascii answer malformed arguments on the host, before they look
for a device, and belong to the C ABI like every other entry point (runs without a GPU)."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("impgpu_batch_calc_perceived_brightness", "impgpu_batch_ascii")


def _fresh_process(body):
    """The argument checks in a process of their own: no env has been started there, whatever this session did before."""
    import sys

    script = "import sys\nsys.path.insert(0, %r)\nimport ctypes as C\nimport ngx_http_imgproc_amd as imp\nlib = imp.lib\n" % ROOT + body
    r = subprocess.run([sys.executable, "-c", script], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


BRIGHTNESS = """
INV, DEV = imp.IMP_ERROR_INVALID_ARGS, imp.IMP_ERROR_DEVICE
n = 3
bufs = [(C.c_ubyte * 64)() for _ in range(n)]
# stand-ins for three handles: never dereferenced, the call refuses or misses the device first
images = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in bufs])
vals = (C.c_float * n)(*[-1.0] * n)
codes = (C.c_int * n)(*[-1] * n)
launches = C.c_int(-1)
run = lib.impgpu_batch_calc_perceived_brightness
assert run(None, n, vals, codes, C.byref(launches)) == INV
assert launches.value == 0
assert run(images, n, None, codes, None) == INV
assert run(images, n, vals, None, None) == INV
assert run(images, -1, vals, codes, None) == INV
assert run(images, 257, vals, codes, None) == INV
assert list(codes) == [-1] * n and list(vals) == [-1.0] * n        # nothing answered for a malformed call
# well-formed: only now is the device missed
launches.value = -1
assert run(images, n, vals, codes, C.byref(launches)) == DEV
assert list(codes) == [DEV] * n and launches.value == 0
assert run(images, 0, vals, codes, None) == DEV
twice = (C.c_void_p * n)(images[0], images[1], images[0])           # brightness only reads: repeats are not malformed
assert run(twice, n, vals, codes, None) == DEV
print("brightness ok")
"""

ASCII = """
INV, DEV = imp.IMP_ERROR_INVALID_ARGS, imp.IMP_ERROR_DEVICE
n = 3
bufs = [(C.c_ubyte * 64)() for _ in range(n)]
texts = [(C.c_ubyte * 64)(*[0xA5] * 64) for _ in range(n)]
images = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in bufs])
args = (C.c_char_p * n)(b"", None, b"wide")
outs = (C.c_void_p * n)(*[C.addressof(t) for t in texts])
caps = (C.c_long * n)(64, 64, 64)
lens = (C.c_long * n)(*[-7] * n)
codes = (C.c_int * n)(*[-1] * n)
launches = C.c_int(-1)
run = lib.impgpu_batch_ascii
assert run(None, args, n, outs, caps, lens, codes, C.byref(launches)) == INV
assert launches.value == 0
assert run(images, args, n, None, caps, lens, codes, None) == INV
assert run(images, args, n, outs, None, lens, codes, None) == INV
assert run(images, args, n, outs, caps, None, codes, None) == INV
assert run(images, args, n, outs, caps, lens, None, None) == INV
assert run(images, args, -1, outs, caps, lens, codes, None) == INV
assert run(images, args, 257, outs, caps, lens, codes, None) == INV
twice = (C.c_void_p * n)(images[0], images[1], images[0])           # written in place: the same handle twice is malformed
assert run(twice, args, n, outs, caps, lens, codes, None) == INV
assert list(codes) == [-1] * n and list(lens) == [-7] * n
assert all(bytes(t) == b"\\xa5" * 64 for t in texts)
launches.value = -1
assert run(images, args, n, outs, caps, lens, codes, C.byref(launches)) == DEV
assert list(codes) == [DEV] * n and launches.value == 0
assert run(images, None, n, outs, caps, lens, codes, None) == DEV   # args itself may be NULL
assert run(images, args, 0, outs, caps, lens, codes, None) == DEV
assert all(bytes(t) == b"\\xa5" * 64 for t in texts)
print("ascii ok")
"""


def test_batch_brightness_checks_its_arguments_before_the_device():
    assert "brightness ok" in _fresh_process(BRIGHTNESS)


def test_batch_ascii_checks_its_arguments_before_the_device():
    assert "ascii ok" in _fresh_process(ASCII)


def _declared():
    text = open(os.path.join(ROOT, "include", "impgpu.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return set(re.findall(r"\b(impgpu_[a-z0-9_]+)\s*\(", text))


def test_both_calls_are_declared_exported_and_bound():
    import ngx_http_imgproc_amd as imp
    from ngx_http_imgproc_amd import _lib

    raw = C.CDLL(imp.LIB_PATH)
    for name in NEW:
        assert name in _declared(), name
        assert hasattr(raw, name), name
        assert name in _lib.SIGNATURES, name
    assert callable(imp.batch_calc_perceived_brightness) and callable(imp.batch_ascii)


def test_header_still_compiles_as_c99_and_the_calls_take_these_arguments(tmp_path):
    src = tmp_path / "t.c"
    src.write_text(
        '#include "impgpu.h"\n'
        "int main(void) {\n"
        "    int (*b)(const impgpu_image* const*, int, float*, int*, int*) = impgpu_batch_calc_perceived_brightness;\n"
        "    int (*a)(impgpu_image* const*, const char* const*, int, unsigned char* const*, const long*, long*, int*, int*) = impgpu_batch_ascii;\n"
        "    (void)a; (void)b;\n"
        "    return IMP_OK;\n"
        "}\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(tmp_path / "t.o")])
