"""impgpu_batch_resize_mixed_ex: declared, exported, and answering malformed arguments on the host before it looks for a
device (runs without a GPU)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbol_is_declared_and_exported():
    import ngx_http_imgproc_amd as imp
    from ngx_http_imgproc_amd._lib import SIGNATURES

    with open(os.path.join(ROOT, "include", "impgpu.h")) as fh:
        header = fh.read()
    m = re.search(r"int\s+impgpu_batch_resize_mixed_ex\s*\(([^)]*)\)\s*;", header)
    assert m, "include/impgpu.h does not declare impgpu_batch_resize_mixed_ex"
    assert len(m.group(1).split(",")) == 6 and "int* launches" in m.group(1)
    assert "impgpu_batch_resize_mixed_ex" in SIGNATURES and len(SIGNATURES["impgpu_batch_resize_mixed_ex"][1]) == 6
    assert C.CDLL(imp.LIB_PATH).impgpu_batch_resize_mixed_ex          # AttributeError: not exported


def test_arguments_are_checked_before_the_device():
    import ngx_http_imgproc_amd as imp

    lib = imp.lib
    INV = imp.IMP_ERROR_INVALID_ARGS
    run = lib.impgpu_batch_resize_mixed_ex
    src, dst = (C.c_ubyte * 4096)(), (C.c_ubyte * 1024)()
    sp, dp = C.cast(src, C.c_void_p).value, C.cast(dst, C.c_void_p).value

    def items(*tuples):
        return (imp.ResizeItem * len(tuples))(*[imp.ResizeItem(*t) for t in tuples])

    good = (sp, 32, 32, 128, dp, 16, 16, 64)
    launches = C.c_int(-1)
    assert run(None, 2, 4, 0, None, C.byref(launches)) == INV and launches.value == 0
    launches.value = -1
    assert run(items(good), -1, 4, 0, None, C.byref(launches)) == INV and launches.value == 0
    assert run(items(good), 1, 5, 0, None, None) == INV
    assert run(items(good), 1, 2, 1, None, None) == INV
    for bad in [(None, 32, 32, 128, dp, 16, 16, 64), (sp, 32, 32, 128, None, 16, 16, 64), (sp, 0, 32, 128, dp, 16, 16, 64),
                (sp, 32, 32, 127, dp, 16, 16, 64), (sp, 32, 32, 128, dp, 16, 0, 64), (sp, 32, 32, 128, dp, 16, 16, 63)]:
        launches.value = -1
        assert run(items(good, bad, good), 3, 4, 0, None, C.byref(launches)) == INV, bad     # a malformed item among good ones
        assert launches.value == 0
    # well-formed: only now is the device missed (CPU run), with and without the counter
    launches.value = -1
    assert run(items(good, good), 2, 4, 0, None, C.byref(launches)) == imp.IMP_ERROR_DEVICE
    assert launches.value == 0
    assert run(items(good), 1, 4, 1, None, None) == imp.IMP_ERROR_DEVICE
    assert imp.batch_resize_mixed([good, good], 4, count_launches=True) == (imp.IMP_ERROR_DEVICE, 0)
    assert imp.batch_resize_mixed([good, good], 4) == imp.IMP_ERROR_DEVICE                    # (the old return value)
