"""impgpu_batch_decode_png answers malformed arguments on the host, before it looks for a device, and a well-formed call
without impgpu_env_start with IMP_ERROR_DEVICE (runs without a GPU)."""
import ctypes as C
import io

import numpy as np
from PIL import Image


def _png(h, w):
    b = io.BytesIO()
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(b, "PNG")
    return b.getvalue()


def test_batch_decode_png_checks_its_arguments_before_the_device():
    import ngx_http_imgproc_amd as imp

    lib = imp.lib
    INV = imp.IMP_ERROR_INVALID_ARGS
    keep = [_png(4, 5), _png(7, 3)]
    n = len(keep)
    blobs = (C.c_char_p * n)(*keep)
    sizes = (C.c_size_t * n)(*[len(b) for b in keep])
    images = (C.c_void_p * n)()
    codes = (C.c_int * n)(*[-1] * n)
    launches = C.c_int(-1)

    dec = lib.impgpu_batch_decode_png
    assert dec(None, sizes, n, images, codes, C.byref(launches)) == INV
    assert dec(blobs, None, n, images, codes, None) == INV
    assert dec(blobs, sizes, n, None, codes, None) == INV
    assert dec(blobs, sizes, n, images, None, None) == INV
    assert dec(blobs, sizes, -1, images, codes, None) == INV
    assert dec(blobs, sizes, 257, images, codes, None) == INV
    assert list(codes) == [-1] * n                          # nothing answered for a malformed call
    assert launches.value == -1

    # well-formed: only now is the device missed (CPU run: impgpu_env_start has not been called)
    assert dec(blobs, sizes, n, images, codes, C.byref(launches)) == imp.IMP_ERROR_DEVICE
    assert launches.value == 0
    assert list(images) == [None] * n
    assert dec(blobs, sizes, 0, images, codes, None) == imp.IMP_ERROR_DEVICE


def test_batch_decode_png_wrapper_raises_without_a_device():
    import ngx_http_imgproc_amd as imp

    try:
        imp.batch_decode_png([_png(2, 2)])
    except imp.ImpError as e:
        assert e.code == imp.IMP_ERROR_DEVICE
    else:
        raise AssertionError("a batch decode without impgpu_env_start returned")
