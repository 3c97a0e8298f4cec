"""impgpu_batch_run_ops answers malformed arguments on the host, before it looks for a device (runs without a GPU)."""
import ctypes as C


def test_batch_run_ops_checks_its_arguments_before_the_device():
    import ngx_http_imgproc_amd as imp
    from ngx_http_imgproc_amd._lib import CConfig, CJob

    lib = imp.lib
    INV = imp.IMP_ERROR_INVALID_ARGS
    bufs = [(C.c_ubyte * 64)() for _ in range(3)]
    n = 3
    # stand-ins for three handles: never dereferenced, the call refuses or misses the device first
    images = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in bufs])
    jobs = (CJob * n)()
    cfg = CConfig()
    cfgs = (C.POINTER(CConfig) * n)(*[C.pointer(cfg)] * n)
    codes = (C.c_int * n)(*[-1] * n)
    steps = (C.c_int * n)(*[-1] * n)
    launches = C.c_int(-1)

    run = lib.impgpu_batch_run_ops
    assert run(None, jobs, cfgs, n, codes, steps, C.byref(launches)) == INV
    assert launches.value == 0
    assert run(images, None, cfgs, n, codes, steps, None) == INV
    assert run(images, jobs, None, n, codes, steps, None) == INV
    assert run(images, jobs, cfgs, n, None, steps, None) == INV
    assert run(images, jobs, cfgs, n, codes, None, None) == INV
    assert run(images, jobs, cfgs, -1, codes, steps, None) == INV
    assert run(images, jobs, cfgs, 4097, codes, steps, None) == INV
    assert list(codes) == [-1] * n                          # nothing answered for a malformed call

    twice = (C.c_void_p * n)(images[0], images[1], images[0])
    assert run(twice, jobs, cfgs, n, codes, steps, None) == INV
    assert list(codes) == [-1] * n

    # well-formed: only now is the device missed, as by the other batch entry points (CPU run)
    assert run(images, jobs, cfgs, n, codes, steps, C.byref(launches)) == imp.IMP_ERROR_DEVICE
    assert list(codes) == [imp.IMP_ERROR_DEVICE] * n and list(steps) == [0] * n
    assert launches.value == 0
    assert run(images, jobs, cfgs, 0, codes, steps, None) == imp.IMP_ERROR_DEVICE
    # NULL entries are requests of their own (impgpu_run_ops answers them), not a malformed call
    holes = (C.c_void_p * n)(None, images[1], None)
    assert run(holes, jobs, cfgs, n, codes, steps, None) == imp.IMP_ERROR_DEVICE
