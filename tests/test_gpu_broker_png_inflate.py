"""PNG uploads through a broker started with --png-inflate device: the uploads' zlib streams are inflated by k_png_inflate
instead of on the broker's host threads, and every answer is byte for byte the answer of a broker started without the
option.  A value the option does not know ends the broker with status 2 and the usage text.  The broker-starting helpers
are test_gpu_broker.py's."""
import os
import subprocess
import threading

import numpy as np
import pytest

from test_gpu_broker import _photo, scaling  # noqa: F401  (fixtures, by import)
from test_gpu_broker_png_batch import _png

pytestmark = pytest.mark.gpu


def _uploads():
    """eight PNG uploads as test_gpu_broker_png_batch.py sends them (gray for JPEG answers, BGRA for PNG and frame answers, BGR
    for all three), zlib levels 0 / 1 / 6 / 9; the last one is cut in half: the same refusal both ways"""
    out = []
    for k in range(8):
        bgr = _photo(200 + 24 * k, 260 + 16 * k, 60 + k)
        src = bgr[:, :, 1:2].copy() if k in (0, 6) else np.dstack([bgr, (bgr[:, :, 1] // 2 + 90).astype(np.uint8)]) if k in (1, 5) else bgr
        out.append(_png(src, compress_level=[6, 0, 1, 9][k % 4]))
    out[7] = out[7][:len(out[7]) // 2]
    return out


def _answers(scaling, name, extra):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B

    p = scaling.start_broker(name, threads=1, gather_us=3000, slots=16, extra=["--slot-mb", "8"] + extra)
    uploads = _uploads()
    got = [None] * len(uploads)
    try:
        start = threading.Barrier(len(uploads))

        def one(k):
            c = B.Client(name)
            try:
                start.wait()
                kind = [B.OUT_JPEG, B.OUT_PNG, B.OUT_FRAME][k % 3]
                rc, code, step, answer, a = c.run(blob=uploads[k], resize="160,0", out=kind, quality=86)
                got[k] = (rc, code, answer.tobytes() if isinstance(answer, np.ndarray) else answer)
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(k,)) for k in range(len(uploads))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
    return got


def test_png_uploads_with_the_device_inflate(scaling):  # noqa: F811
    host = _answers(scaling, "/impgpu-test-pnginf-h-%d" % os.getpid(), [])
    dev = _answers(scaling, "/impgpu-test-pnginf-d-%d" % os.getpid(), ["--png-inflate", "device"])
    assert all(g is not None for g in host + dev)
    answered = sum(1 for rc, code, _ in host if (rc, code) == (0, 0))
    assert 4 <= answered < 8, [g[:2] for g in host]
    for k, (h, d) in enumerate(zip(host, dev)):
        assert h == d, k
    from ngx_http_imgproc_amd.build import BROKER

    p = subprocess.run([BROKER, "--png-inflate", "nonsense"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage: impgpu_broker" in p.stderr and "--png-inflate host|device" in p.stderr
