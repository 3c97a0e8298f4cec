"""A broker started with --jpeg-accept progressive decodes progressive JPEG uploads on the device: every answer is the
oracle's file for Pillow's pixels, and progressive and sequential uploads share batches.  Without the option the same
uploads stay NOT_TAKEN.  The broker-starting helpers are test_gpu_broker.py's (each broker child runs under their limits)."""
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_broker import scaling  # noqa: F401  (fixture, by import)
from test_gpu_chain import oracle_chain
from test_jpeg_prog_host import EXPECTED, fixture, old_fixture, written

pytestmark = pytest.mark.gpu


def _work():
    """(upload, the oracle's answer)"""
    work = []
    for name in ("c420_q50_400x300", "gray_q75_640x480", "c420_q10_smooth_320x240", "c444_q100_noise_64x48", "c420_q90_dri4_95x51"):
        work.append((fixture(name, "prog"), EXPECTED[name]))
    for name in ("c420_q50_400x300", "c444_q100_noise_64x48"):          # sequential uploads in the same gathers
        blob = fixture(name, "seq")
        rc, want = orc.jpeg_decode(blob)
        assert rc == 0
        work.append((blob, want))
    rc, want = orc.jpeg_decode(old_fixture("c420_q30_noise_64x64"))
    work.append((written("c420_q30_noise_64x64", "mozjpeg_like"), want))
    out = []
    for blob, pixels in work:
        rc, _, small = oracle_chain(pixels, resize="160,0")
        assert rc == 0
        rc, answer = orc.jpeg_encode(small, 86)
        assert rc == 0
        out.append((blob, answer))
    return out


def test_progressive_uploads_through_the_broker(scaling):  # noqa: F811
    name = "/impgpu-test-jprog-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=3000, slots=16, extra=["--slot-mb", "8", "--jpeg-accept", "progressive"])
    try:
        from ngx_http_imgproc_amd import broker as B

        work = _work()
        errors, sizes = [], []
        start = threading.Barrier(len(work))

        def one(k):
            blob, want = work[k]
            c = B.Client(name)
            try:
                for _ in range(4):
                    start.wait()
                    rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=B.OUT_JPEG, quality=86)
                    if (rc, code) != (0, 0) or got != want:
                        errors.append((k, rc, code))
                    sizes.append(a.batch_size)
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(k,)) for k in range(len(work))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert max(sizes) > 1, "no upload shared its batch"
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]


def test_a_default_broker_still_says_not_taken(scaling):  # noqa: F811
    name = "/impgpu-test-jprogn-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=0, slots=4, extra=["--slot-mb", "8"])
    try:
        from ngx_http_imgproc_amd import broker as B

        c = B.Client(name)
        try:
            work = _work()
            for blob, _ in work[:2]:
                rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=B.OUT_JPEG, quality=86)
                assert (rc, code) == (0, B.NOT_TAKEN)
            blob, want = work[5]                                         # a sequential upload is answered as ever
            rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=B.OUT_JPEG, quality=86)
            assert (rc, code) == (0, 0) and got == want
        finally:
            c.close()
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
