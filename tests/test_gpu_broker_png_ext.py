"""A broker started with --png-accept all decodes palette, 1/2/4-bit gray and Adam7 uploads on the device: every answer is
the oracle's file for Pillow's pixels, and the uploads share batches.  Without the option the same uploads stay NOT_TAKEN.
The broker-starting helpers are test_gpu_broker.py's."""
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
import png_ext_writer as W
from test_gpu_broker import scaling  # noqa: F401  (fixture, by import)
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu


def _work():
    rng = np.random.default_rng(0xB60)
    work = []
    for k, (colour, depth, il) in enumerate([(3, 8, 0), (3, 4, 1), (3, 1, 0), (0, 2, 0), (0, 4, 1), (2, 8, 1), (6, 8, 1), (0, 8, 1)]):
        blob, want = W.random_file(rng, colour, depth, il, 180 + 16 * k, 150 + 8 * k)
        assert np.array_equal(W.pillow(blob), want)
        rc, _, small = oracle_chain(want, resize="160,0")
        assert rc == 0
        rc, answer = orc.jpeg_encode(small, 86)
        assert rc == 0
        work.append((blob, answer))
    return work


def test_png_ext_uploads_through_the_broker(scaling):  # noqa: F811
    name = "/impgpu-test-pngx-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=3000, slots=16, extra=["--slot-mb", "8", "--png-accept", "all"])
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


def test_without_the_option_they_stay_not_taken(scaling):  # noqa: F811
    name = "/impgpu-test-pngn-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=0, slots=4, extra=["--slot-mb", "8"])
    try:
        from ngx_http_imgproc_amd import broker as B

        c = B.Client(name)
        try:
            for blob, _ in _work()[:2]:
                rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=B.OUT_JPEG, quality=86)
                assert (rc, code) == (0, B.NOT_TAKEN)
        finally:
            c.close()
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
