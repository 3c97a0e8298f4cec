"""PNG answers through the broker (IMPB_OUT_PNG): the file tests/png_enc_model.py writes for the frame the operators leave,
alone and in batches shared with JPEG answers.  The broker-starting helpers are test_gpu_broker.py's."""
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
import png_enc_model as model
from conftest import noise_image
from test_gpu_broker import _client, _photo, broker, scaling  # noqa: F401  (fixtures, by import)
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu


def test_png_answers_alone(broker):  # noqa: F811
    name, _ = broker
    B, c = _client(name)
    try:
        # a JPEG file decoded on the device, resized, answered as PNG
        rc, blob = orc.jpeg_encode(_photo(480, 640, 21), 90)
        rc, frame = orc.jpeg_decode(blob)
        rc_o, small = orc.resize(frame, "224,0")
        for level in (1, 6, 9):
            rc, code, step, got, a = c.run(blob=blob, resize="224,0", out=B.OUT_PNG, quality=level)
            assert (rc, code, rc_o) == (0, 0, 0) and got == model.encode(small)
        # a BGRA frame from a host decoder keeps its alpha; a gray one stays gray
        rgba = noise_image(120, 160, 4, 5)
        rc, code, step, got, a = c.run(frame=rgba, resize="100,60", out=B.OUT_PNG, quality=9)
        rc_o, _, want = oracle_chain(rgba, resize="100,60")
        assert (rc, code, rc_o) == (0, 0, 0) and got == model.encode(want)
        gray = noise_image(50, 70, 1, 6)
        rc, code, step, got, a = c.run(frame=gray, out=B.OUT_PNG, quality=3)
        rc_o, _, want = oracle_chain(gray)
        assert (rc, code, rc_o) == (0, 0, 0) and got == model.encode(want)
        # level 0 stays with the host encoder; other levels are refused
        rc, code, step, got, a = c.run(frame=gray, out=B.OUT_PNG, quality=0)
        assert (rc, code) == (0, 1)                          # IMP_ERROR_UNSUPPORTED
        rc, code, step, got, a = c.run(frame=gray, out=B.OUT_PNG, quality=10)
        assert (rc, code) == (0, 50)                         # IMP_ERROR_INVALID_ARGS
    finally:
        c.close()


def test_png_and_jpeg_answers_in_shared_batches(scaling):  # noqa: F811
    name = "/impgpu-test-png-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=3000, slots=16, extra=["--slot-mb", "8"])
    try:
        from ngx_http_imgproc_amd import broker as B

        work = []
        for k in range(8):
            rc, blob = orc.jpeg_encode(_photo(300 + 20 * k, 400, 30 + k), 90)
            rc, frame = orc.jpeg_decode(blob)
            rc, small = orc.resize(frame, "160,0")
            if k % 2:
                work.append((blob, B.OUT_PNG, 9, model.encode(small)))
            else:
                rc, want = orc.jpeg_encode(small, 86)
                work.append((blob, B.OUT_JPEG, 86, want))
        errors, sizes = [], []
        start = threading.Barrier(len(work))

        def one(k):
            blob, out, q, want = work[k]
            c = B.Client(name)
            try:
                for _ in range(4):
                    start.wait()
                    rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=out, quality=q)
                    if (rc, code) != (0, 0) or got != want:
                        errors.append((k, rc, code))
                    if out == B.OUT_PNG:
                        sizes.append(a.batch_size)
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(k,)) for k in range(len(work))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors
        assert max(sizes) > 1, "no PNG answer shared its batch"
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
