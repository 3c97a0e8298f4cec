"""Gray uploads through the broker: baseline gray JPEG and 8-bit gray PNG files decode on the device to one-channel frames,
and their requests now ride impgpu_batch_run_ops' shared launches (gray resize -> promotion -> the BGR groups).  Alone or
eight to a batch, every answer must be the file the oracle writes for that request."""
import os
import threading

import numpy as np
import pytest

import oracle_lib as orc
import png_enc_model as model
from conftest import noise_image, smooth_image
from png_writer import write_png
from test_gpu_broker import _client, broker, scaling  # noqa: F401  (fixtures, by import)
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu

JOBS = [dict(resize="120,0"), dict(crop="1,1,c,c", resize="100,0", filters=["gamma=1.4"])]


def _uploads():
    """(file, the gray frame the oracle decodes from it): four JPEG and four PNG files of eight sizes, odd widths among them."""
    out = []
    for k in range(8):
        h, w = 203 + 31 * k, 301 + 47 * k
        a = smooth_image(h, w, 1, 90 + k) if k % 4 < 2 else noise_image(h, w, 1, 2300 + k)
        if k % 2:
            blob = write_png(a[:, :, 0], [y % 5 for y in range(h)], 0)
            rc, frame = orc.png_decode(blob)
        else:
            rc, blob = orc.jpeg_encode(a, 90)
            assert rc == 0
            rc, frame = orc.jpeg_decode(blob)
        assert rc == 0 and frame.shape == (h, w, 1), (rc, frame.shape)
        out.append((blob, frame))
    return out


def _cases(B):
    """(request, the oracle's answer file) for every upload, job and answer format."""
    cases = []
    for blob, frame in _uploads():
        for job in JOBS:
            rc, _, small = oracle_chain(frame, **job)
            assert rc == 0 and small.shape[2] == 3                     # promoted at the filtering step (bridge.c:613-618)
            rc, jpg = orc.jpeg_encode(small, 86)
            assert rc == 0
            cases.append((dict(blob=blob, out=B.OUT_JPEG, quality=86, **job), jpg))
            cases.append((dict(blob=blob, out=B.OUT_PNG, quality=9, **job), model.encode(small)))
    return cases


def test_gray_uploads_alone(broker):  # noqa: F811
    name, _ = broker
    B, c = _client(name)
    try:
        for kw, want in _cases(B):
            rc, code, step, got, a = c.run(**kw)
            assert (rc, code) == (0, 0), (kw["resize"], kw["out"], rc, code, step, B.Client.last_error())
            assert got == want, (kw["resize"], kw["out"], len(kw["blob"]))
    finally:
        c.close()


def test_gray_uploads_eight_to_a_batch(scaling):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B

    cases = _cases(B)
    n_clients = 8
    name = "/impgpu-test-gray-%d" % os.getpid()
    # one lane that launches as soon as eight requests are in (or after 0.2 s): the eight clients, released together, share it
    p = scaling.start_broker(name, threads=1, gather_us=200000, slots=16, extra=["--slot-mb", "8", "--batch", str(n_clients)])
    errors, sizes = [], []
    try:
        start = threading.Barrier(n_clients)

        def one(t):
            c = B.Client(name)
            try:
                for r in range(len(cases) // n_clients):
                    kw, want = cases[(r * n_clients + 5 * t) % len(cases)]
                    start.wait(timeout=120)
                    rc, code, step, got, a = c.run(**kw)
                    sizes.append(a.batch_size)
                    if (rc, code) == (0, 0) and a.channels != 3:
                        errors.append((t, "answer channels", a.channels))   # (promoted: bridge.c:613-618)
                    if (rc, code) != (0, 0) or got != want:
                        errors.append((t, kw["resize"], kw["out"], rc, code, step))
            except Exception as e:                                     # (reported below, in the test's thread)
                errors.append((t, repr(e)))
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(t,)) for t in range(n_clients)]
        for th in ts:
            th.start()
        for th in ts:
            th.join(timeout=600)
        assert not any(th.is_alive() for th in ts)
    finally:
        err = scaling.stop_broker(p)
    assert p.returncode == 0, err[-800:]
    assert not errors, errors[:8]
    assert max(sizes) == n_clients, sizes                              # eight gray uploads of different workers in one batch
