"""PNG uploads through the broker: the PNG files of a batch are decoded by ONE impgpu_batch_decode_png call.  Every answer --
JPEG, PNG or frame, from a PNG or a JPEG upload, alone or sharing its batch -- must be the oracle's; a file the device does
not decode comes back IMPB_NOT_TAKEN for that request alone.  The broker-starting helpers are test_gpu_broker.py's."""
import io
import os
import threading

import numpy as np
import pytest
from PIL import Image

import oracle_lib as orc
import png_enc_model as model
from test_gpu_broker import _photo, scaling  # noqa: F401  (fixtures, by import)
from test_gpu_chain import oracle_chain

pytestmark = pytest.mark.gpu


def _png(arr, mode=None, **kw):
    """arr in B,G,R(,A) order (or one channel) -> a PNG file; mode="P" writes a palette file"""
    a = arr[:, :, 0] if arr.shape[2] == 1 else arr[:, :, [2, 1, 0] + ([3] if arr.shape[2] == 4 else [])]
    im = Image.fromarray(np.ascontiguousarray(a))
    if mode:
        im = im.convert(mode)
    b = io.BytesIO()
    im.save(b, "PNG", **kw)
    return b.getvalue()


def _pillow(blob):
    a = np.asarray(Image.open(io.BytesIO(blob)))
    if a.ndim == 2:
        return a[:, :, None]
    return np.ascontiguousarray(a[:, :, [2, 1, 0] + ([3] if a.shape[2] == 4 else [])])


def _work(B):
    """(upload, answer kind, quality, what the oracle answers) -- PNG uploads of every kind the device decodes, two JPEG uploads,
    one palette PNG (the device does not decode it: NOT_TAKEN)"""
    work = []
    for k in range(10):
        bgr = _photo(200 + 24 * k, 260 + 16 * k, 40 + k)
        if k in (3, 7):
            rc, blob = orc.jpeg_encode(bgr, 90)
            rc, frame = orc.jpeg_decode(blob)
        else:
            if k in (0, 6):                                    # gray (JPEG answers: the chain turns it to BGR first)
                src = bgr[:, :, 1:2].copy()
            elif k in (1, 5):                                  # BGRA: PNG and frame answers keep the alpha
                src = np.dstack([bgr, (bgr[:, :, 1] // 2 + 90).astype(np.uint8)])
            else:
                src = bgr
            blob = _png(src, compress_level=k % 10)
            frame = _pillow(blob)
        rc, _, small = oracle_chain(frame, resize="160,0")
        assert rc == 0
        kind = [B.OUT_JPEG, B.OUT_PNG, B.OUT_FRAME][k % 3]
        if kind == B.OUT_JPEG:
            rc, want = orc.jpeg_encode(small, 86)
            work.append((blob, kind, 86, want))
        elif kind == B.OUT_PNG:
            work.append((blob, kind, 9, model.encode(small)))
        else:
            work.append((blob, kind, 86, small))
    palette = _png(_photo(90, 120, 77), mode="P")
    work.append((palette, B.OUT_JPEG, 86, None))
    return work


def test_png_uploads_from_concurrent_clients(scaling):  # noqa: F811
    """eleven clients (PNG uploads of 1 / 3 / 4 channels, two JPEG uploads, a palette PNG) send together, four rounds: every
    answer is the oracle's, batches are shared, the palette file alone is NOT_TAKEN"""
    name = "/impgpu-test-pngb-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=3000, slots=16, extra=["--slot-mb", "8"])
    try:
        from ngx_http_imgproc_amd import broker as B

        work = _work(B)
        errors, png_sizes, palette_sizes = [], [], []
        start = threading.Barrier(len(work))

        def one(k):
            blob, out, q, want = work[k]
            c = B.Client(name)
            try:
                for _ in range(4):
                    start.wait()
                    rc, code, step, got, a = c.run(blob=blob, resize="160,0", out=out, quality=q)
                    if want is None:
                        if (rc, code) != (0, B.NOT_TAKEN):
                            errors.append((k, rc, code))
                        palette_sizes.append(a.batch_size)
                        continue
                    same = np.array_equal(got, want) if out == B.OUT_FRAME else got == want
                    if (rc, code) != (0, 0) or not same:
                        errors.append((k, rc, code))
                    if blob[:4] == b"\x89PNG":
                        png_sizes.append(a.batch_size)
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(k,)) for k in range(len(work))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert max(png_sizes) > 1, "no PNG upload shared its batch"
        assert max(palette_sizes) > 1, "the palette file never shared its batch"
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]


def test_one_batch_holds_png_and_jpeg_uploads(scaling):  # noqa: F811
    """two clients, one PNG upload and one JPEG upload, sent together until one batch holds both (batch_size 2 on both
    answers: with two requests in flight that batch is the pair); both answers are the oracle's"""
    name = "/impgpu-test-pngm-%d" % os.getpid()
    p = scaling.start_broker(name, threads=1, gather_us=5000, slots=4, extra=["--slot-mb", "8"])
    try:
        from ngx_http_imgproc_amd import broker as B

        bgr = _photo(300, 400, 91)
        png = _png(bgr)
        rc, jpg = orc.jpeg_encode(_photo(280, 360, 92), 90)
        rc, jframe = orc.jpeg_decode(jpg)
        want = []
        for frame in (_pillow(png), jframe):
            rc, _, small = oracle_chain(frame, resize="160,0")
            want.append(orc.jpeg_encode(small, 86)[1])
        rounds = 20
        sizes = [[0] * rounds, [0] * rounds]
        errors = []
        start = threading.Barrier(2)

        def one(k):
            c = B.Client(name)
            try:
                for i in range(rounds):
                    start.wait()
                    rc, code, step, got, a = c.run(blob=(png, jpg)[k], resize="160,0", out=B.OUT_JPEG, quality=86)
                    if (rc, code) != (0, 0) or got != want[k]:
                        errors.append((k, i, rc, code))
                    sizes[k][i] = a.batch_size
            finally:
                c.close()

        ts = [threading.Thread(target=one, args=(k,)) for k in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert any(a == 2 and b == 2 for a, b in zip(*sizes)), sizes
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
