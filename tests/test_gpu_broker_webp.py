"""WebP uploads through a broker started with --webp-accept lossless: an IMPB_IN_FILE request whose bytes start
RIFF....WEBP is decoded on the device (impgpu_batch_decode_webp) and its answer is byte for byte the answer the worker gets
today by decoding on the host and sending the pixels as IMPB_IN_FI32 -- alone, and eight to a batch mixed with JPEG and PNG
uploads.  A lossy file is NOT_TAKEN; without the option every WebP file is NOT_TAKEN as before.  The broker-starting
helpers are test_gpu_broker.py's."""
import os
import subprocess
import threading

import numpy as np
import pytest

import webp_dec_fixtures as F
from test_gpu_broker import _photo, scaling  # noqa: F401  (fixtures, by import)
from test_gpu_broker_png_batch import _png

pytestmark = pytest.mark.gpu
NAMES = ("p_tiling_318x222_m3", "p_flat_300x300_m6", "p_noise_160x120_m0", "p_tiling_318x222_m0")


def _webps():
    fx = {f[0]: f for f in F.load()}
    return [(fx[n][1], fx[n][2]) for n in NAMES]


def _send(B, c, k, upload, kind):
    """upload: ("file", bytes) or ("fi32", B,G,R,A frame: FreeImage's bitmap is its rows bottom-up)"""
    quality = 6 if kind == B.OUT_PNG else 86                 # (a PNG answer's `quality` is its compression level)
    if upload[0] == "file":
        rc, code, step, answer, a = c.run(blob=upload[1], resize="120,0", out=kind, quality=quality)
    else:
        rc, code, step, answer, a = c.run(fi32=np.ascontiguousarray(upload[1][::-1]).reshape(upload[1].shape[0], -1), resize="120,0", out=kind, quality=quality)
    return rc, code, answer.tobytes() if isinstance(answer, np.ndarray) else answer


def _answers(scaling, name, extra, uploads, together):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B

    p = scaling.start_broker(name, threads=1, gather_us=3000 if together else 0, slots=16, extra=["--slot-mb", "8"] + extra)
    got = [None] * len(uploads)
    try:
        if together:
            start = threading.Barrier(len(uploads))

            def one(k):
                c = B.Client(name)
                try:
                    start.wait()
                    got[k] = _send(B, c, k, uploads[k], [B.OUT_JPEG, B.OUT_PNG, B.OUT_FRAME][k % 3])
                finally:
                    c.close()

            ts = [threading.Thread(target=one, args=(k,)) for k in range(len(uploads))]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
        else:
            c = B.Client(name)
            try:
                for k in range(len(uploads)):
                    got[k] = _send(B, c, k, uploads[k], [B.OUT_JPEG, B.OUT_PNG, B.OUT_FRAME][k % 3])
            finally:
                c.close()
    finally:
        err = scaling.stop_broker(p)
        assert p.returncode == 0, err[-800:]
    return got


def _batch(as_files):
    """eight uploads: four WebP files (or their frames as FreeImage bitmaps), two JPEG and two PNG files"""
    from PIL import Image
    import io

    out = []
    webps = _webps()
    for k in range(8):
        if k % 2 == 0:
            blob, frame = webps[k // 2]
            out.append(("file", blob) if as_files else ("fi32", frame))
        elif k % 4 == 1:
            bio = io.BytesIO()
            Image.fromarray(_photo(200 + 8 * k, 260, 70 + k)[:, :, ::-1]).save(bio, "JPEG", quality=90)
            out.append(("file", bio.getvalue()))
        else:
            out.append(("file", _png(_photo(180, 240 + 8 * k, 80 + k), compress_level=6)))
    return out


def test_webp_uploads_with_the_option_alone_and_eight_to_a_batch(scaling):  # noqa: F811
    pid = os.getpid()
    for together in (False, True):
        files = _answers(scaling, "/impgpu-test-webp-f%d-%d" % (together, pid), ["--webp-accept", "lossless"], _batch(True), together)
        pixels = _answers(scaling, "/impgpu-test-webp-p%d-%d" % (together, pid), [], _batch(False), together)
        assert all(g is not None for g in files + pixels)
        assert all((rc, code) == (0, 0) for rc, code, _ in files), [g[:2] for g in files]
        for k, (f, p) in enumerate(zip(files, pixels)):
            assert f == p, (together, k)


def test_lossy_files_and_brokers_without_the_option(scaling):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B
    from ngx_http_imgproc_amd.build import BROKER

    pid = os.getpid()
    lossless = _webps()[2][0]
    got = _answers(scaling, "/impgpu-test-webp-l-%d" % pid, ["--webp-accept", "lossless"], [("file", F.read("lossy.webp")), ("file", lossless), ("file", F.damaged()[1][1])], False)
    assert [g[:2] for g in got] == [(0, B.NOT_TAKEN), (0, 0), (0, B.NOT_TAKEN)]
    for extra in ([], ["--webp-accept", "none"]):
        got = _answers(scaling, "/impgpu-test-webp-n%d-%d" % (len(extra), pid), extra, [("file", lossless), ("file", F.read("lossy.webp"))], False)
        assert [g[:2] for g in got] == [(0, B.NOT_TAKEN), (0, B.NOT_TAKEN)]
    p = subprocess.run([BROKER, "--webp-accept", "nonsense"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "usage: impgpu_broker" in p.stderr and "--webp-accept none|lossless" in p.stderr
