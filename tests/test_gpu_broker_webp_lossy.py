"""WebP uploads through a broker started with --webp-accept all: lossy (VP8 key frame) and lossless files join the batch's
one impgpu_batch_decode_webp_ex call and answer byte for byte what the same requests answer when the worker decodes on the
host and sends the pixels as IMPB_IN_FI32.  With --webp-accept lossless a lossy file is still NOT_TAKEN.  The
broker-starting helpers are test_gpu_broker_webp.py's."""
import os
import subprocess

import pytest

import webp_dec_fixtures as L
import webp_lossy_dec_fixtures as F
from test_gpu_broker import scaling  # noqa: F401  (fixture, by import)
from test_gpu_broker_webp import _answers

pytestmark = pytest.mark.gpu
LOSSY = ("p_photo_160x120_q50_m0", "p_screen_160x120_q75_m0", "h_inner_edges", "p_dither_53x37_q90_m6")
LOSSLESS = ("p_tiling_318x222_m3", "p_noise_160x120_m0")


def _uploads(as_files):
    fx = {f[0]: f for f in F.load()}
    lx = {f[0]: f for f in L.load()}
    picked = [fx[n] for n in LOSSY] + [lx[n] for n in LOSSLESS]
    return [("file", blob) if as_files else ("fi32", frame) for _, blob, frame in picked]


def test_lossy_and_lossless_uploads_answer_as_their_pixels_do(scaling):  # noqa: F811
    pid = os.getpid()
    for together in (False, True):
        files = _answers(scaling, "/impgpu-test-webpl-f%d-%d" % (together, pid), ["--webp-accept", "all"], _uploads(True), together)
        pixels = _answers(scaling, "/impgpu-test-webpl-p%d-%d" % (together, pid), [], _uploads(False), together)
        assert all(g is not None for g in files + pixels)
        assert all((rc, code) == (0, 0) for rc, code, _ in files), [g[:2] for g in files]
        for k, (f, p) in enumerate(zip(files, pixels)):
            assert f == p, (together, k)


def test_with_lossless_a_lossy_file_is_still_not_taken(scaling):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B
    from ngx_http_imgproc_amd.build import BROKER

    pid = os.getpid()
    lossy, lossless = _uploads(True)[0], _uploads(True)[-1]
    got = _answers(scaling, "/impgpu-test-webpl-l-%d" % pid, ["--webp-accept", "lossless"], [lossy, lossless], False)
    assert [g[:2] for g in got] == [(0, B.NOT_TAKEN), (0, 0)]
    got = _answers(scaling, "/impgpu-test-webpl-a-%d" % pid, ["--webp-accept", "all"], [lossy, lossless, ("file", dict(F.damaged())["d_badstart"]), ("file", dict(F.refused())["r_alph"])], False)
    assert [g[:2] for g in got] == [(0, 0), (0, 0), (0, B.NOT_TAKEN), (0, B.NOT_TAKEN)]
    p = subprocess.run([BROKER, "--webp-accept", "nonsense"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--webp-accept none|lossless|all" in p.stderr
