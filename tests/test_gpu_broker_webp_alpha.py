"""WebP uploads with alpha (VP8X + ALPH + `VP8 `) through a broker started with --webp-accept alpha: they join the batch's
one impgpu_batch_decode_webp_ex call and answer byte for byte what the same requests answer when the worker decodes on the
host (Pillow's RGBA frame) and sends the pixels as IMPB_IN_FI32.  With --webp-accept all such a file is still NOT_TAKEN.
The broker-starting helpers are test_gpu_broker_webp.py's."""
import os
import subprocess

import pytest

import webp_alpha_dec_fixtures as F
import webp_dec_fixtures as L
import webp_lossy_dec_fixtures as LY
from test_gpu_broker import scaling  # noqa: F401  (fixture, by import)
from test_gpu_broker_webp import _answers

pytestmark = pytest.mark.gpu
ALPHA = ("h_mask_vp8l_gradient_pre1", "h_noise_raw_vertical_129x3", "p_checker_q50_m4", "h_chunks_around", "p_ramp_q100_m6", "h_saturate_raw_gradient")


def _uploads(as_files):
    picked = [F.get(n) for n in ALPHA] + [f for f in LY.load() if f[0] == "p_photo_160x120_q50_m0"] + [f for f in L.load() if f[0] == "p_noise_160x120_m0"]
    return [("file", blob) if as_files else ("fi32", frame) for _, blob, frame in picked]


def test_alpha_uploads_answer_as_their_pixels_do(scaling):  # noqa: F811
    pid = os.getpid()
    for together in (False, True):
        files = _answers(scaling, "/impgpu-test-webpa-f%d-%d" % (together, pid), ["--webp-accept", "alpha"], _uploads(True), together)
        pixels = _answers(scaling, "/impgpu-test-webpa-p%d-%d" % (together, pid), [], _uploads(False), together)
        assert all(g is not None for g in files + pixels)
        assert all((rc, code) == (0, 0) for rc, code, _ in files), [g[:2] for g in files]
        for k, (f, p) in enumerate(zip(files, pixels)):
            assert f == p, (together, k)


def test_with_all_an_alpha_file_is_still_not_taken_and_the_usage_line_names_the_value(scaling):  # noqa: F811
    from ngx_http_imgproc_amd import broker as B
    from ngx_http_imgproc_amd.build import BROKER

    pid = os.getpid()
    alpha, lossy = _uploads(True)[0], _uploads(True)[-2]
    got = _answers(scaling, "/impgpu-test-webpa-l-%d" % pid, ["--webp-accept", "all"], [alpha, lossy], False)
    assert [g[:2] for g in got] == [(0, B.NOT_TAKEN), (0, 0)]
    got = _answers(scaling, "/impgpu-test-webpa-a-%d" % pid, ["--webp-accept", "alpha"],
                   [alpha, lossy, ("file", dict(F.damaged())["d_method2"]), ("file", dict(F.refused())["r_alph_twice"])], False)
    assert [g[:2] for g in got] == [(0, 0), (0, 0), (0, B.NOT_TAKEN), (0, B.NOT_TAKEN)]
    p = subprocess.run([BROKER, "--webp-accept", "nonsense"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--webp-accept none|lossless|all|alpha" in p.stderr
