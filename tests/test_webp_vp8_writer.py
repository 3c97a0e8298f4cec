"""tests/webp_vp8_writer.py -- the model of the lossy WebP answer, written from include/impgpu.h's paragraph alone -- against
libwebp: every case file opens in Pillow, and Pillow's pixels equal, exactly, the model's own reconstruction passed through a
numpy statement of libwebp's output conversion (fancy upsampling, fixed-point YUV -> RGB).  Exact equality over frames of
several macroblocks is the proof that the tables, the inverse transforms, the border rule and the contexts are the
decoder's: any drift compounds across the frame.  The cases are the smallest at which each rule can go wrong; CASES and
encoded() are shared with the host twin's, the sanitizers' and the device's tests."""
import functools
import io
import os
import re

import numpy as np
import pytest
from PIL import Image

import webp_vp8_tables as T
import webp_vp8_writer as V
from conftest import ROOT

WAVES = 8                                                    # macroblock rows the device keeps in flight (VP8_WAVES)
# width x height: padding and odd chroma cells; one macroblock; a second column; 3x3 macroblocks (every border rule and an
# interior); two rows = 2 partitions; nine rows = 8 partitions, partition 0 holding two; more rows than are in flight, plus one
SIZES = [(1, 1), (15, 17), (16, 16), (17, 16), (33, 47), (130, 20), (40, 136), (24, 16 * (WAVES + 1) + 1)]


def content(kind, w, h):
    rng = np.random.default_rng(w * 1000 + h)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise_bgr":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "noise_gray":
        return rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    if kind == "ramp_bgr":
        return np.stack([(3 * x + y) % 256, (x + 2 * y) % 256, (255 - 2 * x - y) % 256], axis=2).astype(np.uint8)
    if kind == "ramp_gray":
        return ((2 * x + 3 * y) % 256).astype(np.uint8).reshape(h, w, 1).copy()
    if kind == "flat_bgr":
        return np.ascontiguousarray(np.broadcast_to(np.array([40, 200, 90], np.uint8), (h, w, 3)))
    if kind == "stripes_bgr":                                 # saturated: the reconstruction clamps
        f = np.zeros((h, w, 3), np.uint8)
        f[:, (x[0] // 3) % 2 == 0] = (255, 0, 255)
        f[(y[:, 0] // 5) % 2 == 0] ^= 255
        return f
    if kind == "stripes_gray":
        return (((x // 2 + y // 3) % 2) * 255).astype(np.uint8).reshape(h, w, 1).copy()
    if kind == "alpha_bgra":
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        f[..., :3] = content("ramp_bgr", w, h)
        return f
    if kind == "opaque_bgra":
        f = np.full((h, w, 4), 255, np.uint8)
        f[..., :3] = content("ramp_bgr", w, h)
        return f
    raise KeyError(kind)


def _cases():
    cases = {}
    for w, h in SIZES:
        cases["noise_bgr_%dx%d_q100" % (w, h)] = (content("noise_bgr", w, h), 100)     # levels of 67 and more: the longest category
        cases["ramp_bgr_%dx%d_q75" % (w, h)] = (content("ramp_bgr", w, h), 75)
    for kind, q in [("flat_bgr", 50), ("stripes_bgr", 50), ("stripes_gray", 0), ("alpha_bgra", 75), ("opaque_bgra", 50), ("noise_gray", 100),
                    ("ramp_gray", 0), ("ramp_bgr", 0), ("ramp_bgr", 50), ("ramp_bgr", 100), ("noise_bgr", 50)]:
        cases["%s_33x47_q%d" % (kind, q)] = (content(kind, 33, 47), q)
    cases["alpha_bgra_15x17_q50"] = (content("alpha_bgra", 15, 17), 50)               # an odd ALPH chunk: the pad byte
    cases["flat_bgr_40x136_q75"] = (content("flat_bgr", 40, 136), 75)                 # empty partitions
    return cases


CASES = _cases()


@functools.lru_cache(maxsize=None)
def encoded(name):
    frame, q = CASES[name]
    return V.encode(frame, q)


def pillow(blob):
    im = Image.open(io.BytesIO(blob))
    im.load()
    assert im.format == "WEBP"
    return im


@pytest.mark.parametrize("name", sorted(CASES))
def test_pillow_shows_the_models_reconstruction(name):
    frame, q = CASES[name]
    h, w, c = frame.shape
    e = encoded(name)
    im = pillow(e.file)
    assert im.size == (w, h)
    varied = c == 4 and not (frame[..., 3] == 255).all()
    assert im.mode == ("RGBA" if varied else "RGB")
    got = np.asarray(im)
    assert np.array_equal(got[..., :3], V.decoded_rgb(e.y, e.u, e.v, w, h))
    if varied:
        assert np.array_equal(got[..., 3], frame[..., 3])
    assert (b"VP8X" in e.file[:20]) == varied


def test_the_cases_reach_what_they_are_for():
    assert np.abs(encoded("noise_bgr_33x47_q100").levels).max() >= 67
    assert encoded("flat_bgr_33x47_q50").skipped[1:].all()
    assert len(encoded("ramp_bgr_130x20_q75").partitions) == 2
    assert len(encoded("ramp_bgr_40x136_q75").partitions) == 8
    assert len(encoded("ramp_bgr_24x%d_q75" % (16 * (WAVES + 1) + 1)).partitions) == 8
    e = encoded("stripes_bgr_33x47_q50")
    assert e.y.max() == 255 or e.y.min() == 0                         # the clamp was reached
    modes = np.concatenate([encoded(n).ymodes for n in CASES])
    assert set(modes.tolist()) == {V.DC, V.V, V.H, V.TM}
    assert len(encoded("alpha_bgra_15x17_q50").file) % 2 == 0


def test_quality_buys_psnr():
    frame = content("ramp_bgr", 33, 47)
    psnr = []
    for q in (10, 90):
        e = V.encode(frame, q)
        rgb = V.decoded_rgb(e.y, e.u, e.v, 33, 47).astype(np.float64)
        psnr.append(10 * np.log10(255.0 ** 2 / np.mean((rgb - frame[..., ::-1]) ** 2)))
    assert psnr[1] > psnr[0]
    assert V.quant_index(0) == 127 and V.quant_index(100) == 0 and V.quant_index(75) == 32


def test_the_headers_tables_are_the_models():
    text = open(os.path.join(ROOT, "include", "impgpu_vp8_tables.h")).read()
    for name, want in [("COEF_PROBS", T.COEF_PROBS), ("UPDATE_PROBS", T.UPDATE_PROBS), ("DC_STEPS", T.DC_STEPS), ("AC_STEPS", T.AC_STEPS)]:
        body = re.search(r"#define IMPGPU_VP8_%s \{(.*?)\}" % name, text, re.S).group(1)
        assert [int(v) for v in re.findall(r"\d+", body)] == want, name
    assert len(T.COEF_PROBS) == len(T.UPDATE_PROBS) == 4 * 8 * 3 * 11 and len(T.DC_STEPS) == len(T.AC_STEPS) == 128
