"""tests/webp_writer.py IS the definition of the lossless WebP file (include/impgpu.h, "WEBP ANSWERS"); this file checks
the definition against an independent implementation: every file the writer makes must decode, with Pillow's libwebp, to
exactly the pixels that went in -- colour and alpha.  Shapes from 1 x 1 over one tile exactly to several tiles with ragged
edges; contents from noise to flat colour (every code in the simple form); every predictor mode through forced modes.  The
CASES are shared with the host twin's and the device's tests."""
import struct

import numpy as np
import pytest

import webp_writer as W

import ngx_http_imgproc_amd as imp

T = 1 << W.TILE_BITS
# width x height
SHAPES = [(1, 1), (1, 70), (70, 1), (2, 2), (17, 37), (T, T), (T + 1, T), (33, 65)]


def _rng(name, w, h):
    return np.random.default_rng(sum(name.encode()) * 1000003 + w * 131 + h)


def content(name, w, h):
    rng = _rng(name, w, h)
    y, x = np.mgrid[0:h, 0:w]
    if name == "noise_bgr":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if name == "noise_gray":
        return rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
    if name == "gradient_bgr":
        base = np.stack([3 * x + y, 2 * x + 2 * y, x + 3 * y], axis=2)
        return ((base + rng.integers(0, 4, (h, w, 3))) & 255).astype(np.uint8)
    if name == "gradient_gray":
        return (((2 * x + 3 * y)[..., None] + rng.integers(0, 3, (h, w, 1))) & 255).astype(np.uint8)
    if name == "flat_bgr":
        return np.broadcast_to(np.array([200, 130, 77], np.uint8), (h, w, 3)).copy()
    if name == "flat_black":                                         # (0,0)'s residual is 0 too: every code is simple
        return np.zeros((h, w, 3), np.uint8)
    if name == "two_colours":
        pick = rng.integers(0, 2, (h, w))
        return np.array([[10, 200, 30], [250, 20, 90]], np.uint8)[pick]
    if name == "bgra_holes":
        f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        f[..., 3] = np.where(rng.integers(0, 3, (h, w)) == 0, 0, 255)
        return f
    if name == "bgra_graded":
        f = np.stack([3 * x + y, 2 * x + 2 * y, x + 3 * y, 5 * x + 7 * y], axis=2)
        return ((f + rng.integers(0, 3, (h, w, 4))) & 255).astype(np.uint8)
    assert name == "bgra_opaque", name
    f = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    f[..., 3] = 255
    return f


CONTENTS = ["noise_bgr", "noise_gray", "gradient_bgr", "gradient_gray", "flat_bgr", "flat_black", "two_colours", "bgra_holes", "bgra_graded",
            "bgra_opaque"]
CASES = {"%s_%dx%d" % (name, w, h): content(name, w, h) for name in CONTENTS for (w, h) in SHAPES}


def forced_cases():
    """three shapes with a random mode per tile, every mode 0..13 present in each"""
    out = []
    for k, (w, h, name) in enumerate([(33, 65, "gradient_bgr"), (70, 70, "bgra_graded"), (130, 67, "noise_gray")]):
        tx, ty = W.tiles_of(w, h)
        assert tx * ty >= W.MODES
        rng = np.random.default_rng(40 + k)
        modes = np.concatenate([np.arange(W.MODES), rng.integers(0, W.MODES, tx * ty - W.MODES)]).astype(np.uint8)
        rng.shuffle(modes)
        assert set(modes.tolist()) == set(range(W.MODES))
        out.append(("%s_%dx%d" % (name, w, h), content(name, w, h), modes))
    return out


def expect_pixels(frame, mode):
    """what Pillow must return for `frame`: R,G,B[,A]"""
    a = W.argb_of(frame)
    if mode == "RGBA":
        return np.stack([a[..., 1], a[..., 2], a[..., 3], a[..., 0]], axis=2).astype(np.uint8)
    assert mode == "RGB", mode
    assert (a[..., 0] == 255).all(), "an RGB answer for a frame with alpha"
    return np.stack([a[..., 1], a[..., 2], a[..., 3]], axis=2).astype(np.uint8)


def decodes_to(blob, frame):
    mode, px = W.decode(blob)
    return np.array_equal(px, expect_pixels(frame, mode))


def check_structure(blob, frame):
    h, w = frame.shape[:2]
    c = 1 if frame.ndim == 2 else frame.shape[2]
    assert blob[:4] == b"RIFF" and blob[8:16] == b"WEBPVP8L"
    riff, = struct.unpack("<I", blob[4:8])
    payload, = struct.unpack("<I", blob[16:20])
    assert riff == len(blob) - 8 and len(blob) % 2 == 0
    assert len(blob) == 20 + payload + (payload & 1)
    if payload & 1:
        assert blob[-1] == 0
    assert blob[20] == 0x2F
    bits = int.from_bytes(blob[21:25], "little")
    assert (bits & 0x3FFF) + 1 == w and ((bits >> 14) & 0x3FFF) + 1 == h and (bits >> 29) == 0
    assert ((bits >> 28) & 1) == int(c == 4 and bool((frame[..., 3] != 255).any()))
    assert len(blob) <= imp.webp_encode_bound(w, h, c)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_file_decodes_to_its_pixels(name):
    frame = CASES[name]
    blob = W.write(frame)
    check_structure(blob, frame)
    assert decodes_to(blob, frame)
    assert W.file_size(frame) == len(blob)


@pytest.mark.parametrize("name,frame,modes", forced_cases(), ids=[c[0] for c in forced_cases()])
def test_every_predictor_mode_decodes(name, frame, modes):
    blob = W.write(frame, forced_modes=modes)
    check_structure(blob, frame)
    assert decodes_to(blob, frame)


@pytest.mark.parametrize("mode", range(W.MODES))
def test_each_mode_alone(mode):
    frame = content("bgra_graded", 37, 21)
    tx, ty = W.tiles_of(37, 21)
    assert decodes_to(W.write(frame, forced_modes=np.full(tx * ty, mode, np.uint8)), frame)


@pytest.mark.parametrize("tile_bits", [3, 4, 5])
def test_the_other_tile_sizes_decode_too(tile_bits):
    frame = content("gradient_bgr", 70, 45)
    assert decodes_to(W.write(frame, tile_bits=tile_bits), frame)


def test_a_flat_black_frame_is_all_simple_codes():
    """every code has one used symbol: 98 + 51 header bits, no bit for any tile or pixel, whatever the size"""
    for (w, h) in SHAPES:
        assert len(W.write(CASES["flat_black_%dx%d" % (w, h)])) == 40


def test_a_gray_frame_is_its_bgr_frame():
    g = content("noise_gray", 33, 20)
    assert W.write(g) == W.write(np.repeat(g, 3, axis=2)) == W.write(g[..., 0])


def test_the_chooser_leaves_mode_0_to_the_edges_of_a_ramp():
    """a pure horizontal ramp: L leaves a constant residual, 0xff000000 leaves the ramp itself"""
    h, w = 4 * T, 6 * T
    ramp = np.broadcast_to((2 * np.arange(w, dtype=np.int64))[None, :, None] & 255, (h, w, 3)).astype(np.uint8)
    modes = W.chosen_modes(ramp)
    assert modes.shape == (4, 6)
    assert (modes[1:, 1:] != 0).all()
    assert decodes_to(W.write(ramp), ramp)


def test_a_tie_goes_to_the_lowest_mode():
    """flat black: every mode predicts 0xff000000-equal residuals of zero cost"""
    assert (W.chosen_modes(np.zeros((40, 40, 3), np.uint8)) == 0).all()


def test_the_bound_refuses_what_the_calls_refuse():
    assert imp.webp_encode_bound(16384, 16384, 4) > 0
    for (w, h, c) in [(0, 1, 3), (1, 0, 3), (16385, 1, 3), (1, 16385, 1), (4, 4, 2), (4, 4, 5)]:
        assert imp.webp_encode_bound(w, h, c) == 0
