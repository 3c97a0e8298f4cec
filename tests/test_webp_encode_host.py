"""impgpu_webp_encode_host -- the lane code of csrc/imp_webp_enc.h (what the six launches run per lane) on one thread, no
device -- must write, byte for byte, what tests/webp_writer.py writes: on every case of test_webp_writer, on forced modes
and on random frames of mixed channel counts and row pitches.  Refusals, their codes, and that nothing is written behind a
file or on a refusal (guard bytes).  impgpu_request_webp_lossless on the request lines of the issue."""
import ctypes as C

import numpy as np
import pytest

import webp_writer as W
from test_webp_writer import CASES, content, forced_cases

import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import lib

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = imp.IMP_OK, imp.IMP_ERROR_UNSUPPORTED, imp.IMP_ERROR_MALLOC_FAILED, imp.IMP_ERROR_INVALID_ARGS


def padded(frame, pad, rng):
    """the frame as a view into rows `pad` bytes longer, the padding random"""
    h, w, c = frame.shape
    parent = rng.integers(0, 256, (h, w * c + pad), dtype=np.uint8)
    parent[:, : w * c] = frame.reshape(h, w * c)
    return np.lib.stride_tricks.as_strided(parent, shape=(h, w, c), strides=(w * c + pad, c, 1)), parent


def random_frames(seed, count):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w, h, c = int(rng.integers(1, 81)), int(rng.integers(1, 81)), int(rng.choice([1, 3, 4]))
        kind = int(rng.integers(0, 4))
        if kind == 0:
            f = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        elif kind == 1:                                             # smooth: the predictors have something to find
            y, x = np.mgrid[0:h, 0:w]
            f = ((np.stack([(k + 1) * x + (4 - k) * y for k in range(c)], axis=2) + rng.integers(0, 3, (h, w, c))) & 255).astype(np.uint8)
        elif kind == 2:                                             # few colours
            colours = int(rng.integers(1, 6))
            f = rng.integers(0, 256, (colours, c), dtype=np.uint8)[rng.integers(0, colours, (h, w))]
        else:                                                       # blocks of flat colour
            f = np.repeat(np.repeat(rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, c), dtype=np.uint8), 8, axis=0), 8, axis=1)[:h, :w]
        f = np.ascontiguousarray(f)
        if c == 4 and rng.integers(0, 2):
            f[..., 3] = 255
        out.append((f, int(rng.choice([0, 0, 1, 3, 16]))))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_writes_the_writers_bytes(name):
    frame = CASES[name]
    rc, blob, n, intact = imp.encode_webp_host(frame)
    assert rc == OK and intact
    assert blob == W.write(frame)


@pytest.mark.parametrize("name,frame,modes", forced_cases(), ids=[c[0] for c in forced_cases()])
def test_forced_modes(name, frame, modes):
    rc, blob, n, intact = imp.encode_webp_host(frame, forced_modes=modes)
    assert rc == OK and intact
    assert blob == W.write(frame, forced_modes=modes)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_frames_and_steps(seed):
    rng = np.random.default_rng(100 + seed)
    for k, (frame, pad) in enumerate(random_frames(seed, 20)):
        view, parent = padded(frame, pad, rng)
        before = parent.copy()
        rc, blob, n, intact = imp.encode_webp_host(view)
        assert rc == OK and intact, k
        assert blob == W.write(frame), (k, frame.shape, pad)
        assert np.array_equal(parent, before)


def test_capacity():
    frame = content("gradient_bgr", 33, 65)
    want = W.write(frame)
    rc, blob, n, intact = imp.encode_webp_host(frame, capacity=len(want))
    assert rc == OK and intact and blob == want
    rc, blob, n, intact = imp.encode_webp_host(frame, capacity=len(want) - 1)
    assert rc == MALLOC_FAILED and blob is None and n == len(want) and intact
    rc, blob, n, intact = imp.encode_webp_host(frame, capacity=0)
    assert rc == MALLOC_FAILED and n == len(want) and intact


def test_refusals():
    rc, blob, n, intact = imp.encode_webp_host(np.zeros((4, 4, 2), np.uint8))
    assert rc == UNSUPPORTED and n == 0 and intact
    rc, blob, n, intact = imp.encode_webp_host(np.zeros((1, 16385, 1), np.uint8), capacity=1 << 20)
    assert rc == UNSUPPORTED and n == 0 and intact
    rc, blob, n, intact = imp.encode_webp_host(np.zeros((16385, 1, 3), np.uint8), capacity=1 << 20)
    assert rc == UNSUPPORTED and n == 0 and intact
    frame = content("noise_bgr", 33, 65)
    modes = np.zeros(15, np.uint8)
    modes[14] = 14
    rc, blob, n, intact = imp.encode_webp_host(frame, forced_modes=modes)
    assert rc == INVALID_ARGS and n == 0 and intact
    buf = np.full(4096, 0xA5, np.uint8)
    n = C.c_size_t(7)
    flat = np.zeros((4, 4, 3), np.uint8)
    for args in [(None, 4, 4, 3, 12), (flat.ctypes.data, 0, 4, 3, 12), (flat.ctypes.data, 4, -1, 3, 12), (flat.ctypes.data, 4, 4, 3, 11)]:
        assert lib.impgpu_webp_encode_host(*args, None, buf.ctypes.data, 4096, C.byref(n)) == INVALID_ARGS
        assert n.value == 0 and (buf == 0xA5).all()
    assert lib.impgpu_webp_encode_host(flat.ctypes.data, 4, 4, 3, 12, None, buf.ctypes.data, 4096, None) == INVALID_ARGS
    assert (buf == 0xA5).all()


def test_a_large_side_is_taken():
    frame = np.zeros((1, 16384, 1), np.uint8)
    frame[0, ::3, 0] = 9
    rc, blob, n, intact = imp.encode_webp_host(frame)
    assert rc == OK and intact and blob == W.write(frame)


@pytest.mark.parametrize("uri,ext,want", [
    ("/a.jpg?format=webp&quality=256", "jpg", 1),
    ("/a.jpg?format=webp&quality=300", "jpg", 1),
    ("/a.jpg?format=webp&quality=511", "jpg", 1),
    ("/a.jpg?format=webp&quality=75", "jpg", 0),
    ("/a.jpg?format=webp&quality=512", "jpg", 0),
    ("/a.jpg?format=webp", "jpg", 0),
    ("/a.webp?quality=256", "webp", 1),
    ("/a.jpg?format=png&quality=9", "jpg", 0),
])
def test_request_webp_lossless(uri, ext, want):
    r = imp.Request(uri, ext)
    assert r.code == OK
    assert r.webp_lossless == want
    assert lib.impgpu_request_webp_lossless(None) == 0
