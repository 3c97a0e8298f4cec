"""impgpu_webp_lossy_encode_host -- the lane code of csrc/imp_webp_lossy.h (what the five launches run per lane) on one
thread, no device -- must write, byte for byte, what tests/webp_vp8_writer.py writes, and decide what it decides (modes,
levels, reconstruction): on every case of test_webp_vp8_writer and on random frames of mixed channel counts and row
pitches.  Refusals, their codes, and that nothing is written behind a file or on a refusal (guard bytes); the bound;
impgpu_request_webp_quality on request lines."""
import ctypes as C

import numpy as np
import pytest

import webp_vp8_writer as V
from test_webp_encode_host import padded
from test_webp_vp8_writer import CASES, content, encoded

import ngx_http_imgproc_amd as imp
from ngx_http_imgproc_amd._lib import lib

OK, UNSUPPORTED, MALLOC_FAILED, INVALID_ARGS = imp.IMP_OK, imp.IMP_ERROR_UNSUPPORTED, imp.IMP_ERROR_MALLOC_FAILED, imp.IMP_ERROR_INVALID_ARGS


def random_frames(seed, count):
    """[(frame, row padding, quality)]"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        w, h, c = int(rng.integers(1, 50)), int(rng.integers(1, 50)), int(rng.choice([1, 3, 4]))
        kind = int(rng.integers(0, 3))
        if kind == 0:
            f = rng.integers(0, 256, (h, w, c), dtype=np.uint8)
        elif kind == 1:
            y, x = np.mgrid[0:h, 0:w]
            f = ((np.stack([(k + 1) * x + (4 - k) * y for k in range(c)], axis=2) + rng.integers(0, 3, (h, w, c))) & 255).astype(np.uint8)
        else:                                                       # blocks of flat colour: skipped macroblocks
            f = np.repeat(np.repeat(rng.integers(0, 256, ((h + 15) // 16, (w + 15) // 16, c), dtype=np.uint8), 16, axis=0), 16, axis=1)[:h, :w]
        f = np.ascontiguousarray(f)
        if c == 4 and rng.integers(0, 2):
            f[..., 3] = 255
        out.append((f, int(rng.choice([0, 0, 1, 3, 16])), int(rng.choice([0, 30, 50, 75, 90, 100]))))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_host_twin_writes_the_models_bytes(name):
    frame, q = CASES[name]
    e = encoded(name)
    rc, blob, n, intact, d = imp.encode_webp_lossy_host(frame, q, details=True)
    assert rc == OK and intact
    assert np.array_equal(d["modes"][:, 0], e.ymodes) and np.array_equal(d["modes"][:, 1], e.uvmodes)
    assert np.array_equal(d["levels"], e.levels)
    assert np.array_equal(d["y"], e.y) and np.array_equal(d["u"], e.u) and np.array_equal(d["v"], e.v)
    assert blob == e.file
    assert n <= imp.webp_lossy_encode_bound(frame.shape[1], frame.shape[0], frame.shape[2])
    assert imp.encode_webp_lossy_host(frame, q)[:2] == (OK, e.file)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_frames_and_steps(seed):
    rng = np.random.default_rng(100 + seed)
    for k, (frame, pad, q) in enumerate(random_frames(seed, 12)):
        view, parent = padded(frame, pad, rng)
        before = parent.copy()
        rc, blob, n, intact = imp.encode_webp_lossy_host(view, q)
        assert rc == OK and intact, k
        assert blob == V.encode(frame, q).file, (k, frame.shape, pad, q)
        assert np.array_equal(parent, before)


def test_capacity():
    frame, q = CASES["ramp_bgr_33x47_q75"]
    want = encoded("ramp_bgr_33x47_q75").file
    rc, blob, n, intact = imp.encode_webp_lossy_host(frame, q, capacity=len(want))
    assert rc == OK and intact and blob == want
    rc, blob, n, intact = imp.encode_webp_lossy_host(frame, q, capacity=len(want) - 1)
    assert rc == MALLOC_FAILED and blob is None and n == len(want) and intact
    rc, blob, n, intact = imp.encode_webp_lossy_host(frame, q, capacity=0)
    assert rc == MALLOC_FAILED and n == len(want) and intact


def test_refusals():
    rc, blob, n, intact = imp.encode_webp_lossy_host(np.zeros((4, 4, 2), np.uint8))
    assert rc == UNSUPPORTED and n == 0 and intact
    rc, blob, n, intact = imp.encode_webp_lossy_host(np.zeros((1, 16384, 1), np.uint8), capacity=1 << 20)
    assert rc == UNSUPPORTED and n == 0 and intact
    rc, blob, n, intact = imp.encode_webp_lossy_host(np.zeros((16384, 1, 3), np.uint8), capacity=1 << 20)
    assert rc == UNSUPPORTED and n == 0 and intact
    flat = np.zeros((4, 4, 3), np.uint8)
    for q in (-1, 101, 256):
        rc, blob, n, intact = imp.encode_webp_lossy_host(flat, q)
        assert rc == INVALID_ARGS and n == 0 and intact
    buf = np.full(4096, 0xA5, np.uint8)
    n = C.c_size_t(7)
    for args in [(None, 4, 4, 3, 12), (flat.ctypes.data, 0, 4, 3, 12), (flat.ctypes.data, 4, -1, 3, 12), (flat.ctypes.data, 4, 4, 3, 11)]:
        assert lib.impgpu_webp_lossy_encode_host(*args, 75, buf.ctypes.data, 4096, C.byref(n)) == INVALID_ARGS
        assert n.value == 0 and (buf == 0xA5).all()
    assert lib.impgpu_webp_lossy_encode_host(flat.ctypes.data, 4, 4, 3, 12, 75, buf.ctypes.data, 4096, None) == INVALID_ARGS
    assert (buf == 0xA5).all()
    assert imp.webp_lossy_encode_bound(4, 4, 2) == 0 and imp.webp_lossy_encode_bound(16384, 4, 3) == 0 and imp.webp_lossy_encode_bound(0, 4, 3) == 0


def test_the_largest_side_is_taken():
    frame = np.zeros((1, 16383, 1), np.uint8)
    frame[0, ::7, 0] = 200
    rc, blob, n, intact = imp.encode_webp_lossy_host(frame, 50)
    assert rc == OK and intact
    e = V.encode(frame, 50)
    assert blob == e.file


def test_batch_arguments_are_checked_before_a_device_is_looked_for():
    one = (C.c_void_p * 1)()
    sizes, codes, q = (C.c_size_t * 1)(), (C.c_int * 1)(), (C.c_int * 1)(75)
    f = lib.impgpu_batch_encode_webp_lossy
    assert f(None, 1, q, one, sizes, sizes, codes, None) == INVALID_ARGS
    assert f(one, 1, None, one, sizes, sizes, codes, None) == INVALID_ARGS
    assert f(one, -1, q, one, sizes, sizes, codes, None) == INVALID_ARGS
    assert f(one, 257, q, one, sizes, sizes, codes, None) == INVALID_ARGS
    q[0] = 101
    assert f(one, 1, q, one, sizes, sizes, codes, None) == INVALID_ARGS
    assert f(None, 0, None, None, None, None, None, None) == OK
    assert lib.impgpu_image_encode_webp_lossy(None, 75, None, 0, None) == INVALID_ARGS


@pytest.mark.parametrize("uri,ext,want", [
    ("/a.jpg?format=webp", "jpg", 75),                               # absent
    ("/a.webp?resize=10x10", "webp", 75),
    ("/a.jpg?format=webp&quality=0", "jpg", 75),
    ("/a.jpg?format=webp&quality=60", "jpg", 60),
    ("/a.webp?quality=100", "webp", 100),
    ("/a.webp?quality=101", "webp", 100),
    ("/a.webp?quality=255", "webp", 100),
    ("/a.webp?quality=256", "webp", -1),                             # lossless
    ("/a.webp?quality=300", "webp", -1),
    ("/a.jpg?quality=60", "jpg", -1),
    ("/a.webp?format=jpg&quality=60", "webp", -1),
    ("/a.jpg?format=png&quality=9", "jpg", -1),
])
def test_request_webp_quality(uri, ext, want):
    r = imp.Request(uri, ext)
    assert r.code == OK
    assert r.webp_quality == want
    assert not (r.webp_quality >= 0 and r.webp_lossless)
    assert lib.impgpu_request_webp_quality(None) == -1
