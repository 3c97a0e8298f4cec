"""The PNG answer on the device (impgpu_image_encode_png / impgpu_batch_encode_png): the file libpng 1.6.37 + zlib 1.2.11
write at OpenCV 2.4.9's settings, byte for byte -- against the libpng fixtures and the Python model of
tests/png_enc_model.py."""
import ctypes as C
import io
import json
import os
import threading

import numpy as np
import pytest

import png_enc_model as model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_enc")


def enc(imp, frame, level=9):
    im = imp.Image(frame)
    try:
        return im.encode_png(level)
    finally:
        im.release()


def test_fixtures_byte_equal(gpu):
    imp = gpu
    with open(os.path.join(GOLD, "manifest.json")) as fh:
        man = json.load(fh)
    files = np.load(os.path.join(GOLD, "cases.npz"))
    for case in man["cases"]:
        frame = model.make_frame(case["kind"], case["h"], case["w"], case["c"], case["seed"])
        rc, blob = enc(imp, frame)
        assert rc == 0, case
        assert blob == files[case["key"]].tobytes(), case


def test_levels_give_one_file(gpu):
    frame = model.make_frame("smooth", 50, 70, 3, 1)
    want = model.encode(frame)
    for level in range(1, 10):
        assert enc(gpu, frame, level) == (0, want)


def test_random_against_model(gpu):
    rng = np.random.default_rng(0x5EED)
    for i in range(60):
        h, w, c = int(rng.integers(1, 300)), int(rng.integers(1, 300)), int(rng.choice([1, 3, 4]))
        kind = ["smooth", "noise", "flat", "stripes%d" % int(rng.integers(1, 600))][i % 4]
        frame = model.make_frame(kind, h, w, c, i)
        if i % 5 == 0:                                       # mixed content: noise patches on a smooth frame
            frame = frame.copy()
            frame[h // 3:h // 2, w // 4:w // 2] = rng.integers(0, 256, frame[h // 3:h // 2, w // 4:w // 2].shape, dtype=np.uint8)
        rc, blob = enc(gpu, frame)
        assert rc == 0 and blob == model.encode(frame), (kind, h, w, c)


def test_batch_equals_lone_calls(gpu):
    imp = gpu
    rng = np.random.default_rng(64)
    frames = []
    for i in range(64):
        h, w, c = int(rng.integers(1, 260)), int(rng.integers(1, 260)), int(rng.choice([1, 3, 4]))
        frames.append(model.make_frame(["smooth", "noise", "flat", "stripes7"][i % 4], h, w, c, i))
    ims = [imp.Image(f) for f in frames]
    try:
        got = imp.batch_encode_png(ims, 6)
        lone = [im.encode_png(9) for im in ims]
    finally:
        for im in ims:
            im.release()
    assert got == lone
    for (rc, blob), f in zip(got, frames):
        assert rc == 0 and blob == model.encode(f)


def test_refusals_and_capacity(gpu):
    imp = gpu
    frame = model.make_frame("smooth", 20, 30, 3, 0)
    assert enc(imp, frame, 0)[0] == imp.IMP_ERROR_UNSUPPORTED
    assert enc(imp, frame, 10)[0] == imp.IMP_ERROR_INVALID_ARGS
    assert enc(imp, frame, -1)[0] == imp.IMP_ERROR_INVALID_ARGS
    assert imp.lib.impgpu_png_encode_bound(8, 8, 2) == 0           # (no 2-channel frame can be made: upload and wrap refuse it)
    im = imp.Image(frame)
    try:
        want = model.encode(frame)
        buf = np.full(len(want) + 8, 0xEE, np.uint8)
        n = C.c_size_t()
        rc = imp.lib.impgpu_image_encode_png(im.h, 9, buf.ctypes.data, len(want) - 1, C.byref(n))
        assert rc == imp.IMP_ERROR_MALLOC_FAILED and n.value == len(want)
        assert (buf == 0xEE).all(), "a refused encode wrote into the buffer"
        rc = imp.lib.impgpu_image_encode_png(im.h, 9, buf.ctypes.data, len(want), C.byref(n))
        assert rc == 0 and buf[:n.value].tobytes() == want and (buf[n.value:] == 0xEE).all()
    finally:
        im.release()


def test_crop_view_and_album(gpu):
    imp = gpu
    big = model.make_frame("smooth", 90, 120, 4, 3)
    im = imp.Image(big)
    try:
        x, y, w, h = 7, 11, 61, 45
        view = imp.Image.wrap(im.device_ptr + y * im.step + x * 4, w, h, 4, im.step)
        try:
            assert view.step > w * 4
            assert view.encode_png(9) == (0, model.encode(np.ascontiguousarray(big[y:y + h, x:x + w])))
        finally:
            view.release()
    finally:
        im.release()
    frames = [model.make_frame("noise", 30, 40, 3, s) for s in range(3)]
    al = imp.Image.album(frames)
    try:
        assert al.encode_png(9) == (0, model.encode(frames[0]))
    finally:
        al.release()


def test_threads(gpu):
    imp = gpu
    frames = [model.make_frame(["smooth", "noise"][i % 2], 100 + i, 120, 3, i) for i in range(8)]
    want = [model.encode(f) for f in frames]
    errors = []

    def work(k):
        try:
            for _ in range(3):
                rc, blob = enc(imp, frames[k])
                if rc != 0 or blob != want[k]:
                    errors.append(k)
        except Exception as e:                               # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(k,)) for k in range(len(frames))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors


def test_round_trip(gpu):
    imp = gpu
    from PIL import Image as PILImage

    for c in (1, 3, 4):
        frame = model.make_frame("smooth", 64, 80, c, c)
        rc, blob = enc(imp, frame)
        assert rc == 0
        rc, back = imp.Image.decode_png(blob)
        assert rc == 0
        try:
            assert np.array_equal(back.numpy(), frame)
        finally:
            back.release()
        pil = np.asarray(PILImage.open(io.BytesIO(blob)))
        if c == 1:
            assert np.array_equal(pil, frame[:, :, 0])
        else:
            order = [2, 1, 0] + ([3] if c == 4 else [])
            assert np.array_equal(pil, frame[:, :, order])
