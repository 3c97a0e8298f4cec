"""Lossy WebP answers written on the device (impgpu_image_encode_webp_lossy / impgpu_batch_encode_webp_lossy): the five
launches of csrc/imp_webp_lossy.hip.  The file must equal, byte for byte, the host twin's (which test_webp_lossy_host pins
to tests/webp_vp8_writer.py) on the cases of test_webp_vp8_writer; Pillow's libwebp must decode a device-written file to the
model's reconstruction.  Nothing at or behind out[length] may be written, a window of a parent is read in place and the
parent stays as it was, a batch gives what the lone calls give in the launches of one, and two runs give the same bytes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_vp8_writer as V
import window_guard as WG
from conftest import ROOT
from test_gpu_webp_encode import _RawImage
from test_webp_lossy_host import INVALID_ARGS, MALLOC_FAILED, OK, UNSUPPORTED
from test_webp_vp8_writer import CASES, content, encoded, pillow

pytestmark = pytest.mark.gpu
LAUNCHES = 5


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_the_host_twins(gpu, name):
    frame, q = CASES[name]
    rc, expect, n_host, intact = gpu.encode_webp_lossy_host(frame, q)
    assert rc == OK
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp_lossy(im, q)
    assert rc == OK and intact and n == len(expect)
    assert got == expect
    rc, again, n2, intact = gpu.encode_webp_lossy(im, q, capacity=n)             # an exact fit succeeds; the same bytes again
    assert rc == OK and intact and again == got
    rc, none, n3, intact = gpu.encode_webp_lossy(im, q, capacity=n - 1)          # one byte short: the size, nothing written
    assert rc == MALLOC_FAILED and none is None and n3 == n and intact
    im.release()


@pytest.mark.parametrize("name", ["ramp_bgr_33x47_q75", "noise_bgr_40x136_q100", "alpha_bgra_33x47_q75", "stripes_gray_33x47_q0"])
def test_pillow_decodes_a_device_file_to_the_reconstruction(gpu, name):
    frame, q = CASES[name]
    h, w, c = frame.shape
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp_lossy(im, q)
    im.release()
    assert rc == OK and intact
    e = encoded(name)
    shown = np.asarray(pillow(got))
    assert np.array_equal(shown[..., :3], V.decoded_rgb(e.y, e.u, e.v, w, h))
    if name.startswith("alpha"):
        assert np.array_equal(shown[..., 3], frame[..., 3])


def test_many_rows_and_columns(gpu):
    """more macroblock rows than wavefronts several times over, rows long enough for every wavefront to wait and to be waited for"""
    frame = content("ramp_bgr", 200, 150)
    frame[40:90, 30:120] = content("noise_bgr", 90, 50)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp_lossy(im, 60)
    assert rc == OK and intact and got == gpu.encode_webp_lossy_host(frame, 60)[1]
    rc, again, n, intact = gpu.encode_webp_lossy(im, 60)                          # two runs: the same bytes
    assert rc == OK and again == got
    im.release()


def test_a_wide_frame_keeps_fewer_rows_in_flight(gpu):
    """at the largest width the border rows of three macroblock rows fill the LDS: four rows, so a slot is taken again"""
    rng = np.random.default_rng(5)
    frame = np.repeat(rng.integers(0, 256, (49, 16383 // 32 + 1, 3), dtype=np.uint8), 32, axis=1)[:, :16383].copy()
    frame[::3, ::5, 1] ^= 0x55
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp_lossy(im, 40, capacity=1 << 22)
    assert rc == OK and intact and got == gpu.encode_webp_lossy_host(frame, 40, capacity=1 << 22)[1]
    im.release()


@pytest.mark.parametrize("kind,c,name", [("a1", 3, "ramp_bgr"), ("a4", 4, "alpha_bgra"), ("a1", 1, "ramp_gray"), ("a16", 4, "opaque_bgra")])
def test_a_window_of_a_parent_is_read_in_place(gpu, kind, c, name):
    w, h = 45, 33
    frame = content(name, w, h)
    lay = WG.layout_for(kind, w, h, c)
    g = WG.GuardedParent(lay, [frame])
    assert lay.step > w * c
    im = g.wrap(gpu, w, h, c)
    rc, got, n, intact = gpu.encode_webp_lossy(im, 75)
    assert rc == OK and intact and got == gpu.encode_webp_lossy_host(frame, 75)[1]
    rep = g.report(gpu, fresh=True)
    assert rep.intact, WG.describe(rep)
    im.release()


def test_a_batch_is_its_lone_calls_in_the_launches_of_one(gpu):
    rng = np.random.default_rng(3)
    names = ["ramp_gray", "ramp_bgr", "alpha_bgra", "noise_bgr", "opaque_bgra", "flat_bgr", "stripes_bgr", "noise_gray"]
    frames, qs = [], []
    for k in range(14):
        w, h = (int(rng.integers(1, 70)), int(rng.integers(1, 70))) if k else (130, 67)
        frames.append(content(names[k % len(names)], w, h))
        qs.append([0, 50, 75, 100, 33][k % 5])
    images = [gpu.Image(f) for f in frames]
    lone = [gpu.encode_webp_lossy(im, q) for im, q in zip(images, qs)]
    for f, q, r in zip(frames, qs, lone):
        assert r[0] == OK and r[3] and r[1] == gpu.encode_webp_lossy_host(f, q)[1]
    album = gpu.Image.album([content("ramp_bgr", 20, 12)] * 2)
    # no entry point makes a 2-channel handle: one is described by hand over a gray image's memory (12 x 9 of 2 channels)
    gray = gpu.Image(content("ramp_gray", 24, 9))
    two = _RawImage(gray.device_ptr, 12, 9, 2, gray.step, 0, False, 1, 0)
    entries = images[:5] + [C.addressof(two)] + images[5:9] + [album] + images[9:]
    quals = qs[:5] + [75] + qs[5:9] + [75] + qs[9:]
    caps = [None] * len(entries)
    caps[3] = lone[3][2] - 1                                                       # one byte short
    caps[5] = 4096
    caps[10] = 4096
    rc, results, launches = gpu.batch_encode_webp_lossy(entries, quals, capacities=caps)
    assert rc == OK and len(results) == 16
    assert all(r[3] for r in results)                                              # nothing behind a file, nothing for the refused
    expect = lone[:5] + [None] + lone[5:9] + [None] + lone[9:]
    for k, (r, e) in enumerate(zip(results, expect)):
        if e is None:
            assert r[0] == UNSUPPORTED and r[1] is None and r[2] == 0, k
        elif k == 3:
            assert r[0] == MALLOC_FAILED and r[1] is None and r[2] == e[2], k
        else:
            assert r[0] == OK and r[1] == e[1] and r[2] == e[2], k
    rc, res1, launches1 = gpu.batch_encode_webp_lossy([images[0]], [qs[0]])
    assert rc == OK and res1[0][1] == lone[0][1]
    assert launches == launches1 == LAUNCHES
    rc, res0, launches0 = gpu.batch_encode_webp_lossy([album, C.addressof(two)], [75, 75], capacities=[4096, 4096])
    assert rc == OK and [r[0] for r in res0] == [UNSUPPORTED, UNSUPPORTED] and launches0 == 0
    rc, res_none, launches_none = gpu.batch_encode_webp_lossy([], [])
    assert rc == OK and launches_none == 0
    rc, res_many, launches_many = gpu.batch_encode_webp_lossy([], [], count=257)
    assert rc == INVALID_ARGS and launches_many == 0
    rc, res_q, launches_q = gpu.batch_encode_webp_lossy([images[0], images[1]], [75, 101])
    assert rc == INVALID_ARGS and launches_q == 0 and all(r[3] for r in res_q)
    for im in images + [album, gray]:
        im.release()


def test_groups_under_the_stage_cap(gpu):
    """a call past $IMPGPU_STAGE_CAP_MB goes in groups of five launches each and gives the same files"""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
from test_webp_vp8_writer import content
imp.env_start(0)
frames = [content("ramp_bgr", 130, 67), content("noise_bgr", 100, 90), content("alpha_bgra", 120, 80), content("ramp_bgr", 400, 300)]
images = [imp.Image(f) for f in frames]
rc, res, launches = imp.batch_encode_webp_lossy(images, [75] * 4)
assert rc == 0 and launches %% 5 == 0 and launches > 5, (rc, launches)
for f, r in zip(frames[:3], res[:3]):
    assert r[0] == 0 and r[3] and r[1] == imp.encode_webp_lossy_host(f, 75)[1]
assert res[3][0] == imp.IMP_ERROR_MALLOC_FAILED and res[3][2] == 0 and res[3][3]
for im in images:
    im.release()
imp.env_destroy()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, IMPGPU_STAGE_CAP_MB="4"))
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]


def test_the_lone_call_refuses_an_album_and_a_quality(gpu):
    album = gpu.Image.album([content("ramp_bgr", 20, 12)] * 3)
    rc, got, n, intact = gpu.encode_webp_lossy(album, 75, capacity=4096)
    assert rc == UNSUPPORTED and got is None and n == 0 and intact
    album.release()
    im = gpu.Image(content("ramp_bgr", 20, 12))
    for q in (-1, 101):
        rc, got, n, intact = gpu.encode_webp_lossy(im, q, capacity=4096)
        assert rc == INVALID_ARGS and got is None and n == 0 and intact
    im.release()


def test_no_env_no_device_is_looked_for():
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
rc, res, launches = imp.batch_encode_webp_lossy([], [], count=257)
assert rc == imp.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
rc, res, launches = imp.batch_encode_webp_lossy([None], [101])
assert rc == imp.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
rc, res, launches = imp.batch_encode_webp_lossy([None], [75])
assert rc == imp.IMP_ERROR_DEVICE and res[0][0] == imp.IMP_ERROR_DEVICE and launches == 0, (rc, res, launches)
assert imp.encode_webp_lossy_host(np.zeros((3, 3, 3), np.uint8))[0] == 0
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]
