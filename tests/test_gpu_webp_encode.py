"""Lossless WebP answers written on the device (impgpu_image_encode_webp / impgpu_batch_encode_webp): the six launches of
csrc/imp_webp_enc.hip.  The file must equal, byte for byte, what tests/webp_writer.py writes -- the writer, never the
library, says what the bytes are -- and the host twin's; one file per case goes through Pillow's libwebp and must come back
as the frame's pixels.  Nothing at or behind out[length] may be written, a window of a parent is read in place and the
parent stays as it was, a batch gives what the lone calls give in the launches of one, and two runs give the same bytes.

Shapes: 1x1, 1x70, 70x1, 17x37, 33x65, 64x64 and 130x67 cross a tile edge (16), a stream item (1024 symbols) and several
items; `scan_block_529x497` has 1088 tiles (past one mode-image item of 1024) and 257 pixel items (past one block of 256 of
k_webp_scan)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_writer as W
import window_guard as WG
from conftest import ROOT
from test_webp_encode_host import INVALID_ARGS, MALLOC_FAILED, OK, UNSUPPORTED
from test_webp_writer import content, decodes_to

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 70), (70, 1), (17, 37), (33, 65), (64, 64), (130, 67)]
KINDS = {"gray": "gradient_gray", "bgr": "gradient_bgr", "bgra": "bgra_graded"}
_want = {}


def want(frame, key, modes=None):
    """the writer's bytes, computed once per case"""
    if key not in _want:
        _want[key] = W.write(frame, forced_modes=modes)
    return _want[key]


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("w,h", SHAPES)
def test_file_is_the_writers_and_decodes_to_the_frame(gpu, w, h, kind):
    frame = content(KINDS[kind], w, h)
    expect = want(frame, (kind, w, h))
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im)
    assert rc == OK and intact and n == len(expect)
    assert got == expect
    assert gpu.encode_webp_host(frame)[1] == got
    assert decodes_to(got, frame)
    rc, again, n2, intact = gpu.encode_webp(im, capacity=n)                      # an exact fit succeeds; the same bytes again
    assert rc == OK and intact and again == got
    rc, none, n3, intact = gpu.encode_webp(im, capacity=n - 1)                   # one byte short: the size, nothing written
    assert rc == MALLOC_FAILED and none is None and n3 == n and intact
    im.release()


@pytest.mark.parametrize("name", ["noise_bgr", "flat_black", "flat_bgr", "two_colours", "bgra_holes", "bgra_opaque", "noise_gray"])
def test_other_contents(gpu, name):
    frame = content(name, 70, 45)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im)
    assert rc == OK and intact and got == want(frame, (name, 70, 45))
    assert decodes_to(got, frame)
    im.release()


def test_scan_block_529x497(gpu):
    """more than 256 workgroups a launch, where a compute unit holds two of them: k_webp_emit once went wrong only here"""
    frame = content("gradient_bgr", 529, 497)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im)
    assert rc == OK and intact and got == want(frame, ("scan", 529, 497))
    rc, again, n, intact = gpu.encode_webp(im)                                   # two runs: the same bytes
    assert rc == OK and again == got
    assert decodes_to(got, frame)
    im.release()


def test_forced_modes_reach_every_predictor(gpu):
    w, h = 130, 67
    frame = content("bgra_graded", w, h)
    tx, ty = W.tiles_of(w, h)
    rng = np.random.default_rng(8)
    modes = np.concatenate([np.arange(W.MODES), rng.integers(0, W.MODES, tx * ty - W.MODES)]).astype(np.uint8)
    rng.shuffle(modes)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im, forced_modes=modes)
    assert rc == OK and intact and got == want(frame, ("forced", w, h), modes)
    assert got == gpu.encode_webp_host(frame, forced_modes=modes)[1]
    assert decodes_to(got, frame)
    bad = modes.copy()
    bad[-1] = 14
    rc, got, n, intact = gpu.encode_webp(im, forced_modes=bad)
    assert rc == INVALID_ARGS and n == 0 and intact
    im.release()


@pytest.mark.parametrize("kind,c,name", [("a1", 3, "gradient_bgr"), ("a4", 4, "bgra_graded"), ("a1", 1, "gradient_gray"), ("a1", 4, "bgra_holes")])
def test_a_window_of_a_parent_is_read_in_place(gpu, kind, c, name):
    w, h = 61, 33
    frame = content(name, w, h)
    lay = WG.layout_for(kind, w, h, c)
    g = WG.GuardedParent(lay, [frame])
    assert lay.step > w * c
    im = g.wrap(gpu, w, h, c)
    rc, got, n, intact = gpu.encode_webp(im)
    assert rc == OK and intact and got == want(frame, ("window", name))
    rep = g.report(gpu, fresh=True)
    assert rep.intact, WG.describe(rep)
    im.release()


class _RawImage(C.Structure):                                        # csrc/imp_internal.h: struct impgpu_image
    _fields_ = [("d", C.c_void_p), ("w", C.c_int), ("h", C.c_int), ("c", C.c_int), ("step", C.c_int), ("cap", C.c_size_t), ("owned", C.c_bool),
                ("frames", C.c_int), ("fstride", C.c_size_t)]


def test_a_batch_is_its_lone_calls_in_the_launches_of_one(gpu):
    rng = np.random.default_rng(3)
    names = ["gradient_gray", "gradient_bgr", "bgra_graded", "noise_bgr", "two_colours", "bgra_holes", "flat_black", "flat_bgr"]
    frames = []
    for k in range(22):
        w, h = (int(rng.integers(1, 90)), int(rng.integers(1, 90))) if k else (130, 67)
        frames.append(content(names[k % len(names)], w, h))
    images = [gpu.Image(f) for f in frames]
    lone = [gpu.encode_webp(im) for im in images]
    for f, r in zip(frames, lone):
        assert r[0] == OK and r[3] and r[1] == W.write(f)
    album = gpu.Image.album([content("gradient_bgr", 20, 12)] * 2)
    # no entry point makes a 2-channel handle: one is described by hand over a gray image's memory (12 x 9 of 2 channels)
    gray = gpu.Image(content("gradient_gray", 24, 9))
    two = _RawImage(gray.device_ptr, 12, 9, 2, gray.step, 0, False, 1, 0)
    entries = images[:5] + [C.addressof(two)] + images[5:13] + [album] + images[13:]
    caps = [None] * len(entries)
    caps[3] = lone[3][2] - 1                                                       # one byte short
    caps[5] = 4096
    caps[14] = 4096
    rc, results, launches = gpu.batch_encode_webp(entries, capacities=caps)
    assert rc == OK and len(results) == 24
    assert all(r[3] for r in results)                                              # nothing behind a file, nothing for the refused
    expect = lone[:5] + [None] + lone[5:13] + [None] + lone[13:]
    for k, (r, e) in enumerate(zip(results, expect)):
        if e is None:
            assert r[0] == UNSUPPORTED and r[1] is None and r[2] == 0, k
        elif k == 3:
            assert r[0] == MALLOC_FAILED and r[1] is None and r[2] == e[2], k
        else:
            assert r[0] == OK and r[1] == e[1] and r[2] == e[2], k
    rc, res1, launches1 = gpu.batch_encode_webp([images[0]])
    assert rc == OK and res1[0][1] == lone[0][1]
    assert launches == launches1 == 6
    rc, res0, launches0 = gpu.batch_encode_webp([album, C.addressof(two)], capacities=[4096, 4096])
    assert rc == OK and [r[0] for r in res0] == [UNSUPPORTED, UNSUPPORTED] and launches0 == 0
    rc, res_none, launches_none = gpu.batch_encode_webp([])
    assert rc == OK and launches_none == 0
    rc, res_many, launches_many = gpu.batch_encode_webp([], count=257)
    assert rc == INVALID_ARGS and launches_many == 0
    for im in images + [album, gray]:
        im.release()


def test_the_lone_call_refuses_an_album(gpu):
    album = gpu.Image.album([content("gradient_bgr", 20, 12)] * 3)
    rc, got, n, intact = gpu.encode_webp(album, capacity=4096)
    assert rc == UNSUPPORTED and got is None and n == 0 and intact
    album.release()


def test_no_env_no_device_is_looked_for():
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
rc, res, launches = imp.batch_encode_webp([], count=257)
assert rc == imp.IMP_ERROR_INVALID_ARGS and launches == 0, (rc, launches)
rc, res, launches = imp.batch_encode_webp([None])
assert rc == imp.IMP_ERROR_DEVICE and res[0][0] == imp.IMP_ERROR_DEVICE and launches == 0, (rc, res, launches)
assert imp.encode_webp_host(np.zeros((3, 3, 3), np.uint8))[0] == 0
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]
