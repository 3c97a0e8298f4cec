"""Lossless WebP answers with backward references written on the device (impgpu_image_encode_webp_flags /
impgpu_batch_encode_webp_flags with IMPGPU_WEBP_ENC_BACKREFS): the seven launches of csrc/imp_webp_enc.hip, k_webp_parse
among them.  The file must equal, byte for byte, what tests/webp_lz_writer.py writes and what the host twin writes, and
decode through Pillow's libwebp to the frame.  The cases are test_webp_lz_writer's: 1x1, 1x7, 7x1, widths 2 and 3, 32x32
(one item exactly), 41x25 (a second item of one position), 64x33 flat (references of exactly 1024), 300x9 (the vertical
candidates read an earlier item) and 529x497 (past 256 workgroups), with planted matches under forced mode 0 and the
chooser's contents.  flags = 0 is the flag-less call in six launches; a window of a parent is read in place; a batch is its
lone calls in seven launches; a refused frame changes no other entry; a capacity too small reports the length alone."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_lz_writer as LZ
import webp_writer as W
import window_guard as WG
from conftest import ROOT
from test_gpu_webp_encode import _RawImage
from test_webp_encode_host import INVALID_ARGS, MALLOC_FAILED, OK, UNSUPPORTED
from test_webp_lz_writer import BIG, CASES, fixture, lz_content, want
from test_webp_writer import content, decodes_to

pytestmark = pytest.mark.gpu

LZF = 1                                                              # IMPGPU_WEBP_ENC_BACKREFS


@pytest.mark.parametrize("name", sorted(CASES))
def test_file_is_the_models_and_the_host_twins(gpu, name):
    frame, modes = CASES[name]
    expect = want(name)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im, forced_modes=modes, flags=LZF)
    assert rc == OK and intact and n == len(expect)
    assert got == expect
    assert gpu.encode_webp_host(frame, forced_modes=modes, flags=LZF)[1] == got
    assert decodes_to(got, frame)
    rc, again, n2, intact = gpu.encode_webp(im, forced_modes=modes, capacity=n, flags=LZF)      # an exact fit; the same bytes again
    assert rc == OK and intact and again == got
    rc, none, n3, intact = gpu.encode_webp(im, forced_modes=modes, capacity=n - 1, flags=LZF)   # one byte short: the size alone
    assert rc == MALLOC_FAILED and none is None and n3 == n and intact
    im.release()


@pytest.mark.parametrize("name", sorted(BIG))
def test_past_256_workgroups_529x497(gpu, name):
    frame, modes = BIG[name]
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im, forced_modes=modes, flags=LZF)
    assert rc == OK and intact and got == want(name)
    rc, again, n, intact = gpu.encode_webp(im, forced_modes=modes, flags=LZF)                   # two runs: the same bytes
    assert rc == OK and again == got
    assert decodes_to(got, frame)
    im.release()


@pytest.mark.parametrize("name,w,h", [("noise_bgr", 70, 45), ("bgra_opaque", 33, 20), ("noise_gray", 130, 67)])
def test_a_frame_without_a_match_is_the_flagless_file(gpu, name, w, h):
    frame = content(name, w, h)
    im = gpu.Image(frame)
    rc, got, n, intact = gpu.encode_webp(im, flags=LZF)
    assert rc == OK and intact
    assert got == gpu.encode_webp(im)[1] == W.write(frame)
    im.release()


def test_flags_0_is_the_flagless_call(gpu):
    for name in ["flat_bgr_64x33", "dither_41x25", "rows2_300x9"]:
        frame, modes = CASES[name]
        im = gpu.Image(frame)
        assert gpu.encode_webp(im, forced_modes=modes, flags=0) == gpu.encode_webp(im, forced_modes=modes)
        assert gpu.encode_webp(im, forced_modes=modes)[1] == W.write(frame, forced_modes=modes)
        im.release()


def test_an_unknown_flag_is_refused(gpu):
    im = gpu.Image(content("flat_bgr", 8, 8))
    for flags in (2, 3, -1):
        rc, got, n, intact = gpu.encode_webp(im, flags=flags, capacity=4096)
        assert rc == INVALID_ARGS and got is None and n == 0 and intact
        rc, res, launches = gpu.batch_encode_webp([im], capacities=[4096], flags=flags)
        assert rc == INVALID_ARGS and launches == 0 and res[0][3]
    im.release()


@pytest.mark.parametrize("kind,c,name", [("a1", 3, "screenshot"), ("a4", 4, "bgra_holes"), ("a1", 1, "gradient_gray"), ("a1", 3, "dither")])
def test_a_window_of_a_parent_is_read_in_place(gpu, kind, c, name):
    w, h = 61, 33
    frame = lz_content(name, w, h)
    lay = WG.layout_for(kind, w, h, c)
    g = WG.GuardedParent(lay, [frame])
    assert lay.step > w * c
    im = g.wrap(gpu, w, h, c)
    rc, got, n, intact = gpu.encode_webp(im, flags=LZF)
    assert rc == OK and intact and got == LZ.write(frame)
    rep = g.report(gpu, fresh=True)
    assert rep.intact, WG.describe(rep)
    im.release()


def test_a_batch_is_its_lone_calls_in_seven_launches(gpu):
    rng = np.random.default_rng(4)
    names = ["gradient_gray", "screenshot", "bgra_holes", "noise_bgr", "two_colours", "dither", "flat_black", "flat_bgr", "bgra_graded"]
    frames = []
    for k in range(20):
        w, h = (int(rng.integers(1, 90)), int(rng.integers(1, 90))) if k else (130, 67)
        frames.append(lz_content(names[k % len(names)], w, h))
    images = [gpu.Image(f) for f in frames]
    lone = [gpu.encode_webp(im, flags=LZF) for im in images]
    for f, r in zip(frames, lone):
        assert r[0] == OK and r[3] and r[1] == LZ.write(f)
    album = gpu.Image.album([content("gradient_bgr", 20, 12)] * 2)
    gray = gpu.Image(content("gradient_gray", 24, 9))                              # a 2-channel handle, described by hand
    two = _RawImage(gray.device_ptr, 12, 9, 2, gray.step, 0, False, 1, 0)
    entries = images[:5] + [C.addressof(two)] + images[5:13] + [album] + images[13:]
    caps = [None] * len(entries)
    caps[3] = lone[3][2] - 1                                                       # one byte short
    caps[5] = 4096
    caps[14] = 4096
    rc, results, launches = gpu.batch_encode_webp(entries, capacities=caps, flags=LZF)
    assert rc == OK and len(results) == 22
    assert all(r[3] for r in results)                                              # nothing behind a file, nothing for the refused
    expect = lone[:5] + [None] + lone[5:13] + [None] + lone[13:]
    for k, (r, e) in enumerate(zip(results, expect)):
        if e is None:
            assert r[0] == UNSUPPORTED and r[1] is None and r[2] == 0, k            # a refused frame changes no other entry
        elif k == 3:
            assert r[0] == MALLOC_FAILED and r[1] is None and r[2] == e[2], k
        else:
            assert r[0] == OK and r[1] == e[1] and r[2] == e[2], k
    rc, res1, launches1 = gpu.batch_encode_webp([images[0]], flags=LZF)
    assert rc == OK and res1[0][1] == lone[0][1]
    assert launches == launches1 == 7
    rc, res0, launches0 = gpu.batch_encode_webp([images[0], images[1]], flags=0)
    assert rc == OK and launches0 == 6
    assert [r[1] for r in res0] == [W.write(frames[0]), W.write(frames[1])]
    rc, res_plain, launches_plain = gpu.batch_encode_webp([images[0], images[1]])
    assert rc == OK and launches_plain == 6 and [r[1] for r in res_plain] == [r[1] for r in res0]
    rc, res_none, launches_none = gpu.batch_encode_webp([album, C.addressof(two)], capacities=[4096, 4096], flags=LZF)
    assert rc == OK and [r[0] for r in res_none] == [UNSUPPORTED, UNSUPPORTED] and launches_none == 0
    for im in images + [album, gray]:
        im.release()


def test_groups_under_the_stage_cap_count_the_token_plane():
    """$IMPGPU_STAGE_CAP_MB = 1: a 130x67 frame takes 199 936 bytes of a group with the flag (file bound, residuals, token
    plane, both work areas), so five fit and six go in two groups of seven launches; without the flag it takes 154 112 and
    six go in one group -- as they would with the flag if the token plane were left out of the sum.  529x497 does not fit."""
    code = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, %r)
import numpy as np
import ngx_http_imgproc_amd as imp
import webp_lz_writer as LZ
from test_webp_lz_writer import fixture
imp.env_start(0)
frames = [fixture("screenshot" if k %% 2 else "dither", 130, 67) for k in range(6)]
images = [imp.Image(f) for f in frames]
rc, res, launches = imp.batch_encode_webp(images, flags=imp.WEBP_ENC_BACKREFS)
assert rc == 0 and launches == 14, (rc, launches)
assert [r[1] for r in res[:2]] == [LZ.write(f) for f in frames[:2]] and all(r[0] == 0 and r[3] for r in res)
assert res[5][1] == imp.encode_webp_host(frames[5], flags=imp.WEBP_ENC_BACKREFS)[1]
rc, res, launches = imp.batch_encode_webp(images)
assert rc == 0 and launches == 6, (rc, launches)
big = imp.Image(fixture("screenshot", 529, 497))
rc, blob, n, intact = imp.encode_webp(big, flags=imp.WEBP_ENC_BACKREFS)
assert rc == imp.IMP_ERROR_MALLOC_FAILED and n == 0 and intact, (rc, n)
imp.env_destroy()
print("ok")
""" % (ROOT, os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, IMPGPU_STAGE_CAP_MB="1"))
    assert r.returncode == 0 and r.stdout.split()[-1:] == ["ok"], r.stderr[-1500:]


def test_the_size_fixtures_on_the_device(gpu):
    """the 320x240 frames of the size conditions: the device's files ARE the model's, on which the conditions are asserted"""
    for name in ("flat", "screenshot", "dither", "photo"):
        frame = content("flat_bgr", 320, 240) if name == "flat" else fixture(name, 320, 240)
        im = gpu.Image(frame)
        rc, got, n, intact = gpu.encode_webp(im, flags=LZF)
        assert rc == OK and intact and got == LZ.write(frame), name
        im.release()
