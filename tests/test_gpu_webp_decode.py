"""impgpu_image_decode_webp / impgpu_batch_decode_webp on the device against Pillow's frames for the fixtures of
tests/golden/webp_dec (Pillow-encoded at methods 0 / 3 / 6 and the hand-written streams of webp_dec_cases.py): alone, the
whole set in calls of at most 256 files with a lossy and two damaged files in the middle of each, a call of one, a call cut into two groups by
$IMPGPU_STAGE_CAP_MB, and a decoded frame going on through resize like an uploaded one."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_dec_fixtures as F
from conftest import ROOT

pytestmark = pytest.mark.gpu
LAUNCHES = 3                                      # IMPGPU_WEBP_DEC_LAUNCHES: tables, pixels, inverse -- a group


def _frames(results):
    out = []
    for rc, im in results:
        out.append((rc, None if im is None else im.numpy()))
        if im is not None:
            im.release()
    return out


def test_every_fixture_alone(gpu):
    imp = gpu
    wrong = []
    for name, blob, expected in F.load():
        rc, im = imp.ops.decode_webp(blob)
        if rc != F.IMP_OK or im.shape != expected.shape or not np.array_equal(im.numpy(), expected):
            wrong.append((name, rc))
        if im is not None:
            im.release()
    assert not wrong, wrong[:10]


def test_the_whole_set_in_one_call_with_refused_and_damaged_files_in_the_middle(gpu):
    """every fixture, in calls of at most 256 files (what a call takes): 253 fixtures a call and the three others in its middle"""
    imp = gpu
    every = F.load()
    damaged = F.damaged()
    host = [imp.ops.webp_decode_host(blob)[0] for _, blob in damaged]
    assert host == [F.IMP_ERROR_DECODE_FAILED] * 2
    covered = []
    for at in range(0, len(every), 253):
        fixtures = every[at:at + 253]
        half = len(fixtures) // 2
        blobs = [b for _, b, _ in fixtures[:half]] + [damaged[0][1], F.read("lossy.webp"), damaged[1][1]] + [b for _, b, _ in fixtures[half:]]
        want = [e for _, _, e in fixtures[:half]] + [None] * 3 + [e for _, _, e in fixtures[half:]]
        codes = [0] * half + [host[0], F.IMP_ERROR_UNSUPPORTED, host[1]] + [0] * (len(fixtures) - half)
        assert len(blobs) <= 256
        results, launches = imp.ops.batch_decode_webp(blobs)
        assert launches == LAUNCHES
        got = _frames(results)
        assert [rc for rc, _ in got] == codes
        for k, ((rc, frame), e) in enumerate(zip(got, want)):
            assert (frame is None) == (e is None) and (e is None or np.array_equal(frame, e)), (at, k)
        covered += [name for name, _, _ in fixtures]
    assert covered == [name for name, _, _ in every] and len(set(covered)) == len(every) >= 301


def test_a_call_of_one_and_calls_nothing_is_launched_for(gpu):
    imp = gpu
    name, blob, expected = [f for f in F.load() if f[0] == "p_rgba_53x37_m6"][0]
    results, launches = imp.ops.batch_decode_webp([blob])
    (rc, frame), = _frames(results)
    assert rc == 0 and launches == LAUNCHES and np.array_equal(frame, expected)
    rc, im = imp.ops.decode_webp(blob)
    assert rc == 0 and np.array_equal(im.numpy(), frame)
    im.release()
    results, launches = imp.ops.batch_decode_webp([F.read("lossy.webp"), F.read("not_webp.png"), blob[:40]])
    assert [rc for rc, _ in results] == [F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED] and launches == 0
    assert imp.ops.batch_decode_webp([]) == ([], 0)


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401
import numpy as np
import ngx_http_imgproc_amd as imp
import webp_dec_fixtures as F
imp.env_start(0)
names = sys.argv[2].split(",")
fx = {f[0]: f for f in F.load()}
results, launches = imp.ops.batch_decode_webp([fx[n][1] for n in names])
ok = sum(1 for (rc, im), n in zip(results, names) if rc == 0 and np.array_equal(im.numpy(), fx[n][2]))
print(json.dumps({"launches": launches, "ok": ok}))
imp.env_destroy()
"""


def test_a_call_cut_into_two_groups_by_the_stage_cap():
    """IMPGPU_STAGE_CAP_MB=1 in a fresh process (the cap is read once).  The 300 x 300 frames take 369 152 bytes of a
    group's block each and the 318 x 222 ones 293 632: the third file passes the cap, the last three fit in a second group."""
    names = ["p_flat_300x300_m0", "p_flat_300x300_m3", "p_flat_300x300_m6", "p_tiling_318x222_m0", "p_tiling_318x222_m3"]
    env = dict(os.environ, IMPGPU_STAGE_CAP_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, ",".join(names)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r == {"launches": 2 * LAUNCHES, "ok": len(names)}, r


def test_a_decoded_frame_goes_on_like_an_uploaded_one(gpu):
    """resize of the decoded frame against resize of the same pixels through impgpu_image_upload_fi32 (FreeImage's bitmap:
    bottom-up, B,G,R,A)"""
    imp = gpu
    from ngx_http_imgproc_amd._lib import lib

    for name in ("p_tiling_318x222_m3", "p_rgba_53x37_m0", "p_pal17_61x37_m6"):
        _, blob, expected = [f for f in F.load() if f[0] == name][0]
        rc, dec = imp.ops.decode_webp(blob)
        assert rc == 0
        h, w, _ = expected.shape
        bits = np.ascontiguousarray(expected[::-1])
        handle = C.c_void_p()
        assert lib.impgpu_image_upload_fi32(bits.ctypes.data, w, h, w * 4, C.byref(handle)) == 0
        up = imp.Image(handle=handle.value)
        assert np.array_equal(up.numpy(), expected)
        assert dec.resize("40,0") == imp.IMP_OK and up.resize("40,0") == imp.IMP_OK
        assert dec.shape == up.shape and dec.numpy().tobytes() == up.numpy().tobytes(), name
        dec.release()
        up.release()
