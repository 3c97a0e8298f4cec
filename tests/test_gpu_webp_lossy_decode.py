"""impgpu_image_decode_webp_ex / impgpu_batch_decode_webp_ex with IMPGPU_WEBP_ACCEPT_LOSSY on the device, against Pillow's
frames and the host model's for the fixtures of tests/golden/webp_lossy_dec: the whole set in one call, a handful alone, a
call that mixes lossless, lossy, refused and damaged files, the launch counts of lossy-only, lossless-only, mixed and
nothing-accepted calls, a call cut into groups by $IMPGPU_STAGE_CAP_MB, and accept 0 against the call without _ex."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_dec_fixtures as L
import webp_lossy_dec_fixtures as F
from conftest import ROOT

pytestmark = pytest.mark.gpu
A = F.ACCEPT_LOSSY
LOSSLESS, LOSSY = 3, 3                            # IMPGPU_WEBP_DEC_LAUNCHES, IMPGPU_WEBP_DEC_LOSSY_LAUNCHES -- a group


def _frames(results):
    out = []
    for rc, im in results:
        out.append((rc, None if im is None else im.numpy()))
        if im is not None:
            im.release()
    return out


def test_all_fixtures_in_one_call_equal_pillow_and_the_host_model(gpu):
    imp = gpu
    fixtures = F.load()
    assert 180 <= len(fixtures) <= 256
    results, launches = imp.ops.batch_decode_webp([b for _, b, _ in fixtures], accept=A)
    assert launches == LOSSY
    wrong = []
    for (name, blob, expected), (rc, frame) in zip(fixtures, _frames(results)):
        hrc, host, _, _ = imp.ops.webp_decode_host(blob, accept=A)
        if rc != 0 or hrc != 0 or not np.array_equal(frame, expected) or not np.array_equal(frame, host):
            wrong.append((name, rc, hrc))
    assert not wrong, wrong[:10]


def test_a_handful_alone(gpu):
    imp = gpu
    fx = {f[0]: f for f in F.load()}
    for name in ("p_photo_53x37_q50_m3", "p_photo_1x1_q0_m0", "h_bmode_mix", "h_parts8_rows9", "h_inner_edges", "h_cat6_ac_m", "s_cols1", "s_16383x1"):
        _, blob, expected = fx[name]
        rc, im = imp.ops.decode_webp(blob, accept=A)
        assert rc == 0 and im.shape == expected.shape and np.array_equal(im.numpy(), expected), name
        im.release()


def _mixed():
    fx = {f[0]: f for f in F.load()}
    lx = {f[0]: f for f in L.load()}
    cuts = {c[0]: c for c in F.truncated()}
    items = [("lossy", fx["h_bmode_mix"][1], fx["h_bmode_mix"][2]), ("lossless", lx["p_rgba_53x37_m3"][1], lx["p_rgba_53x37_m3"][2]),
             ("damaged", cuts["h_bmode_mix-4-last"][1], None), ("refused", dict(F.refused())["r_alph"], None),
             ("lossy", fx["p_photo_53x37_q50_m3"][1], fx["p_photo_53x37_q50_m3"][2]), ("damaged", dict(F.damaged())["d_badstart"], None),
             ("damaged", L.damaged()[1][1], None), ("lossy", fx["s_cols2"][1], fx["s_cols2"][2]), ("refused", L.read("anim.webp"), None),
             ("damaged", cuts["p_photo_53x37_q50_m3-92-last"][1], None), ("lossless", lx["h_colour"][1], lx["h_colour"][2]),
             ("lossy", fx["h_normal_l63_s0"][1], fx["h_normal_l63_s0"][2])]
    return items


def test_a_mixed_call_gives_each_files_lone_result(gpu):
    imp = gpu
    items = _mixed()
    results, launches = imp.ops.batch_decode_webp([b for _, b, _ in items], accept=A)
    assert launches == LOSSLESS + LOSSY
    got = _frames(results)
    for k, ((kind, blob, expected), (rc, frame)) in enumerate(zip(items, got)):
        lone_rc, im = imp.ops.decode_webp(blob, accept=A)
        assert rc == lone_rc, (k, kind, rc, lone_rc)
        assert rc == {"lossy": 0, "lossless": 0, "damaged": F.IMP_ERROR_DECODE_FAILED, "refused": F.IMP_ERROR_UNSUPPORTED}[kind], (k, kind, rc)
        if rc == 0:
            assert np.array_equal(frame, expected) and np.array_equal(im.numpy(), expected), (k, kind)   # damaged neighbours changed nothing
            im.release()
        else:
            assert frame is None and im is None


def test_launch_counts(gpu):
    imp = gpu
    items = _mixed()
    lossy = [b for k, b, _ in items if k == "lossy"]
    lossless = [b for k, b, _ in items if k == "lossless"]
    assert imp.ops.batch_decode_webp(lossy, accept=A)[1] == LOSSY
    assert imp.ops.batch_decode_webp(lossy[:1], accept=A)[1] == LOSSY
    assert imp.ops.batch_decode_webp(lossless, accept=A)[1] == LOSSLESS
    assert imp.ops.batch_decode_webp(lossless + lossy, accept=A)[1] == LOSSLESS + LOSSY
    results, launches = imp.ops.batch_decode_webp(lossy, accept=0)
    assert launches == 0 and [rc for rc, _ in results] == [F.IMP_ERROR_UNSUPPORTED] * len(lossy)
    # files the host front already refuses or fails: nothing is launched for them
    front = [b for _, b in F.refused() + F.damaged()] + [L.read("anim.webp"), L.read("not_webp.png")]
    results, launches = imp.ops.batch_decode_webp(front, accept=A)
    assert launches == 0 and all(rc in (F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED) for rc, _ in results)
    assert imp.ops.batch_decode_webp([], accept=A) == ([], 0)


def test_accept_0_equals_the_old_call(gpu):
    imp = gpu
    blobs = [b for _, b, _ in _mixed()]
    old, old_launches = imp.ops.batch_decode_webp(blobs)
    new, new_launches = imp.ops.batch_decode_webp(blobs, accept=0)
    assert old_launches == new_launches == LOSSLESS
    for (rc0, f0), (rc1, f1) in zip(_frames(old), _frames(new)):
        assert rc0 == rc1 and (f0 is None) == (f1 is None) and (f0 is None or np.array_equal(f0, f1))
    lossy = F.read("p_photo_53x37_q50_m3.webp")
    assert imp.ops.decode_webp(lossy, accept=0)[0] == imp.ops.decode_webp(lossy)[0] == F.IMP_ERROR_UNSUPPORTED


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401
import numpy as np
import ngx_http_imgproc_amd as imp
import webp_lossy_dec_fixtures as F
imp.env_start(0)
names = sys.argv[2].split(",")
fx = {f[0]: f for f in F.load()}
results, launches = imp.ops.batch_decode_webp([fx[n][1] for n in names], accept=1)
ok = sum(1 for (rc, im), n in zip(results, names) if rc == 0 and np.array_equal(im.numpy(), fx[n][2]))
print(json.dumps({"launches": launches, "ok": ok}))
imp.env_destroy()
"""


def test_a_call_cut_into_groups_by_the_stage_cap():
    """IMPGPU_STAGE_CAP_MB=1 in a fresh process (the cap is read once).  A 16383-long frame has 1024 macroblocks: 384 bytes
    of planes and 4 of filter words each, the contexts, the descriptor and the chunk make about 0.43 MB of a group's block, so
    two share a group under a cap of 1 MB and a third does not: the five files make at least two groups."""
    names = ["s_16383x1", "s_1x16383", "s_16383x1", "s_1x16383", "h_bmode_mix"]
    env = dict(os.environ, IMPGPU_STAGE_CAP_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, ",".join(names)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] == len(names) and r["launches"] % 3 == 0 and r["launches"] >= 2 * LOSSY, r


def test_cut_files_get_the_info_calls_code_from_the_batch_call(gpu):
    """files cut short as files: the batch call, the lone call and impgpu_webp_info_ex give one code, with and without the
    bit; nothing is launched for a file the container walk fails"""
    imp = gpu
    blob = F.read("p_photo_53x37_q50_m3.webp")
    cuts = [blob[:n] for n in (0, 11, 12, 20, 25, 40, len(blob) // 2, len(blob) - 1)]
    for accept in (0, A):
        results, launches = imp.ops.batch_decode_webp(cuts, accept=accept)
        assert launches == 0
        for cut, (rc, im) in zip(cuts, results):
            assert im is None and rc == imp.ops.webp_info(cut, accept=accept)[0] == imp.ops.decode_webp(cut, accept=accept)[0] != 0, (accept, len(cut))
    old, _ = imp.ops.batch_decode_webp(cuts)
    assert [rc for rc, _ in old] == [rc for rc, _ in imp.ops.batch_decode_webp(cuts, accept=0)[0]] == [imp.ops.webp_info(c)[0] for c in cuts]
