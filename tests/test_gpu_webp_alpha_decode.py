"""impgpu_image_decode_webp_ex / impgpu_batch_decode_webp_ex with IMPGPU_WEBP_ACCEPT_LOSSY | IMPGPU_WEBP_ACCEPT_ALPHA on the
device (k_webp_alpha behind the lossy and the lossless launches), against Pillow's RGBA frames and the host model's for the
fixtures of tests/golden/webp_alpha_dec: the whole set in one call, a handful alone, a call that mixes lossless, plain lossy,
raw-alpha and VP8L-alpha files of every filter with refused and damaged ones, the launch counts, the calls without the bit,
a call cut into groups by $IMPGPU_STAGE_CAP_MB, and the guard that the merge touches byte 3 only.  Before this feature every
accept=3 call on an alpha file answers IMP_ERROR_UNSUPPORTED."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import webp_alpha_dec_fixtures as F
import webp_dec_fixtures as L
import webp_lossy_dec_fixtures as LY
from conftest import ROOT

pytestmark = pytest.mark.gpu
A = F.ACCEPT
LOSSLESS, LOSSY, ALPHA = 3, 3, 1                  # IMPGPU_WEBP_DEC_LAUNCHES, _LOSSY_LAUNCHES, _ALPHA_LAUNCHES -- a group


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
    assert 140 <= len(fixtures) <= 256
    results, launches = imp.ops.batch_decode_webp([b for _, b, _ in fixtures], accept=A)
    assert launches == LOSSY + ALPHA + LOSSLESS
    wrong = []
    for (name, blob, expected), (rc, frame) in zip(fixtures, _frames(results)):
        hrc, host, _, _ = imp.ops.webp_decode_host(blob, accept=A)
        if rc != 0 or hrc != 0 or not np.array_equal(frame, expected) or not np.array_equal(frame, host):
            wrong.append((name, rc, hrc))
    assert not wrong, wrong[:10]


def test_a_handful_alone(gpu):
    imp = gpu
    for name in ("p_noise_q50_m6", "p_checker_q100_m0", "h_noise_raw_gradient_65x129", "h_noise_vp8l_gradient_65x129", "h_noise_raw_horizontal_129x1",
                 "h_noise_vp8l_vertical_1x129", "h_long_raw_gradient_16383x1", "h_long_raw_vertical_1x16383", "h_saturate_vp8l_gradient", "h_flag_no_alph", "h_own_answer_53x37"):
        _, blob, expected = F.get(name)
        rc, im = imp.ops.decode_webp(blob, accept=A)
        assert rc == 0 and im.shape == expected.shape and np.array_equal(im.numpy(), expected), name
        im.release()


def _mixed():
    lx = {f[0]: f for f in L.load()}
    ly = {f[0]: f for f in LY.load()}
    items = [("ok", lx["p_rgba_53x37_m3"][1], lx["p_rgba_53x37_m3"][2]), ("ok", ly["h_bmode_mix"][1], ly["h_bmode_mix"][2])]
    for f in F.FILTERS:
        for kind in ("raw", "vp8l"):
            _, blob, expected = F.get("h_noise_%s_%s_63x65" % (kind, f))
            items.append(("ok", blob, expected))
    items.insert(4, ("refused", dict(F.refused())["r_alph_twice"], None))
    items.insert(6, ("damaged", dict(F.damaged())["d_vp8l_half"], None))          # fails on the device: its stream runs past its chunk
    items.insert(7, ("damaged", dict(F.damaged())["d_raw_one_short"], None))
    items.append(("damaged", dict(F.damaged())["d_vp8_badstart"], None))
    items.append(("ok", F.get("p_ramp_q100_m4")[1], F.get("p_ramp_q100_m4")[2]))
    return items


def test_a_mixed_call_gives_each_files_lone_result(gpu):
    imp = gpu
    items = _mixed()
    results, launches = imp.ops.batch_decode_webp([b for _, b, _ in items], accept=A)
    assert launches == LOSSLESS + LOSSY + ALPHA
    for k, ((kind, blob, expected), (rc, frame)) in enumerate(zip(items, _frames(results))):
        lone_rc, im = imp.ops.decode_webp(blob, accept=A)
        assert rc == lone_rc, (k, kind, rc, lone_rc)
        assert rc == {"ok": 0, "damaged": F.IMP_ERROR_DECODE_FAILED, "refused": F.IMP_ERROR_UNSUPPORTED}[kind], (k, kind, rc)
        if rc == 0:
            assert np.array_equal(frame, expected) and np.array_equal(im.numpy(), expected), (k, kind)   # damaged neighbours changed nothing
            im.release()
        else:
            assert frame is None and im is None


def test_launch_counts(gpu):
    imp = gpu
    raw = [F.get("h_noise_raw_%s_64x64" % f)[1] for f in F.FILTERS]
    vp8l = [F.get("h_noise_vp8l_%s_64x64" % f)[1] for f in F.FILTERS]
    plain = [LY.read("h_bmode_mix.webp"), F.read("h_flag_no_alph.webp")]
    lossless = [L.read("p_rgba_53x37_m3.webp")]
    assert imp.ops.batch_decode_webp(raw, accept=A)[1] == LOSSY + ALPHA == 4
    assert imp.ops.batch_decode_webp(raw[:1], accept=A)[1] == 4
    assert imp.ops.batch_decode_webp(vp8l, accept=A)[1] == LOSSY + ALPHA + LOSSLESS == 7
    assert imp.ops.batch_decode_webp(vp8l[3:], accept=A)[1] == 7
    assert imp.ops.batch_decode_webp(raw + vp8l + plain, accept=A)[1] == 7
    assert imp.ops.batch_decode_webp(raw + lossless, accept=A)[1] == 7
    assert imp.ops.batch_decode_webp(plain, accept=A)[1] == LOSSY
    assert imp.ops.batch_decode_webp(lossless, accept=A)[1] == LOSSLESS
    assert imp.ops.batch_decode_webp(plain + lossless, accept=A)[1] == LOSSY + LOSSLESS
    # files the host front already refuses or fails: nothing is launched for them
    front = [b for n, b in F.refused() + F.damaged() if "vp8l" not in n]
    results, launches = imp.ops.batch_decode_webp(front, accept=A)
    assert launches == 0 and all(rc in (F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED) for rc, _ in results)
    assert imp.ops.batch_decode_webp([], accept=A) == ([], 0)


def test_without_the_alpha_bit_nothing_changes(gpu):
    imp = gpu
    blobs = [b for n, b, _ in F.load() if n != "h_flag_no_alph"]
    results, launches = imp.ops.batch_decode_webp(blobs, accept=F.ACCEPT_LOSSY)
    assert launches == 0 and [rc for rc, _ in results] == [F.IMP_ERROR_UNSUPPORTED] * len(blobs)
    mixed = [b for _, b, _ in _mixed()]
    for accept in (0, F.ACCEPT_ALPHA):
        old, old_launches = imp.ops.batch_decode_webp(mixed)
        new, new_launches = imp.ops.batch_decode_webp(mixed, accept=accept)
        assert old_launches == new_launches == LOSSLESS
        for (rc0, f0), (rc1, f1) in zip(_frames(old), _frames(new)):
            assert rc0 == rc1 and (f0 is None) == (f1 is None) and (f0 is None or np.array_equal(f0, f1))
    blob = F.get("p_noise_q50_m6")[1]
    assert imp.ops.decode_webp(blob, accept=2)[0] == imp.ops.decode_webp(blob, accept=0)[0] == imp.ops.decode_webp(blob)[0] == F.IMP_ERROR_UNSUPPORTED
    # accept=1 on the mixed call: the lossy route's answers, each alpha file refused
    one, launches = imp.ops.batch_decode_webp(mixed, accept=F.ACCEPT_LOSSY)
    assert launches == LOSSLESS + LOSSY
    for (kind, blob, _), (rc, im) in zip(_mixed(), one):
        assert rc == (F.IMP_ERROR_UNSUPPORTED if b"ALPH" in blob[:64] else 0), kind
        if im is not None:
            im.release()


def test_the_merge_touches_byte_3_only(gpu):
    imp = gpu
    for name in ("h_noise_raw_gradient_63x65", "h_noise_vp8l_horizontal_65x63", "p_noise_q100_m4"):
        _, blob, expected = F.get(name)
        bare = LY.cases.container(LY.cases.vp8_payload(blob))
        rc, im = imp.ops.decode_webp(blob, accept=A)
        brc, bim = imp.ops.decode_webp(bare, accept=F.ACCEPT_LOSSY)
        assert rc == 0 and brc == 0
        got, plain = im.numpy(), bim.numpy()
        im.release()
        bim.release()
        assert np.array_equal(got[:, :, :3], plain[:, :, :3]) and (plain[:, :, 3] == 255).all(), name
        assert np.array_equal(got[:, :, 3], expected[:, :, 3]) and (got[:, :, 3] != 255).any(), name


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import torch  # noqa: F401
import numpy as np
import ngx_http_imgproc_amd as imp
import webp_alpha_dec_fixtures as F
imp.env_start(0)
names = sys.argv[2].split(",")
results, launches = imp.ops.batch_decode_webp([F.get(n)[1] for n in names], accept=3)
ok = sum(1 for (rc, im), n in zip(results, names) if rc == 0 and np.array_equal(im.numpy(), F.get(n)[2]))
print(json.dumps({"launches": launches, "ok": ok}))
imp.env_destroy()
"""


def test_a_call_cut_into_groups_by_the_stage_cap():
    """IMPGPU_STAGE_CAP_MB=1 in a fresh process (the cap is read once).  A 16383-long frame with a raw plane takes about
    0.44 MB of a group's block (0.40 MB of planes, its chunk, its 16 KB of alpha), so two share a group under the cap of
    1 MB and a third does not; a 65x129 file with a VP8L plane takes about 0.1 MB, its scratch plane and its stream's blocks
    counted.  Five long files and two such files in this order make exactly three groups -- two long ones, two long ones, the
    last long one with both VP8L planes -- so 3 + 1, 3 + 1 and 3 + 1 + 3 launches."""
    names = ["h_long_raw_gradient_16383x1", "h_long_raw_horizontal_1x16383", "h_long_raw_vertical_16383x1", "h_long_raw_none_1x16383",
             "h_long_raw_horizontal_16383x1", "h_noise_vp8l_gradient_65x129", "h_noise_vp8l_vertical_65x129"]
    env = dict(os.environ, IMPGPU_STAGE_CAP_MB="1")
    p = subprocess.run([sys.executable, "-c", _CHILD, ROOT, ",".join(names)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads(p.stdout.strip().splitlines()[-1])
    assert r["ok"] == len(names) and r["launches"] == 2 * (LOSSY + ALPHA) + (LOSSY + ALPHA + LOSSLESS) == 15, r
