"""impgpu_webp_decode_host_ex / impgpu_webp_info_ex / impgpu_webp_alpha_info (no device) with IMPGPU_WEBP_ACCEPT_LOSSY |
IMPGPU_WEBP_ACCEPT_ALPHA: the alpha route's host front and k_webp_alpha's lane code, one lane after the other, against
Pillow's libwebp on the fixtures of tests/golden/webp_alpha_dec.  Before this feature accept=3 on a file with an ALPH chunk
is IMP_ERROR_UNSUPPORTED and impgpu_webp_alpha_info does not exist."""
import json
import os

import numpy as np

import webp_alpha_dec_cases as cases
import webp_alpha_dec_fixtures as F
import webp_lossy_dec_fixtures as LY
from ngx_http_imgproc_amd import ops

A = F.ACCEPT
BACKREF, CACHE, INDEXING, PREDICTOR = 0x40, 0x10, 0x8, 0x1
BUNDLE_2, BUNDLE_4, BUNDLE_8 = 0x800, 0x1000, 0x2000


def test_every_fixture_decodes_to_pillows_rgba_frame():
    fixtures = F.load()
    assert 140 <= len(fixtures) <= 256
    wrong = []
    for name, blob, expected in fixtures:
        rc, frame, info, intact = ops.webp_decode_host(blob, accept=A)
        if rc != F.IMP_OK or not intact or frame.shape != expected.shape or not (frame == expected).all() or info[7] != 1:
            wrong.append((name, rc))
    assert not wrong, wrong[:10]


def test_the_fixture_set_covers_every_filter_method_and_seam():
    """impgpu_webp_alpha_info says what each file holds"""
    seen, pillow = set(), set()
    sizes = {}
    for name, blob, expected in F.load():
        rc, (method, filt, pre, feat) = ops.webp_alpha_info(blob)
        if name == "h_flag_no_alph":
            assert rc == F.IMP_ERROR_UNSUPPORTED and (expected[:, :, 3] == 255).all()
            continue
        assert rc == F.IMP_OK, name
        assert F.alph_header(blob) == method | filt << 2 | pre << 4, name
        assert (feat == 0) == (method == 0), name
        seen.add((method, filt, pre))
        sizes.setdefault((method, filt), set()).add(expected.shape[:2])
        if name.startswith("p_"):
            pillow.add(F.alph_header(blob))
    assert {(m, f) for m, f, _ in seen} == {(m, f) for m in (0, 1) for f in range(4)}
    assert {p for _, _, p in seen} == {0, 1}
    assert pillow == {0x00, 0x01, 0x05, 0x11}                  # why the hand-assembled files exist: never vertical, never gradient
    for key, shapes in sizes.items():                          # every filter x method at the seams of a 64-lane scan and a 64-row band
        assert {s for hw in shapes for s in hw} >= {1, 2, 63, 64, 65, 129}, key
    for f in range(4):                                         # the format's longest row and column
        for name in ("h_long_raw_%s_16383x1" % F.FILTERS[f], "h_long_raw_%s_1x16383" % F.FILTERS[f]):
            assert ops.webp_alpha_info(F.get(name)[1]) == (F.IMP_OK, [0, f, 0, 0]) and 16383 in F.get(name)[2].shape


def test_vp8l_planes_reach_the_lossless_decoders_corners():
    feat = {name: ops.webp_alpha_info(blob)[1][3] for name, blob, _ in F.load()}
    assert feat["h_levels2_vp8l_none"] & BUNDLE_8 and feat["h_levels4_vp8l_none"] & BUNDLE_4 and feat["h_levels16_vp8l_none"] & BUNDLE_2
    assert not feat["h_levels40_vp8l_none"] & INDEXING and len(np.unique(F.get("h_levels40_vp8l_none")[2][:, :, 3])) > 16
    assert feat["h_lz_vp8l_horizontal"] & BACKREF and feat["h_writer_vp8l_gradient"] & PREDICTOR
    assert feat["h_dither_vp8l_vertical"] & CACHE
    for name, levels in (("h_levels2_vp8l_none", 2), ("h_levels4_vp8l_none", 4), ("h_levels16_vp8l_none", 16)):
        assert len(np.unique(F.get(name)[2][:, :, 3])) == levels


def test_the_gradient_fixture_saturates_both_ways_and_the_edge_planes_differ_from_the_general_rule():
    a = F.get("h_saturate_raw_gradient")[2][:, :, 3]
    assert cases.gradient_saturates(a)
    assert (F.get("h_saturate_vp8l_gradient")[2][:, :, 3] == a).all()
    # row 0 under the vertical filter and column 0 under the horizontal one follow their own rule: a decoder that used the
    # general rule there (top of row 0 = 0, left of column 0 = 0) would return the residuals themselves
    for f, filt in ((cases.HORIZONTAL, "horizontal"), (cases.VERTICAL, "vertical"), (cases.GRADIENT, "gradient")):
        a = F.get("h_edges_raw_" + filt)[2][:, :, 3]
        r = cases.residuals(a, f)
        assert (r[0, 1:] != a[0, 1:]).any() and (r[1:, 0] != a[1:, 0]).any()


def test_container_details():
    assert len(cases.find_chunk(F.read("h_pad_raw_64x65.webp"), b"ALPH")) % 2 == 1      # the pad byte is there
    assert len(cases.find_chunk(F.read("h_long_alph_raw.webp"), b"ALPH")) == 1 + 64 * 64 + 3
    assert cases.find_chunk(F.read("h_flag_no_alph.webp"), b"ALPH") is None
    assert F.read("h_flag_no_alph.webp")[20] & 0x10
    rc, frame, _, _ = ops.webp_decode_host(F.read("h_flag_no_alph.webp"), accept=F.ACCEPT_LOSSY)   # as the lossy route took it
    assert rc == F.IMP_OK and (frame == F.get("h_flag_no_alph")[2]).all()


def test_a_repeated_vp8x_is_skipped_and_the_first_one_speaks():
    """VP8X(flag) ALPH VP8X(another canvas, no flag) `VP8 ` is the canonical file with one more skipped chunk; a first VP8X
    without the flag refuses the ALPH whatever a second one says"""
    _, blob, expected = F.get("h_noise_raw_gradient_64x64")
    a, v = cases.find_chunk(blob, b"ALPH"), cases.find_chunk(blob, b"VP8 ")
    again = cases.riff(cases.vp8x(64, 64), cases.chunk(b"ALPH", a), cases.vp8x(7, 9, 0), cases.chunk(b"VP8 ", v))
    rc, frame, _, _ = ops.webp_decode_host(again, accept=A)
    assert rc == F.IMP_OK and (frame == expected).all()
    again = cases.riff(cases.vp8x(64, 64), cases.vp8x(7, 9, 0), cases.chunk(b"ALPH", a), cases.chunk(b"VP8 ", v))
    rc, frame, _, _ = ops.webp_decode_host(again, accept=A)
    assert rc == F.IMP_OK and (frame == expected).all()
    for first in (cases.vp8x(64, 64, 0), cases.vp8x(7, 9)):
        late = cases.riff(first, cases.vp8x(64, 64), cases.chunk(b"ALPH", a), cases.chunk(b"VP8 ", v))
        assert ops.webp_decode_host(late, capacity=1 << 16, accept=A)[0] == ops.webp_info(late, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED
        assert ops.webp_alpha_info(late)[0] == F.IMP_ERROR_UNSUPPORTED


def test_bgr_is_the_bare_vp8_chunks():
    for name, blob, expected in F.load()[::5]:
        bare = LY.cases.container(LY.cases.vp8_payload(blob))
        rc, frame, _, _ = ops.webp_decode_host(bare, accept=F.ACCEPT_LOSSY)
        assert rc == F.IMP_OK and (frame[:, :, :3] == expected[:, :, :3]).all() and (frame[:, :, 3] == 255).all(), name


def test_info_gives_the_geometry():
    for name, blob, expected in F.load():
        assert ops.webp_info(blob, accept=A) == (F.IMP_OK, expected.shape[1], expected.shape[0], 4), name


def test_refused_and_damaged_files_give_their_codes():
    assert {n for n, _ in F.refused()} == {"r_alph_before_vp8l", "r_alph_behind_image", "r_alph_twice", "r_alph_no_vp8x", "r_alph_flag_clear",
                                           "r_canvas_differs", "r_anim", "r_anmf"}
    for name, blob in F.refused():
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED, name
        assert ops.webp_info(blob, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED, name
        assert ops.webp_alpha_info(blob)[0] == F.IMP_ERROR_UNSUPPORTED, name
    assert {n for n, _ in F.damaged()} == {"d_alph_empty", "d_alph_header_only", "d_method2", "d_method3", "d_pre2", "d_pre3", "d_reserved40", "d_reserved80",
                                           "d_raw_one_short", "d_vp8l_transform_twice", "d_vp8l_half", "d_vp8_badstart"}
    for name, blob in F.damaged():
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0] == F.IMP_ERROR_DECODE_FAILED, name
        assert ops.webp_alpha_info(blob)[0] == F.IMP_ERROR_DECODE_FAILED, name
        if "vp8l" not in name:                                 # what the header byte and the sizes already show, the info call shows too
            assert ops.webp_info(blob, accept=A)[0] == F.IMP_ERROR_DECODE_FAILED, name
    # the file the lossy route's tests refuse is a canonical one (a raw plane of zeros): taken with the new bit, refused without
    rc, frame, _, _ = ops.webp_decode_host(LY.read("r_alph.webp"), accept=A)
    assert rc == F.IMP_OK and frame.shape == (48, 48, 4) and (frame[:, :, 3] == 0).all()
    assert ops.webp_decode_host(LY.read("r_alph.webp"), capacity=1 << 16, accept=F.ACCEPT_LOSSY)[0] == F.IMP_ERROR_UNSUPPORTED


def test_cut_alph_payloads_follow_pillows_verdicts():
    cuts = F.truncated()
    with open(os.path.join(F.HERE, "verdicts.json")) as f:
        assert len(cuts) == len(json.load(f)) == len(cases.CUTS) == 20
    assert any(ok for _, _, ok, _, _ in cuts) and any(not ok for _, _, ok, _, _ in cuts)
    assert {F.alph_header(F.read(name + ".webp")) & 3 for _, _, _, _, name in cuts} == {0, 1}      # raw and VP8L payloads
    for label, blob, ok, same, name in cuts:
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=F.get(name)[2].size, accept=A)
        assert intact and rc == (F.IMP_OK if ok else F.IMP_ERROR_DECODE_FAILED), (label, rc, ok)
        if ok:
            assert same and np.array_equal(frame, F.get(name)[2]), label     # (a cut Pillow decodes to another frame would need that frame stored)


def test_without_the_bit_every_fixture_gets_the_verdict_it_got_before():
    """accept 0 and 2 are the calls without _ex (these files hold no VP8L image: refused); accept 1 is the lossy route, which
    refuses a file at its ALPH chunk -- unless the chunk lies behind the image, where that walk never gets to"""
    every = [(n, b) for n, b, _ in F.load()] + F.refused() + F.damaged() + [(c[0], c[1]) for c in F.truncated()]
    for name, blob in every:
        old = ops.webp_decode_host(blob, capacity=1 << 12)[0]
        assert old == ops.webp_info(blob)[0]
        for accept in (0, F.ACCEPT_ALPHA):
            assert ops.webp_decode_host(blob, capacity=1 << 12, accept=accept)[0] == old, name
            assert ops.webp_info(blob, accept=accept) == ops.webp_info(blob), name
        want = F.IMP_ERROR_UNSUPPORTED
        if name == "h_flag_no_alph":
            want = F.IMP_OK
        if name == "r_alph_behind_image":
            want = F.IMP_OK
        assert ops.webp_info(blob, accept=F.ACCEPT_LOSSY)[0] == want, name
        assert ops.webp_alpha_info(blob)[0] != F.IMP_OK or ops.webp_decode_host(blob, capacity=1 << 12, accept=F.ACCEPT_LOSSY)[0] == F.IMP_ERROR_UNSUPPORTED, name
    # lossless and plain lossy files: the new bit changes nothing
    for name, blob, expected in LY.load()[::9]:
        old = ops.webp_decode_host(blob, accept=F.ACCEPT_LOSSY)
        new = ops.webp_decode_host(blob, accept=A)
        assert old[0] == new[0] == F.IMP_OK and (old[1] == new[1]).all() and old[2] == new[2], name
        assert ops.webp_alpha_info(blob)[0] == F.IMP_ERROR_UNSUPPORTED
    import webp_dec_fixtures as L
    for name, blob, expected in L.load()[::9]:
        old, new = ops.webp_decode_host(blob), ops.webp_decode_host(blob, accept=A)
        assert old[0] == new[0] == F.IMP_OK and (old[1] == new[1]).all() and old[2] == new[2], name
    for name, blob in LY.damaged() + LY.refused():
        if name == "r_alph":                                   # (a canonical alpha file: see the test above)
            continue
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0] == ops.webp_decode_host(blob, capacity=1 << 16, accept=F.ACCEPT_LOSSY)[0], name


def test_the_guard_band_and_one_byte_short():
    for name in ("h_noise_vp8l_gradient_63x65", "h_noise_raw_vertical_65x129", "p_noise_q50_m6"):
        _, blob, expected = F.get(name)
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected.size, guard=4096, accept=A)
        assert rc == F.IMP_OK and intact and (frame == expected).all()
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected.size - 1, guard=4096, accept=A)
        assert rc == F.IMP_ERROR_MALLOC_FAILED and frame is None and intact


def test_the_projects_own_answers_come_back():
    """encode_webp_lossy_host of a B,G,R,A frame writes VP8X + a raw ALPH + `VP8 `: the alpha comes back exactly, B,G,R are the
    encoder's reconstruction"""
    from webp_vp8_writer import decoded_rgb

    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:37, 0:53]
    frame = np.clip(np.stack([xx * 4, yy * 6, (xx + yy) * 2, xx * 0], 2), 0, 255).astype(np.uint8)
    frame[:, :, 3] = rng.integers(0, 256, (37, 53))
    # the committed fixture is such a file: written by the encoder, judged by Pillow, decoded on the device with the others
    _, blob, expected = F.get("h_own_answer_53x37")
    assert blob == ops.encode_webp_lossy_host(cases.own_frame(), 75)[1] and (expected[:, :, 3] == cases.own_frame()[:, :, 3]).all()
    for quality in (20, 75):
        rc, blob, n, intact, det = ops.encode_webp_lossy_host(frame, quality, details=True)
        assert rc == 0 and intact
        assert ops.webp_alpha_info(blob) == (F.IMP_OK, [0, 0, 0, 0])
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=F.ACCEPT_LOSSY)[0] == F.IMP_ERROR_UNSUPPORTED
        rc, got, info, intact = ops.webp_decode_host(blob, accept=A)
        assert rc == 0 and intact and (got[:, :, 3] == frame[:, :, 3]).all()
        assert np.array_equal(got[:, :, 2::-1], decoded_rgb(det["y"], det["u"], det["v"], 53, 37))


def test_the_generator_writes_what_is_committed(tmp_path, monkeypatch):
    """regenerating the fixtures reproduces every file, expected.npz's frames and verdicts.json"""
    import pytest
    pytest.importorskip("PIL")
    monkeypatch.setattr(cases, "HERE", str(tmp_path))
    cases.main()
    names = sorted(f for f in os.listdir(F.HERE))
    assert names == sorted(os.listdir(str(tmp_path)))
    for f in names:
        if f.endswith(".webp") or f == "verdicts.json":
            with open(os.path.join(str(tmp_path), f), "rb") as g:
                assert g.read() == F.read(f), f
    new, old = np.load(os.path.join(str(tmp_path), "expected.npz")), np.load(os.path.join(F.HERE, "expected.npz"))
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert np.array_equal(new[k], old[k]), k
