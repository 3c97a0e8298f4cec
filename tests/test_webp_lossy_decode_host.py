"""impgpu_webp_decode_host_ex / impgpu_webp_info_ex (no device): the lossy WebP decoder's lane code, one lane after the other,
against Pillow's libwebp on the fixtures of tests/golden/webp_lossy_dec -- Pillow-encoded frames at qualities 0..100 and
methods 0 / 3 / 6, the hand-written key frames of webp_vp8_dec_cases.py, refused, damaged and truncated files.  Every _ex
symbol and the accept keyword are missing from the tree before this feature."""
import numpy as np

import webp_dec_fixtures as L
import webp_lossy_dec_fixtures as F
from ngx_http_imgproc_amd import ops

A = F.ACCEPT_LOSSY
FEATURES = {
    "segments": 0x1, "map update": 0x2, "delta values": 0x4, "simple filter": 0x8, "normal filter": 0x10, "sharpness": 0x20,
    "lf deltas": 0x40, "2 partitions": 0x80, "4 partitions": 0x100, "8 partitions": 0x200, "B_PRED": 0x400, "probability update": 0x800,
    "skip off": 0x1000, "dq y1 dc": 0x2000, "dq y2 dc": 0x4000, "dq y2 ac": 0x8000, "dq uv dc": 0x10000, "dq uv ac": 0x20000,
    "DCT_CAT6": 0x40000, "cropped width": 0x80000, "cropped height": 0x100000,
}


def _decoded():
    return [(name, expected, ops.webp_decode_host(blob, accept=A)) for name, blob, expected in F.load()]


def test_every_fixture_decodes_to_pillows_frame():
    fixtures = F.load()
    assert len(fixtures) >= 180
    wrong = []
    for name, expected, (rc, frame, info, intact) in _decoded():
        if rc != F.IMP_OK or not intact or frame.shape != expected.shape or not (frame == expected).all() or info[7] != 1:
            wrong.append((name, rc, info))
    assert not wrong, wrong[:10]


def test_the_fixture_set_covers_every_feature_bit_and_every_mode():
    seen, modes, pillow = 0, 0, 0
    for name, _, (rc, _, info, _) in _decoded():
        assert rc == F.IMP_OK, name
        seen |= info[0]
        modes |= info[1]
        if name.startswith("p_"):
            pillow |= info[0]
    assert sorted(FEATURES.values()) == [1 << k for k in range(21)]
    missing = [what for what, bit in FEATURES.items() if not seen & bit]
    assert not missing and seen == 0x1FFFFF, (missing, hex(seen))
    assert modes == 0x3FFFF, hex(modes)                       # four 16x16 modes, four chroma modes, ten sub-block modes
    # why the hand-written files exist: Pillow's encoder never writes these
    # (more than one partition, the simple filter, a sharpness, lf deltas, delta values)
    assert not pillow & (0x8 | 0x20 | 0x40 | 0x80 | 0x100 | 0x200 | 0x4), hex(pillow)
    # and what single files are there for
    for name, bit in (("h_simple_l20", 0x8), ("h_lfdelta_neg", 0x40), ("h_parts8_rows9", 0x200), ("h_seg_delta", 0x4), ("h_skip_off", 0x1000),
                      ("h_cat6_y2_p", 0x40000), ("h_probs_type3", 0x800), ("h_dq_uvac_m_q0", 0x20000), ("h_normal_l63_s7", 0x20)):
        assert ops.webp_decode_host(F.read(name + ".webp"), accept=A)[2][0] & bit, name
    for m in range(10):                                       # a file of one sub-block mode meets that mode alone
        assert ops.webp_decode_host(F.read("h_bmode_%d.webp" % m), accept=A)[2][1] >> 8 == 1 << m


def test_each_seam_file_reaches_its_seam():
    """info[3] / info[4]: macroblock columns and rows; info[2]: token partitions"""
    info = {name: ops.webp_decode_host(F.read(name + ".webp"), accept=A)[2] for name in ("s_cols1", "s_cols2", "s_rows40", "s_16383x1", "s_1x16383")}
    assert info["s_cols1"][3] == 1 and info["s_cols1"][4] > 1              # no left neighbour anywhere, above-right always replicated
    assert info["s_cols2"][3] == 2                                          # the rightmost column is also the first with a left edge
    assert info["s_rows40"][4] == 40 and info["s_rows40"][2] == 8           # every partition five times over
    assert info["s_16383x1"][3:5] == [1024, 1] and info["s_1x16383"][3:5] == [1, 1024]
    for name in info:
        assert info[name][0] & 0x10, name                                   # all through the normal filter


def test_info_gives_the_geometry_without_decoding():
    for name, blob, expected in F.load():
        assert ops.webp_info(blob, accept=A) == (F.IMP_OK, expected.shape[1], expected.shape[0], 4), name
        assert ops.webp_info(blob, accept=0)[0] == F.IMP_ERROR_UNSUPPORTED and ops.webp_info(blob)[0] == F.IMP_ERROR_UNSUPPORTED


def test_refused_and_damaged_files_give_their_codes():
    assert {n for n, _ in F.refused()} == {"r_alph", "r_inter", "r_hidden"}
    for name, blob in F.refused():
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED, name
        assert ops.webp_info(blob, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED, name
    assert {n for n, _ in F.damaged()} == {"d_badstart", "d_version5", "d_first_past_chunk", "d_table_past_chunk"}
    for name, blob in F.damaged():
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0] == F.IMP_ERROR_DECODE_FAILED, name
    for f in ("anim.webp", "not_webp.png"):
        assert ops.webp_decode_host(L.read(f), capacity=1 << 16, accept=A)[0] == F.IMP_ERROR_UNSUPPORTED, f


def test_truncated_partitions_follow_libwebps_end_rule():
    """Pillow's verdict for each cut was recorded when the files were written: a failure only once a byte past the end had
    to be loaded, looked at per macroblock"""
    cuts = F.truncated()
    assert len(cuts) == 24 and any(ok for _, _, ok, _, _ in cuts) and any(not ok for _, _, ok, _, _ in cuts)
    expected = {name: e for name, _, e in F.load()}
    for label, blob, ok, same, name in cuts:
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected[name].size, accept=A)
        assert intact and rc == (F.IMP_OK if ok else F.IMP_ERROR_DECODE_FAILED), (label, rc, ok)
        if ok:
            assert np.array_equal(frame, expected[name]) == same, label


def test_accept_0_is_the_call_without_ex():
    for name, blob, _ in F.load():
        assert ops.webp_decode_host(blob, capacity=1 << 12, accept=0)[0] == F.IMP_ERROR_UNSUPPORTED, name
    for name, blob, expected in L.load()[::7]:
        for accept in (0, A):
            rc, frame, info, intact = ops.webp_decode_host(blob, accept=accept)
            old = ops.webp_decode_host(blob)
            assert (rc, info, intact) == (old[0], old[2], True) and (frame == expected).all() and (frame == old[1]).all(), name
            assert ops.webp_info(blob, accept=accept) == ops.webp_info(blob)
    assert ops.webp_decode_host(L.read("lossy.webp"), capacity=1 << 16, accept=0)[0] == F.IMP_ERROR_UNSUPPORTED
    assert ops.webp_decode_host(L.read("lossy.webp"), accept=A)[0] == F.IMP_OK


def test_the_guard_band_behind_an_exact_fit_is_intact_and_one_byte_short_is_refused():
    for name in ("p_photo_53x37_q50_m3", "h_bmode_mix", "s_cols1"):
        blob = F.read(name + ".webp")
        expected = [e for n, _, e in F.load() if n == name][0]
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected.size, guard=4096, accept=A)
        assert rc == F.IMP_OK and intact and (frame == expected).all()
        rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected.size - 1, guard=4096, accept=A)
        assert rc == F.IMP_ERROR_MALLOC_FAILED and frame is None and intact


def test_the_encoders_own_files_decode_to_the_encoders_reconstruction():
    """encode_webp_lossy_host over its tests' kinds of frames: the decoder shows what the encoder reconstructed"""
    from webp_vp8_writer import decoded_rgb

    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:37, 0:53]
    smooth = np.clip(np.stack([xx * 4, yy * 6, (xx + yy) * 2, np.full_like(xx, 255)], 2), 0, 255).astype(np.uint8)
    for frame in (rng.integers(0, 256, (37, 53, 4), dtype=np.uint8) | np.array([0, 0, 0, 255], np.uint8), smooth, smooth[:16, :16], smooth[:1, :1], smooth[:33, :17, :3],
                  smooth[:, :, 1:2]):
        frame = np.ascontiguousarray(frame)
        for quality in (0, 50, 100):
            rc, blob, n, intact, det = ops.encode_webp_lossy_host(frame, quality, details=True)
            assert rc == 0 and intact
            h, w = frame.shape[:2]
            rc, got, info, intact = ops.webp_decode_host(blob, accept=A)
            assert rc == 0 and intact and info[7] == 1
            assert np.array_equal(got[:, :, 2::-1], decoded_rgb(det["y"], det["u"], det["v"], w, h)), (frame.shape, quality)


def _file_cuts():
    """lossy files cut anywhere as FILES (sizes not rewritten): inside the RIFF header, the chunk header, the frame tag, both
    kinds of partition; alone and inside VP8X"""
    out = []
    for name in ("p_photo_53x37_q50_m3", "h_vp8x_chunks", "h_parts2_rows3"):
        blob = F.read(name + ".webp")
        for n in sorted({0, 11, 12, 19, 20, 25, 29, 30, 40, len(blob) // 2, len(blob) - 5, len(blob) - 1}):
            out.append(("%s[:%d]" % (name, n), blob[:n]))
    return out


def test_cut_files_without_the_bit_answer_as_the_calls_without_ex():
    seen = set()
    for label, blob in _file_cuts():
        old = ops.webp_info(blob)
        assert ops.webp_info(blob, accept=0) == old, label
        assert ops.webp_decode_host(blob, capacity=1 << 16, accept=0)[0] == ops.webp_decode_host(blob, capacity=1 << 16)[0] == old[0], label
        seen.add(old[0])
    assert seen == {F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED}      # (a name before a size: UNSUPPORTED once `VP8 ` is read)


def test_cut_files_with_the_bit_get_one_code_from_info_and_decode():
    """a `VP8 ` chunk that runs past the file is IMP_ERROR_DECODE_FAILED in every call; where the header can still be read
    the info call's code is the one the decode call gives before it needs room"""
    seen = set()
    for label, blob in _file_cuts():
        irc = ops.webp_info(blob, accept=A)[0]
        drc = ops.webp_decode_host(blob, capacity=1 << 16, accept=A)[0]
        assert irc == drc, (label, irc, drc)
        seen.add(irc)
        if 20 <= len(blob) and blob[12:16] == b"VP8 ":                         # a lone chunk: past the file, or only its pad byte lost
            past = len(blob) < 20 + int.from_bytes(blob[16:20], "little")
            assert irc == (F.IMP_ERROR_DECODE_FAILED if past else F.IMP_OK), label
    # UNSUPPORTED: fewer than the 12 bytes of a RIFF header; OK: the file that lost only a byte of the chunks BEHIND its image
    assert seen == {F.IMP_OK, F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED}
