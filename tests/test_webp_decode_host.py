"""impgpu_webp_decode_host / impgpu_webp_info (no device): the lossless WebP decoder's lane code, one lane after the other,
against Pillow's libwebp on the fixtures of tests/golden/webp_dec -- Pillow-encoded frames at methods 0 / 3 / 6 and the
hand-written streams of webp_dec_cases.py.  Every new symbol is missing from the tree before this feature."""
import numpy as np

import webp_dec_fixtures as F
from ngx_http_imgproc_amd import ops

FEATURES = {
    "predictor": 0x0001, "colour transform": 0x0002, "subtract green": 0x0004, "colour indexing": 0x0008, "colour cache": 0x0010,
    "more than one group": 0x0020, "backward reference": 0x0040, "simple code": 0x0080, "distance code above 24": 0x0100,
    "mapped distance clamped to 1": 0x0200, "one pixel a value": 0x0400, "two pixels a value": 0x0800, "four pixels a value": 0x1000,
    "eight pixels a value": 0x2000,
}


def test_every_fixture_decodes_to_pillows_frame():
    fixtures = F.load()
    assert len(fixtures) >= 200
    wrong = []
    for name, blob, expected in fixtures:
        rc, frame, info, intact = ops.webp_decode_host(blob)
        if rc != F.IMP_OK or not intact or frame.shape != expected.shape or not (frame == expected).all():
            wrong.append((name, rc, info))
    assert not wrong, wrong[:10]


def test_the_fixture_set_covers_every_feature_bit():
    """the OR of the host model's feature words over the whole set"""
    seen, by_kind = 0, {"p_": 0, "h_": 0}
    for name, blob, _ in F.load():
        rc, _, info, _ = ops.webp_decode_host(blob)
        assert rc == F.IMP_OK, name
        seen |= info[0]
        by_kind[name[:2]] |= info[0]
    assert sorted(FEATURES.values()) == [1 << k for k in range(14)]
    missing = [what for what, bit in FEATURES.items() if not seen & bit]
    assert not missing and seen == 0x3FFF, (missing, hex(seen), {k: hex(v) for k, v in by_kind.items()})
    # what the hand-written streams are there for
    for name, bit in (("h_clamp018", 0x0200), ("h_dist025", 0x0100), ("h_groups4", 0x0020), ("h_simple2", 0x0080), ("h_cache11", 0x0010), ("h_colour", 0x0002)):
        blob = F.read(name + ".webp")
        assert ops.webp_decode_host(blob)[2][0] & bit, name


def test_info_gives_the_geometry():
    for name, blob, expected in F.load():
        assert ops.webp_info(blob) == (F.IMP_OK, expected.shape[1], expected.shape[0], 4), name


def test_a_small_capacity_is_refused_with_nothing_written():
    name, blob, expected = [f for f in F.load() if f[0] == "p_photo_17x13_m3"][0]
    rc, frame, _, intact = ops.webp_decode_host(blob, capacity=expected.size - 1)
    assert rc == F.IMP_ERROR_MALLOC_FAILED and frame is None and intact


def test_lossy_animated_and_foreign_files_are_unsupported():
    for f in ("lossy.webp", "anim.webp", "not_webp.png"):
        blob = F.read(f)
        assert ops.webp_info(blob)[0] == F.IMP_ERROR_UNSUPPORTED, f
        assert ops.webp_decode_host(blob, capacity=1 << 16)[0] == F.IMP_ERROR_UNSUPPORTED, f
    # a version other than 0, and a VP8X container that announces an animation
    blob = bytearray(F.read("p_photo_17x13_m0.webp"))
    blob[24] |= 0x20
    assert ops.webp_info(bytes(blob))[0] == F.IMP_ERROR_UNSUPPORTED


def test_a_vp8x_container_with_other_chunks_is_taken():
    name, blob, expected = [f for f in F.load() if f[0] == "p_rgba_53x37_m3"][0]
    chunk = blob[12:]
    vp8x = b"VP8X" + (10).to_bytes(4, "little") + bytes([0x10, 0, 0, 0]) + (52).to_bytes(3, "little") + (36).to_bytes(3, "little")
    extra = b"EXIF" + (5).to_bytes(4, "little") + b"abcde\0" + b"zzzz" + (2).to_bytes(4, "little") + b"ab"
    body = b"WEBP" + vp8x + extra + chunk
    rc, frame, _, intact = ops.webp_decode_host(b"RIFF" + len(body).to_bytes(4, "little") + body)
    assert rc == F.IMP_OK and intact and (frame == expected).all()
    # a chunk whose size runs past the file
    broken = b"WEBP" + vp8x + b"EXIF" + (1 << 20).to_bytes(4, "little") + chunk
    assert ops.webp_decode_host(b"RIFF" + len(broken).to_bytes(4, "little") + broken, capacity=1 << 16)[0] == F.IMP_ERROR_DECODE_FAILED


def test_the_damaged_files_fail():
    for name, blob in F.damaged():
        assert ops.webp_decode_host(blob)[0] == F.IMP_ERROR_DECODE_FAILED, name


def test_prefixes_and_mutations_end_in_one_of_three_codes_inside_the_buffer():
    rng = np.random.default_rng(77)
    fixtures = {f[0]: f for f in F.load()}
    for name in ("p_photo_17x13_m3", "h_cache04"):
        _, blob, expected = fixtures[name]
        variants = [blob[:n] for n in range(len(blob))]
        for _ in range(200):
            b = bytearray(blob)
            b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
            variants.append(bytes(b))
        seen = set()
        for v in variants:
            # (a mutation of the size bits asks for another frame: the buffer is what the header the decoder reads asks for)
            irc, w, h, _ = ops.webp_info(v)
            cap = w * h * 4 if irc == F.IMP_OK else expected.size
            rc, frame, _, intact = ops.webp_decode_host(v, capacity=cap)
            assert intact, (name, len(v))
            assert rc in (F.IMP_OK, F.IMP_ERROR_UNSUPPORTED, F.IMP_ERROR_DECODE_FAILED), (name, rc)
            assert rc != F.IMP_OK or frame.shape == (h, w, 4)
            seen.add(rc)
        assert F.IMP_OK in seen and F.IMP_ERROR_DECODE_FAILED in seen and F.IMP_ERROR_UNSUPPORTED in seen, (name, seen)
