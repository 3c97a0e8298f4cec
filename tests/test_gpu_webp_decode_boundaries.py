"""The boundary fixtures of webp_dec_cases.boundary_cases() (tests/golden/webp_dec/h_b_*.webp: round edges, matches at the
wave's width, the predictor's second band of 256 rows, codes past the 10-bit table, 324 groups, the largest sides,
sub-images with matches and a cache) on the device against Pillow's frames: a family a call, the round and match files
alone and again, the longest sides next to a 1 x 1 file.  tests/test_webp_decode_boundaries_host.py proves what each file
reaches; tests/test_gpu_webp_decode.py decodes them with the rest of the directory too."""
import numpy as np
import pytest

import webp_dec_fixtures as F

pytestmark = pytest.mark.gpu
LAUNCHES = 3                                      # IMPGPU_WEBP_DEC_LAUNCHES
FAMILIES = {"a": 13, "b": 22, "c": 20, "d": 12, "e": 2, "f": 5, "g": 4}


def boundary(letters):
    return [f for f in F.load() if f[0].startswith("h_b_") and f[0][4] in letters]


def decode_together(imp, fixtures):
    """one call -> the names whose frame is not Pillow's"""
    results, launches = imp.ops.batch_decode_webp([blob for _, blob, _ in fixtures])
    assert launches == LAUNCHES
    wrong = []
    for (name, _, expected), (rc, im) in zip(fixtures, results):
        if rc != F.IMP_OK or im.shape != expected.shape or not np.array_equal(im.numpy(), expected):
            wrong.append((name, rc))
        if im is not None:
            im.release()
    return wrong


def test_each_family_in_one_call_is_pillows(gpu):
    wrong = {}
    for letter, count in sorted(FAMILIES.items()):
        fixtures = boundary(letter)
        assert len(fixtures) == count, letter
        bad = decode_together(gpu, fixtures)
        if bad:
            wrong[letter] = bad
    assert not wrong, wrong


def test_the_round_and_match_files_alone_and_again(gpu):
    imp = gpu
    wrong = []
    for name, blob, expected in boundary("ab"):
        frames = []
        for _ in range(2):
            rc, im = imp.ops.decode_webp(blob)
            frames.append(None if rc != F.IMP_OK else im.numpy().tobytes())
            if im is not None:
                im.release()
        if frames[0] is None or frames[0] != frames[1] or frames[0] != expected.tobytes():
            wrong.append(name)
    assert not wrong, wrong


def test_the_longest_sides_next_to_one_pixel(gpu):
    by_name = {f[0]: f for f in F.load()}
    names = ["h_b_f_pcg_1x16383", "p_photo_1x1_m0", "h_b_f_pcg_16383x1", "h_b_f_pal2_16383x1", "p_photo_1x1_m6"]
    assert by_name["h_b_f_pcg_1x16383"][2].shape == (16383, 1, 4) and by_name["h_b_f_pcg_16383x1"][2].shape == (1, 16383, 4)
    assert by_name["p_photo_1x1_m0"][2].shape == (1, 1, 4)
    assert decode_together(gpu, [by_name[n] for n in names]) == []
