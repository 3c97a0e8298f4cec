"""The checker on wide AREA cells of gray frames: orc.cv_resize(..., INTER_AREA) on one channel against an exact
overlap-area average in float64.

test_gpu_wide_area_cover compares the bytes of the wide-cell kernels on gray frames with the oracle, so the oracle itself is
pinned here on the same shapes by independent code, as test_oracle_wide_area pins it for colour: cvResize accumulates in
float32 and rounds once, so it may differ from the exact average by the rounding of a value near a half: at most 1."""
import numpy as np
import pytest

import oracle_lib as orc
from test_gpu_gray_mix import widest_cell
from test_oracle_wide_area import SHAPES, overlap_weights

# (sw, sh, dw, dh) -> the widest horizontal cell, in source columns, and what the shape reaches
COVER_SHAPES = {
    (1401, 40, 70, 3): 21,       # the first width past the compile-time windows; two strips, the second partial
    (605, 90, 30, 7): 21,        # one partial strip
    (1300, 60, 33, 3): 41,       # y factor exactly 20
    (2509, 50, 130, 17): 21,     # three strips, two bands
    (1261, 37, 64, 37): 21,      # y untouched
    (700, 900, 30, 20): 24,      # 45-row cells
    (50, 7, 1, 2): 50,           # one column, W = sw
    (4090, 9, 64, 2): 65,        # the longest line, the multi-piece fetch
    (1331, 40, 70, 3): 20,       # stays with the bodies that have compile-time windows
    (4200, 9, 64, 2): 67,        # past the rule: the table kernel
}
W_MIN, W_MAX = 21, 66
ACCEPTED = [s for s, w in COVER_SHAPES.items() if W_MIN <= w <= W_MAX]
OLD_PATH, PAST_RULE = (1331, 40, 70, 3), (4200, 9, 64, 2)


def test_the_shapes_are_what_they_claim():
    assert all(s in SHAPES for s in COVER_SHAPES)
    for (sw, _, dw, _), w in COVER_SHAPES.items():
        assert widest_cell(sw, dw) == w, (sw, dw, widest_cell(sw, dw), w)
    assert len(ACCEPTED) == 8 and OLD_PATH not in ACCEPTED and PAST_RULE not in ACCEPTED


@pytest.mark.parametrize("shape", list(COVER_SHAPES), ids=lambda s: "%dx%d-%dx%d" % s)
def test_gray_area_is_the_overlap_average(shape):
    sw, sh, dw, dh = shape
    rng = np.random.Generator(np.random.PCG64(0x1A4DA000 + sw + 7 * dw))
    src = rng.integers(0, 256, size=(sh, sw, 1), dtype=np.uint8)
    wx, wy = overlap_weights(sw, dw), overlap_weights(sh, dh)
    exact = np.einsum("ys,sx,dx->yd", wy, src[:, :, 0].astype(np.float64), wx, optimize=True)
    got = orc.cv_resize(src, dw, dh, orc.INTER_AREA)
    assert got.shape[:2] == (dh, dw) and got.dtype == np.uint8
    worst = float(np.abs(got.reshape(dh, dw).astype(np.float64) - exact).max())
    print("%s gray: largest difference %.4f" % (shape, worst))
    assert worst <= 1.0, worst
