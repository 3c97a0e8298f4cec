"""The checker on wide AREA cells: orc.cv_resize(..., INTER_AREA) against an exact overlap-area average in float64.

The GPU tests of the wide-cell kernels (test_gpu_wide_area) compare bytes with the oracle, so the oracle itself is pinned
here on the same shapes by independent code: two weight matrices (the length of the overlap of every destination cell with
every source pixel, over the cell's length) and one einsum.  cvResize accumulates in float32 and rounds once, so it may
differ from the exact average by the rounding of a value near a half: at most 1."""
import numpy as np
import pytest

import oracle_lib as orc

# (sw, sh, dw, dh): the smallest shapes at which the wide-cell body can go wrong (what each one hits: test_gpu_wide_area)
SHAPES = [(1401, 40, 70, 3), (1331, 40, 70, 3), (605, 90, 30, 7), (1009, 45, 37, 5), (1300, 60, 33, 3), (2509, 50, 130, 17),
          (1261, 37, 64, 37), (700, 900, 30, 20), (50, 7, 1, 2), (4090, 9, 64, 2), (4200, 9, 64, 2), (1210, 403, 60, 20)]


def overlap_weights(ssize, dsize):
    """W[d, s] = |[d * scale, (d + 1) * scale) n [s, s + 1)| / scale, scale = ssize / dsize: every row sums to 1."""
    scale = ssize / dsize
    d = np.arange(dsize, dtype=np.float64)[:, None]
    s = np.arange(ssize, dtype=np.float64)[None, :]
    lo = np.maximum(d * scale, s)
    hi = np.minimum(np.minimum((d + 1) * scale, float(ssize)), s + 1)
    return np.clip(hi - lo, 0, None) / scale


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_area_is_the_overlap_average(shape, c):
    sw, sh, dw, dh = shape
    rng = np.random.Generator(np.random.PCG64(0x1A4D9000 + sw + 7 * dw + c))
    src = rng.integers(0, 256, size=(sh, sw, c), dtype=np.uint8)
    wx, wy = overlap_weights(sw, dw), overlap_weights(sh, dh)
    assert np.allclose(wx.sum(axis=1), 1, atol=1e-12) and np.allclose(wy.sum(axis=1), 1, atol=1e-12)
    exact = np.einsum("ys,sxc,dx->ydc", wy, src.astype(np.float64), wx, optimize=True)
    got = orc.cv_resize(src, dw, dh, orc.INTER_AREA)
    assert got.shape == (dh, dw, c) and got.dtype == np.uint8
    worst = float(np.abs(got.astype(np.float64) - exact).max())
    print("%s c=%d: largest difference %.4f" % (shape, c, worst))
    assert worst <= 1.0, worst
