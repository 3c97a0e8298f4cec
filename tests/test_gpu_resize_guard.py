"""Every lone resize kernel family under guard: pixels against the oracle AND every byte around the destination windows
against a canary (resize_guard).  launch_cn picks its kernels by scale, channel count, frame count and the alignment of
the six pointers and pitches, so each family runs under the alignment classes that keep it selected and under the class
just across the boundary, where its narrow fallback runs.

Shapes are (width, height).  Each case runs a lone frame and a small batch (9 frames where the kernel deals frames to the
XCDs in groups of 8); the cases that need a big launch to be selected at all repeat three distinct frames."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image
from resize_guard import CANARY, describe, guarded_batch
from test_gpu_area_windows import model_rows_plan

pytestmark = pytest.mark.gpu

NN, LINEAR, CUBIC, AREA, LANCZOS = orc.INTER_NN, orc.INTER_LINEAR, orc.INTER_CUBIC, orc.INTER_AREA, orc.INTER_LANCZOS4
NAMES = {NN: "nn", LINEAR: "linear", CUBIC: "cubic", AREA: "area", LANCZOS: "lanczos"}
DST_CLASSES = {1: ("a16", "a4", "a1"), 3: ("a16", "a4", "a1"), 4: ("a16", "a4")}


def check(gpu, c, src, dst, interp, counts, align, src_align=None, seed=0):
    (sw, sh), (dw, dh) = src, dst
    for count in counts:
        frames = [noise_image(sh, sw, c, 8000 + seed + i) for i in range(min(3, count))]
        g = guarded_batch(gpu, frames, dw, dh, c, interp, count, align, src_align)
        where = (NAMES[interp], c, src, dst, count, align, src_align)
        for i in range(len(frames), count):
            assert np.array_equal(g.windows[i], g.windows[i % len(frames)]), (where, "frame", i)
        for i, f in enumerate(frames):
            assert np.array_equal(g.windows[i], orc.cv_resize(f, dw, dh, interp)), (where, "oracle", i)
        assert g.intact, (where, describe(g))


def test_bgra_off_the_4_byte_grid_is_rejected(gpu):
    import torch

    src = torch.zeros(64 * 64 * 4 + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((32 * 32 * 4 + 4096,), CANARY, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for sp, sstep, dp, dstep in ((1, 256, 0, 128), (0, 257, 0, 128), (0, 256, 3, 128), (0, 256, 0, 131)):
        with pytest.raises(gpu.ImpError) as e:
            gpu.batch_cv_resize(src.data_ptr() + sp, 0, 60, 60, sstep, dst.data_ptr() + dp, 0, 30, 30, dstep, 4, 1, AREA)
        assert e.value.code == gpu.IMP_ERROR_INVALID_ARGS
    gpu.sync()
    assert bool((dst == CANARY).all())


# ---- NN: k_resize_nn<1|3|4>
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("src,dst", [((37, 41), (13, 11)), ((13, 11), (40, 41))], ids=["shrink", "grow"])
def test_nn(gpu, c, src, dst):
    for align in DST_CLASSES[c]:
        check(gpu, c, src, dst, NN, (1, 3), align)


# ---- gather taps: k_resize_taps<2|4|8, 1|3|4> -- gray at any scale, colour above 2 on an axis, and BGR whose source rows
# are off the 4-byte grid (the strips' fallback)
@pytest.mark.parametrize("interp", [LINEAR, CUBIC, LANCZOS], ids=lambda m: NAMES[m])
@pytest.mark.parametrize("c", [1, 3, 4])
def test_taps(gpu, c, interp):
    for align in DST_CLASSES[c]:
        check(gpu, c, (90, 200), (30, 67), interp, (1, 3), align)
    if c == 1:
        for align in ("a16", "a1"):
            check(gpu, 1, (40, 30), (60, 45), interp, (1, 3), align)          # an enlargement
            check(gpu, 1, (300, 150), (200, 100), interp, (1, 3), align)      # a scale below 2
    if c == 3:
        for src, dst in (((96, 54), (192, 108)), ((300, 150), (200, 100))):
            if not (interp == CUBIC and dst[1] > src[1]):                      # (that one is the CUBIC enlargement's)
                check(gpu, 3, src, dst, interp, (1, 3), "a4", src_align="a1")


# ---- rolling strips: k_resize_strip<2|4|8, 3|4> and k_resize_strip2 at the row patterns (1,0), (1,2), (2,1).  The
# pattern (0,1) needs two destination rows on one source row at the top of the frame, which (d + 0.5) * scale - 0.5 gives
# for no scale: it is not reachable from a lone frame.  (2,1) holds for at most four destination rows (scale 1.75).
# 16-byte (BGR: 4-byte) patch stores under the aligned class, the narrow ones under the next.
STRIPS = [((96, 54), (192, 108)),        # 2x up: (1,0)
          ((300, 150), (200, 100)),      # 1.5x down: (1,2)
          ((150, 90), (300, 60)),        # x grows 2x, y shrinks 1.5x
          ((150, 7), (100, 4)),          # 1.75x down on y, four rows: (2,1)
          ((333, 77), (500, 100)),       # no period: k_resize_strip
          ((150, 97), (300, 60))]        # no period while y shrinks: CUBIC's k_resize_strip


# (CUBIC comes to the strips only when y shrinks: its enlargements are test_cubic_enlargement's)
STRIP_CASES = [(g, m) for g in STRIPS for m in (LINEAR, CUBIC, LANCZOS) if not (m == CUBIC and g[1][1] >= g[0][1])]


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("geom,interp", STRIP_CASES, ids=lambda v: NAMES[v] if isinstance(v, int) else "%dx%d-%dx%d" % (v[0] + v[1]))
def test_strips(gpu, geom, interp, c):
    src, dst = geom
    for align in (("a16", "a4") if c == 4 else ("a4", "a1")):
        check(gpu, c, src, dst, interp, (1, 3), align, src_align="a16" if align == "a16" else "a4")


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("geom,count", [(STRIPS[0], 300), (STRIPS[1], 300), (STRIPS[3], 2050)], ids=["up2", "down1.5", "down1.75"])
def test_strips_lanczos_static_schedule(gpu, geom, count, c):
    """The eight-tap static schedule needs strips of 16 rows or more, which a launch takes from 8192 waves on: 300 frames
    of 108 or 100 rows, 2050 of four."""
    src, dst = geom
    for align in (("a16", "a4") if c == 4 else ("a4", "a1")):
        check(gpu, c, src, dst, LANCZOS, (count,), align, src_align="a16" if align == "a16" else "a4")


# ---- exact halves: the DMA rings (sources on the 16-byte grid; BGR: widths that are multiples of 16) and the
# register-rolling kernels (everything else).  260 and 264 leave a partial last column strip, 131 is an odd half width;
# 130 rows are two 60-row strips and a partial one.
@pytest.mark.parametrize("interp", [LINEAR, CUBIC, LANCZOS], ids=lambda m: NAMES[m])
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("sw", [260, 262, 264, 272])
def test_exact_halves(gpu, sw, c, interp):
    src, dst = (sw, 260), (sw // 2, 130)
    dsts = ("a16", "a4") if c == 4 else ("a16", "a4", "a1")
    for align in dsts:
        check(gpu, c, src, dst, interp, (1, 9), align, src_align="a16")        # the ring where the width allows it
    check(gpu, c, src, dst, interp, (1, 9), dsts[-1], src_align="a4")           # the rolling kernels


@pytest.mark.parametrize("c", [3, 4])
def test_exact_halves_one_row(gpu, c):
    """One destination row out of three source rows: the columns step by two, the row weights are not mirror-symmetric."""
    for src_align in ("a16", "a4"):
        for interp in (CUBIC, LANCZOS):
            check(gpu, c, (272, 3), (136, 1), interp, (1, 9), "a4", src_align=src_align)


# ---- CUBIC enlargement: k_resize_up_cubic4 / 3 <0|2|3|4>
UPS = [((64, 33), (64, 66)), ((64, 45), (192, 135)), ((32, 50), (128, 200)), ((41, 37), (123, 37)), ((70, 30), (77, 90)),
       ((100, 161), (515, 333))]


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("geom", UPS, ids=lambda g: "%dx%d-%dx%d" % (g[0] + g[1]))
def test_cubic_enlargement(gpu, geom, c):
    src, dst = geom
    for align in DST_CLASSES[c]:
        check(gpu, c, src, dst, CUBIC, (1, 3), align)


# ---- whole-factor AREA: k_area2x2_c4 (even widths) / v4 (odd) / v3, k_area_boxc<8>, k_area_boxl<4, 3..7> and <3, 2..8>,
# k_resize_area_int beyond (a factor of 9, gray, BGR rows off the 4-byte grid)
@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("isx,isy", [(2, 2), (2, 3), (3, 2), (4, 3), (5, 1), (6, 2), (7, 3), (8, 2), (9, 2), (3, 9)])
def test_whole_factor_area(gpu, isx, isy, c):
    for dw in (5, 17, 130):
        for dh in (1, 9):
            for align in DST_CLASSES[c]:
                check(gpu, c, (dw * isx, dh * isy), (dw, dh), AREA, (1, 3), align, seed=dw)


# ---- general AREA, four columns per lane: k_resize_area_rows4<3|4, 2..5> -- 160 columns or more and 2048 waves
ROWS4_DW, ROWS4_DH, ROWS4_SH, ROWS4_COUNT = 261, 9, 12, 515


def _rows4_width(w):
    """The first source width whose widest cell is w columns at ROWS4_DW destination columns."""
    for sw in range(ROWS4_DW + 1, 5 * ROWS4_DW):
        plan = model_rows_plan(sw, ROWS4_DW, ROWS4_DH, ROWS4_COUNT)
        if plan and plan[0] == w and sw % ROWS4_DW:
            assert plan[1] == 8                                # 515 * 5 strips * 2 bands >= 4096: bands of 8 rows, 2060 waves
            return sw
    raise AssertionError(w)


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", [2, 3, 4, 5])
def test_area_four_columns_per_lane(gpu, w, c):
    sw = _rows4_width(w)
    for align, src_align in ((("a16", "a16"), ("a4", "a4")) if c == 4 else (("a4", "a4"), ("a1", "a4"), ("a4", "a1"))):
        check(gpu, c, (sw, ROWS4_SH), (ROWS4_DW, ROWS4_DH), AREA, (ROWS4_COUNT,), align, src_align=src_align)


# ---- general AREA through the run tables: k_resize_area<1|3|4> -- gray, and colour at factors above 18
@pytest.mark.parametrize("c", [1, 3, 4])
def test_area_tables(gpu, c):
    for align in DST_CLASSES[c]:
        check(gpu, c, (17 * 21 + 5, 19), (17, 9), AREA, (1, 3), align)
        if c == 1:
            check(gpu, c, (353, 48), (70, 37), AREA, (1, 3), align)


# ---- fused tails
def _tail(gpu, c, src, dst, counts, align, src_align, rotations, where):
    from test_gpu_chain import oracle_chain

    (sw, sh), (dw, dh) = src, dst
    ov = noise_image(12, 20, 4, 8600 + c)
    wm = ("r", "b", 0, 0, 70)                                  # touches the right and the bottom edge
    cfg = gpu.Config()
    assert cfg.prepare_watermark(ov, *wm) == 0
    try:
        for count in counts:
            frames = [noise_image(sh, sw, c, 8700 + i) for i in range(min(3, count))]
            for rot in rotations:
                g = guarded_batch(gpu, frames, dw, dh, c, AREA, count, align, src_align, rotate=rot, config=cfg)
                for i in range(len(frames), count):
                    assert np.array_equal(g.windows[i], g.windows[i % len(frames)]), (where, count, rot, "frame", i)
                for i, f in enumerate(frames):
                    rc, step, want = oracle_chain(f, resize="%d,%d" % (dw, dh), filters=["rotate=%d" % rot] if rot else [],
                                                  overlay=ov, wm=wm)
                    assert rc == 0 and np.array_equal(g.windows[i], want), (where, count, rot, "oracle", i)
                assert g.intact, (where, count, rot, describe(g))
    finally:
        cfg.release()


@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("dh", [50, 52, 64])
def test_area_rotate_tail(gpu, dh, c):
    """launch_area_rotate at all four turns.  515 frames take bands of 16 rows: a quarter turn then stores runs of 16
    pixels, the last band's run is 2 (dh 50), 4 (52: BGRA's 16-byte store ends on the row's last pixel) or 16 pixels
    (64: BGR's 48 bytes do); 3 frames take single rows.  Off the 4-byte grid the unfused fallback runs."""
    src, dst = (100, (dh * 4 + 2) // 3), (70, dh)
    for align in (("a16", "a4") if c == 4 else ("a16", "a4", "a1")):
        _tail(gpu, c, src, dst, (3, 515), align, "a4" if align == "a1" else align, (0, 90, 180, 270), (dh, c, align))


@pytest.mark.parametrize("rw", [130, 131])
@pytest.mark.parametrize("rh", [50, 52])
def test_area_2x2_rotate_tail(gpu, rw, rh):
    """Exact halves with a quarter turn: k_area2x2_turn (even halved widths), k_area2x2_rotate_bgra (odd ones); a source
    off the 16-byte grid and BGR take the unfused fallback."""
    src, dst = (2 * rw, 2 * rh), (rw, rh)
    for align in ("a16", "a4"):
        _tail(gpu, 4, src, dst, (3, 9), align, "a16", (90, 270), (rw, rh, align))
    _tail(gpu, 4, src, dst, (3,), "a4", "a4", (90, 270), (rw, rh, "src a4"))
    _tail(gpu, 3, src, dst, (3,), "a4", "a4", (90, 270), (rw, rh, "bgr"))
