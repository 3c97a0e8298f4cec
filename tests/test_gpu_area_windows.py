"""Every window width of the row-streaming AREA body, on every path that instantiates it.

area_rows_body<CN, W> exists for W = 1..20 three times over (k_resize_area_rows, k_resize_area_mix, k_resize_area_mix_tail);
the window is the widest horizontal cell of the geometry.  With 70 destination columns (two column strips, the second a
partial one) and 70 * (W - 2) + 3 source columns the planner answers W for every W in 3..20, and 71 source columns give
W = 2.  No fractional x scale gives W = 1 (a cell longer than one pixel touches two); the one geometry that does is an x
scale of exactly 1 under a fractional y scale, every cell one whole source pixel: test_lone_window_of_one.  Likewise, when
the x scale is a whole number and the y scale is not, the cells are exactly `scale` wide and the planner's widening loop
adds a column at 4, 8, 12 and 16 (WIDENED below); no fractional x scale up to 1400 source columns widens.

Everything runs under the guard of resize_guard: pixels against the oracle, every byte around the windows against the
canary."""
import numpy as np
import pytest

import oracle_lib as orc
from conftest import noise_image
from resize_guard import CANARY, CLASSES, Layout, describe, guard_report, guarded_batch

gpu_test = pytest.mark.gpu

MIX_NV = 5                                                 # imp_resize.hip: windows of up to 4 * MIX_NV source columns
DW, DH, SH = 70, 37, 48                                     # two column strips; a partial last band at 4 and at 16 rows; scale_y ~ 1.3
WIDTHS = list(range(2, 4 * MIX_NV + 1))


# ---- a mirror of imp::area_max_count (imp_tables.cpp) and area_rows_plan (imp_resize.hip): keep in step with them
def model_max_count(ssize, dsize, scale):
    most = 0
    for d in range(dsize):
        f1 = d * scale
        f2 = f1 + scale
        s1, s2 = int(np.ceil(f1)), int(np.floor(f2))
        s2 = min(s2, ssize - 1)
        s1 = min(s1, s2)
        most = max(most, int(s1 - f1 > 1e-3) + (s2 - s1) + int(f2 - s2 > 1e-3))
    return most


def model_rows_plan(sw, dw, dh, frames, even=False):
    """(W, rows per band, columns the widening loop added) or None when the row-streaming body does not take the geometry."""
    scale_x = 1.0 / (float(dw) / sw)
    ww = widest = model_max_count(sw, dw, scale_x)
    if even:
        ww += ww & 1
    while ww <= 4 * MIX_NV and 63 * scale_x + ww + 8 > 256 * ((ww + 3) // 4):
        ww += 2 if even else 1
    if ww < 1 or ww > 4 * MIX_NV or sw < ww or sw < 4:
        return None
    b = 16
    nstrips = (dw + 63) // 64
    while b > 4 and frames * nstrips * ((dh + b - 1) // b) < 4096:
        b //= 2
    while b > 1 and frames * nstrips * ((dh + b - 1) // b) < 1024:
        b //= 2
    return ww, b, ww - widest - ((widest & 1) if even else 0)


def source_width(w):
    return 71 if w == 2 else DW * (w - 2) + 3


# x scale a whole number, y scale not: cells exactly 4 / 8 / 12 / 16 wide, the window one wider
WIDENED = [(4 * DW, 5), (8 * DW, 9), (12 * DW, 13), (16 * DW, 17)]
# frames for 1, 4 and 16 destination rows per band at DW x DH (not multiples of the XCD group of 8)
COUNT_BH = {1: 1, 4: 53, 16: 685}


def ragged_widths(w, c):
    """Source widths that keep window w at DW columns and end their rows at every phase of the 16-byte granule (and, for
    BGR, off the 4-byte grid)."""
    found = {}
    for sw in range(source_width(w), source_width(w) + 64):
        plan = model_rows_plan(sw, DW, DH, 3)
        if plan is None or plan[0] != w:
            continue
        key = (sw * c) % 16 if (sw * c) % 4 == 0 else "off4-%d" % ((sw * c) % 4)
        found.setdefault(key, sw)
    return found


def test_window_table_covers_every_width():
    for w in WIDTHS:
        for frames, bh in ((1, 1), (3, 1), (53, 4), (685, 16), (700, 16)):
            assert model_rows_plan(source_width(w), DW, DH, frames) == (w, bh, 0), (w, frames)
        assert source_width(w) % DW and SH % DH                  # neither scale is whole: the general AREA path
    assert sorted({model_rows_plan(source_width(w), DW, DH, 1)[0] for w in WIDTHS}) == list(range(2, 21))
    # the headline geometries
    assert model_rows_plan(1920, 224, 224, 1)[0] == 10 and model_rows_plan(3840, 224, 224, 1)[0] == 18
    assert model_rows_plan(DW, DW, DH, 3) == (1, 1, 0)         # x scale exactly 1: the one-column window
    # the widening loop: whole x scales of 4, 8, 12, 16 (20 leaves the body: the window would be 21)
    for sw, w in WIDENED:
        assert model_rows_plan(sw, DW, DH, 3) == (w, 1, 1), sw
    assert model_rows_plan(20 * DW, DW, DH, 3) is None
    # the mixed kernels carry the even windows: every width rounds up to its even neighbour
    assert sorted({model_rows_plan(source_width(w), DW, DH, 2, even=True)[0] for w in WIDTHS}) == list(range(2, 21, 2))
    # the ragged-end widths exist for every phase
    for w in (2, 5, 12, 20):
        assert set(ragged_widths(w, 4)) >= ({0, 4, 8, 12} if w > 2 else {4}), (w, ragged_widths(w, 4))
        bgr = ragged_widths(w, 3)
        assert any(str(k).startswith("off4") for k in bgr) or w == 2, (w, bgr)
    # the unaligned-BGR kernel's classes: ceil(widest cell / 4) = 1..5
    assert [(model_max_count(source_width(w), DW, 1.0 / (float(DW) / source_width(w))) + 3) // 4
            for w in (3, 7, 11, 15, 19)] == [1, 2, 3, 4, 5]


def test_guard_layout_classes():
    """resize_guard's layouts are in their class and keep their guards: pitch padding, rows between frames, 256 bytes and
    two rows in front and behind."""
    for cls in CLASSES:
        for row_bytes, rows, count in ((39, 11, 3), (280, 37, 9), (1, 1, 1), (528, 130, 9)):
            lay = Layout(row_bytes, rows, count, cls)
            assert lay.in_class() and lay.step > row_bytes and lay.stride >= (rows + 2) * lay.step
            assert lay.offset >= 256 and lay.offset >= 2 * lay.step and lay.total - lay.last >= max(256, 2 * lay.step)
            flat = np.zeros(lay.total, np.uint8)
            lay.windows(flat)[...] = 1
            assert int(flat.sum()) == row_bytes * rows * count


def test_guard_sees_every_stray_byte():
    """One changed byte anywhere around the windows is reported: the pitch padding, the rows between frames, the bytes in
    front of the first frame and behind the last; bytes inside the windows are not."""
    for cls in CLASSES:
        lay = Layout(39, 11, 3, cls)
        row_end = lay.offset + 4 * lay.step + lay.row_bytes              # frame 0, row 4: the first byte of its padding
        strays = [0, lay.offset - 1, row_end, row_end + lay.step - lay.row_bytes - 1, lay.offset + lay.rows * lay.step,
                  lay.offset + lay.stride - 1, lay.offset + lay.stride + lay.row_bytes, lay.last, lay.total - 1]
        for at in strays:
            flat = np.full(lay.total, CANARY, np.uint8)
            lay.windows(flat)[...] = 7
            flat[at] = 0xA4
            windows, intact, touched = guard_report(flat, lay)
            assert not intact and touched == [(at, at - lay.offset)] and (windows == 7).all(), (cls, at)
        flat = np.full(lay.total, CANARY, np.uint8)
        lay.windows(flat)[...] = 7
        windows, intact, touched = guard_report(flat, lay)
        assert intact and not touched and windows.shape == (3, 11, 39) and (windows == 7).all()


def _sources(sw, sh, c, seed, n=3):
    return [noise_image(sh, sw, c, seed + i) for i in range(n)]


def _check(g, frames, dw, dh, where):
    """Every frame equals its repeat, the distinct ones equal the oracle, and nothing around the windows changed."""
    period = len(frames)
    for i in range(period, g.windows.shape[0]):
        assert np.array_equal(g.windows[i], g.windows[i % period]), (where, "frame", i)
    for i, f in enumerate(frames):
        want = orc.cv_resize(f, dw, dh, orc.INTER_AREA)
        assert np.array_equal(g.windows[i], want), (where, "oracle", i)
    assert g.intact, (where, describe(g))


def _lone(gpu, sw, sh, dw, dh, c, count, align, where, **kw):
    frames = _sources(sw, sh, c, 9000 + sw + c, min(3, count))
    g = guarded_batch(gpu, frames, dw, dh, c, orc.INTER_AREA, count, align, **kw)
    _check(g, frames, dw, dh, where)


# ---- 1. the lone path
@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", WIDTHS)
def test_lone_sweep(gpu, w, c):
    align = "a16" if w % 2 == 0 else "a4"
    for bh in (1, 4):
        _lone(gpu, source_width(w), SH, DW, DH, c, COUNT_BH[bh], align, (w, c, bh))


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", [2, 11, 20])
def test_lone_sweep_full_bands(gpu, w, c):
    _lone(gpu, source_width(w), SH, DW, DH, c, COUNT_BH[16], "a16" if c == 4 else "a4", (w, c, 16))


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("sw,w", WIDENED)
def test_lone_widened_windows(gpu, sw, w, c):
    for count in (1, 53):
        _lone(gpu, sw, SH, DW, DH, c, count, "a16", (sw, w, c, count))


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
def test_lone_window_of_one(gpu, c):
    """x untouched, y shrunk by 1.3: W = 1, alone and behind the tail."""
    for count in (1, 53):
        _lone(gpu, DW, SH, DW, DH, c, count, "a4", (1, c, count))
    _tail(gpu, DW, SH, DW, DH, c, 3, "a16", (1, c, 3))


# ---- 2. the vertical walk: cells whose only row is a partial one, rows shared between neighbours, tall cells
@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("dh", [1, 9, 37])
@pytest.mark.parametrize("scale_y", [1.014, 2.5, 7.3, 18.04, 40.3])
def test_vertical_walk(gpu, scale_y, dh, c):
    sh = max(dh + 1, int(round(dh * scale_y)))
    _lone(gpu, source_width(7), sh, DW, dh, c, 3, "a4", (scale_y, dh, c))


# ---- 3. the ragged last granule, with the last source row ending its parent
@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", [2, 5, 12, 20])
def test_ragged_last_granule(gpu, w, c):
    widths = ragged_widths(w, c)
    assert widths
    for key, sw in sorted(widths.items(), key=lambda kv: kv[1]):
        sstep = (sw * c + 3) & ~3                           # the tightest pitch on the 4-byte grid: a row's end is the next row's start
        for count in (1, 53):
            _lone(gpu, sw, SH, DW, DH, c, count, "a4", (w, c, key, sw, count), sstep=sstep, src_at_end=True)


# ---- 4. the tail on the lone path: all four rotations, an overlay clipped by the right edge
def _tail(gpu, sw, sh, dw, dh, c, count, align, where):
    from test_gpu_chain import oracle_chain

    frames = _sources(sw, sh, c, 9500 + sw + c, min(3, count))
    ov = noise_image(11, 30, 4, 9600 + c)
    wm = ("r", "b", -9, 3, 65)                              # hangs over the right edge, sits above the bottom one
    cfg = gpu.Config()
    assert cfg.prepare_watermark(ov, *wm) == 0
    try:
        for rot in (0, 90, 180, 270):
            g = guarded_batch(gpu, frames, dw, dh, c, orc.INTER_AREA, count, align, rotate=rot, config=cfg)
            for i in range(len(frames), count):
                assert np.array_equal(g.windows[i], g.windows[i % len(frames)]), (where, rot, "frame", i)
            for i, f in enumerate(frames):
                rc, step, want = oracle_chain(f, resize="%d,%d" % (dw, dh), filters=["rotate=%d" % rot] if rot else [],
                                              overlay=ov, wm=wm)
                assert rc == 0 and np.array_equal(g.windows[i], want), (where, rot, "oracle", i)
            assert g.intact, (where, rot, describe(g))
    finally:
        cfg.release()


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", WIDTHS)
def test_tail_sweep(gpu, w, c):
    _tail(gpu, source_width(w), SH, DW, DH, c, 3, "a4" if w % 2 == 0 else "a16", (w, c, 3))


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
@pytest.mark.parametrize("w", [2, 20])
def test_tail_sweep_full_bands(gpu, w, c):
    _tail(gpu, source_width(w), SH, DW, DH, c, 700, "a16", (w, c, 700))


# ---- 5. BGR rows off the 4-byte grid: k_resize_area_cells<3, NV, R>
@gpu_test
@pytest.mark.parametrize("rows", ["R1", "R4"])
@pytest.mark.parametrize("nv", [1, 2, 3, 4, 5])
def test_unaligned_bgr_cells(gpu, nv, rows):
    w = 4 * nv - 1
    sw = source_width(w)
    dh, sh = 9, 12
    count = 3 if rows == "R1" else 1030                     # ceil(70 * ceil(9 / 4) / 256) = 1 block a frame: 1024 frames or more
    for dst_align in ("a1", "a4"):
        _lone(gpu, sw, sh, DW, dh, 3, count, dst_align, (nv, rows, dst_align), src_align="a1", sstep=sw * 3 + 1)


@gpu_test
@pytest.mark.parametrize("w", [3, 7, 11, 15, 19])
def test_aligned_bgr_source_odd_destination_pitch(gpu, w):
    """The sibling: the source stays on the 4-byte grid (k_resize_area_rows), the destination rows do not (byte stores)."""
    for count in (3, 53):
        _lone(gpu, source_width(w), SH, DW, DH, 3, count, "a1", (w, count), src_align="a4")


# ---- 6. the mixed launches
@gpu_test
@pytest.mark.parametrize("c", [3, 4])
def test_mixed_resize_every_width(gpu, c):
    import torch
    from test_gpu_int_mix import Frame, _check_frames

    rng = np.random.Generator(np.random.PCG64(0x1A4D9700 + c))
    frames = [Frame(torch, rng, c, source_width(w), SH, DW, DH, orc.INTER_AREA) for w in WIDTHS for _ in range(2)]
    torch.cuda.synchronize()
    rc, launches = gpu.batch_resize_mixed([f.item(0) for f in frames], c, count_launches=True)
    assert rc == 0 and launches >= 1, (rc, launches)
    _check_frames(gpu, frames, c, "every width")


@gpu_test
@pytest.mark.parametrize("c", [3, 4])
def test_batched_requests_every_width(gpu, c):
    from test_gpu_batch_ops import Configs, Req, _release, check_against_loop, check_against_oracle, run_both

    cf = Configs(gpu)
    cf.add("plain")
    cf.add("wm", noise_image(11, 30, 4, 9800 + c), ("r", "b", -9, 3, 65))
    reqs = []
    for k, w in enumerate(WIDTHS):
        job = {"resize": "%d,%d" % (DW, DH)}
        if k % 4:
            job["filters"] = ["rotate=%d" % (90 * (k % 4))]
        if k % 3 == 1:
            job["need_flatten"] = 1
        reqs.append(Req(noise_image(SH, source_width(w), c, 9900 + w), "wm" if k % 2 else "plain", **job))
    res, launches, ims, clones, loop = run_both(gpu, cf, reqs)
    check_against_loop(res, ims, clones, loop)
    check_against_oracle(cf, reqs, res, ims)
    assert all(r == (0, 7) for r in res), res
    _release(ims, clones)
    cf.release()
